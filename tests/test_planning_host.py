"""``sampling_gpmpc_amd/_planning.py`` (no GPU needed): the Adam update against ``torch.optim.Adam`` bit for bit, the squared violation
against a loop, every branch of the input handling and of the planners' argument checks, and that each piece exists once."""
import glob
import math
import os

import pytest
import torch

from sampling_gpmpc_amd import _planning
from sampling_gpmpc_amd._lib import GpmpcError

F64 = torch.float64
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sampling_gpmpc_amd")
CPU = torch.device("cpu")


def test_adam_update_has_the_bits_of_torch_optim_adam():
    gen = torch.Generator().manual_seed(20)
    p0 = torch.randn(3, 4, 2, dtype=F64, generator=gen)
    grads = [torch.randn(3, 4, 2, dtype=F64, generator=gen) for _ in range(6)]
    lr = 0.05
    want = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([want], lr=lr)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    for it, g in enumerate(grads, start=1):
        want.grad = g.clone()
        opt.step()
        before = (p.clone(), m.clone(), v.clone())
        p_new, m_new, v_new = _planning.adam_update(p, m, v, g, it, lr)
        assert all(torch.equal(a, b) for a, b in zip((p, m, v), before))           # nothing is changed in place
        p, m, v = p_new, m_new, v_new
        state = opt.state[want]
        assert torch.equal(p, want.detach()), it
        assert torch.equal(m, state["exp_avg"]) and torch.equal(v, state["exp_avg_sq"]), it
    assert not torch.equal(p, p0)


def _violation_problem():
    gen = torch.Generator().manual_seed(5)
    n, T, R = 3, 4, 5
    val = torch.randn(n, T, R, dtype=F64, generator=gen)
    sd = 0.3 * torch.rand(n, T, R, dtype=F64, generator=gen)
    inf = float("inf")
    lo = torch.tensor([[-0.5, -inf, -inf, 0.2, -inf]] * T, dtype=F64)
    hi = torch.tensor([[inf, 0.4, inf, 1.0, -0.1]] * T, dtype=F64)
    lo[2:, 1] = -1.0                                                     # a side that is finite at some stages only
    hi[0, 3] = inf
    return val, sd, lo, hi


def _violation_loop(upper, lower, lo, hi):
    out = [0.0] * upper.shape[0]
    for s in range(upper.shape[0]):
        for t in range(upper.shape[1]):
            for r in range(upper.shape[2]):
                if math.isfinite(float(hi[t, r])):
                    out[s] += max(float(upper[s, t, r]) - float(hi[t, r]), 0.0) ** 2
                if math.isfinite(float(lo[t, r])):
                    out[s] += max(float(lo[t, r]) - float(lower[s, t, r]), 0.0) ** 2
    return torch.tensor(out, dtype=F64)


@pytest.mark.parametrize("form", ["tightened", "sampled"])
def test_squared_violation_against_a_loop(form):
    """Both calling forms: ``chance_constraint_penalty`` passes ``val + sd`` and ``val - sd``, ``sampled_tube_penalty`` ``val`` twice.
    The loop adds the same 2 T R = 40 squares per item in another order: 64 roundings of the result cover it.  No NaN reaches the
    gradient from a side that is not finite."""
    val, sd, lo, hi = _violation_problem()
    val.requires_grad_(True)
    upper, lower = (val + sd, val - sd) if form == "tightened" else (val, val)
    got = _planning.squared_violation(upper, lower, lo[None], hi[None])
    want = _violation_loop(upper.detach(), lower.detach(), lo, hi)
    assert got.shape == (3,) and float(want.min()) > 0
    assert float((got.detach() - want).abs().max()) <= 64 * 2.0 ** -52 * float(want.max())
    grad, = torch.autograd.grad(got.sum(), val)
    assert bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0
    # a row without a finite side takes no part at all
    assert not grad[:, :, 2].any()


def test_rollout_inputs_every_branch():
    x1, xn = torch.zeros(4), torch.zeros(7, 4)
    U2, Un = torch.zeros(5, 2, dtype=torch.float32), torch.zeros(7, 5, 2, dtype=F64)
    for x0, U in ((x1, U2), (xn, U2), (x1, Un), (xn, Un), (x1.tolist(), U2.tolist())):
        for n in (None, 7):
            a, b = _planning.rollout_inputs(x0, U, 4, 2, CPU, n=n)
            assert a.dtype == b.dtype == F64 and a.is_contiguous() and b.is_contiguous() and a.device == b.device == CPU
            assert a.shape == torch.Size(torch.as_tensor(x0).shape) and b.shape == torch.Size(torch.as_tensor(U).shape)
    # a strided view comes back contiguous, and the conversions keep the graph
    wide = torch.zeros(5, 4, dtype=F64, requires_grad=True)
    a, b = _planning.rollout_inputs(x1, wide[:, ::2], 4, 2, CPU)
    assert b.is_contiguous() and b.requires_grad
    b.sum().backward()
    assert torch.equal(wide.grad, torch.tensor([[1.0, 0.0, 1.0, 0.0]] * 5, dtype=F64))
    # without n any number of rows goes, and the message names the label
    _planning.rollout_inputs(torch.zeros(3, 4), torch.zeros(9, 5, 2), 4, 2, CPU)
    bad_x0 = [torch.zeros(3), torch.zeros(()), torch.zeros(7, 3), torch.zeros(1, 7, 4)]
    bad_U = [torch.zeros(5, 3), torch.zeros(2), torch.zeros(7, 5, 1), torch.zeros(1, 7, 5, 2)]
    for n, rows in ((None, "B"), (7, "7")):
        for x0 in bad_x0:
            with pytest.raises(GpmpcError, match=rf"x0 must be \(4,\) or \({rows}, 4\)"):
                _planning.rollout_inputs(x0, U2, 4, 2, CPU, n=n)
        for U in bad_U:
            with pytest.raises(GpmpcError, match=rf"U must be \(H, 2\) or \({rows}, H, 2\)"):
                _planning.rollout_inputs(x1, U, 4, 2, CPU, n=n)
    with pytest.raises(GpmpcError, match=r"x0 must be \(4,\) or \(Ns, 4\)"):
        _planning.rollout_inputs(torch.zeros(3), U2, 4, 2, CPU, label="Ns")
    # n given: a per-item array must have n rows
    with pytest.raises(GpmpcError, match=r"x0 must be \(4,\) or \(7, 4\)"):
        _planning.rollout_inputs(torch.zeros(6, 4), U2, 4, 2, CPU, n=7)
    with pytest.raises(GpmpcError, match=r"U must be \(H, 2\) or \(7, H, 2\)"):
        _planning.rollout_inputs(x1, torch.zeros(6, 5, 2), 4, 2, CPU, n=7)


def test_like_input():
    g = torch.arange(6.0, dtype=F64).reshape(3, 2)
    assert _planning.like_input(g, True) is g and torch.equal(_planning.like_input(g, False), g.sum(0))


def test_check_planner_args_every_branch():
    cost = lambda tube, U: U.sum()                                      # noqa: E731
    U3, U2 = torch.zeros(4, 5, 1), torch.zeros(5, 1)
    for who, rank, U0, other, text in (("plan_inputs", 3, U3, U2, "(B, H, nu)"), ("plan_inputs_sampled", 2, U2, U3, "(H, nu)")):
        ok = dict(U0=U0, cost=cost, steps=3, lr=0.1)
        _planning.check_planner_args(who, ok["U0"], rank, ok["cost"], ok["steps"], ok["lr"], text)
        _planning.check_planner_args(who, U0, rank, cost, 0, 1, text)                # no step at all, an integer rate
        for bad, what in ((dict(cost=None), "cost"), (dict(steps=-1), "steps"), (dict(steps=2.5), "steps"), (dict(steps=True), "steps"),
                          (dict(lr=0.0), "lr"), (dict(lr=-1.0), "lr"), (dict(lr=float("nan")), "lr"), (dict(lr=float("inf")), "lr"),
                          (dict(lr="0.1"), "lr"), (dict(lr=True), "lr"), (dict(U0=other), "U0"), (dict(U0=U0.tolist()), "U0")):
            kw = dict(ok)
            kw.update(bad)
            with pytest.raises(GpmpcError, match=f"{who}: {what} must be"):
                _planning.check_planner_args(who, kw["U0"], rank, kw["cost"], kw["steps"], kw["lr"], text)
        with pytest.raises(GpmpcError) as e:
            _planning.check_planner_args(who, other, rank, cost, 3, 0.1, text)
        assert text in str(e.value)


def test_each_piece_exists_once():
    src = {os.path.basename(p): open(p).read() for p in glob.glob(os.path.join(PKG, "*.py"))}
    assert [f for f, s in src.items() if "torch.lerp(" in s] == ["_planning.py"]
    assert [f for f, s in src.items() if "dtype=torch.uint8" in s] == ["_lib.py"]
    assert src["pathwise.py"].count("x0 must be") <= 1
    for f in ("pathwise.py", "moments.py", "mle.py"):
        assert "adam_update(" in src[f], f
    for f in ("pathwise.py", "moments.py"):
        for name in ("rollout_inputs(", "like_input(", "check_planner_args(", "squared_violation("):
            assert name in src[f] and f"def {name}" not in src[f] and f"def _{name}" not in src[f], (f, name)
    for f in ("pathwise.py", "small_ball.py", "hulls.py", "tube_rows.py"):
        assert "_lib.workspace(" in src[f], f
