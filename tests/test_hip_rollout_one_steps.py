"""rollout_one_steps_kernel - one generated body per step index (csrc/rollout_one.hip, tools/gen_rollout_one.py: one_solve_t<t>) -
against the epoch loop of rollout_one_kernel, the two forms of a LEAN launch that GPMPC_ROLLOUT_ONE_STEPS=1 / =0 select.  Both run
the same operations in the same order, so X_traj and info are compared with np.array_equal; every launch asserts the kernel
(gpmpc_debug_last_rollout_path) and the form (gpmpc_debug_last_rollout_one_form) it took.

  * Ns = 3, every H in 1 .. 30, feedback on and off: every static step is the last step of some launch (its exit), every epoch
    change and every block that wraps into the next group is crossed.  H = 1 has no instance of the kernel (rollout_one_sizing:
    H >= 2): the pinned launch falls to the generic kernel under either value of the knob, which the case asserts.
  * Ns = 5, H = 30, beta = 0.7, feedback off, per-sample start states: the clip sends steps through the cold block that
    stands beside the static steps' spine (and shares their one rare branch with the root retry and the launch's end).
  * Ns = 300 (more chains than the chip has compute units) and Ns = 2048 (two rounds of one wave per SIMD), H = 30.
  * Ns = 8, H = 30 with the inputs of tests/golden/make_rollout_one_parent_xtraj.py: bit for bit the parent's X_traj
    (tests/golden/rollout_one_parent_xtraj.npz), steps form.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KNOB = "GPMPC_ROLLOUT_ONE_STEPS"
H_MAX = 30


def _maker():
    spec = importlib.util.spec_from_file_location("make_rollout_one_parent_xtraj", os.path.join(GOLDEN, "make_rollout_one_parent_xtraj.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


class _Ctx:
    def __init__(self):
        import sampling_gpmpc_amd as sg
        from sampling_gpmpc_amd import _lib
        self.sg, self._lib, self.lib = sg, _lib, _lib.load()
        self.mk = _maker()
        self.cases = {}

    def case(self, Ns, feedback):
        """(agent, base samples for H_MAX steps, per-sample start states) for Ns samples: built once, shared by every H"""
        if (Ns, feedback) not in self.cases:
            from sampling_gpmpc_amd.workloads import fs_params
            p = fs_params(self.mk.PNAME, Ns, H_MAX, nograd=False, feedback=feedback)
            p["common"]["use_cuda"] = True
            p["agent"]["base_sample_generator"] = "counter"
            agent = self.sg.Agent(p, self.sg.make_env(p))
            g = torch.Generator().manual_seed(4100 + Ns)
            z = torch.randn(H_MAX, Ns * 3, generator=g, dtype=torch.float64).clamp(-2.5, 2.5).to(agent.torch_device)
            x0 = torch.tensor(p["env"]["start"][:2], dtype=torch.float64) + 0.3 * torch.randn(Ns, 2, generator=g, dtype=torch.float64)
            self.cases[(Ns, feedback)] = (agent, z, x0.to(agent.torch_device))
        return self.cases[(Ns, feedback)]

    def launch(self, monkeypatch, case, H, feedback, steps, x0=None, beta=None):
        """one LEAN launch pinned to ONE under GPMPC_ROLLOUT_ONE_STEPS = steps: (X_traj, info, path, form)"""
        from sampling_gpmpc_amd.rollout import rollout_device
        from sampling_gpmpc_amd.workloads import synthetic_u_ff
        agent, z, _ = case
        monkeypatch.setenv(KNOB, "1" if steps else "0")
        self.lib.gpmpc_rollout_pin_kernel(self._lib.KERNEL_ONE)
        try:
            res = rollout_device(agent, synthetic_u_ff(1, H), z.reshape(-1), z.shape[1], H=H, mode=self._lib.MODE_RECONDITIONED,
                                 use_model_without_derivatives=False, use_feedback=feedback, x0=x0, var_zero_thr=-1.0, beta=beta,
                                 want_samples=False)
            path, form = self.lib.gpmpc_debug_last_rollout_path(), self.lib.gpmpc_debug_last_rollout_one_form()
            return res.X_traj.cpu().numpy(), res.info.cpu().numpy(), path, form
        finally:
            self.lib.gpmpc_rollout_pin_kernel(-1)

    def both(self, monkeypatch, Ns, H, feedback, per_sample=False, beta=None):
        case = self.case(Ns, feedback)
        x0 = case[2] if per_sample else None
        Xl, il, pl, fl = self.launch(monkeypatch, case, H, feedback, False, x0, beta)
        Xs, is_, ps, fs = self.launch(monkeypatch, case, H, feedback, True, x0, beta)
        assert (pl, fl) == (self._lib.KERNEL_ONE, 0), f"loop launch: path {pl} form {fl}"
        assert (ps, fs) == (self._lib.KERNEL_ONE, 1), f"steps launch: path {ps} form {fs}"
        print(f"Ns={Ns} H={H} feedback={feedback}: max abs diff X {np.abs(Xs - Xl).max():.3e}, info bits {np.bitwise_or.reduce(il):#x}")
        assert np.isfinite(Xl).all()
        assert np.array_equal(Xs, Xl)
        assert np.array_equal(is_, il)
        return Xs, is_


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    return _Ctx()


@pytest.mark.parametrize("feedback", [True, False])
@pytest.mark.parametrize("H", list(range(1, H_MAX + 1)))
def test_every_step_is_a_launchs_last(ctx, monkeypatch, H, feedback):
    if H == 1:                                                    # no instance of ONE: the same generic launch either way
        case = ctx.case(3, feedback)
        Xl, il, pl, _ = ctx.launch(monkeypatch, case, H, feedback, False)
        Xs, is_, ps, _ = ctx.launch(monkeypatch, case, H, feedback, True)
        assert pl != ctx._lib.KERNEL_ONE and ps == pl
        assert np.array_equal(Xs, Xl) and np.array_equal(is_, il)
        return
    ctx.both(monkeypatch, 3, H, feedback)


def test_cold_block_beside_the_static_steps(ctx, monkeypatch):
    case = ctx.case(5, False)
    X, _ = ctx.both(monkeypatch, 5, H_MAX, False, per_sample=True, beta=0.7)
    # the clip did act: the same launch without it (the shipped beta) takes other values
    Xw, _, _, _ = ctx.launch(monkeypatch, case, H_MAX, False, True, case[2], None)
    assert not np.array_equal(X, Xw)


@pytest.mark.parametrize("Ns", [300, 2048])
def test_more_chains_than_a_round(ctx, monkeypatch, Ns):
    ctx.both(monkeypatch, Ns, H_MAX, True)


@pytest.mark.parametrize("feedback", [True, False])
def test_x_traj_has_the_parents_bits_at_h30(ctx, monkeypatch, feedback):
    mk = ctx.mk
    assert mk.NS == 8
    with np.load(os.path.join(GOLDEN, "rollout_one_parent_xtraj.npz")) as z:
        ref = z[mk.key(30, feedback)]
    monkeypatch.setenv(KNOB, "1")
    X, _, _ = mk.launch(mk.inputs(ctx.sg, feedback), 30, feedback, ctx._lib.KERNEL_ONE)
    assert ctx.lib.gpmpc_debug_last_rollout_one_form() == 1
    print(f"H=30 feedback={feedback}: max abs diff to the parent's X_traj {np.abs(X - ref).max():.3e}")
    assert X.shape == ref.shape and np.array_equal(X, ref)
