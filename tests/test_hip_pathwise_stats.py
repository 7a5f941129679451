"""``gpmpc_pathwise_tube_stats`` / ``pathwise_tube_stats`` on the device: bit-equality with the unfused device path (draw, fit, rollout,
torch reductions), the CPU reference of tests/pathwise_stats_reference.py, chunking, the non-finite rule and the host wrapper.

Every run uses ``offset = 1000`` and is made with ``max_groups = 2`` (8 waves: every wave walks 8 or 9 of the 67 samples) and with the
library's grid.  Shapes are the smallest at which the kernel can go wrong (``pathwise_stats_reference.RUNS``); tolerances are the
``tube`` figures of ``pathwise_reference.tolerances(WORST_AB[run])``: a maximum of deviations moves by no more than the largest
deviation, so the reductions need none of their own."""
import numpy as np
import pytest
import torch

import sampling_gpmpc_amd as sg
from sampling_gpmpc_amd.pathwise import PathwiseSamples, merge_tube_stats, pathwise_tube_stats, tube_stats_of
from tests import pathwise_stats_reference as sref
from tests.test_hip_pathwise import DEV, dev, plan_env_of
from tests.test_pathwise_stats_host import same, tube_tol

pytestmark = pytest.mark.gpu
OFFSET = sref.OFFSET
GROUPS = (2, None)


def inputs(run):
    name, M, Ns, H = sref.RUNS[run]
    c, x0, U = sref.shared_inputs(run)
    plan, env = plan_env_of(name)
    return plan, env, c, dev(x0), dev(U), M, Ns


def thresholds(run):
    X, centre, scale = sref.tube(run)
    if X.shape[2] == 1:
        return (0.0,)
    return sref.thresholds(sref.stats(X, centre, OFFSET, scale)["sup"], tube_tol(run))[0]


def fused(run, groups, x0=None, U=None, centre=None, Ns=None, offset=OFFSET, eps=None, want_sup=True):
    plan, env, c, x0_d, U_d, M, Ns_run = inputs(run)
    _, centre_ref, scale = sref.tube(run)
    return pathwise_tube_stats(plan, x0_d if x0 is None else x0, U_d if U is None else U, Ns_run if Ns is None else Ns, M, c.seed, offset,
                               centre=dev(centre_ref) if centre is None else centre, scale=scale, eps=thresholds(run) if eps is None else eps,
                               want_sup=want_sup, env_desc=env, max_groups=groups)


def cpu(stats):
    torch.cuda.synchronize()
    import dataclasses
    return dataclasses.replace(stats, **{f: getattr(stats, f).cpu() for f in ("dev_max", "dev_arg", "box_lo", "box_hi", "sup", "n_within",
                                                                           "n_nonfinite") if getattr(stats, f) is not None})


@pytest.mark.parametrize("run", list(sref.RUNS))
def test_the_fused_call_has_the_bits_of_draw_rollout_and_torch_reductions(run):
    plan, env, c, x0, U, M, Ns = inputs(run)
    _, centre, scale = sref.tube(run)
    eps = thresholds(run)
    X = PathwiseSamples.draw(plan, Ns, M, c.seed, OFFSET).rollout(x0, U, env_desc=env)
    want = cpu(tube_stats_of(X, dev(centre), OFFSET, scale, eps, want_sup=True))
    assert int(want.n_nonfinite) == 0 and bool(torch.isfinite(want.sup).all())
    # the statement itself, spelled out once more on the tube
    Xc = X.cpu()
    d = (Xc - torch.from_numpy(centre)[None]).abs()
    assert torch.equal(want.dev_max, d.amax(0).T) and torch.equal(want.box_lo, Xc.amin(0).T) and torch.equal(want.box_hi, Xc.amax(0).T)
    assert torch.equal(want.sup, (d / torch.from_numpy(scale)[None, :, None]).amax((1, 2)))
    assert torch.equal(want.n_within, torch.tensor([int((want.sup <= e).sum()) for e in eps]))
    got = {g: cpu(fused(run, g)) for g in GROUPS}
    for g in GROUPS:
        same(got[g], want)                                                  # dev_arg: 1000 + the lowest index of the maximum
    same(got[2], got[None])
    assert int(got[2].dev_arg.min()) >= OFFSET and int(got[2].dev_arg.max()) < OFFSET + Ns
    # outputs that are not asked for are not needed
    few = cpu(fused(run, 2, eps=(), want_sup=False))
    assert few.sup is None and few.n_within is None and torch.equal(few.dev_max, want.dev_max) and torch.equal(few.dev_arg, want.dev_arg)


@pytest.mark.parametrize("run", list(sref.RUNS))
def test_against_the_cpu_reference(run):
    X, centre, scale = sref.tube(run)
    eps = thresholds(run)
    want = sref.stats(X, centre, OFFSET, scale, eps)
    got = cpu(fused(run, 2))
    tol = tube_tol(run)
    worst = {}
    for f in ("dev_max", "box_lo", "box_hi"):
        worst[f] = float((np.abs(getattr(got, f).numpy() - want[f]) / scale[None, :]).max())
    worst["sup"] = float(np.abs(got.sup.numpy() - want["sup"]).max())       # already in units of the scale
    print(run, {k: f"{v:.2e} / {tol:.2e}" for k, v in worst.items()}, "n_within", got.n_within.tolist(), want["n_within"].tolist())
    for f, v in worst.items():
        assert v <= tol, (run, f, v, tol)
    assert got.n_within.tolist() == want["n_within"].tolist()               # the thresholds keep 100 tolerances from every value
    assert int(got.n_nonfinite) == 0 and got.Ns == want["Ns"] and got.offset == OFFSET


@pytest.mark.parametrize("run", ["pend_fb", "car_fb"])
def test_a_run_cut_into_calls_merges_to_the_same_bits(run):
    whole = cpu(fused(run, None))
    parts = [cpu(fused(run, g, Ns=n, offset=o)) for g, (o, n) in zip((2, None, 1), ((1000, 13), (1013, 41), (1054, 13)))]
    same(merge_tube_stats(parts), whole)
    same(merge_tube_stats(parts[::-1]), whole)


@pytest.mark.parametrize("run", ["pend_fb", "car_nofb"])
def test_a_non_finite_state_is_never_ignored(run):
    plan, env, c, x0, U, M, Ns = inputs(run)
    H, nx = U.shape[0], x0.shape[0]
    fine = cpu(fused(run, 2))
    Ub = U.clone()
    Ub[2] = float("nan")
    inf = float("inf")
    for g in GROUPS:
        got = cpu(fused(run, g, U=Ub))
        for f in ("dev_max", "dev_arg", "box_lo", "box_hi"):                # stages <= 2 are those of the finite run
            assert torch.equal(getattr(got, f)[:3], getattr(fine, f)[:3]), f
        assert bool((got.dev_max[3:] == inf).all()) and bool((got.box_lo[3:] == -inf).all()) and bool((got.box_hi[3:] == inf).all())
        assert bool((got.dev_arg[3:] == OFFSET).all())
        assert bool((got.sup == inf).all()) and got.n_within.tolist() == [0] * len(got.eps) and int(got.n_nonfinite) == Ns
    xb = x0.clone()
    xb[nx - 1] = float("nan")
    got = cpu(fused(run, 2, x0=xb))
    assert bool((got.dev_max == inf).all()) and bool((got.box_lo == -inf).all()) and bool((got.box_hi == inf).all())
    assert bool((got.dev_arg == OFFSET).all()) and bool((got.sup == inf).all()) and got.n_within.tolist() == [0] * len(got.eps)
    assert int(got.n_nonfinite) == Ns and tuple(got.dev_max.shape) == (H + 1, nx)
    # a centre entry that is not finite poisons its own entry and every sample's sup, and no state
    _, centre, _ = sref.tube(run)
    cb = dev(centre).clone()
    cb[0, 1] = inf
    got = cpu(fused(run, 2, centre=cb))
    assert float(got.dev_max[1, 0]) == inf and int(got.dev_arg[1, 0]) == OFFSET and bool((got.sup == inf).all())
    keep = torch.ones_like(fine.dev_max, dtype=torch.bool)
    keep[1, 0] = False
    assert torch.equal(got.dev_max[keep], fine.dev_max[keep]) and torch.equal(got.box_lo, fine.box_lo) and int(got.n_nonfinite) == 0


def test_the_host_wrapper_centres_on_the_mean_function():
    """centre=None is the rollout of the Z = 0 sample of the same frequencies: stage 0 has no deviation, and the call equals the one with
    that centre passed explicitly."""
    from tests.helpers import closed_loop_params
    p = closed_loop_params("params_pendulum1D_samples", 8, 5, 1, 2)
    p["common"]["use_cuda"] = True
    p["agent"]["base_sample_generator"] = "counter"
    agent = sg.Agent(p, sg.make_env(p))
    x0 = torch.tensor(np.array(p["env"]["start"], dtype=np.float64))
    assert tuple(x0.shape) == (2,)
    U = 0.3 * torch.sin(torch.arange(5, dtype=torch.float64))[:, None]
    got = pathwise_tube_stats(agent, x0, U, 67, 128, seed=21, offset=OFFSET, eps=(0.01, 1.0), want_sup=True)
    pw = PathwiseSamples.draw(agent, 67, 128, 21, OFFSET)
    centre = pw.mean_only().rollout(x0, U)[0]
    explicit = pathwise_tube_stats(agent, x0, U, 67, 128, seed=21, offset=OFFSET, centre=centre, eps=(0.01, 1.0), want_sup=True, max_groups=3)
    same(cpu(got), cpu(explicit))
    assert not bool(got.dev_max[0].any()) and bool((got.dev_max[1:, 1] > 0).all())       # (the angle's first step does not see the GP)
    same(cpu(got), cpu(tube_stats_of(pw.rollout(x0, U), centre, OFFSET, None, (0.01, 1.0), want_sup=True)))
    assert torch.equal(got.tightening(), got.dev_max) and tuple(got.probability().shape) == (2,)
    assert DEV in str(got.dev_max.device)
