"""rollout_one_kernel after the bookkeeping left the step's spine (csrc/rollout_one.hip, profiles/one_spine.md): one exponent formula
for the grid-axis lanes and the lanes of appended points, INFO_VAR_CLAMPED from a running minimum of the three variances that is
tested once behind the step loop, the variance floor in the cold block only.  Pattern of test_rollout_one_append_steps.py: both
kernels pinned, the path of every launch asserted, rollout_fast_kernel - an independent implementation of the same arithmetic - as
the reference on the same base samples.

Tolerances: those of ``test_hip_parity.test_one_chain_mfma_rollout_against_oracle`` (X: rtol 1e-9 / atol 1e-11, Y: rtol 1e-7 /
atol 1e-11); the info bits agree apart from INFO_VAR_CLAMPED, which is compared where it does not hang on the last bits of a
variance (see clamp_bit_checks).
"""
import numpy as np
import pytest
import torch

from tests.helpers import fs_params, synthetic_u_ff

pytestmark = pytest.mark.gpu

X_TOL = dict(rtol=1e-9, atol=1e-11)
Y_TOL = dict(rtol=1e-7, atol=1e-11)
PNAME = "params_pendulum1D_samples"
H_MAX = 30
NS = 3
FLOORS = [10.0 ** e for e in range(-14, 3)]          # a decade grid, 1e-14 .. 1e2
GRID_H = [2, 5, 6, 12, 30]
U_FF = synthetic_u_ff(1, H_MAX)                      # ONE input sequence: a launch of H steps reads its first H rows


@pytest.fixture(scope="module")
def sg():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    import sampling_gpmpc_amd as pkg
    pkg._lib.load()
    return pkg


_cases = {}


def case(sg, feedback):
    """(agent, z, per-sample start states), made once per module: the horizon is a launch argument, so one agent and one slab
    of base samples (step-major, H_MAX steps) serve every H - and a launch of H steps is the head of a launch of H' > H steps."""
    if feedback not in _cases:
        p = fs_params(PNAME, NS, H_MAX, nograd=False, feedback=feedback)
        p["common"]["use_cuda"] = True
        p["agent"]["base_sample_generator"] = "counter"
        agent = sg.Agent(p, sg.make_env(p))
        g = torch.Generator().manual_seed(5100 + int(feedback))
        z = torch.randn(H_MAX, NS * 3, generator=g, dtype=torch.float64).clamp(-2.5, 2.5).to(agent.torch_device)
        x0 = (torch.tensor(p["env"]["start"][:2], dtype=torch.float64) + 0.3 * torch.randn(NS, 2, generator=g, dtype=torch.float64))
        _cases[feedback] = (agent, z, x0.to(agent.torch_device))
    return _cases[feedback]


def launch(sg, kern, H, feedback, outputs=False, floor=None, beta=None):
    """one pinned launch of H steps; floor: the GP descriptor's var_floor for this launch"""
    from sampling_gpmpc_amd import _lib
    from sampling_gpmpc_amd.rollout import rollout_device
    lib = _lib.load()
    agent, z, x0 = case(sg, feedback)
    desc = agent._plan(use_grad=True).desc
    saved = desc.var_floor
    try:
        if floor is not None:
            desc.var_floor = float(floor)
        lib.gpmpc_rollout_pin_kernel(kern)
        # (var_zero_thr < 0 and no optional outputs: the LEAN instantiation)
        res = rollout_device(agent, U_FF[:H], z.reshape(-1), z.shape[1], H=H, mode=_lib.MODE_RECONDITIONED,
                             use_model_without_derivatives=False, use_feedback=feedback, x0=x0, var_zero_thr=-1.0, beta=beta,
                             want_samples=outputs)
        path = lib.gpmpc_debug_last_rollout_path()
        assert path == kern, f"kernel path {path}, pinned {kern}"
        return res.X_traj.cpu().numpy(), (res.Y.cpu().numpy() if outputs else None), res.info.cpu().numpy()
    finally:
        lib.gpmpc_rollout_pin_kernel(-1)
        desc.var_floor = saved


# ---- (a) parity against rollout_fast --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("outputs", [False, True], ids=["lean", "outputs"])
@pytest.mark.parametrize("feedback", [True, False], ids=["feedback", "open_loop"])
@pytest.mark.parametrize("H", [2, 3, 6, 11, 30])
def test_one_against_fast(sg, H, feedback, outputs):
    """a start state per sample; with Y / Xi requested the non-LEAN instantiation runs (the `store` path of the entries)"""
    from sampling_gpmpc_amd import _lib
    X1, Y1, i1 = launch(sg, _lib.KERNEL_ONE, H, feedback, outputs)
    Xf, Yf, i_f = launch(sg, _lib.KERNEL_FAST, H, feedback, outputs)
    msg = f"H={H} feedback={feedback} outputs={outputs}: max abs diff X {np.abs(X1 - Xf).max():.3e}"
    if outputs:
        msg += f" Y {np.abs(Y1 - Yf).max():.3e}"
    print(msg)
    assert np.isfinite(X1).all()
    np.testing.assert_allclose(X1, Xf, **X_TOL)
    if outputs:
        np.testing.assert_allclose(Y1, Yf, **Y_TOL)
    np.testing.assert_array_equal(i1 & ~_lib.INFO_VAR_CLAMPED, i_f & ~_lib.INFO_VAR_CLAMPED)


# ---- (b), (c) the clamp bit ---------------------------------------------------------------------------------------------------
def clamp_bit_checks(sg, feedback, beta):
    """INFO_VAR_CLAMPED of rollout_one: "some step's variance was below the floor", kept as a running minimum across the launch.

    * floor -1: clear for every sample; floor 10 x outputscale (above the prior variance of the value slot): set for every sample
    * monotone in the horizon: a launch of H steps is the head of a launch of H' > H steps (same inputs, same floor), so a bit set
      at H is set at H' - a minimum that forgot a step at an epoch change or in the cold block would break this
    * against rollout_fast: its variances differ from rollout_one's in the last bits, so the bits are compared where
      rollout_fast gives the same answer at floor / 4 and at 4 floor - there the answer does not hang on those bits.  At least
      half of the (floor, H, sample) grid has to qualify and the bit has to be set somewhere below H = 30.
    * the trajectories agree with rollout_fast's at every floor of the grid (the floored variance is formed in the cold block)"""
    from sampling_gpmpc_amd import _lib
    CL = _lib.INFO_VAR_CLAMPED
    agent, _, _ = case(sg, feedback)
    os_ = float(agent._plan(use_grad=True).desc.outputscale[0])
    for H in (2, 7, 30):
        _, _, lo = launch(sg, _lib.KERNEL_ONE, H, feedback, floor=-1.0, beta=beta)
        _, _, hi = launch(sg, _lib.KERNEL_ONE, H, feedback, floor=10.0 * os_, beta=beta)
        assert not (lo & CL).any(), f"H={H}: INFO_VAR_CLAMPED with a negative floor: {lo}"
        assert ((hi & CL) != 0).all(), f"H={H}: no INFO_VAR_CLAMPED with a floor of 10 x outputscale: {hi}"
    one = np.zeros((len(FLOORS), len(GRID_H), NS), dtype=bool)
    qualifies = np.zeros_like(one)
    fast = np.zeros_like(one)
    for i, F in enumerate(FLOORS):
        for j, H in enumerate(GRID_H):
            X1, _, i1 = launch(sg, _lib.KERNEL_ONE, H, feedback, floor=F, beta=beta)
            Xf, _, _ = launch(sg, _lib.KERNEL_FAST, H, feedback, floor=F, beta=beta)
            # (the floor bounds the clip interval: where it is above the variance the trajectories depend on it)
            np.testing.assert_allclose(X1, Xf, err_msg=f"floor={F:g} H={H}", **X_TOL)
            one[i, j] = (i1 & CL) != 0
            f_lo = (launch(sg, _lib.KERNEL_FAST, H, feedback, floor=F / 4, beta=beta)[2] & CL) != 0
            f_hi = (launch(sg, _lib.KERNEL_FAST, H, feedback, floor=4 * F, beta=beta)[2] & CL) != 0
            qualifies[i, j] = f_lo == f_hi
            fast[i, j] = f_hi
    print(f"feedback={feedback} beta={beta}: bit set in {int(one.sum())} of {one.size} (floor, H, sample); "
          f"{int(qualifies.sum())} qualify for the comparison with rollout_fast; "
          f"set below H = 30 in {int(one[:, :-1].sum())}; first H with the bit per floor (sample 0): "
          f"{[next((GRID_H[j] for j in range(len(GRID_H)) if one[i, j, 0]), None) for i in range(len(FLOORS))]}")
    for j in range(len(GRID_H) - 1):
        lost = one[:, j] & ~one[:, j + 1]
        assert not lost.any(), f"bit set at H={GRID_H[j]} and clear at H={GRID_H[j + 1]}: (floor, sample) {np.argwhere(lost).tolist()}"
    assert 2 * int(qualifies.sum()) >= qualifies.size, f"only {int(qualifies.sum())} of {qualifies.size} grid entries qualify"
    assert one[:, :-1].any(), "the bit is never set below H = 30: the monotonicity check is vacuous"
    bad = qualifies & (one != fast)
    assert not bad.any(), f"rollout_one's bit differs from rollout_fast's at (floor, H, sample) {np.argwhere(bad).tolist()}"


def test_clamp_bit(sg):
    clamp_bit_checks(sg, feedback=True, beta=None)


def test_clamp_bit_beside_the_cold_block(sg):
    """beta = 0.7 clips a slot in most steps (P(|z| > 0.7) = 0.48 per slot): the cold block (clip with the floored variance,
    repair of the speculated next state) runs next to the running minimum; feedback off"""
    clamp_bit_checks(sg, feedback=False, beta=0.7)
