"""rollout_one_kernel's append is selected by the step index (n_h = 3 t): every step t = 0 .. 28 has a block of its own in which
the incomplete tile row, the lanes of the new rows and the selects of the diagonal tiles are compile-time constants
(csrc/rollout_one.hip, section (vi)).  A wrong block shows only from the step after it, so every block is made the last
appending step of one launch (H = t + 2), against rollout_fast_kernel - an independent implementation of the same arithmetic -
on the same base samples.  Both kernels are pinned and the path each launch took is asserted.

Tolerances: those of ``test_hip_parity.test_one_chain_mfma_rollout_against_oracle`` (X: rtol 1e-9 / atol 1e-11, Y: rtol 1e-7 /
atol 1e-11); the info bits agree apart from INFO_VAR_CLAMPED.
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


@pytest.fixture(scope="module")
def sg():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    import sampling_gpmpc_amd as pkg
    pkg._lib.load()
    return pkg


_cases = {}


def case(sg, Ns, feedback):
    """(agent, z, per-sample start states) of a launch size, made once per module: the horizon is a launch argument, so one
    agent and one slab of base samples (step-major, H_MAX steps) serve every H."""
    key = (Ns, feedback)
    if key not in _cases:
        p = fs_params(PNAME, Ns, H_MAX, nograd=False, feedback=feedback)
        p["common"]["use_cuda"] = True
        p["agent"]["base_sample_generator"] = "counter"
        agent = sg.Agent(p, sg.make_env(p))
        g = torch.Generator().manual_seed(4200 + Ns)
        z = torch.randn(H_MAX, Ns * 3, generator=g, dtype=torch.float64).clamp(-2.5, 2.5).to(agent.torch_device)
        x0 = (torch.tensor(p["env"]["start"][:2], dtype=torch.float64) + 0.3 * torch.randn(Ns, 2, generator=g, dtype=torch.float64))
        _cases[key] = (agent, z, x0.to(agent.torch_device))
    return _cases[key]


def one_against_fast(sg, Ns, H, feedback=True, outputs=False, per_sample=False, beta=None):
    from sampling_gpmpc_amd import _lib
    from sampling_gpmpc_amd.rollout import rollout_device
    lib = _lib.load()
    agent, z, x0 = case(sg, Ns, feedback)
    out = {}
    try:
        for kern in (_lib.KERNEL_ONE, _lib.KERNEL_FAST):
            lib.gpmpc_rollout_pin_kernel(kern)
            # (var_zero_thr < 0 and no optional outputs: the LEAN instantiation)
            res = rollout_device(agent, synthetic_u_ff(1, H), z.reshape(-1), z.shape[1], H=H, mode=_lib.MODE_RECONDITIONED,
                                 use_model_without_derivatives=False, use_feedback=feedback, x0=x0 if per_sample else None,
                                 var_zero_thr=-1.0, beta=beta, want_samples=outputs)
            path = lib.gpmpc_debug_last_rollout_path()
            assert path == kern, f"kernel path {path}, pinned {kern}"
            out[kern] = (res.X_traj.cpu().numpy(), res.Y.cpu().numpy() if outputs else None, res.info.cpu().numpy())
    finally:
        lib.gpmpc_rollout_pin_kernel(-1)
    (X1, Y1, i1), (Xf, Yf, i_f) = out[_lib.KERNEL_ONE], out[_lib.KERNEL_FAST]
    msg = f"Ns={Ns} H={H} feedback={feedback} outputs={outputs}: max abs diff X {np.abs(X1 - Xf).max():.3e}"
    if outputs:
        msg += f" Y {np.abs(Y1 - Yf).max():.3e}"
    print(msg)
    assert np.isfinite(X1).all()
    np.testing.assert_allclose(X1, Xf, **X_TOL)
    if outputs:
        np.testing.assert_allclose(Y1, Yf, **Y_TOL)
    np.testing.assert_array_equal(i1 & ~_lib.INFO_VAR_CLAMPED, i_f & ~_lib.INFO_VAR_CLAMPED)
    return i1


@pytest.mark.parametrize("H", range(2, H_MAX + 1))
def test_every_step_block_is_the_last_append_of_a_launch(sg, H):
    """LEAN instantiation.  The block of step t = H - 2 is the last one to append; H = 11, 16 and 27 are the first launches to run
    the wrap blocks (t = 9, 14, 25: rows that reach into the next group's first diagonal tile)."""
    one_against_fast(sg, 3, H)


@pytest.mark.parametrize("H", [2, 5, 11, 16, 27, 30])
def test_step_blocks_with_the_optional_outputs(sg, H):
    """Y and Xi requested: the non-LEAN instantiation has blocks of its own."""
    one_against_fast(sg, 3, H, outputs=True)


def test_step_blocks_beside_the_clip_and_repair(sg):
    """beta = 0.7 clips a slot in most steps (P(|z| > 0.7) = 0.48 per slot): the cold block (clip, repair of the speculated next
    state) runs next to the step blocks; feedback off, a start state per sample."""
    one_against_fast(sg, 5, H_MAX, feedback=False, per_sample=True, beta=0.7)


def test_step_blocks_with_more_chains_than_compute_units(sg):
    one_against_fast(sg, 300, H_MAX)
