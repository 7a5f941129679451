"""rollout_one_kernel with the ROTATED step loop (the next step's kernel entries are issued between the first pivot of
the sample's roots and the append): the edge horizons of the rotation, both optional-output settings, and the
out-of-line REPAIR paths that recompute the speculated next state when y[0] was replaced after the first pivot.

Everything goes through the public entry point ``rollout_device``; the kernel is asserted (path 4) and compared with
``rollout_fast_kernel`` (``GPMPC_ROLLOUT_ONE=0``, path 1) on the same base samples, at the tolerances of
``test_hip_parity.test_one_chain_mfma_rollout_against_oracle`` (X: rtol 1e-9 / atol 1e-11, Y: rtol 1e-7 / atol 1e-11).

The root retry (``info & ROOT_JITTER_MASK``) has no case here: no shape of the existing suite sets that bit for this
kernel (the posterior variances of a 30-step rollout stay between 2e-7 and 7e-5 in the CPU oracle's run, the label noise
keeps the appended points from making the 3 x 3 covariance singular), and no input was found with the CPU oracle that
makes the un-jittered 3 x 3 root fail.  ``test_repair_paths_report_no_root_retry`` records that the
bit stays clear, so a shape that does reach it shows up.
"""
import numpy as np
import pytest
import torch

from tests.helpers import fs_params, synthetic_u_ff

pytestmark = pytest.mark.gpu

X_TOL = dict(rtol=1e-9, atol=1e-11)
Y_TOL = dict(rtol=1e-7, atol=1e-11)
PNAME = "params_pendulum1D_samples"


@pytest.fixture(scope="module")
def sg():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    import sampling_gpmpc_amd as pkg
    pkg._lib.load()
    return pkg


def make_agent(sg, Ns, H, feedback=None, seed=7):
    p = fs_params(PNAME, Ns, H, nograd=False, feedback=feedback)
    p["agent"]["base_sample_generator"] = "vectorized"
    torch.manual_seed(seed)
    pg = {**p, "common": {**p["common"], "use_cuda": True}}
    return sg.Agent(pg, sg.make_env(pg))


def launch(sg, agent, H, monkeypatch, one, z=None, **kw):
    """One launch of the re-conditioned rollout on the agent's base samples (slab [t][1], as the forward-sampling loop)."""
    from sampling_gpmpc_amd import _lib
    from sampling_gpmpc_amd.rollout import rollout_device
    if one:
        monkeypatch.delenv("GPMPC_ROLLOUT_ONE", raising=False)
    else:
        monkeypatch.setenv("GPMPC_ROLLOUT_ONE", "0")
    erv = agent.epistimic_random_vector.to(device=agent.torch_device, dtype=torch.float64).contiguous()
    per_slab = agent.ns * agent.g_ny * 3
    if z is None:
        z = erv.reshape(-1)[per_slab:]
    res = rollout_device(agent, synthetic_u_ff(agent.nu, H), z, erv.shape[1] * per_slab, H=H, mode=_lib.MODE_RECONDITIONED,
                         use_model_without_derivatives=False, **kw)
    path = _lib.load().gpmpc_debug_last_rollout_path()
    assert path == (4 if one else 1), f"kernel path {path}: " + ("rollout_one_kernel" if one else "rollout_fast_kernel") + " was not selected"
    cpu = lambda t: None if t is None else t.cpu().numpy()
    return cpu(res.X_traj), cpu(res.Y), cpu(res.Xi), cpu(res.info)


def compare(tag, a, b):
    Xa, Ya, Xia, _ = a
    Xb, Yb, Xib, _ = b
    msg = f"{tag}: max abs diff X {np.abs(Xa - Xb).max():.3e}"
    assert np.isfinite(Xa).all()
    if Ya is not None:
        msg += f" Y {np.abs(Ya - Yb).max():.3e} Xi {np.abs(Xia - Xib).max():.3e}"
    print(msg)
    np.testing.assert_allclose(Xa, Xb, **X_TOL)
    if Ya is not None:
        np.testing.assert_allclose(Ya, Yb, **Y_TOL)
        np.testing.assert_allclose(Xia, Xib, **X_TOL)


@pytest.mark.parametrize("want_samples", [True, False])
@pytest.mark.parametrize("feedback", [True, False])
@pytest.mark.parametrize("H", [2, 3, 4, 30])
def test_rotated_loop_against_rollout_fast(sg, H, feedback, want_samples, monkeypatch):
    """H = 2: prologue + one rotated step + the tail step; H = 3, 4: the first wrap of the incomplete tile; H = 30: all epochs.
    Without the optional outputs only X_traj exists to compare."""
    agent = make_agent(sg, 9, H, feedback=feedback)
    one = launch(sg, agent, H, monkeypatch, True, want_samples=want_samples, use_feedback=feedback)
    fast = launch(sg, agent, H, monkeypatch, False, want_samples=want_samples, use_feedback=feedback)
    assert (one[1] is None) == (not want_samples)
    compare(f"H={H} feedback={feedback} samples={want_samples}", one, fast)


@pytest.mark.parametrize("feedback", [True, False])
def test_repair_after_clip_of_slot_0(sg, feedback, monkeypatch):
    """beta = 0.5 clips slot 0 in 62 % of the draws (P(|z_0| > 0.5), standard-normal z_0): in most steps the y[0] the next
    state was speculated from is replaced, and the cold block recomputes state, input and exponential.  Against beta = 1e6
    on the same z the sampled Y differ in EVERY (sample, step) pair of the CPU oracle's run of this shape (Ns = 16, H = 30:
    share 1.0 over all slots, 0.996 for slot 0 alone - after the first clip the chains' states differ for good); the test
    asks for at least a quarter before it compares the small-beta run with rollout_fast."""
    Ns, H = 16, 30
    agent = make_agent(sg, Ns, H, feedback=feedback, seed=11)
    small = launch(sg, agent, H, monkeypatch, True, beta=0.5, use_feedback=feedback)
    wide = launch(sg, agent, H, monkeypatch, True, beta=1e6, use_feedback=feedback)
    differ = (small[1].reshape(Ns, H, 3) != wide[1].reshape(Ns, H, 3)).any(-1)
    share0 = float((small[1].reshape(Ns, H, 3)[:, 0, 0] != wide[1].reshape(Ns, H, 3)[:, 0, 0]).mean())
    print(f"clipped (sample, step) pairs: {differ.mean():.3f}; slot 0 of step 0: {share0:.3f}")
    assert differ.mean() >= 0.25
    fast = launch(sg, agent, H, monkeypatch, False, beta=0.5, use_feedback=feedback)
    compare(f"beta=0.5 feedback={feedback}", small, fast)
    # and without the optional outputs (the other branch of the stores inside the repair)
    small_x = launch(sg, agent, H, monkeypatch, True, beta=0.5, use_feedback=feedback, want_samples=False)
    np.testing.assert_array_equal(small_x[0], small[0])


@pytest.mark.parametrize("thr", [1e-4, 1e-5])
def test_repair_after_variance_is_zero(sg, thr, monkeypatch):
    """The variance-is-zero replacement returns the mean for all three slots: y[0] changes in every such step.  The posterior
    variances of step 0 are (3.6e-6, 6.6e-5, 6.6e-6) and fall from there (CPU oracle): under 1e-4 every step is replaced, under
    1e-5 the first two steps are sampled and later ones replaced.  A replaced step ignores z, so with the threshold 1e-4 step 0
    must return bit for bit what a launch with z = 0 returns (there y = 0 + mu)."""
    Ns, H = 9, 12
    agent = make_agent(sg, Ns, H, seed=3)
    one = launch(sg, agent, H, monkeypatch, True, var_zero_thr=thr)
    fast = launch(sg, agent, H, monkeypatch, False, var_zero_thr=thr)
    compare(f"var_zero_thr={thr}", one, fast)
    off = launch(sg, agent, H, monkeypatch, True, var_zero_thr=-1.0)
    assert (one[1] != off[1]).any(), "the threshold replaced nothing"
    if thr == 1e-4:
        erv = agent.epistimic_random_vector
        zero = torch.zeros(erv.numel(), dtype=torch.float64, device=agent.torch_device)
        mean_run = launch(sg, agent, H, monkeypatch, True, z=zero, var_zero_thr=-1.0)
        Y, Ym, Yoff = (r[1].reshape(Ns, H, 3) for r in (one, mean_run, off))
        assert (Y[:, 0] == Ym[:, 0]).all(), "step 0 did not return the mean exactly"
        assert (Yoff[:, 0] != Ym[:, 0]).any()
        np.testing.assert_array_equal(one[0], mean_run[0])          # every step replaced: the whole rollout is the mean rollout


def test_repair_paths_report_no_root_retry(sg, monkeypatch):
    """(see the module docstring) the shapes above leave ROOT_JITTER_MASK clear: the retry's repair is not exercised here."""
    from sampling_gpmpc_amd import _lib
    agent = make_agent(sg, 16, 30, seed=11)
    info = launch(sg, agent, 30, monkeypatch, True, beta=0.5)[3]
    print("info bits:", sorted(set(int(i) for i in info)))
    assert not (info & _lib.INFO_ROOT_JITTER_MASK).any()
