"""GPU: the joint draw (gpmpc_joint_sample_pending, mode J) on the case table of tests/joint_variants.py - other training sets (16 .. 65
observed real slots, grids and scattered points, value-only and with gradient labels) and other hyperparameters than the two shipped
models - against the CPU oracle.  The cases reach joint_real_mfma_kernel<., 4> (49 .. 64 real slots), the real block with three tasks
per point on the matrix pipe (Tr = 3), the dispatcher's boundaries (64 | 65 real slots, the 36 KB pair tables, 416 | 417 conditioning
slots) and per-task hyperparameters that the shipped ones cannot tell apart.  tests/test_joint_variants_host.py has checked on the CPU
that every case is as well conditioned as the shipped car, that the oracle's own covariance moves by less than 1e-8 max|Sigma_o| under a
reversal of its conditioning set, and that the oracle's result is more than 100 tolerances from the shipped GP's.

Every comparison is joint_draw_comparison_block of tests/test_hip_parity.py at its own tolerances and its default covariance bound of
1e-7 max|Sigma_o|: mean, variance, covariance, the samples at the kernel's own jitter level on the oracle's covariance, the legitimacy
of a retry, the Jacobians.  Per call the state of the draw (joint_call_state) is asserted first: the path that ran, the cached rows,
whether pending rows were used, and the kernel steps of the call's own launch plan against the table."""
import warnings

import numpy as np
import pytest
import torch

from tests import joint_variants as jv
from tests.test_hip_parity import joint_call_state, joint_draw_comparison_block, sg  # noqa: F401

pytestmark = pytest.mark.gpu

T = jv.T


def _ids(cases):
    return [c.name for c in cases]


PINNED = [c for c in jv.CASES if c.group != "eigh"]
NOPEND = [c for c in jv.CASES if c.steps_nopend is not None]
AUTO = [c for c in jv.CASES if c.steps_auto is not None]
EIGH = [c for c in jv.CASES if c.group == "eigh"]
assert {c.group for c in NOPEND} == {"NQ4", "deriv", "limit"} and len(EIGH) == 1
assert {c.group for c in jv.CASES} - {c.group for c in AUTO} == {"limit", "lds", "eigh"}


def _check_layout(case, agent):
    plan = agent.model_i.plan
    assert (int(plan.desc.N_r), int(plan.n_r), bool(plan.real_has_grad)) == (case.N_r, case.n_r, case.real_has_grad)
    assert int(plan.desc.real_has_grad) == int(case.real_has_grad)


def _draws_against_oracle(sg, case, mode):
    """_joint_draw_against_oracle's loop (tests/test_hip_parity.py) on the pair jv.make_pair builds.  ``mode``: "pinned" / "nopend" - the
    matrix-pipe path pinned, the oracle follows the kernel (the HIP Agent's hallucinated-set generation survives: its factor cache is
    hit from k = 2 on) - or "auto" - the dispatcher's own choice, the HIP Agent is assigned the oracle's tensors after every draw."""
    lib = sg._lib.load()
    expected = {"pinned": case.steps, "nopend": case.steps_nopend, "auto": case.steps_auto}[mode]
    agent, oagent, p = jv.make_pair(sg, case)
    H, figures = case.H, []
    lib.gpmpc_joint_pin_path(sg._lib.JOINT_AUTO if mode == "auto" else sg._lib.JOINT_MFMA)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for it, (x_h, u_h) in enumerate(jv.draw_points(case, p)):
                agent.train_hallucinated_dynGP(it)
                oagent.train_hallucinated_dynGP(it)
                if it == 0:
                    _check_layout(case, agent)
                bx = agent.get_batch_x_hat_u_diff(x_h, u_h)
                obx = oagent.get_batch_x_hat_u_diff(x_h, u_h)
                outs = agent.dyn_fg_jacobians(bx, it)
                st = joint_call_state(sg, agent)
                tag = f"{case.name} {mode} k={it}"
                print(f"{tag}: {case.n_r} + {st['n_ho']} slots, cached rows {st['n_cached_rows']}, pending mask {st['pending_mask']}, "
                      f"used_pending {st['used_pending']}; {st['plan']}")
                steps = st["plan"].split("|")[1].strip()
                assert steps == expected[it]
                valu = steps.startswith("joint_kernel(")
                assert st["path"] == (sg._lib.JOINT_VALU if valu else sg._lib.JOINT_MFMA)
                if mode != "auto" and not (case.group == "lds" and case.H == 42 and it == 0):
                    # the pinned path ran - or, beyond 64 real slots, the VALU path although the matrix pipe is pinned
                    assert st["path"] == (sg._lib.JOINT_MFMA if case.NQ is not None else sg._lib.JOINT_VALU)
                assert st["n_ho"] == it * H * T and st["plan"].startswith(f"path={st['path']} batches=1 ")
                assert st["n_cached_rows"] == (0 if mode == "auto" else max(0, it - 1) * H * T)
                assert st["used_pending"] == (mode == "pinned" and steps.startswith("joint_chol_mfma(pend_use)"))
                assert st["used_pending"] == (mode == "pinned" and it >= 2 and case.NQ is not None)
                assert not st["bits"] & (sg._lib.INFO_TRAIN_CHOL_FAIL | sg._lib.INFO_ROOT_EIGH)
                oouts = oagent.dyn_fg_jacobians(obx, it)
                assert not oagent.model_i_call.root_info.used_eigh
                spread, _ = jv.reversed_order_spread(oagent, oagent.env_model.get_g_xu_hat(obx))
                err, scale = joint_draw_comparison_block(agent, oagent, p, it, outs, oouts, tag=tag)
                lvl = (agent.model_i_call.last_info.cpu().numpy() >> 1) & 7
                print(f"{tag}: |Sigma - Sigma_o| {err / scale:.2e} max|Sigma_o|, the oracle's reversed-order spread {spread / scale:.2e} "
                      f"max|Sigma_o| ({scale:.2e}); jitter levels 0..{int(lvl.max())}: {np.bincount(lvl.reshape(-1), minlength=4).tolist()}")
                figures.append((err / scale, spread / scale))
                if mode == "auto":
                    agent.Hallcinated_X_train = oagent.Hallcinated_X_train.to(agent.torch_device)
                    agent.Hallcinated_Y_train = oagent.Hallcinated_Y_train.to(agent.torch_device)
                else:
                    oagent.Hallcinated_X_train = agent.Hallcinated_X_train.cpu()
                    oagent.Hallcinated_Y_train = agent.Hallcinated_Y_train.cpu()
    finally:
        lib.gpmpc_joint_pin_path(sg._lib.JOINT_AUTO)
    return figures


@pytest.mark.parametrize("case", PINNED, ids=_ids(PINNED))
def test_matrix_pipe_pinned_against_oracle(sg, case, monkeypatch):
    """(a) The matrix-pipe path pinned, the oracle follows the kernel, pending rows on: k = 0 joint_real_mfma(TEST), k = 1
    joint_real_mfma(FACTOR) + joint_chol_mfma(pend_use), from k = 2 joint_chol_mfma(pend_use) behind a hit cache - with NQ = 3 or 4 as
    the case's n_r decides.  Beyond 64 real slots the VALU path runs although the matrix pipe is pinned; with pair tables beyond 36 KB
    (64 real points, H = 42) k = 0 is the VALU head and k = 1 joint_test_mfma(FACTOR) instead of the real kernel; the limit group ends
    on 416 slots in one launch, 417 (a BOTTOM launch of one slot) and 423.

    (d) The cases with gradient labels on the real data take the block's own sample check (rtol 2e-5, atol 1e-8 at the kernel's jitter
    level on the oracle's covariance) like every other case, not the atol 2e-4 on branch-matched rows of
    test_derivative_observing_real_data: that test compares the two sides' draws directly, where a different jitter branch moves a
    sample by O(sqrt(jitter)); the block re-derives the reference draw at the level the kernel took, so the reason does not apply."""
    monkeypatch.setenv("GPMPC_JOINT_PENDING", "1")
    _draws_against_oracle(sg, case, "pinned")


@pytest.mark.parametrize("case", NOPEND, ids=_ids(NOPEND))
def test_matrix_pipe_without_pending_rows_against_oracle(sg, case, monkeypatch):
    """(b) GPMPC_JOINT_PENDING=0: from k = 2 on the new rows are joint_test_mfma(FACTOR) against the cached columns, so that kernel's
    run tables meet the real blocks of NQ = 4 and of three tasks per real point."""
    monkeypatch.setenv("GPMPC_JOINT_PENDING", "0")
    _draws_against_oracle(sg, case, "nopend")


@pytest.mark.parametrize("case", AUTO, ids=_ids(AUTO))
def test_unpinned_against_oracle(sg, case, monkeypatch):
    """(c) The dispatcher's own choice, the HIP Agent follows the oracle (nothing cached): at 36 and 72 hallucinated slots with
    m T = 36 it is joint_kernel(HEAD) + joint_tail_mfma behind the real kernel's k = 0."""
    monkeypatch.setenv("GPMPC_JOINT_PENDING", "1")
    _draws_against_oracle(sg, case, "auto")
    assert all(s.startswith("joint_kernel(HEAD,") and s.endswith(" joint_tail_mfma()") for s in case.steps_auto[1:])


@pytest.mark.parametrize("case", EIGH, ids=_ids(EIGH))
def test_eigh_root_behind_the_real_kernel(sg, case):
    """(e) The car's shipped jitter of 1e-20 on 63 real slots: joint_real_mfma<., 4>(TEST), every Cholesky retry fails, the eigh root for
    the whole batch.  The assertions of test_joint_draw_eigh_fallback_distribution - eigenvector signs are solver specific, so parity
    is asserted on what is well defined: mean, variance, the clip band - plus the covariance bound."""
    lib = sg._lib.load()
    agent, oagent, p = jv.make_pair(sg, case)
    (x_h, u_h), = jv.draw_points(case, p)
    agent.train_hallucinated_dynGP(0)
    oagent.train_hallucinated_dynGP(0)
    _check_layout(case, agent)
    lib.gpmpc_joint_pin_path(sg._lib.JOINT_MFMA)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            y = agent.sample_gp(agent.env_model.get_g_xu_hat(agent.get_batch_x_hat_u_diff(x_h, u_h)).contiguous(),
                                base_samples=agent.epistimic_random_vector[0][0])
            st = joint_call_state(sg, agent)
    finally:
        lib.gpmpc_joint_pin_path(sg._lib.JOINT_AUTO)
    print(f"{case.name}: {st['plan']}")
    assert st["plan"].split("|")[1].strip() == case.steps[0] and st["path"] == sg._lib.JOINT_MFMA
    oagent.sample_gp(oagent.env_model.get_g_xu_hat(oagent.get_batch_x_hat_u_diff(x_h, u_h)), base_samples=oagent.epistimic_random_vector[0][0])
    post, opost = agent.model_i_call, oagent.model_i_call
    assert opost.root_info.used_eigh, "oracle expected to take the eigh branch at jitter 1e-20"
    bits = int(post.last_info.max().item())
    assert bits & sg._lib.INFO_ROOT_FAIL and bits & sg._lib.INFO_ROOT_EIGH
    np.testing.assert_allclose(post.mean.cpu().numpy(), opost.mean.numpy(), rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(post.variance.cpu().numpy(), opost.variance.numpy(), rtol=1e-4, atol=1e-12)
    assert torch.isfinite(y).all()
    mean, var = opost.mean.numpy(), opost.variance.numpy()
    band = p["agent"]["Dyn_gp_beta"] * np.sqrt(var)
    assert (np.abs(y.cpu().numpy() - mean) <= band * (1 + 1e-6) + 1e-12).all()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        S = post.covariance_matrix.cpu().numpy()
    So = opost.covariance_matrix.numpy()
    err, scale = float(np.abs(S - So).max()), float(np.abs(So).max())
    print(f"{case.name}: |Sigma - Sigma_o| {err / scale:.2e} max|Sigma_o| ({scale:.2e})")
    assert err < 1e-7 * scale
