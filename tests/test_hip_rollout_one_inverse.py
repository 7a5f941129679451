"""rollout_one_kernel computes the inverse of group K's diagonal tiles (P.gd[K]) inside the NEXT step's one_solve<K> from epoch
K = 3 on, and inline only in epoch 2, in the last step of an epoch and for the wrap block (csrc/rollout_one.hip, section (vi)).
An inverse that was left pending, or computed from the wrong group's state, shows in the output of the last step of a launch
that ends there: the launches below end on the step before, at and after every epoch change (the epochs start at t = 4, 10,
15, 20 and 26), inside epoch 2 and on the last appending step.

(a) against rollout_fast_kernel - an independent implementation of the same arithmetic - on the same base samples, both kernels
    pinned and the path of each launch asserted; tolerances: those of tests/test_rollout_one_append_steps.py for this pair
    (X: rtol 1e-9 / atol 1e-11, Y: rtol 1e-7 / atol 1e-11).
(b) bit for bit against tests/golden/rollout_one_parent_xtraj.npz: X_traj of the commit before the inverse moved, for the same
    seeded inputs (tests/golden/make_rollout_one_parent_xtraj.py wrote it and builds the inputs of this file).
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

X_TOL = dict(rtol=1e-9, atol=1e-11)
Y_TOL = dict(rtol=1e-7, atol=1e-11)
HS = [2, 5, 6, 10, 11, 12, 15, 16, 17, 20, 21, 22, 26, 27, 28, 29, 30]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _maker():
    spec = importlib.util.spec_from_file_location("make_rollout_one_parent_xtraj", os.path.join(GOLDEN, "make_rollout_one_parent_xtraj.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    import sampling_gpmpc_amd as sg
    from sampling_gpmpc_amd import _lib
    _lib.load()
    mk = _maker()
    assert mk.NS == 8
    return mk, _lib, {fb: mk.inputs(sg, fb) for fb in (True, False)}


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, "rollout_one_parent_xtraj.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("feedback", [True, False])
@pytest.mark.parametrize("H", HS)
def test_launch_ending_around_every_epoch_change_against_fast(ctx, H, feedback):
    """LEAN instantiation (X_traj) and the instantiation with the optional outputs (X_traj and Y)"""
    mk, _lib, cases = ctx
    for outputs in (False, True):
        X1, Y1, i1 = mk.launch(cases[feedback], H, feedback, _lib.KERNEL_ONE, outputs)
        Xf, Yf, i_f = mk.launch(cases[feedback], H, feedback, _lib.KERNEL_FAST, outputs)
        msg = f"H={H} feedback={feedback} outputs={outputs}: max abs diff X {np.abs(X1 - Xf).max():.3e}"
        if outputs:
            msg += f" Y {np.abs(Y1 - Yf).max():.3e}"
        print(msg)
        assert np.isfinite(X1).all()
        np.testing.assert_allclose(X1, Xf, **X_TOL)
        if outputs:
            np.testing.assert_allclose(Y1, Yf, **Y_TOL)
        np.testing.assert_array_equal(i1 & ~_lib.INFO_VAR_CLAMPED, i_f & ~_lib.INFO_VAR_CLAMPED)


@pytest.mark.parametrize("feedback", [True, False])
@pytest.mark.parametrize("H", [12, 17, 30])
def test_x_traj_has_the_parents_bits(ctx, golden, H, feedback):
    mk, _lib, cases = ctx
    assert tuple(mk.GOLDEN_H) == (12, 17, 30)
    X, _, _ = mk.launch(cases[feedback], H, feedback, _lib.KERNEL_ONE)
    ref = golden[mk.key(H, feedback)]
    print(f"H={H} feedback={feedback}: max abs diff to the parent's X_traj {np.abs(X - ref).max():.3e}")
    assert X.shape == ref.shape and np.array_equal(X, ref)
