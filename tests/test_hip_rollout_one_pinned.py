"""rollout_one_kernel's prologue issues its loads with addresses that are valid in every lane (the lanes behind the horizon read
step 0 and are zeroed afterwards) and uses them behind one_init; the step blocks select the diagonal-tile state (ud / drow / dcol
of group K, ud1 / drow1 / dcol1 of group K + 1) by the step index and an epoch change hands group K + 1's triple over
(csrc/rollout_one.hip).  A base sample or input taken from the wrong lane, a select under the wrong mask or a hand-over that
misses a step shows in the last step of a launch that ends there.  H = 5 / 6 end just before and just after the first epoch change
(t = 4), H = 7 is the first launch that runs a full step of epoch 3, H = 11, 16, 21, 27 run the first step after the changes at
t = 10, 15, 20, 26; together they hit a step that wraps into the next group and a step that reaches into the next tile row in
every epoch; H = 2 leaves 62 lanes behind the horizon.

(a) against rollout_fast_kernel - an independent implementation of the same arithmetic - on the same base samples, both kernels
    pinned and the path of each launch asserted, both instantiations (LEAN, and the one with the optional outputs); tolerances:
    those of tests/test_hip_rollout_one_inverse.py (X: rtol 1e-9 / atol 1e-11, Y: rtol 1e-7 / atol 1e-11).
(b) bit for bit against tests/golden/rollout_one_parent_xtraj.npz for H = 30 (the inputs are those of
    tests/golden/make_rollout_one_parent_xtraj.py, Ns = 8).
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

X_TOL = dict(rtol=1e-9, atol=1e-11)
Y_TOL = dict(rtol=1e-7, atol=1e-11)
HS = [2, 5, 6, 7, 11, 16, 21, 27, 30]
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


@pytest.mark.parametrize("outputs", [False, True], ids=["lean", "outputs"])
@pytest.mark.parametrize("feedback", [True, False])
@pytest.mark.parametrize("H", HS)
def test_launch_against_fast(ctx, H, feedback, outputs):
    mk, _lib, cases = ctx
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
def test_x_traj_has_the_parents_bits_at_h30(ctx, feedback):
    mk, _lib, cases = ctx
    with np.load(os.path.join(GOLDEN, "rollout_one_parent_xtraj.npz")) as z:
        ref = z[mk.key(30, feedback)]
    X, _, _ = mk.launch(cases[feedback], 30, feedback, _lib.KERNEL_ONE)
    print(f"H=30 feedback={feedback}: max abs diff to the parent's X_traj {np.abs(X - ref).max():.3e}")
    assert X.shape == ref.shape and np.array_equal(X, ref)
