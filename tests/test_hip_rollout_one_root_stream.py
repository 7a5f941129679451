"""The static steps' ONE root stream and literal-EXEC selects (csrc/rollout_one.hip: one_chol_rest1, one_lane_put) against the epoch
loop of rollout_one_kernel, which keeps the two interleaved root streams and the run-time selects: X_traj and info compared with
np.array_equal.  Every case runs H = 30 - each of the thirty static bodies is code of its own - with Ns = 4 and per-sample start
states, feedback on and off:

  * the shipped beta (no clip in most steps);
  * beta = 0.7: the clip sends steps through the cold block;
  * beta = 0.3: slots 1 and 2 of the draw clip in most steps, so the values handed over from the draw's lane (lane r_t where the
    step's own point lane factors S + noise: steps 2, 4, 12, 20, 28) decide what is appended and with it every later step;
  * one chain whose info carries the bits root_small_fast_retry sets.  At the shipped hyperparameters no FINITE input was found
    that fails the root of S (tried: base samples all zero, 1e-9 and 1e3 times the usual ones, start states on a grid point, all
    equal, at 1e3 - the posterior covariance stays positive definite); a non-finite state does (a NaN S fails every pivot test,
    the three retries fail too: info 0x17).  The case starts one of its four chains at NaN: that chain's X_traj is compared as bit
    patterns, the other three as numbers, info as is.

The helpers (agent, inputs, the pinned launch and the form it took) are those of tests/test_hip_rollout_one_steps.py.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
H = 30
NS = 4


def _steps_module():
    spec = importlib.util.spec_from_file_location("_one_steps_helpers", os.path.join(HERE, "test_hip_rollout_one_steps.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    return _steps_module()._Ctx()


@pytest.fixture(scope="module")
def unclipped(ctx):
    """X_traj of the shipped beta per feedback setting, computed once (the clipped cases must differ from it)"""
    return {}


@pytest.mark.parametrize("feedback", [True, False])
@pytest.mark.parametrize("beta", [None, 0.7, 0.3])
def test_steps_form_has_the_loop_forms_bits(ctx, monkeypatch, unclipped, beta, feedback):
    X, info = ctx.both(monkeypatch, NS, H, feedback, per_sample=True, beta=beta)
    assert X.shape == (NS, 2, H + 1)
    if beta is None:
        unclipped[feedback] = X.copy()
    else:
        if feedback not in unclipped:
            unclipped[feedback], _ = ctx.both(monkeypatch, NS, H, feedback, per_sample=True, beta=None)
        differ = np.any(X != unclipped[feedback], axis=1)          # [Ns, H + 1]: the state of a step differs from the unclipped run
        first = [int(np.argmax(d)) if d.any() else -1 for d in differ]
        print(f"beta={beta} feedback={feedback}: first state that differs from the unclipped run, per chain: {first}")
        assert all(f >= 0 for f in first)                          # the clip acted in every chain


@pytest.mark.parametrize("feedback", [True, False])
def test_root_retry_chain(ctx, monkeypatch, feedback):
    case = ctx.case(NS, feedback)
    agent, z, x0 = case
    x0 = x0.clone()
    x0[2, :] = float("nan")
    Xl, il, pl, fl = ctx.launch(monkeypatch, case, H, feedback, False, x0, None)
    Xs, is_, ps, fs = ctx.launch(monkeypatch, case, H, feedback, True, x0, None)
    assert (pl, fl) == (ctx._lib.KERNEL_ONE, 0) and (ps, fs) == (ctx._lib.KERNEL_ONE, 1)
    print(f"feedback={feedback}: info loop {[hex(int(v)) for v in il]}, steps {[hex(int(v)) for v in is_]}")
    assert (int(il[2]) >> 1) & 7 != 0                              # the retry ran in the chain that started at NaN ...
    assert all((int(il[k]) >> 1) & 7 == 0 for k in (0, 1, 3))      # ... and in no other
    assert np.array_equal(is_, il)
    keep = [0, 1, 3]
    assert np.isfinite(Xl[keep]).all()
    assert np.array_equal(Xs[keep], Xl[keep])
    assert np.array_equal(np.ascontiguousarray(Xs[2]).view(np.uint64), np.ascontiguousarray(Xl[2]).view(np.uint64))
