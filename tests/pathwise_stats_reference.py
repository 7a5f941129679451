"""CPU reference of ``gpmpc_pathwise_tube_stats``, shared by tests/test_pathwise_stats_host.py, tests/test_hip_pathwise_stats.py and
tests/test_distributed_tube_stats.py (not a test module).  The normals come from ``agent.counter_base_samples(..., device="cpu")`` (the
rows ``OFFSET ..`` of the stream), the update vectors, the evaluation and the rollout loop from form A of tests/pathwise_reference.py
(``fit_A``, ``eval_A``, ``rollout_with``), the reductions from numpy.

``RUNS`` names every run of the device test: (case of pathwise_reference, M, Ns, H).  x0 and U are those of the case's first sample,
shared by all samples; the centre is the trajectory of the ``Z = 0`` sample (the posterior-mean function) computed here, and the
scale of ``sup`` is the largest ``|X|`` per state dimension - the normalisation of ``pathwise_reference.deviations`` for the tube, so
that an error of ``sup`` is bounded by the tube's tolerance in its own units."""
import functools

import numpy as np

from tests import pathwise_reference as ref

OFFSET = 1000
RUNS = {
    "pend_fb": ("pend_fb", 128, 67, 5),           # 67 is no multiple of 4 or 64
    "car_fb": ("car_fb", 384, 67, 5),             # three frequencies per lane
    "raw64": ("raw64", 128, 67, 5),               # the N_r limit
    "raw7": ("raw7", 128, 67, 1),                 # fewer rows than lanes
    "car_nofb": ("car_nofb", 1024, 5, 5),         # fewer samples than one default workgroup row
    "car_nofb_h0": ("car_nofb", 1024, 5, 0),      # only stage 0
}
# The row of WORST_AB (tests/test_pathwise_host.py) whose `tube` figure a run is held to.  The table has no ("car_nofb", 1024) row: the
# figure is reference A's own error, which follows the conditioning of K + Sigma and not M (car_nofb 4.2e-10 at M = 128, 5.0e-10 at
# 384; car_fb 4.7e-10, 4.0e-10 and 3.1e-10 at 1024), so the car_nofb runs take the case's row at M = 384, its largest.
TABLE_ROW = {"pend_fb": ("pend_fb", 128), "car_fb": ("car_fb", 384), "raw64": ("raw64", 128), "raw7": ("raw7", 128),
             "car_nofb": ("car_nofb", 384), "car_nofb_h0": ("car_nofb", 384)}


def shared_inputs(run):
    """(case, x0 (nx), U (H, nu)) of a run"""
    name, _, _, H = RUNS[run]
    c = ref.CASES[name]()
    return c, c.x0[0].copy(), c.U[0, :H].copy()


def _rollout(c, omega, Z, x0, U):
    Ns = Z.shape[0]
    if U.shape[0] == 0:
        return np.repeat(x0[None, :, None], Ns, axis=0)
    V = ref.fit_A(c, omega, Z)
    X, _ = ref.rollout_with(c, lambda x: ref.eval_A(c, omega, Z, V, x), np.repeat(x0[None], Ns, 0), np.repeat(U[None], Ns, 0))
    return X


@functools.lru_cache(maxsize=None)
def tube(run):
    """(X (Ns, nx, H+1), centre (nx, H+1), scale (nx)) of a run, computed once per process and shared (treat as read-only)"""
    name, M, Ns, _ = RUNS[run]
    c, x0, U = shared_inputs(run)
    omega, Z = ref.draws(name, M, Ns, OFFSET)
    X = _rollout(c, omega, Z, x0, U)
    centre = _rollout(c, omega, np.zeros_like(Z[:1]), x0, U)[0]
    big = np.abs(X).max(axis=(0, 2))
    return X, centre, np.where(big > 0.0, big, 1.0)                       # (a dimension that stays 0, as with H = 0, is left unscaled)


def stats(X, centre, offset, scale=None, eps=()):
    """numpy statement of the outputs for the tube ``X`` of the global ids ``offset ..``: a dict of dev_max, dev_arg, box_lo, box_hi
    ((H+1, nx)), sup (Ns), n_within (n_eps), n_nonfinite, Ns, offset.  A non-finite state counts as +inf / -inf / +inf."""
    bad = ~np.isfinite(X)
    with np.errstate(invalid="ignore"):
        dev = np.abs(X - centre[None])
    dev[~np.isfinite(dev)] = np.inf
    dev_max = dev.max(0)
    arg = np.empty(dev_max.shape, dtype=np.int64)
    for idx in np.ndindex(*dev_max.shape):
        arg[idx] = offset + int(np.flatnonzero(dev[(slice(None),) + idx] == dev_max[idx])[0])
    sc = np.ones(X.shape[1]) if scale is None else np.asarray(scale, dtype=np.float64)
    sup = (dev / sc[None, :, None]).max(axis=(1, 2))
    return {"Ns": X.shape[0], "offset": offset, "dev_max": dev_max.T.copy(), "dev_arg": arg.T.copy(),
            "box_lo": np.where(bad, -np.inf, X).min(0).T.copy(), "box_hi": np.where(bad, np.inf, X).max(0).T.copy(), "sup": sup,
            "n_within": np.array([int((sup <= e).sum()) for e in eps], dtype=np.int64),
            "n_nonfinite": int(bad.any(axis=(1, 2)).sum())}


def thresholds(sup, tol):
    """(eps, margin): per third of the sorted ``sup`` the midpoint of its widest gap between neighbours, and the smallest of those gaps in
    units of ``tol``.  A count against such a threshold can differ from the reference's only if a value moved by half the gap."""
    srt = np.sort(np.asarray(sup, dtype=np.float64))
    gaps = np.diff(srt)
    eps, worst = [], np.inf
    for part in np.array_split(np.arange(gaps.size), min(3, gaps.size)):
        k = int(part[np.argmax(gaps[part])])
        eps.append(0.5 * (srt[k] + srt[k + 1]))
        worst = min(worst, gaps[k] / tol)
    return tuple(eps), float(worst)
