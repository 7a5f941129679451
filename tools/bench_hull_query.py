"""Device hull queries of a tube against what a user would write without them, on the three rollout workloads.

    python tools/bench_hull_query.py [--out profiles/hull_query_bench.md] [--only NAME] [--no-host] [--no-torch]

Per workload the hulls come from one rollout's tube and a second rollout with another base-sample seed is the query tube.
Timed, all in one process: (a) hull_query with every output, (a') hull_query with the reductions only (margins=False) - HIP
events around `reps` back-to-back calls after `warm` warm-up calls, best and median of `rounds` rounds; (b) the same quantities
from torch ops on the device, chunked over the points so that no temporary exceeds 256 MB (under 1 GB in all), by the same
discipline; (c) X.cpu() plus the same expression in vectorised numpy on the host, best of the passes.
The one hard condition is relative: the MEDIAN of (a) below the BEST of (b) and the BEST of (c) at every size.  The script
exits non-zero when it does not hold; with --only, --no-host or --no-torch it is not (fully) evaluated and the script says so.
Bytes: the two state dimensions of the query tube that are read (and the margin matrix that (a) writes), over the best time,
as a fraction of the 6.29 TB/s a streaming copy reaches on this device.
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import sampling_gpmpc_amd as sg
from sampling_gpmpc_amd import _lib
from sampling_gpmpc_amd.rollout import RolloutRunner
from sampling_gpmpc_amd.workloads import fs_params, synthetic_u_ff

WORKLOADS = {
    "pendulum1D": ("params_pendulum1D_samples", 1024, 30, False),
    "car": ("params_car_residual", 4096, 40, False),
    "car_fs": ("params_car_residual_fs", 262144, 40, True),
}
HBM_COPY_TBS = 6.29
TOL = 1e-9


def device_ms(fn, warm, reps, rounds):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return min(out), statistics.median(out)


def rollout_tube(name, seed):
    pname, Ns, H, nograd = WORKLOADS[name]
    p = fs_params(pname, Ns, H, nograd=nograd)
    p["common"]["use_cuda"] = True
    p["agent"]["base_sample_generator"] = "counter"
    p["agent"]["base_sample_seed"] = seed
    agent = sg.Agent(p, sg.make_env(p))
    erv = agent.epistimic_random_vector
    per = Ns * agent.g_ny * (1 if nograd else 3)
    runner = RolloutRunner(agent, synthetic_u_ff(agent.nu, H), erv.reshape(-1)[per:], erv.shape[1] * per, H,
                           _lib.MODE_INDEPENDENT if nograd else _lib.MODE_RECONDITIONED, nograd)
    runner.launch()
    torch.cuda.synchronize()
    return runner.X_traj.clone()


def edges_of(verts, n_verts, xp):
    """Start vertex, edge vector, 1 / |e|^2 and validity of every edge slot, (S, V) each; xp is torch or numpy."""
    S, V = verts.shape[0], verts.shape[1]
    j = xp.arange(V)[None, :] if xp is np else torch.arange(V, device=verts.device)[None, :]
    n = n_verts[:, None]
    valid = j < n
    nxt = (j + 1) % (xp.maximum(n, 1) if xp is np else n.clamp(min=1))
    nxt = xp.where(valid, nxt, 0 * nxt)
    a = xp.where(valid[..., None], verts, 0.0 * verts) if xp is np else torch.where(valid[..., None], verts, torch.zeros_like(verts))
    if xp is np:
        b = np.take_along_axis(a, np.broadcast_to(nxt[..., None], a.shape), axis=1)
    else:
        b = torch.gather(a, 1, nxt[..., None].expand(-1, -1, 2))
    e = b - a
    len2 = e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]
    if xp is np:
        inv = np.where(len2 > 0, 1.0 / np.where(len2 > 0, len2, 1.0), 0.0)
    else:
        inv = torch.where(len2 > 0, 1.0 / torch.where(len2 > 0, len2, torch.ones_like(len2)), torch.zeros_like(len2))
    return a, e, inv, valid


def plain_query(verts, n_verts, X, dims, tol, chunk, xp):
    """The quantities of hull_query from array operations (torch on the device, or numpy on the host)."""
    a, e, inv, valid = edges_of(verts, n_verts, xp)
    ax, ay, ex, ey = a[None, ..., 0], a[None, ..., 1], e[None, ..., 0], e[None, ..., 1]
    Nq, S = X.shape[0], X.shape[2]
    inf = float("inf")
    margin = xp.empty((Nq, S), dtype=X.dtype) if xp is np else torch.empty(Nq, S, dtype=X.dtype, device=X.device)
    three = (n_verts >= 3)[None, :]
    for i0 in range(0, Nq, chunk):
        px, py = X[i0:i0 + chunk, dims[0], :], X[i0:i0 + chunk, dims[1], :]
        dx, dy = px[..., None] - ax, py[..., None] - ay
        o = ex * dy - ey * dx
        t = ((dx * ex + dy * ey) * inv[None]).clip(0.0, 1.0)
        cx, cy = dx - t * ex, dy - t * ey
        d2 = cx * cx + cy * cy
        if xp is np:
            d2 = np.where(valid[None], d2, inf)
            inside = (np.where(valid[None], o, inf) >= 0).all(axis=2) & three
            dist = np.sqrt(d2.min(axis=2))
            m = np.where(inside, dist, -dist)
            m = np.where(np.isfinite(px) & np.isfinite(py), m, np.nan)
        else:
            d2 = torch.where(valid[None], d2, torch.full_like(d2, inf))
            inside = (torch.where(valid[None], o, torch.full_like(o, inf)) >= 0).all(dim=2) & three
            dist = torch.sqrt(d2.min(dim=2).values)
            m = torch.where(inside, dist, -dist)
            m = torch.where(torch.isfinite(px) & torch.isfinite(py), m, torch.full_like(m, float("nan")))
        margin[i0:i0 + chunk] = m
    if xp is np:
        nf = ~np.isnan(margin)
        filled = np.where(nf, margin, inf)
        outside = margin < -tol
        return dict(margin=margin, n_inside=(margin >= -tol).sum(axis=0), n_finite=nf.sum(axis=0), min_margin=filled.min(axis=0),
                    argmin=filled.argmin(axis=0), worst=filled.min(axis=1),
                    first_out=np.where(outside.any(axis=1), outside.argmax(axis=1), -1))
    nf = ~torch.isnan(margin)
    filled = torch.where(nf, margin, torch.full_like(margin, inf))
    mn = filled.min(dim=0)
    outside = margin < -tol
    return dict(margin=margin, n_inside=(margin >= -tol).sum(dim=0), n_finite=nf.sum(dim=0), min_margin=mn.values, argmin=mn.indices,
                worst=filled.min(dim=1).values,
                first_out=torch.where(outside.any(dim=1), outside.to(torch.int8).argmax(dim=1), torch.full_like(outside[:, 0], -1, dtype=torch.int64)))


def run(name, a):
    pname, Ns, H, nograd = WORKLOADS[name]
    X_hull, X = rollout_tube(name, 77), rollout_tube(name, 78)
    h = sg.convex_hulls(X_hull, dims=(0, 1))
    h.raise_on_overflow()
    n_max = int(h.n_verts.max())
    verts, n_verts = h.verts[:, :n_max].contiguous(), h.n_verts.to(torch.int64)     # the torch path is given the trimmed buffer
    state = {}

    def full():
        state["q"] = sg.hull_query(h, X, tol=TOL)

    def lean():
        state["l"] = sg.hull_query(h, X, tol=TOL, margins=False)
    t_full, t_lean = device_ms(full, a.warm, a.reps, a.rounds), device_ms(lean, a.warm, a.reps, a.rounds)
    q = state["q"]
    read_b, write_b = 2 * Ns * (H + 1) * 8, Ns * (H + 1) * 8
    row = {"name": name, "Ns": Ns, "H": H, "full": t_full, "lean": t_lean, "n_v_max": n_max,
           "full_frac": (read_b + write_b) / (t_full[0] * 1e-3) / (HBM_COPY_TBS * 1e12),
           "lean_frac": read_b / (t_lean[0] * 1e-3) / (HBM_COPY_TBS * 1e12),
           "inside": float(q.n_inside.sum()) / max(float(q.n_finite.sum()), 1.0)}
    chunk = max(1, int(256e6 // (8 * (H + 1) * n_max)))
    if not a.no_torch:
        def plain():
            state["t"] = plain_query(verts, n_verts, X, (0, 1), TOL, chunk, torch)
        row["torch"] = device_ms(plain, 2, max(1, a.reps // 4), a.rounds)
        t = state["t"]
        row["agree"] = (bool((t["n_inside"] == q.n_inside).all()) and bool((t["argmin"] == q.argmin).all())
                        and bool((t["first_out"] == q.first_out).all()))
        row["max_diff"] = float((t["margin"] - q.margin).abs().max())
    if not a.no_host:
        vh, nh = verts.cpu().numpy(), n_verts.cpu().numpy()
        best = None
        for _ in range(1 if Ns > 100000 else 2):
            t0 = time.perf_counter()
            Xh = X.cpu().numpy()
            t1 = time.perf_counter()
            plain_query(vh, nh, Xh, (0, 1), TOL, max(1, chunk // 8), np)
            t2 = time.perf_counter()
            c = ((t1 - t0) * 1e3, (t2 - t1) * 1e3)
            best = c if best is None or sum(c) < sum(best) else best
        row["host"] = best
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    rows = []
    for n in WORKLOADS:
        if a.only in (None, n):
            rows.append(run(n, a))
            print(rows[-1], flush=True)
    lines = [f"Device: {_lib.device_info(0)[0]}; HIP events around {a.reps} back-to-back calls after {a.warm} warm-up calls, best "
             f"(median) of {a.rounds} rounds; torch path: {max(1, a.reps // 4)} calls per round after 2; host path: best pass, same "
             f"process.  Query tube: a second rollout with another base-sample seed.  The condition is checked with the median of "
             f"(a) against the best of (b) and of (c).  Fractions are of {HBM_COPY_TBS} TB/s.", "",
             "| workload | Ns | H | (a) all outputs ms | bytes / time of (a) | (a') reductions only ms | bytes / time of (a') | "
             "(b) torch ops on the device ms | (b)/(a) | (c) host: copy + numpy ms | (c)/(a) | max vertices | inside fraction | "
             "(b) agrees |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    ok = True
    for r in rows:
        fa, fl = r["full"], r["lean"]
        if "torch" in r:
            tb = f"{r['torch'][0]:.3f} ({r['torch'][1]:.3f})"
            rb = f"{r['torch'][0] / fa[0]:.0f}x"
            agree = f"{'yes' if r['agree'] else 'NO'}, max margin diff {r['max_diff']:.1e}"
            ok = ok and fa[1] < r["torch"][0]
        else:
            tb, rb, agree = "-", "-", "-"
        if "host" in r:
            c = sum(r["host"])
            hb, rc = f"{r['host'][0]:.2f} + {r['host'][1]:.1f} = {c:.1f}", f"{c / fa[0]:.0f}x"
            ok = ok and fa[1] < c
        else:
            hb, rc = "-", "-"
        lines.append(f"| {r['name']} | {r['Ns']} | {r['H']} | {fa[0]:.4f} ({fa[1]:.4f}) | {100 * r['full_frac']:.1f} % | "
                     f"{fl[0]:.4f} ({fl[1]:.4f}) | {100 * r['lean_frac']:.1f} % | {tb} | {rb} | {hb} | {rc} | {r['n_v_max']} | "
                     f"{r['inside']:.3f} | {agree} |")
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# Device hull queries against torch ops and the host path (tools/bench_hull_query.py)\n\n" + text + "\n")
    if a.only or a.no_host or a.no_torch:
        print("condition (a) < (b), (a) < (c) at all three sizes NOT evaluated in this run (--only / --no-host / --no-torch)", flush=True)
    if not ok:
        sys.exit("hull_query is not faster than the torch path and the host path at every size")


if __name__ == "__main__":
    main()
