"""Device convex hulls of a tube against the host path they replace, on the three rollout workloads.

    python tools/bench_hull.py [--out profiles/hull_bench.md] [--only NAME] [--no-host]

Per workload: (a) the device hull time of gpmpc_convex_hulls on the tube as the rollout left it (HIP events around `reps`
back-to-back calls after `warm` warm-up calls, best and median of `rounds` rounds), (b) the rollout's own time in the same
process and by the same discipline, (c) the host path timed in the same run: X_traj.cpu() plus scipy.spatial.ConvexHull per
step (reference benchmarking/generate_convex_hull.py:88-100), degenerate steps - which Qhull refuses - skipped.
The one hard condition is (a) < (c) at every size, taken the unfavourable way round: the MEDIAN device time against the BEST
host pass.  The script exits non-zero when it does not hold; with --only or --no-host the condition is not (fully) evaluated
and the script says so.
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


def host_path(X_dev, dims):
    from scipy.spatial import ConvexHull
    from scipy.spatial import QhullError
    t0 = time.perf_counter()
    X = X_dev.cpu().numpy()
    t1 = time.perf_counter()
    hulls, skipped = [], 0
    for i in range(X.shape[2]):
        try:
            h = ConvexHull(X[:, list(dims), i])
            hulls.append(h.points[h.vertices])
        except QhullError:
            hulls.append(None)
            skipped += 1
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, hulls, skipped


def run(name, no_host, warm, reps, rounds):
    pname, Ns, H, nograd = WORKLOADS[name]
    p = fs_params(pname, Ns, H, nograd=nograd)
    p["common"]["use_cuda"] = True
    p["agent"]["base_sample_generator"] = "counter"
    agent = sg.Agent(p, sg.make_env(p))
    erv = agent.epistimic_random_vector
    per = Ns * agent.g_ny * (1 if nograd else 3)
    runner = RolloutRunner(agent, synthetic_u_ff(agent.nu, H), erv.reshape(-1)[per:], erv.shape[1] * per, H,
                           _lib.MODE_INDEPENDENT if nograd else _lib.MODE_RECONDITIONED, nograd)
    runner.launch()
    torch.cuda.synchronize()
    X = runner.X_traj
    roll = device_ms(runner.launch, warm, reps, rounds)
    state = {}

    def hull():
        state["h"] = sg.convex_hulls(X, dims=(0, 1))
    dev = device_ms(hull, warm, reps, rounds)
    h = state["h"]
    h.raise_on_overflow()
    n_v = h.n_verts.cpu().numpy()
    row = {"name": name, "Ns": Ns, "H": H, "hull_ms": dev, "rollout_ms": roll, "n_v_max": int(n_v.max()),
           "ws_MB": _lib.load().gpmpc_hull_workspace_bytes(Ns, H + 1, 256) / 1e6}
    if not no_host:
        best = None
        for _ in range(2):                                          # the second pass runs on warm caches
            c = host_path(X, (0, 1))
            best = c if best is None or c[0] + c[1] < best[0] + best[1] else best
        copy_ms, qhull_ms, hulls, skipped = best
        lst = h.to_list(skip_first=False)
        agree = sum(1 for a, b in zip(lst, hulls) if b is not None and {tuple(r) for r in a} == {tuple(r) for r in b})
        row.update(copy_ms=copy_ms, qhull_ms=qhull_ms, skipped=skipped, agree=agree, steps=H + 1)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    rows = [run(n, a.no_host, a.warm, a.reps, a.rounds) for n in WORKLOADS if a.only in (None, n)]
    lines = [f"Device: {_lib.device_info(0)[0]}; HIP events around {a.reps} back-to-back calls after {a.warm} warm-up calls, "
             f"best (median) of {a.rounds} rounds; host path: best of 2 passes, same process.  Ratios use the best device time; "
             f"the condition (a) < (c) is checked with the median device time.", "",
             "| workload | Ns | H | (a) device hulls ms | (b) rollout ms | (a)/(b) | (c) host: copy + Qhull ms | (c)/(a) | "
             "max vertices | Qhull-refused steps | steps with equal vertex sets | workspace MB |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    ok = True
    for r in rows:
        a_ms, b_ms = r["hull_ms"], r["rollout_ms"]
        if "copy_ms" in r:
            c = r["copy_ms"] + r["qhull_ms"]
            host = f"{r['copy_ms']:.2f} + {r['qhull_ms']:.1f} = {c:.1f}"
            ratio = f"{c / a_ms[0]:.0f}x"
            extra = f"{r['skipped']} | {r['agree']} of {r['steps'] - r['skipped']}"
            ok = ok and a_ms[1] < c
        else:
            host, ratio, extra = "-", "-", "- | -"
        lines.append(f"| {r['name']} | {r['Ns']} | {r['H']} | {a_ms[0]:.3f} ({a_ms[1]:.3f}) | {b_ms[0]:.3f} ({b_ms[1]:.3f}) | "
                     f"{a_ms[0] / b_ms[0]:.2f} | {host} | {ratio} | {r['n_v_max']} | {extra} | {r['ws_MB']:.1f} |")
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# Device convex hulls against the host path (tools/bench_hull.py)\n\n" + text + "\n")
    if a.only or a.no_host:
        print("condition (a) < (c) at all three sizes NOT evaluated in this run (--only / --no-host)", flush=True)
    if not ok:
        sys.exit("device hulls are not faster than the host path at every size")


if __name__ == "__main__":
    main()
