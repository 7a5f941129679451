"""The contraction-rate check over all Jacobian pairs against what a user would write without it, and a whole terminal-set fit.

    python tools/bench_contraction.py [--out profiles/contraction_bench.md] [--only pendulum|car] [--no-torch] [--no-host] [--no-fit]

Part 1, per size (pendulum nx 2 nu 1, car nx 4 nu 2; N = 2^20 and 2^23 packed pairs, entries 0.9 I + 0.05 randn / 0.3 randn drawn on
the device from a seed; C = 1 and 8 candidates with kappa(P) = 30; with and without the (C, N) rates output): ``contraction_rates`` -
(a) HIP events around ``reps`` back-to-back calls after ``warm`` warm-up calls, best and median of ``rounds`` rounds, the prepare,
main and finish kernels together.  Bytes: the pairs read once, ``N nx (nx + nu) 8``, over the best time, as a fraction of the
6.29 TB/s a streaming copy reaches on this device (the figure of DESIGN.md section 5); the rates output, where asked for, adds
``C N 8`` bytes of writes that the fraction does not count.  (b) the same arithmetic in batched torch ops on the device -
``torch.linalg.matrix_norm(L^T (A + B K) L^-T, 2)`` on ``(N, n, n)`` -, C = 1, N = 2^20, by the same discipline with fewer calls;
(c) ``.cpu()`` plus the same expression in numpy, C = 1, N = 2^20, one pass.  (b) and (c) are compared with (a) before anything is timed.
Part 2: ``fit_terminal_set`` on a pendulum-like family of 2^20 pairs drawn on the device (wall time of the best of three fits, and
its split into the device checks - host waits included - and the host solves).  No ratio is promised: the table states whatever
comes out.
"""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np                                                           # noqa: E402
import torch                                                                 # noqa: E402

from sampling_gpmpc_amd import _lib                                          # noqa: E402
from sampling_gpmpc_amd.terminal_set import contraction_rates, fit_terminal_set   # noqa: E402

F64 = torch.float64
DIMS = {"pendulum": (2, 1), "car": (4, 2)}
HBM_COPY_TBS = 6.29


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


def pairs(nx, nu, N, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(1000 * nx + seed)
    A = 0.9 * torch.eye(nx, dtype=F64, device=dev) + 0.05 * torch.randn(N, nx, nx, dtype=F64, device=dev, generator=g)
    B = 0.3 * torch.randn(N, nx, nu, dtype=F64, device=dev, generator=g)
    return A, B


def candidates(nx, nu, C, dev):
    rng = np.random.default_rng(nx + 10 * C)
    P, K = [], []
    for _ in range(C):
        Q, _ = np.linalg.qr(rng.normal(size=(nx, nx)))
        P.append((Q * np.logspace(0.0, np.log10(30.0), nx)) @ Q.T)
        K.append(0.2 * rng.normal(size=(nu, nx)))
    P = np.stack(P)
    return torch.as_tensor(0.5 * (P + P.transpose(0, 2, 1))).to(dev), torch.as_tensor(np.stack(K)).to(dev), torch.full((C,), 1.0, dtype=F64, device=dev)


def plain_rates(A, B, P, K, xp):
    """One candidate's rates from array operations (torch on the device, or numpy on the host)."""
    if xp is torch:
        L = torch.linalg.cholesky(P)
        G = L.T @ (A + B @ K) @ torch.linalg.inv(L).T
        return torch.linalg.matrix_norm(G, 2)
    L = np.linalg.cholesky(P)
    G = L.T @ (A + B @ K) @ np.linalg.inv(L).T
    return np.linalg.norm(G, 2, axis=(1, 2))


def run_size(name, logN, a, dev):
    nx, nu = DIMS[name]
    N = 1 << logN
    A, B = pairs(nx, nu, N, dev)
    rows = []
    for C in (1, 8):
        P, K, rho = candidates(nx, nu, C, dev)
        for want in (False, True):
            state = {}

            def ours():
                state["q"] = contraction_rates(A, B, P, K, rho, rates=want)
            ours()
            row = {"name": name, "N": N, "C": C, "rates": want, "nx": nx, "nu": nu}
            cmp_here = C == 1 and want and logN <= 20
            if cmp_here and not a.no_torch:
                t = plain_rates(A, B, P[0], K[0], torch)
                row["torch_diff"] = float(((t - state["q"].rates[0]).abs() / t).max())
            row["ours"] = device_ms(ours, a.warm, a.reps, a.rounds)
            row["frac"] = N * nx * (nx + nu) * 8 / (row["ours"][0] * 1e-3) / (HBM_COPY_TBS * 1e12)
            row["max_rate"] = float(state["q"].max_rate[0])
            if cmp_here and not a.no_torch:
                row["torch"] = device_ms(lambda: plain_rates(A, B, P[0], K[0], torch), 1, 2, 3)
            if cmp_here and not a.no_host:
                t0 = time.perf_counter()
                Ah, Bh = A.cpu().numpy(), B.cpu().numpy()
                t1 = time.perf_counter()
                h = plain_rates(Ah, Bh, P[0].cpu().numpy(), K[0].cpu().numpy(), np)
                t2 = time.perf_counter()
                row["host"] = ((t1 - t0) * 1e3, (t2 - t1) * 1e3)
                row["host_diff"] = float(np.max(np.abs(h - state["q"].rates[0].cpu().numpy()) / h))
            rows.append(row)
            print(row, flush=True)
    return rows


def pendulum_family(N, dev, seed=0):
    """The pendulum-like family of the tests (Euler pendulum about the upright position, perturbed entries), drawn on the device."""
    g = torch.Generator(device=dev).manual_seed(seed)
    dt, l, grav = 0.015, 10.0, 9.81
    th = np.pi + (torch.rand(N, dtype=F64, device=dev, generator=g) - 0.5)
    A = torch.zeros(N, 2, 2, dtype=F64, device=dev)
    A[:, 0, 0] = A[:, 1, 1] = 1.0
    A[:, 0, 1] = dt
    A[:, 1, 0] = -grav * torch.cos(th) * dt / l + 1e-3 * torch.randn(N, dtype=F64, device=dev, generator=g)
    B = torch.zeros(N, 2, 1, dtype=F64, device=dev)
    B[:, 1, 0] = dt * (1.0 + 0.02 * torch.randn(N, dtype=F64, device=dev, generator=g))
    return A, B


def lqr(A, B, Q):
    P = Q.copy()
    for _ in range(20000):
        Pn = Q + A.T @ P @ A - A.T @ P @ B @ np.linalg.solve(np.eye(B.shape[1]) + B.T @ P @ B, B.T @ P @ A)
        done = np.max(np.abs(Pn - P)) <= 1e-13 * np.max(np.abs(Pn))
        P = Pn
        if done:
            break
    return P, -np.linalg.solve(np.eye(B.shape[1]) + B.T @ P @ B, B.T @ P @ A)


def run_fit(dev, logN=20):
    N = 1 << logN
    A, B = pendulum_family(N, dev)
    P0, K0 = lqr(A.mean(0).cpu().numpy(), B.mean(0).cpu().numpy(), np.diag([100.0, 10.0]))
    rows_x = [(np.array([1.0, 0.0]), 0.5), (np.array([0.0, 1.0]), 2.1)]
    rows_u = [(np.array([1.0]), 5.0)]
    best = None
    for it in range(4):                                                        # the first is the warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ts = fit_terminal_set(A, B, 0.995, rows_x, rows_u, P0, K0)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        if it > 0 and (best is None or wall < best["wall"]):
            best = dict(wall=wall, check=ts.timings["check"] * 1e3, solve=ts.timings["solve"] * 1e3, rounds=ts.rounds, ws=len(ts.working_set),
                        newton=ts.newton_steps, max_rate=ts.max_rate, gap=ts.gap_bound, N=N)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-fit", action="store_true")
    ap.add_argument("--logn", type=int, nargs="+", default=[20, 23])
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    dev = _lib.require_hip_device("cuda")
    rows = []
    for n in DIMS:
        if a.only in (None, n):
            for logN in a.logn:
                rows += run_size(n, logN, a, dev)
    lines = [f"Device: {_lib.device_info(0)[0]}; HIP events around {a.reps} back-to-back calls after {a.warm} warm-up calls, best (median) of "
             f"{a.rounds} rounds; torch path: 2 calls per round after 1, 3 rounds; host path: one pass, same process.  Synthetic pairs.  "
             f"Fractions are of {HBM_COPY_TBS} TB/s, the pairs read once (N nx (nx + nu) 8 bytes); the rates output is not counted.", "",
             "| family | nx | nu | N | C | rates | (a) contraction_rates ms | pair bytes / time | (b) torch ops on the device ms | (b)/(a) | "
             "(c) host: copy + numpy ms | (c)/(a) | max rel diff (b), (c) to (a) |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        fa = r["ours"]
        tb, rb = (f"{r['torch'][0]:.2f} ({r['torch'][1]:.2f})", f"{r['torch'][0] / fa[0]:.0f}x") if "torch" in r else ("-", "-")
        hb, rc = (f"{r['host'][0]:.1f} + {r['host'][1]:.0f}", f"{sum(r['host']) / fa[0]:.0f}x") if "host" in r else ("-", "-")
        diff = ", ".join(f"{r[k]:.1e}" for k in ("torch_diff", "host_diff") if k in r) or "-"
        lines.append(f"| {r['name']} | {r['nx']} | {r['nu']} | 2^{int(np.log2(r['N']))} | {r['C']} | {'yes' if r['rates'] else 'no'} | "
                     f"{fa[0]:.4f} ({fa[1]:.4f}) | {100 * r['frac']:.1f} % | {tb} | {rb} | {hb} | {rc} | {diff} |")
    if not a.no_fit:
        f = run_fit(dev)
        print(f, flush=True)
        lines += ["", f"Whole `fit_terminal_set` (pendulum-like family, N = 2^{int(np.log2(f['N']))} pairs on the device, rho 0.995, gap 1e-4, best of three "
                  "after one warm-up fit):", "", "| wall ms | device checks ms (host waits included) | host solves ms | rounds | working set | Newton steps | "
                  "max rate over all pairs | gap bound |", "|---|---|---|---|---|---|---|---|",
                  f"| {f['wall']:.1f} | {f['check']:.1f} | {f['solve']:.1f} | {f['rounds']} | {f['ws']} | {f['newton']} | {f['max_rate']:.8f} | {f['gap']:.2e} |"]
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write("# The contraction-rate check against torch ops and the host path; a whole terminal-set fit (tools/bench_contraction.py)\n\n" + text + "\n")


if __name__ == "__main__":
    main()
