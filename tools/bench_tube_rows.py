"""The tube row check and the slacked tube QP against what a user would write without them.

    python tools/bench_tube_rows.py [--out profiles/tube_rows_bench.md] [--only NAME] [--no-host]

Part 1, per workload: a synthetic tube (states uniform over 1.2 times the state box, so that every row is violated by some samples;
the terminal states of the pendulum around the goal) is checked with ``check_tube`` against the problem's ``ocp_rows`` - (a) HIP events
around ``reps`` back-to-back calls after ``warm`` warm-up calls, best and median of ``rounds`` rounds; (b) the same counts, minima and
per-sample results from torch operations on the device by the same discipline; (c) X.cpu() plus the same expressions in numpy, best
pass.  The results are compared before anything is timed.  Bytes: the tube read once, over the best time, as a fraction of the
6.29 TB/s a streaming copy reaches on this device.  No ratio is promised: the table states whatever comes out.
Part 2: a whole ``solve_tube_qp`` with and without a soft terminal row per sample, at 70 x 17 and 1024 x 30 (wall time, host waits
included: the solver reads step lengths back every iteration).
"""
import argparse
import os
import statistics
import sys
import time
from types import SimpleNamespace

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np                                                           # noqa: E402
import torch                                                                 # noqa: E402

import sampling_gpmpc_amd as sg                                              # noqa: E402
from sampling_gpmpc_amd import _lib                                          # noqa: E402
from sampling_gpmpc_amd import tube_rows as tr                               # noqa: E402
from sampling_gpmpc_amd.workloads import closed_loop_params                         # noqa: E402
from bench_tube_qp import problem                                            # noqa: E402

F64 = torch.float64
WORKLOADS = {"pendulum1D": ("params_pendulum1D_samples", 1024, 30), "car": ("params_car_residual", 4096, 40),
             "car_fs": ("params_car_residual", 262144, 40)}
ELLIPSES = {"n1": [26, 5.0, 9.0, 1.0, 5.67], "n2": [10, 1.0, 9.0, 1.0, 5.67]}          # two obstacles of the reference's car scene
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


def workload(name, dev):
    pname, Ns, H = WORKLOADS[name]
    p = closed_loop_params(pname, Ns, H)
    if "bicycle" in p["env"]["dynamics"]:
        p["env"]["ellipses"] = ELLIPSES
    te, _ = sg.get_reachable_set_ball(p, np.ones(H + 1))
    agent = SimpleNamespace(params=p, tilde_eps_list=te)
    nx, nu = p["agent"]["dim"]["nx"], p["agent"]["dim"]["nu"]
    g = torch.Generator().manual_seed(Ns + H)
    lo, hi = torch.tensor(p["optimizer"]["x_min"], dtype=F64), torch.tensor(p["optimizer"]["x_max"], dtype=F64)
    X = (lo[None, :, None] + (hi - lo)[None, :, None] * (torch.rand(Ns, nx, H + 1, dtype=F64, generator=g) * 1.2 - 0.1))
    if p["env"]["dynamics"] == "Pendulum1D":
        X[:, :, H] = torch.tensor(p["env"]["goal_state"], dtype=F64) + 0.2 * torch.randn(Ns, nx, dtype=F64, generator=g)
    v = 0.1 * torch.randn(H, nu, dtype=F64, generator=g)
    return tr.ocp_rows(agent, v=v).to(dev), X.to(dev).contiguous()


def plain_check(rows, X, tol, xp):
    """The quantities of check_tube from array operations (torch on the device, or numpy on the host)."""
    x = X.permute(0, 2, 1) if xp is torch else X.transpose(0, 2, 1)            # (Ns, T, nx)
    vals = []
    if rows.E is not None:
        lin = x @ rows.E.T
        vals.append(lin if rows.off is None else lin + rows.off[None])
    if rows.M is not None:
        d = x[:, :, None, :] - rows.c[None, None]
        vals.append(xp.einsum("itqk,qkl,itql->itq", d, rows.M, d))
    val = xp.cat(vals, 2) if xp is torch else np.concatenate(vals, 2)
    inf = float("inf")
    fin = xp.isfinite
    use_lo, use_hi = fin(rows.lo), fin(rows.hi)
    where = xp.where
    full = (lambda a, c: torch.full_like(a, c)) if xp is torch else (lambda a, c: np.full_like(a, c))
    m_lo = where(use_lo[None], val - where(use_lo, rows.lo, full(rows.lo, 0.0))[None], full(val, inf))
    m_hi = where(use_hi[None], where(use_hi, rows.hi, full(rows.hi, 0.0))[None] - val, full(val, inf))
    m = xp.minimum(m_lo, m_hi)
    bad = ~fin(x).all(2) if xp is np else ~fin(x).all(dim=2)
    m = where(bad[:, :, None] | (m != m), full(m, -inf), m)                     # active cells only are read below
    active = (use_lo | use_hi)[None]
    mm = where(active, m, full(m, inf))
    out = active & (m < -tol)
    if xp is torch:
        mn = mm.min(dim=0)
        any_out = out.any(dim=2)
        return dict(n_viol=out.sum(dim=0), min_margin=mn.values, argmin=mn.indices, worst=mm.reshape(mm.shape[0], -1).min(dim=1).values,
                    first_out=torch.where(any_out.any(dim=1), any_out.to(torch.int8).argmax(dim=1), torch.full((mm.shape[0],), -1, device=mm.device)))
    any_out = out.any(axis=2)
    return dict(n_viol=out.sum(axis=0), min_margin=mm.min(axis=0), argmin=mm.argmin(axis=0), worst=mm.reshape(mm.shape[0], -1).min(axis=1),
                first_out=np.where(any_out.any(axis=1), any_out.argmax(axis=1), -1))


def run_check(name, a, dev):
    rows, X = workload(name, dev)
    Ns, nx, T = X.shape
    state = {}

    def ours():
        state["q"] = tr.check_tube(rows, X)

    def plain():
        state["t"] = plain_check(rows, X, 0.0, torch)
    ours()
    row = {"name": name, "Ns": Ns, "H": T - 1, "rows": rows.n_rows}
    if not a.no_torch:
        plain()
        q, t = state["q"], state["t"]
        act = torch.isfinite(rows.lo) | torch.isfinite(rows.hi)
        row["agree"] = (bool((t["n_viol"] == q.n_viol).all()) and bool((t["argmin"][act] == q.argmin[act]).all())
                        and bool((t["first_out"] == q.first_out).all()))
        row["max_diff"] = float((t["min_margin"][act] - q.min_margin[act]).abs().max())
    row["ours"] = device_ms(ours, a.warm, a.reps, a.rounds)
    row["frac"] = Ns * nx * T * 8 / (row["ours"][0] * 1e-3) / (HBM_COPY_TBS * 1e12)
    row["safe"] = state["q"].safe_fraction
    if not a.no_torch:
        row["torch"] = device_ms(plain, 2, max(1, a.reps // 4), a.rounds)
    if not a.no_host:
        host_rows = SimpleNamespace(**{k: (None if getattr(rows, k) is None else getattr(rows, k).cpu().numpy()) for k in ("E", "off", "M", "c", "lo", "hi")})
        best = None
        for _ in range(1 if Ns > 100000 else 2):
            t0 = time.perf_counter()
            Xh = X.cpu().numpy()
            t1 = time.perf_counter()
            plain_check(host_rows, Xh, 0.0, np)
            t2 = time.perf_counter()
            c = ((t1 - t0) * 1e3, (t2 - t1) * 1e3)
            best = c if best is None or sum(c) < sum(best) else best
        row["host"] = best
    return row


def run_solve(Ns, H, dev, reps=3):
    qp, _, _, _ = problem(Ns, H, 2, 1, dev)
    hard = sg.solve_tube_qp(qp)
    # a soft terminal row per sample: the quadric |x_H|_P^2 <= delta^2 linearised at the hard solution's tube, delta^2 at the median value
    P = torch.tensor([[4.0, 1.0], [1.0, 2.0]], dtype=F64, device=dev)
    quad = tr.TubeRows(E=None, off=None, M=P[None], c=torch.zeros(1, 2, dtype=F64, device=dev), lo=torch.full((H + 1, 1), -float("inf"), dtype=F64),
                       hi=torch.full((H + 1, 1), float("inf"), dtype=F64))
    ev = tr.tube_rows(hard.X, quad, values=True, gradients=True, per_row=False, per_sample=False)
    hval, g = ev.val, ev.grad
    shift = torch.einsum("itqk,ikt->itq", g, hard.X) - hval
    hi_s = torch.full_like(hval, float("inf"))
    hi_s[:, H] = hval[:, H].median() + shift[:, H]
    soft_qp = qp.clone()
    soft_qp.Es, soft_qp.lo_s, soft_qp.hi_s = g.contiguous(), torch.full_like(hval, -float("inf")), hi_s
    soft_qp.pen_lo_s, soft_qp.pen_hi_s = torch.zeros(1, 2, dtype=F64, device=dev), torch.full((1, 2), 1e6, dtype=F64, device=dev)
    out = {}
    for label, prob in (("hard", qp), ("soft", soft_qp)):
        res = sg.solve_tube_qp(prob)
        torch.cuda.synchronize()
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            res = sg.solve_tube_qp(prob)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        out[label] = (min(times), res.status, res.iterations)
    paying = int((res.es_hi[:, H, 0] > 1e-6).sum())
    return dict(Ns=Ns, H=H, paying=paying, **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-solve", action="store_true")
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda")
    rows = []
    for n in WORKLOADS:
        if a.only in (None, n):
            rows.append(run_check(n, a, dev))
            print(rows[-1], flush=True)
    lines = [f"Device: {_lib.device_info(0)[0]}; HIP events around {a.reps} back-to-back calls after {a.warm} warm-up calls, best (median) of "
             f"{a.rounds} rounds; torch path: {max(1, a.reps // 4)} calls per round after 2; host path: best pass, same process.  Synthetic "
             f"tubes.  Fractions are of {HBM_COPY_TBS} TB/s, the tube read once.", "",
             "| workload | Ns | H | rows | (a) check_tube ms | tube bytes / time | (b) torch ops on the device ms | (b)/(a) | (c) host: copy + numpy ms | "
             "(c)/(a) | safe fraction | (b) agrees |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        fa = r["ours"]
        tb, rb, agree = ((f"{r['torch'][0]:.3f} ({r['torch'][1]:.3f})", f"{r['torch'][0] / fa[0]:.1f}x",
                          f"{'yes' if r['agree'] else 'NO'}, max margin diff {r['max_diff']:.1e}") if "torch" in r else ("-", "-", "-"))
        hb, rc = ((f"{r['host'][0]:.2f} + {r['host'][1]:.1f}", f"{sum(r['host']) / fa[0]:.0f}x") if "host" in r else ("-", "-"))
        lines.append(f"| {r['name']} | {r['Ns']} | {r['H']} | {r['rows']} | {fa[0]:.4f} ({fa[1]:.4f}) | {100 * r['frac']:.1f} % | {tb} | {rb} | {hb} | "
                     f"{rc} | {r['safe']:.4f} | {agree} |")
    if not a.no_solve:
        lines += ["", "Whole `solve_tube_qp` (wall ms, best of 3 after one warm-up solve; status, iterations), pendulum-shaped problem of "
                  "`tools/bench_tube_qp.py`, without and with a soft terminal row per sample (`z = Z = 1e6`):", "",
                  "| Ns | H | hard rows only | with the soft terminal row | samples paying |", "|---|---|---|---|---|"]
        for Ns, H in ((70, 17), (1024, 30)):
            s = run_solve(Ns, H, dev)
            print(s, flush=True)
            lines.append(f"| {Ns} | {H} | {s['hard'][0]:.1f} ({s['hard'][1]}, {s['hard'][2]}) | {s['soft'][0]:.1f} ({s['soft'][1]}, {s['soft'][2]}) | {s['paying']} |")
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# The tube row check against torch ops and the host path; the slacked tube QP (tools/bench_tube_rows.py)\n\n" + text + "\n")


if __name__ == "__main__":
    main()
