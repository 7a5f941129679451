"""The fused small-ball kernel (gpmpc_sup_deviation) against the composition it replaces, on the same device.

    python tools/bench_sup_dev.py [--out profiles/sup_dev_bench.md] [--reps 21] [--warm 3] [--only G_NY,N,LOG2_NS]

Per shape (g_ny, n) x Ns, with a dense random root (Cholesky of A A^T / n) and four thresholds on the 1 %, 10 %, 50 % and 90 %
quantiles of the sup norm:
  (a)  sup_deviation, counts only;          (a') sup_deviation with maxdev (8 bytes per sample written);
  (b)  the composition available without the entry point: gpmpc_base_samples(beta = inf) into (Ns, g_ny n), torch.matmul with
       R^T, abs().amax() over the points and the outputs, compare and sum - with its three phases timed on their own as well.
Protocol: `warm` untimed calls of every variant, then `reps` rounds; a round runs the variants one after another, each between
its own pair of events on the stream (alternating, so drift hits all alike); the MEDIAN over the rounds is reported.  Peak bytes:
torch's peak allocated during one call, above what was allocated before it (root and thresholds excluded).
The condition is relative: the median of (a) and of (a') not above the median of (b) at every shape.  The script writes its
table first and exits non-zero when the condition does not hold; with --only it says that it was not fully evaluated.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import sampling_gpmpc_amd as sg
from sampling_gpmpc_amd import _lib

SHAPES = [(1, 36), (1, 64), (3, 64)]
LOG2_NS = [20, 23]
SEED = 4242
F64 = torch.float64


def dense_root(g_ny, n):
    g = torch.Generator().manual_seed(1000 * g_ny + n)
    A = torch.randn(g_ny, n, n, generator=g, dtype=F64)
    return torch.linalg.cholesky(A @ A.transpose(-1, -2) / n).cuda()


class Composition:
    """gpmpc_base_samples, then torch ops; the phases can run alone (on the buffers the previous phase left)."""

    def __init__(self, R, Ns, eps):
        self.R, self.Ns, self.eps = R, Ns, torch.tensor(eps, dtype=F64, device="cuda")
        self.g_ny, self.n = R.shape[0], R.shape[1]
        self.lib = _lib.load()
        self.z = self.d = self.dev = self.counts = None

    def generate(self):
        self.z = torch.empty(self.Ns, self.g_ny, self.n, dtype=F64, device="cuda")
        _lib.check(self.lib.gpmpc_base_samples(SEED, 1, 1, 0, self.Ns, self.g_ny * self.n, float("inf"), _lib.dptr(self.z), None,
                                               _lib.current_stream_ptr()), "gpmpc_base_samples")

    def product(self):
        self.d = torch.matmul(self.z.transpose(0, 1), self.R.transpose(-1, -2))          # (g_ny, Ns, n)

    def reduce(self):
        self.dev = self.d.abs().amax(-1).amax(0)
        self.counts = (self.dev[:, None] <= self.eps[None, :]).sum(0)

    def __call__(self):
        self.generate()
        self.product()
        self.z = None
        self.reduce()
        self.d = None


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def run(g_ny, n, log2_ns, a):
    Ns = 1 << log2_ns
    R = dense_root(g_ny, n)
    probe = sg.sup_deviation(R, 1 << 16, seed=SEED, want_maxdev=True)
    eps = tuple(sg.sup_deviation_quantile(probe.maxdev, [0.01, 0.1, 0.5, 0.9]).tolist())
    del probe
    comp = Composition(R, Ns, eps)
    state = {}

    def lean():
        state["lean"] = sg.sup_deviation(R, Ns, eps=eps, seed=SEED)

    def full():
        state["full"] = sg.sup_deviation(R, Ns, eps=eps, seed=SEED, want_maxdev=True)

    def whole():
        comp()

    variants = {"lean": lean, "full": full, "comp": whole, "gen": comp.generate, "mm": comp.product, "red": comp.reduce}
    order = ["lean", "full", "comp", "gen", "mm", "red"]          # gen / mm / red leave z and d for each other
    for _ in range(a.warm):
        for k in order:
            variants[k]()
    torch.cuda.synchronize()
    times = {k: [] for k in order}
    for _ in range(a.reps):
        evs = {k: timed(variants[k]) for k in order}
        torch.cuda.synchronize()
        for k, (e0, e1) in evs.items():
            times[k].append(e0.elapsed_time(e1))
    comp.z = comp.d = None
    row = {"g_ny": g_ny, "n": n, "log2_ns": log2_ns, "eps": eps}
    for k in order:
        row[k] = (statistics.median(times[k]), min(times[k]), max(times[k]))
    # agreement: the two sides may differ on samples within round-off of a threshold
    whole()
    lean()
    row["count_diff"] = int((comp.counts - state["lean"].n_within).abs().max())
    row["p"] = state["lean"].probability.tolist()
    state.clear()
    comp.dev = comp.counts = None
    for k in ("lean", "full", "comp"):
        row["peak_" + k] = peak_bytes(variants[k])
        state.clear()
        comp.dev = comp.counts = None
    return row


def mb(b):
    return f"{b / 2 ** 20:.1f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--only", default=None, help="G_NY,N,LOG2_NS")
    a = ap.parse_args()
    if a.reps < 20:
        sys.exit("at least 20 repetitions")
    _lib.require_hip_device("cuda")
    only = tuple(int(v) for v in a.only.split(",")) if a.only else None
    rows = []
    for log2_ns in LOG2_NS:
        for g_ny, n in SHAPES:
            if only in (None, (g_ny, n, log2_ns)):
                rows.append(run(g_ny, n, log2_ns, a))
                print(rows[-1], flush=True)
    lines = [f"Device: {_lib.device_info(0)[0]}.  {a.warm} warm-up calls of every variant, then {a.reps} rounds; in a round each variant "
             "runs once between its own pair of events on the stream; median (min - max) over the rounds, milliseconds.  Peak MB: "
             "torch's peak allocated during one call above what was allocated before it.  (b) = gpmpc_base_samples(beta = inf) + "
             "torch.matmul + abs().amax() + compare; its phases were also timed alone.  Thresholds: the 1 %, 10 %, 50 % and 90 % "
             "quantiles of the sup norm.", "",
             "| g_ny | n | Ns | (a) fused, counts only | (a') fused + maxdev | (b) composition | (b)/(a) | (b)/(a') | (b) generate | "
             "(b) matmul | (b) abs, amax, compare | peak MB (a) | peak MB (a') | peak MB (b) | largest count difference |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    ok = True
    for r in rows:
        f = lambda k: f"{r[k][0]:.3f} ({r[k][1]:.3f} - {r[k][2]:.3f})"
        ok = ok and r["lean"][0] <= r["comp"][0] and r["full"][0] <= r["comp"][0]
        lines.append(f"| {r['g_ny']} | {r['n']} | 2^{r['log2_ns']} | {f('lean')} | {f('full')} | {f('comp')} | "
                     f"{r['comp'][0] / r['lean'][0]:.2f}x | {r['comp'][0] / r['full'][0]:.2f}x | {f('gen')} | {f('mm')} | {f('red')} | "
                     f"{mb(r['peak_lean'])} | {mb(r['peak_full'])} | {mb(r['peak_comp'])} | {r['count_diff']} |")
    lines += ["", "Condition (median of (a) and of (a') not above the median of (b) at every shape): "
              + ("holds" if ok else "DOES NOT HOLD") + ("" if only is None else " - for the one shape of --only; not fully evaluated") + "."]
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("# Fused small-ball kernel against the composition it replaces (tools/bench_sup_dev.py)\n\n" + text + "\n")
    if not ok:
        sys.exit("the fused call is slower than the composition at some shape")


if __name__ == "__main__":
    main()
