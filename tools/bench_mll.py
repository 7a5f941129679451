"""The batched marginal likelihood (gpmpc_marginal_likelihood) against torch on the same device.

    python tools/bench_mll.py [--out profiles/mll_bench.md] [--reps 21] [--warm 3] [--B 1024] [--only NAME]

Shapes: B = 1024 candidates (``restarts`` around the YAML's values, spread 0.2) of the pendulum (1 output: 36 value rows, 108 rows
with all tasks) and of the car (3 outputs: 45 and 135 rows).  Variants:
  (a)  the entry point with the gradient;   (a') the entry point, nll / quad / logdet only;
  (b)  torch autograd of the same formula: the batched kernel matrix from theta, torch.linalg.cholesky, a triangular solve,
       nll.sum().backward();
  (c)  the linear algebra alone on a prebuilt K: batched torch.linalg.cholesky + torch.cholesky_inverse (what any torch version of
       the trace formula has to run before it contracts K^-1 with dK).
Protocol: `warm` untimed calls of every variant, then `reps` rounds; a round runs the variants one after another, each between its
own pair of events on the stream; the MEDIAN over the rounds is reported.  Nothing is asserted about speed: the table records
what was measured.  The agreement column is the largest deviation of (a) from (b) over the batch, nll relative and the gradient
relative to the largest component of its candidate.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import sampling_gpmpc_amd as sg
from sampling_gpmpc_amd import _lib
from sampling_gpmpc_amd.workloads import load_params

F64 = torch.float64
D = 2
SETS = [("pendulum, value rows", "params_pendulum1D_samples", False), ("pendulum, all tasks", "params_pendulum1D_samples", True),
        ("car, value rows", "params_car_residual", False), ("car, all tasks", "params_car_residual", True)]


def kernel_matrices(X, th, T, has_grad):
    """(M, n, n) for candidates th (M, P): K_rbf + diag(nz), rows point-major and task-minor."""
    ell, osc, nz = th[:, :D], th[:, D], th[:, D + 1:D + 1 + T]
    u = 1.0 / (ell * ell)
    r = X[:, None, :] - X[None, :, :]
    q = r[None] * u[:, None, None, :]
    k = osc[:, None, None] * torch.exp(-0.5 * (r[None] * q).sum(-1))
    M, N = th.shape[0], X.shape[0]
    if not has_grad:
        return k + nz[:, 0, None, None] * torch.eye(N, dtype=F64, device=X.device)
    blk = [[None] * T for _ in range(T)]
    blk[0][0] = k
    for b in range(1, T):
        blk[0][b] = k * q[..., b - 1]
        blk[b][0] = -k * q[..., b - 1]
        for a in range(1, T):
            blk[a][b] = k * ((u[:, a - 1, None, None] if a == b else 0.0) - q[..., a - 1] * q[..., b - 1])
    K = torch.stack([torch.stack(row, dim=-1) for row in blk], dim=-2).permute(0, 1, 3, 2, 4).reshape(M, N * T, N * T)
    return K + torch.diag_embed(nz.repeat(1, N))


def torch_nll(X, Y, th, has_grad):
    """(B, g_ny) for th (B, g_ny, P)."""
    B, g_ny, P = th.shape
    T = Y.shape[2]
    K = kernel_matrices(X, th.reshape(B * g_ny, P), T, has_grad)
    y = (Y if has_grad else Y[:, :, :1]).clone()
    y = y[None].expand(B, -1, -1, -1).clone()
    y[..., 0] = y[..., 0] - th[..., -1, None]
    r = y.reshape(B * g_ny, -1, 1)
    L = torch.linalg.cholesky(K)
    w = torch.linalg.solve_triangular(L, r, upper=False)
    n = K.shape[-1]
    nll = 0.5 * (w * w).sum((-1, -2)) + torch.log(torch.diagonal(L, dim1=-2, dim2=-1)).sum(-1) + 0.5 * n * 1.8378770664093453
    return nll.reshape(B, g_ny)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


def run(label, pname, has_grad, a):
    p = load_params(pname)
    p["common"]["use_cuda"] = False
    p["env"]["train_data_has_derivatives"] = has_grad
    X, Y = sg.make_env(p).initial_training_data()
    X, Y = X.cuda(), Y.cuda()
    theta = sg.restarts(sg.theta_from_params(p, True), a.B, spread=0.2, seed=11).cuda()
    T = Y.shape[2]
    Kpre = kernel_matrices(X, theta.reshape(-1, theta.shape[2]), T, has_grad)
    state = {}

    def full():
        state["a"] = sg.marginal_likelihood(X, Y, theta, want_grad=True)

    def lean():
        state["a1"] = sg.marginal_likelihood(X, Y, theta, want_grad=False)

    def autograd():
        th = theta.clone().requires_grad_(True)
        nll = torch_nll(X, Y, th, has_grad)
        nll.sum().backward()
        state["b"] = (nll.detach(), th.grad)

    def linalg():
        state["c"] = torch.cholesky_inverse(torch.linalg.cholesky(Kpre))

    variants = {"full": full, "lean": lean, "autograd": autograd, "linalg": linalg}
    for _ in range(a.warm):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(a.reps):
        evs = {k: timed(fn) for k, fn in variants.items()}
        torch.cuda.synchronize()
        for k, (e0, e1) in evs.items():
            times[k].append(e0.elapsed_time(e1))
    ra, (nll_b, grad_b) = state["a"], state["b"]
    ok = (ra.info == 0) & torch.isfinite(nll_b)
    d_nll = ((ra.nll - nll_b).abs() / nll_b.abs())[ok].max().item()
    d_grad = ((ra.grad - grad_b).abs().amax(-1) / grad_b.abs().amax(-1))[ok].max().item()
    row = {"label": label, "g_ny": int(Y.shape[0]), "n": ra.n, "B": a.B, "failed": int((ra.info != 0).sum()), "d_nll": d_nll, "d_grad": d_grad}
    for k in variants:
        row[k] = (statistics.median(times[k]), min(times[k]), max(times[k]))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--only", default=None, help="a label of SETS")
    a = ap.parse_args()
    if a.reps < 20:
        sys.exit("at least 20 repetitions")
    _lib.require_hip_device("cuda")
    rows = []
    for label, pname, has_grad in SETS:
        if a.only in (None, label):
            rows.append(run(label, pname, has_grad, a))
            print(rows[-1], flush=True)
    lines = [f"Device: {_lib.device_info(0)[0]}.  B = {a.B} candidates (restarts around the YAML's values, spread 0.2, seed 11).  {a.warm} warm-up "
             f"calls of every variant, then {a.reps} rounds; in a round each variant runs once between its own pair of events on the "
             "stream; median (min - max) over the rounds, milliseconds.  (a) gpmpc_marginal_likelihood with the gradient, (a') nll, quad "
             "and logdet only; (b) torch autograd of the same formula (batched kernel matrix, torch.linalg.cholesky, triangular solve, "
             "backward); (c) torch.linalg.cholesky + torch.cholesky_inverse alone on a prebuilt K.  Agreement: (a) against (b) over the "
             "candidates whose factorisation succeeded, nll relative, gradient relative to its candidate's largest component.  No "
             "speed-up is promised or asserted anywhere; this is what was measured.", "",
             "| training set | outputs | rows n | problems | (a) entry point + gradient | (a') entry point, nll only | (b) torch autograd | "
             "(c) torch cholesky + cholesky_inverse | (b)/(a) | (c)/(a) | failed candidates | nll agreement | gradient agreement |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        f = lambda k: f"{r[k][0]:.3f} ({r[k][1]:.3f} - {r[k][2]:.3f})"
        lines.append(f"| {r['label']} | {r['g_ny']} | {r['n']} | {r['B'] * r['g_ny']} | {f('full')} | {f('lean')} | {f('autograd')} | "
                     f"{f('linalg')} | {r['autograd'][0] / r['full'][0]:.2f}x | {r['linalg'][0] / r['full'][0]:.2f}x | {r['failed']} | "
                     f"{r['d_nll']:.1e} | {r['d_grad']:.1e} |")
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("# Batched marginal likelihood against torch on the same device (tools/bench_mll.py)\n\n" + text + "\n")


if __name__ == "__main__":
    main()
