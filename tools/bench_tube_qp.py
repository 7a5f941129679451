#!/usr/bin/env python3
"""Time ``gpmpc_tube_gram``, ``gpmpc_tube_apply`` and a whole ``solve_tube_qp`` and write profiles/tube_qp_bench.md.

    python tools/bench_tube_qp.py [--iters 20] [--out profiles/tube_qp_bench.md]

Shapes: pendulum1D (nx 2, nu 1) Ns = 1024, H = 30; the car (nx 4, nu 2) Ns = 1024, H = 40 and 50.  The models are synthetic
(per-sample noisy damped oscillators under a stabilising feedback, a state box and input rows with active bounds): the kernels'
time does not depend on the values.  The baseline is the same arithmetic as batched torch operations on the device - the
explicit G of every sample by the recurrence, then einsum - written here; the kernels' results are compared with it before
anything is timed.  Needs a HIP device."""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import sampling_gpmpc_amd as sg                                              # noqa: E402
from sampling_gpmpc_amd.tube_qp import TubeQP                                # noqa: E402

F64 = torch.float64
SHAPES = (("pendulum1D", 1024, 30, 2, 1), ("car", 1024, 40, 4, 2), ("car", 1024, 50, 4, 2))


def problem(Ns, H, nx, nu, device, seed=0):
    g = torch.Generator().manual_seed(seed + Ns + H)
    rn = lambda *s: torch.randn(*s, dtype=F64, generator=g)                   # noqa: E731
    dt, nb = 0.1, nx // 2
    A, B = torch.zeros(Ns, nx, H, nx, dtype=F64), torch.zeros(Ns, nx, H, nu, dtype=F64)
    K = torch.zeros(nu, nx, dtype=F64)
    for blk in range(nb):
        p, w = 2 * blk, 2 * blk + 1
        A[:, p, :, p], A[:, p, :, w] = 1.0, dt
        A[:, w, :, p], A[:, w, :, w] = -(1.0 + 0.5 * blk + 0.03 * rn(Ns, H)) * dt, 1.0 - (0.3 + 0.02 * rn(Ns, H)) * dt
        B[:, w, :, blk] = dt * (1.0 + 0.05 * rn(Ns, H))
        K[blk, p], K[blk, w] = -2.0, -1.5
    A = A + B @ K
    c = 0.0005 * rn(Ns, nx, H)
    x0 = torch.tensor([1.0, 0.0, -0.8, 0.0], dtype=F64)[:nx].repeat(Ns, 1)
    box = torch.tensor([1.5, 0.3, 1.5, 0.3], dtype=F64)[:nx].repeat(H + 1, 1) - 0.001 * torch.arange(H + 1, dtype=F64)[:, None]
    inf = torch.full((H + 1, nu), float("inf"), dtype=F64)
    u_hi = inf.clone()
    u_hi[:H] = 1.0
    qp = TubeQP(A=A, B=B, c=c, x0=x0, omega=torch.full((Ns,), 1.0 / Ns, dtype=F64), q=torch.tensor([10.0, 1.0, 6.0, 0.5], dtype=F64)[:nx].repeat(H + 1, 1),
                r=torch.zeros(H + 1, nx, dtype=F64), Qu=torch.tensor([0.01, 0.02], dtype=F64)[:nu], lm=0.05, v_prev=torch.zeros(H, nu, dtype=F64),
                E=torch.cat([torch.eye(nx, dtype=F64), K]), F=torch.cat([torch.zeros(nx, nu, dtype=F64), torch.eye(nu, dtype=F64)]),
                lo=torch.cat([-box, -u_hi], dim=1), hi=torch.cat([box, u_hi], dim=1))
    R = rn(Ns, H + 1, nx, nx)
    Theta = R @ R.transpose(-1, -2) / nx + 0.1 * torch.eye(nx, dtype=F64)
    return qp.to(device), (0.5 * (Theta + Theta.transpose(-1, -2))).to(device), rn(Ns, H, nx, nu).to(device), rn(Ns, H + 1, nx).to(device)


def torch_G(A, B):
    """The explicit G (Ns, H+1, nx, n) by the recurrence, batched over the samples."""
    Ns, nx, H, nu = B.shape
    G = [torch.zeros(Ns, nx, H * nu, dtype=F64, device=A.device)]
    for t in range(H):
        nxt = A[:, :, t, :] @ G[-1]
        nxt[:, :, t * nu:(t + 1) * nu] += B[:, :, t, :]
        G.append(nxt)
    return torch.stack(G, dim=1)


def torch_gram(A, B, Theta, Xi, eta):
    Ns, nx, H, nu = B.shape
    G = torch_G(A, B)
    W = torch.einsum("itkp,itkl,itlq->pq", G, Theta, G)
    M = torch.einsum("itkp,itka->pta", G[:, :H], Xi).reshape(H * nu, H * nu)
    return W + M + M.T, torch.einsum("itkp,itk->p", G, eta)


def torch_apply(A, B, c, x0, V):
    Ns, nx, H, nu = B.shape
    out = []
    for k in range(V.shape[0]):
        x, xs = x0, [x0]
        for t in range(H):
            x = torch.einsum("irc,ic->ir", A[:, :, t, :], x) + B[:, :, t, :] @ V[k, t] + c[:, :, t]
            xs.append(x)
        out.append(torch.stack(xs, dim=2))
    return torch.stack(out)


def time_device(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tube_qp_bench.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_tube_qp.py needs a HIP device: a timing taken elsewhere says nothing about the kernels")
    name, cu, _ = sg._lib.device_info(0)
    rows = []
    for label, Ns, H, nx, nu in SHAPES:
        qp, Theta, Xi, eta = problem(Ns, H, nx, nu, "cuda")
        n = H * nu
        ws = sg.tube_qp.tube_gram_workspace(Ns, H, nx, nu, "cuda")
        V = torch.randn(3, H, nu, dtype=F64, generator=torch.Generator().manual_seed(1)).to("cuda")
        W, b = sg.tube_gram(qp.A, qp.B, Theta, Xi, eta, ws)
        Wt, bt = torch_gram(qp.A, qp.B, Theta, Xi, eta)
        X, Xt = sg.tube_apply(qp.A, qp.B, V, qp.c, qp.x0), torch_apply(qp.A, qp.B, qp.c, qp.x0, V)
        torch.cuda.synchronize()
        dW, db = float((W - Wt).abs().max() / Wt.abs().max()), float((b - bt).abs().max() / bt.abs().max())
        dX = float(((X - Xt).abs().amax(dim=(0, 1, 3)) / Xt.abs().amax(dim=(0, 1, 3))).max())
        if max(dW, db, dX) > 1e-11:
            sys.exit(f"{label} H={H}: the kernels disagree with the torch baseline (W {dW:.1e}, b {db:.1e}, X {dX:.1e}); nothing timed")
        t_g = time_device(lambda: sg.tube_gram(qp.A, qp.B, Theta, Xi, eta, ws), args.iters)
        t_b = time_device(lambda: sg.tube_gram(qp.A, qp.B, None, None, eta, ws), args.iters)
        t_gt = time_device(lambda: torch_gram(qp.A, qp.B, Theta, Xi, eta), max(2, args.iters // 4))
        t_a = time_device(lambda: sg.tube_apply(qp.A, qp.B, V, qp.c, qp.x0), args.iters)
        t_at = time_device(lambda: torch_apply(qp.A, qp.B, qp.c, qp.x0, V), max(2, args.iters // 4))
        res = sg.solve_tube_qp(qp)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            res = sg.solve_tube_qp(qp)
        torch.cuda.synchronize()
        t_s = (time.perf_counter() - t0) * 1e3 / 3
        flop = 2.0 * Ns * H * (2 * nx * nx * n + nx * n * (n + 16) / 2)          # recurrence + Y on the VALU, the lower tiles on the MFMA
        rows.append((label, Ns, H, n, t_g, t_b, t_gt, t_a, t_at, t_s, res.status, res.iterations, flop / (t_g * 1e-3) / 1e12, dW, db, dX))
        print(rows[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# condensed tube QP: ms per call\n\n")
        f.write(f"Device: {name} ({cu} CUs).  `python tools/bench_tube_qp.py --iters {args.iters}`; device times from events around "
                "back-to-back calls after three warm-up calls (the wrappers' output allocations included), the whole solve from the "
                "host clock (it synchronises with the host every iteration: step lengths, the n x n Cholesky).  gram = W and b with "
                "Theta, Xi and eta; b only = the call without Theta; torch = the explicit G of every sample by the recurrence, then "
                "einsum, on the device; apply = 3 sequences.  FLOP: 2 Ns H (2 nx^2 n + nx n (n + 16) / 2).  dW / db / dX: the "
                "kernels against the torch baseline, relative to max |W|, max |b|, the largest |x| of the state dimension.\n\n")
        f.write("| workload | Ns | H | n | gram ms | b only ms | torch gram ms | apply ms | torch apply ms | solve ms | status | iterations | gram TFLOP/s | dW | db | dX |\n")
        f.write("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r[0]} | {r[1]} | {r[2]} | {r[3]} | {r[4]:.4f} | {r[5]:.4f} | {r[6]:.3f} | {r[7]:.4f} | {r[8]:.3f} | {r[9]:.1f} | {r[10]} | {r[11]} | "
                    f"{r[12]:.3f} | {r[13]:.1e} | {r[14]:.1e} | {r[15]:.1e} |\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
