#!/usr/bin/env python3
"""Time ``gpmpc_robust_tube_rollout`` (the robust ellipsoidal tube of B candidates, one launch) and ``gpmpc_pairwise_lipschitz`` (the
sampled Lipschitz constant without an N x N array) and write profiles/robust_tube_bench.md.

    python tools/bench_robust_tube.py [--iters 20] [--out profiles/robust_tube_bench.md]

Rollout, per workload (pendulum1D and car, the shipped training sets, feedback as shipped, H = 10) and B = 1, 1024, 65536: ms per
launch of the kernel, of (a) the same recursion as batched torch operations on the device (``torch.linalg.eigvalsh`` for
``lambda_max``) and of (b) ``moment_rollout`` at the same B and H - the kernel this one shares its GP pass with.  The torch form is
written here on top of ``tools/bench_moments.py``'s ``TorchMoments`` and shares no code with the library or its tests; the kernel's
result is compared with it before anything is timed.
Lipschitz: ``pairwise_lipschitz`` against the reference's own N x N form (``robust_tube_based_GPMPC_koller.py:34-44``) as torch
operations on the device at N = 8192 - the N x N x d differences of one group then take 3.2 GB -, and alone at the grid sizes the
N x N form cannot reach.  Needs a HIP device."""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sampling_gpmpc_amd as sg                                              # noqa: E402
from sampling_gpmpc_amd.workloads import load_params                         # noqa: E402
from bench_moments import TorchMoments, inputs, time_device                  # noqa: E402

F64 = torch.float64
WORKLOADS = (("pendulum1D", "params_pendulum1D_samples", 10, 0.02, 0.005), ("car", "params_car_residual", 10, 0.02, 0.01))
BATCHES = (1, 1024, 65536)
BETA = 2.0
LIP_NN, LIP_ALONE = 8192, (8192, 65536, 262144)
LIP_SHAPE = (4, 4, 6)                                                        # dx, G, df: the car's states against its [df/dx | df/du] rows


class TorchRobust(TorchMoments):
    """The recursion of gpmpc_robust_tube_rollout as batched torch operations (value-only real labels), on any device."""

    def __call__(self, x0, U, l_mu, l_sigma, beta):
        B, H, nx = U.shape[0], U.shape[1], self.nx
        dev = x0.device
        mu, Q = x0.clone(), torch.zeros(B, nx, nx, dtype=F64, device=dev)
        M, Qs = [mu], [Q]
        eye = torch.eye(nx, dtype=F64, device=dev)
        dxi = torch.zeros(2, nx, dtype=F64, device=dev)
        dxi[0, self.sel] = 1.0
        dxi[1] = self.K[0]
        W = torch.linalg.cholesky(eye + self.K.T @ self.K).T

        def outer(X, Y):
            tx, ty = torch.diagonal(X, dim1=1, dim2=2).sum(1), torch.diagonal(Y, dim1=1, dim2=2).sum(1)
            ok = (tx != 0) & (ty != 0)
            c = torch.sqrt(torch.where(ok, tx, torch.ones_like(tx)) / torch.where(ok, ty, torch.ones_like(ty)))
            both = (1.0 + 1.0 / c)[:, None, None] * X + (1.0 + c)[:, None, None] * Y
            return torch.where((ty == 0)[:, None, None], X, torch.where((tx == 0)[:, None, None], Y, both))

        for t in range(H):
            u = U[:, t] + (mu - self.xg) @ self.K.T
            xi = torch.stack([mu[:, self.sel], u[:, 0]], dim=1)
            r = xi[:, None, None, :] - self.X[None, None]
            q = r * self.u[None, :, None, :]
            k = self.os[None, :, None] * torch.exp(-0.5 * (r * q).sum(-1))
            ka = k * self.alpha[None]
            m = ka.sum(-1)
            dm = -(ka[..., None] * q).sum(2)
            v = torch.einsum("oij,boj->boi", self.Linv, k)
            s = (self.os[None] - (v * v).sum(-1)).clamp_min(self.floor)
            dmx = dm @ dxi
            A = eye.repeat(B, 1, 1)
            gd = torch.zeros(B, nx, dtype=F64, device=dev)
            if self.env_id == 0:
                A[:, 0, 1] = self.dt
                A[:, 1, :] += dmx[:, 0]
                nxt = torch.stack([mu[:, 0] + mu[:, 1] * self.dt, mu[:, 1] + m[:, 0]], dim=1)
                gd[:, 1] = s[:, 0]
            else:
                vel = mu[:, 3]
                A[:, :3, :] += vel[:, None, None] * dmx
                A[:, :3, 3] += m
                A[:, 3, :] += self.dt * self.K[1]
                nxt = torch.cat([mu[:, :3] + vel[:, None] * m, (vel + u[:, 1] * self.dt)[:, None]], dim=1)
                gd[:, :3] = (vel * vel)[:, None] * s
            r2 = torch.linalg.eigvalsh(W @ Q @ W.T)[:, -1].clamp_min(0.0)
            ub = 0.5 * l_mu * r2[:, None]
            sb = beta * (gd.sqrt() + l_sigma * r2.sqrt()[:, None])
            Q = outer(outer(torch.diag_embed(nx * sb * sb), torch.diag_embed(nx * ub * ub)), A @ Q @ A.transpose(1, 2))
            mu = nxt
            M.append(mu), Qs.append(Q)
        return torch.stack(M, dim=2), torch.stack(Qs, dim=1)


def lipschitz_nn(X, F, eps=1e-6):
    """The reference's formula per group on the device: N x N x d differences, then the maximum."""
    dn = torch.norm(X.unsqueeze(1) - X.unsqueeze(0), dim=2) + eps
    return torch.stack([(torch.norm(F[:, g].unsqueeze(1) - F[:, g].unsqueeze(0), dim=2) / dn).max() for g in range(F.shape[1])])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "robust_tube_bench.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_robust_tube.py needs a HIP device: a timing taken elsewhere says nothing about the kernels")
    name, cu, _ = sg._lib.device_info(0)
    rows = []
    for label, yaml_name, H, lm, ls in WORKLOADS:
        p = load_params(yaml_name)
        p["common"]["use_cuda"] = True
        p["agent"]["num_dyn_samples"] = 1
        agent = sg.Agent(p, sg.make_env(p))
        tr = TorchRobust(p, "cuda")
        nx = agent.nx
        l_mu, l_sigma = torch.full((nx,), lm, dtype=F64, device="cuda"), torch.full((nx,), ls, dtype=F64, device="cuda")
        for B in BATCHES:
            x0, U = inputs(p, B, H, "cuda")
            rt = sg.robust_tube_rollout(agent, x0, U, l_mu, l_sigma, BETA)
            M, Q = tr(x0, U, l_mu, l_sigma, BETA)
            torch.cuda.synchronize()
            fin = torch.isfinite(Q).all(-1).all(-1).all(-1) & (rt.info == 0)
            dM = float(((rt.mean - M).abs() / M.abs().amax(dim=(0, 2), keepdim=True))[fin].max())
            sc = Q[fin].abs().amax(dim=(0, 2, 3), keepdim=True)
            dQ = float(((rt.cov[fin] - Q[fin]).abs() / torch.where(sc > 0, sc, torch.ones_like(sc))).max())
            it = args.iters if B < 65536 else max(3, args.iters // 4)
            t_k = time_device(lambda: sg.robust_tube_rollout(agent, x0, U, l_mu, l_sigma, BETA), it)
            t_p = time_device(lambda: sg.robust_tube_rollout(agent, x0, U, l_mu, l_sigma, BETA, want_parts=True), it)
            t_m = time_device(lambda: sg.moment_rollout(agent, x0, U), it)
            t_t = time_device(lambda: tr(x0, U, l_mu, l_sigma, BETA), max(2, it // 4))
            rows.append((label, H, B, t_k, t_p, t_m, t_t, float(fin.to(F64).mean()), float(Q[fin].abs().max()), dM, dQ))
            print(rows[-1], flush=True)
    lip = []
    dx, G, df = LIP_SHAPE
    g = torch.Generator().manual_seed(0)
    for N in LIP_ALONE:
        X = torch.rand(N, dx, dtype=F64, generator=g).to("cuda")
        Wm = torch.randn(G, df, dx, dtype=F64, generator=g).to("cuda")
        F = torch.sin(torch.einsum("gfd,nd->ngf", Wm, X)).contiguous()
        it = 10 if N <= 8192 else (3 if N <= 65536 else 1)
        t_k = time_device(lambda: sg.pairwise_lipschitz(X, F), it)
        t_nn, d = float("nan"), float("nan")
        if N == LIP_NN:
            mx, _, _ = sg.pairwise_lipschitz(X, F)
            want = lipschitz_nn(X, F)
            torch.cuda.synchronize()
            d = float(((mx - want).abs() / want).max())
            t_nn = time_device(lambda: lipschitz_nn(X, F), 3)
        pairs = N * (N - 1) / 2
        lip.append((N, t_k, t_nn, pairs * G / (t_k * 1e-3), d))
        print(lip[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# gpmpc_robust_tube_rollout and gpmpc_pairwise_lipschitz: ms per call\n\n")
        f.write(f"Device: {name} ({cu} CUs).  `python tools/bench_robust_tube.py --iters {args.iters}`; device times from events around "
                "back-to-back calls after three warm-up calls (the figures include the Python wrappers' output allocations).\n\n")
        f.write(f"## The rollout (H = 10, beta = {BETA}, Q0 = 0, shared constants)\n\n"
                "kernel = `robust_tube_rollout`, + parts = with `want_parts=True` (r2, sd, jz written too), moments = `moment_rollout` at the "
                "same B and H, (a) = the same recursion as batched torch operations on the device (`torch.linalg.eigvalsh`).  finite: the "
                "share of candidates whose tube stays finite in both forms; max|Q|, max dM, max dQ over those (the kernel against (a), "
                "relative to the largest |centre| of the state dimension / the largest |Q| of the step).\n\n")
        f.write("| workload | H | B | kernel ms | + parts ms | moments ms | (a) torch on device ms | finite | max abs Q | max dM | max dQ |\n")
        f.write("|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r[0]} | {r[1]} | {r[2]} | {r[3]:.4f} | {r[4]:.4f} | {r[5]:.4f} | {r[6]:.3f} | {r[7]:.3f} | {r[8]:.1e} | {r[9]:.1e} | {r[10]:.1e} |\n")
        f.write(f"\n## The Lipschitz estimate (dx = {dx}, G = {G}, df = {df}, eps = 1e-6)\n\n"
                "kernel = `pairwise_lipschitz` (two launches), N x N = the reference's formula per group as torch operations on the device "
                f"(measured at N = {LIP_NN} only: beyond it the N x N x d differences do not fit).  pair-groups/s: N (N - 1) / 2 pairs times G "
                "groups over the kernel's time.  max d: the kernel's maxima against the N x N form's, relative.\n\n")
        f.write("| N | kernel ms | N x N torch on device ms | pair-groups/s | max d |\n|---|---|---|---|---|\n")
        for r in lip:
            nn = "-" if r[2] != r[2] else f"{r[2]:.2f}"
            d = "-" if r[4] != r[4] else f"{r[4]:.1e}"
            f.write(f"| {r[0]} | {r[1]:.3f} | {nn} | {r[3]:.3e} | {d} |\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
