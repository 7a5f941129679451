#!/usr/bin/env python3
"""Time ``gpmpc_moment_rollout`` (the linearised mean / covariance tube of B candidates, one launch) and write
profiles/moments_bench.md.

    python tools/bench_moments.py [--iters 20] [--out profiles/moments_bench.md]

Per workload (pendulum1D H = 30, car H = 40 and 50, the shipped training sets, feedback as shipped) and B = 1, 1024, 65536:
ms per launch of the kernel, of (a) the same arithmetic as batched torch operations on the device and - at B = 1 - of (b) the same
torch code on the CPU.  Both references are written here, from the formulas of include/gpmpc_hip.h, and share no code with the
library or its tests; the kernel's result is compared with (a) before anything is timed.  Needs a HIP device."""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import sampling_gpmpc_amd as sg                                              # noqa: E402
from sampling_gpmpc_amd.workloads import load_params, synthetic_u_ff         # noqa: E402

F64 = torch.float64
WORKLOADS = (("pendulum1D", "params_pendulum1D_samples", 30), ("car", "params_car_residual", 40), ("car", "params_car_residual", 50))
BATCHES = (1, 1024, 65536)


class TorchMoments:
    """The arithmetic of gpmpc_moment_rollout as batched torch operations (value-only real labels), on any device."""

    def __init__(self, params, device):
        env = sg.make_env({**params, "common": {**params["common"], "use_cuda": False}})
        X, Y = env.initial_training_data()
        ag = params["agent"]
        g_ny, D = ag["g_dim"]["ny"], 2
        self.env_id, self.nx, self.nu, self.g_ny = env.env_id, ag["dim"]["nx"], ag["dim"]["nu"], g_ny
        ell = torch.tensor(ag["Dyn_gp_lengthscale"]["both"], dtype=F64).reshape(g_ny, D)
        self.os = torch.tensor(ag["Dyn_gp_outputscale"]["both"], dtype=F64).reshape(g_ny)
        noise = ag["Dyn_gp_task_noises"]["val"][0] * ag["Dyn_gp_task_noises"]["multiplier"] + ag["Dyn_gp_noise"]
        self.u = 1.0 / ell ** 2
        d = X[:, None, :] - X[None, :, :]
        Linv, alpha = [], []
        for o in range(g_ny):
            Kmat = self.os[o] * torch.exp(-0.5 * (d * d * self.u[o]).sum(-1)) + noise * torch.eye(X.shape[0], dtype=F64)
            L = torch.linalg.cholesky(Kmat)
            Linv.append(torch.linalg.solve_triangular(L, torch.eye(X.shape[0], dtype=F64), upper=False))
            alpha.append(torch.cholesky_solve(Y[o, :, :1], L)[:, 0])
        self.fb = bool(ag["feedback"]["use"])
        K = torch.tensor(params["optimizer"]["terminal_tightening"]["K"], dtype=F64).reshape(self.nu, self.nx)
        self.K = K if self.fb else torch.zeros_like(K)
        self.xg = torch.tensor(params["env"]["goal_state"], dtype=F64)[:self.nx]
        self.dt, self.floor = float(params["optimizer"]["dt"]), 1e-10
        self.X, self.Linv, self.alpha = X.to(F64), torch.stack(Linv), torch.stack(alpha)
        for k in ("X", "Linv", "alpha", "u", "os", "K", "xg"):
            setattr(self, k, getattr(self, k).to(device))
        self.sel = 0 if self.env_id == 0 else 2

    def __call__(self, x0, U):
        B, H, nx = U.shape[0], U.shape[1], self.nx
        mu, P = x0.clone(), torch.zeros(B, nx, nx, dtype=F64, device=x0.device)
        M, Ps = [mu], [P]
        eye = torch.eye(nx, dtype=F64, device=x0.device)
        dxi = torch.zeros(2, nx, dtype=F64, device=x0.device)
        dxi[0, self.sel] = 1.0
        dxi[1] = self.K[0]
        for t in range(H):
            u = U[:, t] + (mu - self.xg) @ self.K.T
            xi = torch.stack([mu[:, self.sel], u[:, 0]], dim=1)
            r = xi[:, None, None, :] - self.X[None, None]                       # (B, 1, N, 2)
            q = r * self.u[None, :, None, :]                                   # (B, g_ny, N, 2)
            k = self.os[None, :, None] * torch.exp(-0.5 * (r * q).sum(-1))     # (B, g_ny, N)
            ka = k * self.alpha[None]
            m = ka.sum(-1)
            dm = -(ka[..., None] * q).sum(2)                                   # (B, g_ny, 2)
            v = torch.einsum("oij,boj->boi", self.Linv, k)
            s = (self.os[None] - (v * v).sum(-1)).clamp_min(self.floor)
            dmx = dm @ dxi                                                     # (B, g_ny, nx)
            A = eye.repeat(B, 1, 1)
            GSG = torch.zeros_like(P)
            if self.env_id == 0:
                A[:, 0, 1] = self.dt
                A[:, 1, :] += dmx[:, 0]
                nxt = torch.stack([mu[:, 0] + mu[:, 1] * self.dt, mu[:, 1] + m[:, 0]], dim=1)
                GSG[:, 1, 1] = s[:, 0]
            else:
                vel = mu[:, 3]
                A[:, :3, :] += vel[:, None, None] * dmx
                A[:, :3, 3] += m
                A[:, 3, :] += self.dt * self.K[1]
                nxt = torch.cat([mu[:, :3] + vel[:, None] * m, (vel + u[:, 1] * self.dt)[:, None]], dim=1)
                GSG[:, [0, 1, 2], [0, 1, 2]] = (vel * vel)[:, None] * s
            P = A @ P @ A.transpose(1, 2) + GSG
            mu = nxt
            M.append(mu), Ps.append(P)
        return torch.stack(M, dim=2), torch.stack(Ps, dim=1)


def inputs(params, B, H, device):
    nx, nu = params["agent"]["dim"]["nx"], params["agent"]["dim"]["nu"]
    g = torch.Generator().manual_seed(B + H)
    x0 = torch.tensor(params["env"]["start"], dtype=F64)[:nx] + (torch.rand(B, nx, dtype=F64, generator=g) - 0.5) * 0.04
    U = torch.as_tensor(synthetic_u_ff(nu, H), dtype=F64)[None] + (torch.rand(B, H, nu, dtype=F64, generator=g) - 0.5) * 0.02
    return x0.to(device), U.to(device)


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


def time_host(fn, iters):
    fn()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    return (time.perf_counter() - t0) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "moments_bench.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_moments.py needs a HIP device: a timing taken elsewhere says nothing about the kernel")
    name, cu, _ = sg._lib.device_info(0)
    rows = []
    for label, yaml_name, H in WORKLOADS:
        p = load_params(yaml_name)
        p["common"]["use_cuda"] = True
        p["agent"]["num_dyn_samples"] = 1
        agent = sg.Agent(p, sg.make_env(p))
        tm_dev, tm_cpu = TorchMoments(p, "cuda"), TorchMoments(p, "cpu")
        n_r, g_ny = agent._plan(use_grad=True).n_r, agent.g_ny
        flop = g_ny * (n_r * (n_r + 1) + 14 * n_r) + 4 * agent.nx ** 3           # FMA = 2 FLOP; exponentials not counted
        for B in BATCHES:
            x0, U = inputs(p, B, H, "cuda")
            mt = sg.moment_rollout(agent, x0, U)
            M, P = tm_dev(x0, U)
            torch.cuda.synchronize()
            dM = float(((mt.mean - M).abs() / M.abs().amax(dim=(0, 2), keepdim=True)).max())
            sc = P.abs().amax(dim=(0, 2, 3), keepdim=True)
            dP = float(((mt.cov - P).abs() / torch.where(sc > 0, sc, torch.ones_like(sc))).max())
            it = args.iters if B < 65536 else max(3, args.iters // 4)
            t_k = time_device(lambda: sg.moment_rollout(agent, x0, U), it)
            t_t = time_device(lambda: tm_dev(x0, U), max(2, it // 4))
            t_c = time_host(lambda: tm_cpu(x0.cpu(), U.cpu()), 3) if B == 1 else float("nan")
            rows.append((label, H, B, t_k, t_t, t_c, B * H / (t_k * 1e-3), B * H * flop / (t_k * 1e-3) / 1e12, dM, dP))
            print(rows[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# gpmpc_moment_rollout: ms per launch\n\n")
        f.write(f"Device: {name} ({cu} CUs).  `python tools/bench_moments.py --iters {args.iters}`; device times from events around "
                "back-to-back launches after three warm-up launches (the kernel's figure includes the Python wrapper's output "
                "allocations), the CPU time from the host clock.  (a) = the same arithmetic as batched torch operations on the "
                "device, (b) = that code on the CPU at B = 1.  FLOP: g_ny (n_r (n_r + 1) + 14 n_r) + 4 nx^3 per candidate-step, "
                "exponentials not counted.  max dM / dP: the kernel against (a), relative to the largest |mean| of the state "
                "dimension / the largest |P| of the step.\n\n")
        f.write("| workload | H | B | kernel ms | (a) torch on device ms | (b) torch on CPU ms | candidate-steps/s | TFLOP/s | max dM | max dP |\n")
        f.write("|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            cpu = "-" if np.isnan(r[5]) else f"{r[5]:.2f}"
            f.write(f"| {r[0]} | {r[1]} | {r[2]} | {r[3]:.4f} | {r[4]:.3f} | {cpu} | {r[6]:.3e} | {r[7]:.3f} | {r[8]:.1e} | {r[9]:.1e} |\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
