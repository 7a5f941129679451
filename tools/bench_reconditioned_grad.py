#!/usr/bin/env python3
"""Time ``gpmpc_rollout_vjp`` and one iteration of ``plan_inputs_reconditioned`` and write profiles/reconditioned_grad_bench.md.

    python tools/bench_reconditioned_grad.py --registers-only      (no device needed: prints the code object's figures)
    python tools/bench_reconditioned_grad.py [--rounds 7] [--iters 10] [--torch-samples 64] [--out ...]

Cases: pendulum1D ``Ns = 1024, H = 30`` and the car in mode R ``Ns = 4096, H = 40`` (the shipped training sets, feedback and beta as
shipped, seeded base samples clamped to [-2, 2]).  Per case, medians over ``--rounds`` rounds that alternate between the measured calls
(each round times ``--iters`` back-to-back calls of the VJP between two device events - 100 times as many of the dispatcher's
forward, 10 times as many of the generic one, so that every window is a tenth of a second or more - after warm-up calls and one untimed call), with the minimum
and maximum over the rounds:

* the VJP launch; (i) the forward the dispatcher picks; (ii) the forward pinned to the generic kernel;
* one planner iteration - (a call with 6 steps - a call with 1 step) / 5;
* (iii) ``torch.autograd`` through form A on the device (every step a from-scratch dense Cholesky of [real; own draws], batched over
  the samples; written here from include/gpmpc_hip.h, it shares no code with the library or its tests), forward plus backward, on the
  first ``--torch-samples`` samples (autograd keeps every step's factor: the whole batch does not fit), reported per sample too.

The kernel's gradients are compared with the torch form on those samples before anything is timed; a deviation above 1e-2 ends the
run.  No bar is set for any of these figures: nobody has measured them before.  Timing needs a HIP device."""
import argparse
import os
import re
import statistics
import subprocess
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import sampling_gpmpc_amd as sg                                              # noqa: E402
from sampling_gpmpc_amd.workloads import fs_params, synthetic_u_ff           # noqa: E402

F64 = torch.float64
LIMIT = 1e-2
CASES = (("pendulum1D", "params_pendulum1D_samples", 1024, 30, None), ("car", "params_car_residual_fs", 4096, 40, 3.0))


class TorchFormA:
    """Mode R with fixed base samples as batched torch operations, every step factorised from scratch (value-only real labels)."""

    def __init__(self, params, agent, device):
        ag = params["agent"]
        self.g_ny, self.nx, self.nu = ag["g_dim"]["ny"], ag["dim"]["nx"], ag["dim"]["nu"]
        self.pend = agent.env_model.env_id == 0
        self.X_r = agent.Dyn_gp_X_train.reshape(-1, 2).to(device=device, dtype=F64)
        self.Y_r = agent.Dyn_gp_Y_train[:, :, 0].to(device=device, dtype=F64)
        self.il2 = 1.0 / torch.tensor(ag["Dyn_gp_lengthscale"]["both"], dtype=F64, device=device).reshape(self.g_ny, 2) ** 2
        self.os = torch.tensor(ag["Dyn_gp_outputscale"]["both"], dtype=F64, device=device).reshape(self.g_ny)
        self.noise = torch.tensor(ag["Dyn_gp_task_noises"]["val"], dtype=F64, device=device) * ag["Dyn_gp_task_noises"]["multiplier"] + ag["Dyn_gp_noise"]
        K = torch.tensor(params["optimizer"]["terminal_tightening"]["K"], dtype=F64, device=device).reshape(self.nu, self.nx)
        self.K = K if bool(ag["feedback"]["use"]) else torch.zeros_like(K)
        self.xg = torch.tensor(params["env"]["goal_state"], dtype=F64, device=device)[:self.nx]
        self.dt, self.beta, self.floor, self.dev = float(params["optimizer"]["dt"]), float(ag["Dyn_gp_beta"]), 1e-10, device

    def block(self, xa, xb, il2, os):
        r = xa[..., :, None, :] - xb[..., None, :, :]
        q = r * il2
        k = os * torch.exp(-0.5 * (r * q).sum(-1))
        rows = [[k, k * q[..., 0], k * q[..., 1]]]
        for a in range(2):
            rows.append([-k * q[..., a]] + [k * ((il2[a] if a == b else 0.0) - q[..., a] * q[..., b]) for b in range(2)])
        return torch.stack([torch.stack(row, dim=-1) for row in rows], dim=-2).transpose(-3, -2)     # (..., na, Ta, nb, Tb)

    def __call__(self, x0, U, z):
        Ns, H, N = z.shape[1], U.shape[0], self.X_r.shape[0]
        x = x0.expand(Ns, self.nx)
        eye = lambda n: torch.eye(n, dtype=F64, device=self.dev)                                     # noqa: E731
        Xs, pts, ys = [x], [], [[] for _ in range(self.g_ny)]
        for t in range(H):
            u = U[t] + (x - self.xg) @ self.K.T
            xi = torch.stack([x[:, 0 if self.pend else 2], u[:, 0]], dim=1)
            ph = torch.stack(pts, dim=1) if pts else torch.zeros(Ns, 0, 2, dtype=F64, device=self.dev)
            yt = []
            for o in range(self.g_ny):
                il2, os = self.il2[o], self.os[o]
                Krr = self.block(self.X_r, self.X_r, il2, os)[:, 0, :, 0] + self.noise[0] * eye(N)
                Khr = self.block(ph, self.X_r.expand(Ns, N, 2), il2, os)[..., 0].reshape(Ns, 3 * t, N)
                Khh = self.block(ph, ph, il2, os).reshape(Ns, 3 * t, 3 * t) + torch.diag(self.noise.repeat(t))
                L = torch.linalg.cholesky(torch.cat([torch.cat([Krr.expand(Ns, N, N), Khr.transpose(1, 2)], 2), torch.cat([Khr, Khh], 2)], 1))
                lab = torch.cat([self.Y_r[o].expand(Ns, N)] + ys[o], dim=1)
                k = torch.cat([self.block(self.X_r.expand(Ns, N, 2), xi[:, None], il2, os)[:, :, 0, 0, :],
                               self.block(ph, xi[:, None], il2, os)[:, :, :, 0, :].reshape(Ns, 3 * t, 3)], dim=1)
                v = torch.linalg.solve_triangular(L, k, upper=False)
                w = torch.linalg.solve_triangular(L, lab[..., None], upper=False)
                mu = (v.transpose(1, 2) @ w)[..., 0]
                S = torch.diag(torch.stack([os, os * il2[0], os * il2[1]])) - v.transpose(1, 2) @ v
                S = 0.5 * (S + S.transpose(1, 2))
                var = S.diagonal(dim1=1, dim2=2)
                var = torch.where(var < self.floor, torch.full_like(var, self.floor), var)
                yraw = mu + (torch.linalg.cholesky(S) @ z[t, :, o, :, None])[..., 0]
                sd = self.beta * torch.sqrt(var)
                y = torch.where(yraw <= mu - sd, mu - sd, yraw)
                y = torch.where(y >= mu + sd, mu + sd, y)
                ys[o].append(y)
                yt.append(y)
            pts.append(xi)
            g = torch.stack(yt, dim=1)[:, :, 0]
            if self.pend:
                x = torch.stack([x[:, 0] + x[:, 1] * self.dt, x[:, 1] + g[:, 0]], dim=1)
            else:
                x = torch.cat([x[:, :3] + x[:, 3:4] * g, (x[:, 3] + u[:, 1] * self.dt)[:, None]], dim=1)
            Xs.append(x)
        return torch.stack(Xs, dim=2)


def timed(fn, iters):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def alternating(fns, rounds, iters):
    for fn, _ in fns.values():
        for _ in range(2):
            fn()
    samples = {k: [] for k in fns}
    for _ in range(rounds):
        for k, (fn, div) in fns.items():
            fn()
            samples[k].append(timed(fn, max(1, int(iters / div))))
    return samples


def register_table():
    """[(instance, VGPR, AGPR, SGPR spills, VGPR spills, scratch B / lane, waves / SIMD)] of csrc/rollout_grad.hip from hipcc's remarks"""
    from sampling_gpmpc_amd.csrc import build
    src = os.path.join(build.HERE, "rollout_grad.hip")
    cmd = ([build.HIPCC, "-x", "hip", "--cuda-device-only", "-c", src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"] + build.FLAGS +
           build.EXTRA_FLAGS.get("rollout_grad.hip", []))
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(r.stderr)
    rows = []
    for blk in r.stderr.split("Function Name: ")[1:]:
        m = re.match(r"_ZN5gpmpc\d+rollout_vjp_kernelILb(\d)EEE", blk)
        if m:
            num = lambda key: int(re.search(re.escape(key) + r": (\d+)", blk).group(1))              # noqa: E731
            rows.append(("factor in LDS" if m.group(1) == "1" else "factor in the workspace", num("VGPRs"), num("AGPRs"), num("SGPRs Spill"),
                         num("VGPRs Spill"), num("ScratchSize [bytes/lane]"), num("Occupancy [waves/SIMD]")))
    return rows


def fmt(v):
    return f"{statistics.median(v):.3f} [{min(v):.3f}, {max(v):.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--torch-samples", type=int, default=64)
    ap.add_argument("--registers-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "reconditioned_grad_bench.md"))
    args = ap.parse_args()
    regs = register_table()
    if args.registers_only:
        for row in regs:
            print(row)
        return
    if not torch.cuda.is_available():
        sys.exit("bench_reconditioned_grad.py needs a HIP device: a timing taken elsewhere says nothing about the kernel")
    lib = sg._lib.load()
    name, cu, _ = sg._lib.device_info(0)
    rows = []
    for label, yaml_name, Ns, H, beta in CASES:
        p = fs_params(yaml_name, Ns, H, nograd=False, beta=beta)
        p["common"]["use_cuda"] = True
        small = {**p, "common": {**p["common"], "num_MPC_itrs": 1}, "optimizer": {**p["optimizer"], "SEMPC": {**p["optimizer"]["SEMPC"], "max_sqp_iter": 1}}}
        agent = sg.Agent(small, sg.make_env(p))
        agent.params = p
        g = torch.Generator().manual_seed(Ns + H)
        z = torch.randn(H, Ns, agent.g_ny, 3, dtype=F64, generator=g).clamp(-2.0, 2.0).to("cuda")
        x0 = torch.tensor(p["env"]["start"], dtype=F64)[:agent.nx].to("cuda")
        U = torch.tensor(synthetic_u_ff(agent.nu, H), dtype=F64).to("cuda")
        res = sg.reconditioned_rollout(agent, x0, U, z)
        gX = torch.randn(res.X_traj.shape, dtype=F64, generator=g).to("cuda") / res.X_traj.abs().amax(dim=(0, 2), keepdim=True)
        form_a = TorchFormA(p, agent, "cuda")
        nt = min(Ns, args.torch_samples)

        def torch_grad():
            xs, Us = x0.clone().requires_grad_(True), U.clone().requires_grad_(True)
            X = form_a(xs, Us, z[:, :nt])
            return torch.autograd.grad((gX[:nt] * X).sum(), (xs, Us))

        res_t = sg.reconditioned_rollout(agent, x0, U, z[:, :nt].contiguous())
        got = sg.reconditioned_rollout_vjp(agent, res_t, x0, U, z[:, :nt].contiguous(), gX[:nt].contiguous())
        want = torch_grad()
        torch.cuda.synchronize()
        devs = [float((a - b).abs().max() / b.abs().max()) for a, b in zip(got[:2], want)]
        info = int(got[2].max()) | int(res_t.info.max())
        print(label, "kernel against torch.autograd through form A (%d samples): g_x0 %.1e  g_U %.1e  info %d" % (nt, *devs, info), flush=True)
        L = sg._lib
        if not all(d <= LIMIT for d in devs) or info & (L.INFO_ROOT_FAIL | L.INFO_NEG_1x1 | L.INFO_TRAIN_CHOL_FAIL | L.INFO_STATE_FULL | L.INFO_NONFINITE):
            sys.exit(f"the kernel differs from torch.autograd by more than {LIMIT}: nothing is timed")
        del want

        def cost(X, Uc):
            d = X[:, :, -1] - form_a.xg[None]
            return (d * d).sum(1) + 1e-2 * (Uc * Uc).sum()

        def generic():
            prev = lib.gpmpc_rollout_pin_kernel(sg._lib.KERNEL_GENERIC)
            try:
                return sg.reconditioned_rollout(agent, x0, U, z)
            finally:
                lib.gpmpc_rollout_pin_kernel(prev)

        sg.reconditioned_rollout(agent, x0, U, z)
        picked = lib.gpmpc_rollout_last_kernel()
        fns = {"vjp": (lambda: sg.reconditioned_rollout_vjp(agent, res, x0, U, z, gX), 1),
               "fwd": (lambda: sg.reconditioned_rollout(agent, x0, U, z), 0.01),      # 100 x the calls: a window of 0.1 - 1 s
               "generic": (generic, 0.1),
               "plan1": (lambda: sg.plan_inputs_reconditioned(agent, x0, U, z, cost, 1, 0.05), 2),
               "plan6": (lambda: sg.plan_inputs_reconditioned(agent, x0, U, z, cost, 6, 0.05), 4),
               "torch": (torch_grad, 5)}
        s = alternating(fns, args.rounds, args.iters)
        s["iter"] = [(b6 - b1) / 5.0 for b1, b6 in zip(s["plan1"], s["plan6"])]
        ws = lib.gpmpc_rollout_vjp_workspace_bytes(agent._plan(use_grad=True).desc, Ns, H)
        rows.append((label, Ns, H, picked, s, devs, nt, ws))
        print(label, {k: fmt(v) for k, v in s.items()}, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# gpmpc_rollout_vjp / plan_inputs_reconditioned: ms per call\n\n")
        f.write(f"Device: {name} ({cu} CUs).  `python tools/bench_reconditioned_grad.py --rounds {args.rounds} --iters {args.iters} "
                f"--torch-samples {args.torch_samples}`; the shipped training sets, feedback as shipped, seeded base samples clamped to "
                "[-2, 2].  Device times from events around back-to-back calls, two warm-up calls and one untimed call before every timed "
                "window; calls per window: VJP --iters, forward 100 x, generic forward 10 x, planner calls 1/2 and 1/4, torch 1/5 of that; "
                "the rounds alternate between the calls, each cell is the median and [min, max] over the rounds (the figures "
                "include the Python wrappers' output allocations).  planner iteration = (a 6-step call - a 1-step call) / 5: one forward "
                "launch, one VJP launch, the cost and its autograd, one Adam update.  torch = autograd through form A (every step a "
                "from-scratch dense Cholesky) on the device, forward + backward, on the first samples only (autograd keeps every step's "
                "factor).  One run; no counters were collected; no bar is set for these figures.\n\n")
        f.write("| workload | Ns | H | VJP ms | forward ms (dispatcher: kernel) | generic forward ms | VJP / forward | VJP / generic forward | "
                "planner iteration ms | workspace MB | torch samples | torch forward + backward ms | torch ms per sample / (forward + VJP) ms per sample |\n")
        f.write("|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for label, Ns, H, picked, s, _, nt, ws in rows:
            med = {k: statistics.median(v) for k, v in s.items()}
            f.write(f"| {label} | {Ns} | {H} | {fmt(s['vjp'])} | {fmt(s['fwd'])} (kernel {picked}) | {fmt(s['generic'])} | {med['vjp'] / med['fwd']:.1f} | "
                    f"{med['vjp'] / med['generic']:.1f} | {fmt(s['iter'])} | {ws / 1e6:.0f} | {nt} | {fmt(s['torch'])} | "
                    f"{(med['torch'] / nt) / ((med['fwd'] + med['vjp']) / Ns):.0f} |\n")
        f.write("\nThe kernel against the torch form on the torch samples, taken before anything was timed (largest difference relative to the "
                "largest magnitude):\n\n| workload | g_x0 | g_U |\n|---|---|---|\n")
        for label, _, _, _, _, d, _, _ in rows:
            f.write(f"| {label} | {d[0]:.1e} | {d[1]:.1e} |\n")
        f.write("\nThe code object (hipcc's resource remarks for gfx950, the shipped flags):\n\n| instance | VGPR | AGPR | SGPR spills (to VGPR "
                "lanes) | VGPR spills | scratch B / lane | waves / SIMD by registers |\n|---|---|---|---|---|---|---|\n")
        for row in regs:
            f.write("| " + " | ".join(str(v) for v in row) + " |\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
