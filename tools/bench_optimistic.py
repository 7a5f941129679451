#!/usr/bin/env python3
"""Time ``gpmpc_optimistic_rollout``, ``gpmpc_optimistic_rollout_vjp`` and one iteration of ``plan_inputs_optimistic`` and write
profiles/optimistic_bench.md.

    python tools/bench_optimistic.py --registers-only [--registers profiles/optimistic_registers.json]      (no device needed)
    python tools/bench_optimistic.py [--rounds 7] [--iters 20] [--registers profiles/optimistic_registers.json] [--out ...]

pendulum1D and car (the shipped training sets, feedback as shipped, the YAML's ``Dyn_gp_beta``), ``H = 10``, ``B = 1024`` and
``B = 65536``, ``eta`` uniform in [-1, 1].  Per shape, medians over ``--rounds`` rounds that alternate between the measured calls (each
round times ``--iters`` back-to-back calls between two device events), with the minimum and maximum over the rounds:

* the optimistic forward and its VJP, and one planner iteration - (a call with 6 steps - a call with 1 step) / 5, so that the final
  evaluation and the set-up cancel;
* comparison one: ``moment_rollout`` / ``moment_rollout_vjp`` (both cotangents) in the same rounds - the forward runs the same GP pass
  without the Jacobian and ``A P A^T``;
* comparison two: the same recursion as batched torch operations with ``torch.autograd`` on the device, forward plus backward
  (``TorchOptimistic``, written here from the formulas of include/gpmpc_hip.h; it shares no code with the library or its tests).

The kernel's trajectory and gradients are compared with the torch form before anything is timed; a deviation above 1e-2 ends the run.
``--registers-only`` compiles csrc/optimistic.hip for gfx950 and records VGPR / AGPR / SGPR-spill / private-segment / LDS figures of
every instantiation from the compiler's resource remarks; a timing run copies that table into the report.  Timing needs a HIP device."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import sampling_gpmpc_amd as sg                                              # noqa: E402
from bench_moments import inputs                                             # noqa: E402
from sampling_gpmpc_amd.workloads import load_params                         # noqa: E402

F64 = torch.float64
LIMIT = 1e-2
H = 10
WORKLOADS = (("pendulum1D", "params_pendulum1D_samples"), ("car", "params_car_residual"))
BATCHES = (1024, 65536)


class TorchOptimistic:
    """x+ = env_step(x, u, m + beta eta sqrt(max(s, floor))) as batched torch operations (value-only real labels), on any device."""

    def __init__(self, params, device):
        env = sg.make_env({**params, "common": {**params["common"], "use_cuda": False}})
        X, Y = env.initial_training_data()
        ag = params["agent"]
        g_ny = ag["g_dim"]["ny"]
        self.env_id, self.nx, self.nu = env.env_id, ag["dim"]["nx"], ag["dim"]["nu"]
        ell = torch.tensor(ag["Dyn_gp_lengthscale"]["both"], dtype=F64).reshape(g_ny, 2)
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
        K = torch.tensor(params["optimizer"]["terminal_tightening"]["K"], dtype=F64).reshape(self.nu, self.nx)
        self.K = K if bool(ag["feedback"]["use"]) else torch.zeros_like(K)
        self.xg = torch.tensor(params["env"]["goal_state"], dtype=F64)[:self.nx]
        self.dt, self.floor, self.beta = float(params["optimizer"]["dt"]), 1e-10, float(ag["Dyn_gp_beta"])
        self.X, self.Linv, self.alpha = X.to(F64), torch.stack(Linv), torch.stack(alpha)
        for k in ("X", "Linv", "alpha", "u", "os", "K", "xg"):
            setattr(self, k, getattr(self, k).to(device))
        self.sel = 0 if self.env_id == 0 else 2

    def __call__(self, x0, U, eta):
        x, Xs = x0, [x0]
        for t in range(U.shape[1]):
            u = U[:, t] + (x - self.xg) @ self.K.T
            xi = torch.stack([x[:, self.sel], u[:, 0]], dim=1)
            r = xi[:, None, None, :] - self.X[None, None]                       # (B, 1, N, 2)
            k = self.os[None, :, None] * torch.exp(-0.5 * (r * r * self.u[None, :, None, :]).sum(-1))   # (B, g_ny, N)
            m = (k * self.alpha[None]).sum(-1)
            v = torch.einsum("oij,boj->boi", self.Linv, k)
            s = (self.os[None] - (v * v).sum(-1)).clamp_min(self.floor)
            f = m + self.beta * eta[:, t] * torch.sqrt(s)
            if self.env_id == 0:
                x = torch.stack([x[:, 0] + x[:, 1] * self.dt, x[:, 1] + f[:, 0]], dim=1)
            else:
                vel = x[:, 3]
                x = torch.cat([x[:, :3] + vel[:, None] * f, (vel + u[:, 1] * self.dt)[:, None]], dim=1)
            Xs.append(x)
        return torch.stack(Xs, dim=2)


def deviation(want, got):
    B = want.shape[0]
    sc = want.abs().reshape(B, -1).amax(1)
    return float(((got - want).abs().reshape(B, -1).amax(1) / torch.where(sc > 0, sc, torch.ones_like(sc))).max())


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
    """{name: [ms per call, one entry per round]}, each round timing every function once in turn after three warm-up calls of each.
    One untimed call precedes every timed window: what ran before it (the torch form leaves the caches full of its own tensors)
    would otherwise be charged to the first calls of the window - at B = 65536 that was 8 - 16 % of a 5-call window of the forward."""
    for fn, _ in fns.values():
        for _ in range(3):
            fn()
    samples = {k: [] for k in fns}
    for _ in range(rounds):
        for k, (fn, div) in fns.items():
            fn()
            samples[k].append(timed(fn, max(1, iters // div)))
    return samples


def register_table():
    """[{kernel, env, nrp, hg, vgpr, agpr, sgpr_spill, private, lds, occupancy}] of csrc/optimistic.hip from hipcc's resource remarks."""
    from sampling_gpmpc_amd.csrc import build
    src = os.path.join(build.HERE, "optimistic.hip")
    cmd = [build.HIPCC, "-x", "hip", "--cuda-device-only", "-c", src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"] + build.FLAGS
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(r.stderr)
    rows = []
    for blk in r.stderr.split("Function Name: ")[1:]:
        m = re.match(r"_ZN5gpmpc\d+(optimistic_rollout(?:_vjp)?_kernel)ILi(\d)ELi(\d+)ELb(\d)EEE", blk)
        if not m:
            continue
        num = lambda key: int(re.search(re.escape(key) + r": (\d+)", blk).group(1))          # noqa: E731
        rows.append(dict(kernel=m.group(1), env=int(m.group(2)), nrp=int(m.group(3)), hg=bool(int(m.group(4))), vgpr=num("VGPRs"),
                         agpr=num("AGPRs"), sgpr_spill=num("SGPRs Spill"), vgpr_spill=num("VGPRs Spill"),
                         private=num("ScratchSize [bytes/lane]"), lds=num("LDS Size [bytes/block]"), occupancy=num("Occupancy [waves/SIMD]")))
    return sorted(rows, key=lambda d: (d["kernel"], d["env"], d["hg"], d["nrp"]))


def fmt(v):
    return f"{statistics.median(v):.4f} [{min(v):.4f}, {max(v):.4f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--registers", default=os.path.join(REPO, "profiles", "optimistic_registers.json"))
    ap.add_argument("--registers-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "optimistic_bench.md"))
    args = ap.parse_args()
    if args.registers_only:
        with open(args.registers, "w") as f:
            f.write("[\n" + ",\n".join(json.dumps(row) for row in register_table()) + "\n]\n")
        print("wrote", args.registers)
        return
    if not torch.cuda.is_available():
        sys.exit("bench_optimistic.py needs a HIP device: a timing taken elsewhere says nothing about the kernel")
    name, cu, _ = sg._lib.device_info(0)
    rows = []
    for label, yaml_name in WORKLOADS:
        p = load_params(yaml_name)
        p["common"]["use_cuda"] = True
        p["agent"]["num_dyn_samples"] = 1
        agent = sg.Agent(p, sg.make_env(p))
        to = TorchOptimistic(p, "cuda")
        goal = to.xg
        for B in BATCHES:
            x0, U = inputs(p, B, H, "cuda")
            g = torch.Generator().manual_seed(B)
            eta = (torch.rand(B, H, agent.g_ny, dtype=F64, generator=g) * 2.0 - 1.0).to("cuda")
            tube = sg.optimistic_rollout(agent, x0, U, eta)
            gX = torch.randn(tube.X.shape, dtype=F64, generator=g).to("cuda") / tube.X.abs().amax(dim=(0, 2), keepdim=True)
            mom = sg.moment_rollout(agent, x0, U)
            sc = mom.cov.abs().amax(dim=(0, 2, 3), keepdim=True)
            gP = torch.randn(mom.cov.shape, dtype=F64, generator=g).to("cuda") / torch.where(sc > 0, sc, torch.ones_like(sc))

            def torch_grad():
                leaves = [t.clone().requires_grad_(True) for t in (x0, U, eta)]
                X = to(*leaves)
                return (X.detach(),) + torch.autograd.grad((gX * X).sum(), leaves)

            got = sg.optimistic_rollout_vjp(agent, tube, x0, U, eta, gX)
            want = torch_grad()
            torch.cuda.synchronize()
            dX = float(((tube.X - want[0]).abs() / want[0].abs().amax(dim=(0, 2), keepdim=True)).max())
            devs = [dX] + [deviation(w, k) for w, k in zip(want[1:], got[:3])]
            info = int(tube.info.max()) | int(got[3].max())
            print(label, B, "kernel against torch.autograd: X %.1e  g_x0 %.1e  g_U %.1e  g_eta %.1e  info %d" % (*devs, info), flush=True)
            if not all(d <= LIMIT for d in devs) or info != 0:
                sys.exit(f"the kernel differs from torch.autograd by more than {LIMIT}: nothing is timed")
            del want

            def cost(t, Uc):
                d = t.X[:, :, -1] - goal[None]
                return (d * d).sum(1) + 1e-2 * (Uc * Uc).sum(dim=(1, 2))

            fns = {"fwd": (lambda: sg.optimistic_rollout(agent, x0, U, eta), 1),
                   "vjp": (lambda: sg.optimistic_rollout_vjp(agent, tube, x0, U, eta, gX), 1),
                   "mom_fwd": (lambda: sg.moment_rollout(agent, x0, U), 1),
                   "mom_vjp": (lambda: sg.moment_rollout_vjp(agent, mom, x0, U, None, gX, gP), 1),
                   "plan1": (lambda: sg.plan_inputs_optimistic(agent, x0, U, cost, 1, 0.05, eta, 0.4), 4),
                   "plan6": (lambda: sg.plan_inputs_optimistic(agent, x0, U, cost, 6, 0.05, eta, 0.4), 4),
                   "torch": (torch_grad, 10)}
            s = alternating(fns, args.rounds, args.iters if B < 65536 else max(4, args.iters // 4))
            s["iter"] = [(b6 - b1) / 5.0 for b1, b6 in zip(s["plan1"], s["plan6"])]
            rows.append((label, B, s, devs))
            print(label, B, {k: fmt(v) for k, v in s.items()}, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# gpmpc_optimistic_rollout / gpmpc_optimistic_rollout_vjp / plan_inputs_optimistic: ms per call\n\n")
        f.write(f"Device: {name} ({cu} CUs).  `python tools/bench_optimistic.py --rounds {args.rounds} --iters {args.iters}`; H = {H}, the "
                "shipped training sets (36 / 45 value-only label rows: the `<0, 40, false>` and `<1, 48, false>` instantiations), feedback "
                "and beta as shipped, eta uniform in [-1, 1].  Device times from events around "
                "back-to-back calls, three warm-up calls and one untimed call before every timed window; the rounds alternate between the "
                "calls, each cell is the median and "
                "[min, max] over the rounds (the figures include the Python wrappers' output allocations; a quarter of the iterations "
                "at B = 65536, the planner calls a quarter and the torch form a tenth of that).  planner iteration = (a 6-step call - a "
                "1-step call) / 5: one forward launch, one VJP launch, the cost and its autograd, two Adam updates and the clamp.  "
                "torch = the same recursion as batched torch operations with torch.autograd on the device, forward + backward.\n\n")
        f.write("| workload | B | forward ms | VJP ms | planner iteration ms | `moment_rollout` ms | `moment_rollout_vjp` ms | "
                "forward / moment forward | VJP / moment VJP | torch forward + backward ms | torch / (forward + VJP) |\n")
        f.write("|---|---|---|---|---|---|---|---|---|---|---|\n")
        for label, B, s, _ in rows:
            med = {k: statistics.median(v) for k, v in s.items()}
            f.write(f"| {label} | {B} | {fmt(s['fwd'])} | {fmt(s['vjp'])} | {fmt(s['iter'])} | {fmt(s['mom_fwd'])} | {fmt(s['mom_vjp'])} | "
                    f"{med['fwd'] / med['mom_fwd']:.2f} | {med['vjp'] / med['mom_vjp']:.2f} | {fmt(s['torch'])} | "
                    f"{med['torch'] / (med['fwd'] + med['vjp']):.1f} |\n")
        f.write("\nThe forward against `moment_rollout`, round by round (same round, same order), as ratios:\n\n| workload | B | ratios |\n|---|---|---|\n")
        for label, B, s, _ in rows:
            f.write(f"| {label} | {B} | " + " ".join(f"{a / b:.3f}" for a, b in zip(s["fwd"], s["mom_fwd"])) + " |\n")
        f.write("\nThe kernels against the torch form, taken before anything was timed (X per state dimension relative to its largest "
                "magnitude; gradients per candidate relative to the largest magnitude within the candidate's block):\n\n"
                "| workload | B | X | g_x0 | g_U | g_eta |\n|---|---|---|---|---|---|\n")
        for label, B, _, d in rows:
            f.write(f"| {label} | {B} | " + " | ".join(f"{v:.1e}" for v in d) + " |\n")
        if os.path.exists(args.registers):
            with open(args.registers) as g:
                regs = json.load(g)
            f.write("\nRegisters of every instantiation (hipcc's resource remarks for gfx950, `--registers-only`; env 0 = pendulum1D, 1 = "
                    "car; private B is the frame the compiler reserves, see DESIGN 4.17 - no instantiation contains a scratch "
                    "instruction):\n\n| kernel | env | NRP | HG | VGPR | AGPR | SGPR spills (to VGPR lanes) | VGPR spills | private B | LDS B | "
                    "waves / SIMD by registers |\n|---|---|---|---|---|---|---|---|---|---|---|\n")
            for d in regs:
                f.write(f"| {d['kernel']} | {d['env']} | {d['nrp']} | {int(d['hg'])} | {d['vgpr']} | {d['agpr']} | {d['sgpr_spill']} | "
                        f"{d['vgpr_spill']} | {d['private']} | {d['lds']} | {d['occupancy']} |\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
