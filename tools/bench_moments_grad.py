#!/usr/bin/env python3
"""Time ``gpmpc_moment_rollout_vjp`` (the reverse-mode gradient of the linearised mean / covariance tube of B candidates, one
launch) and write profiles/moments_grad_bench.md.

    python tools/bench_moments_grad.py [--iters 20] [--out profiles/moments_grad_bench.md]

The workloads and batches of tools/bench_moments.py (pendulum1D H = 30, car H = 40 and 50, the shipped training sets, feedback as
shipped; B = 1, 1024, 65536).  Per row: ms per launch of the VJP kernel, of (b) the forward kernel alone, and of (a)
``torch.autograd`` through the same arithmetic as batched torch operations on the device - ``TorchMoments`` of
tools/bench_moments.py, whose Jacobian is written out by hand so that one backward pass suffices - forward plus backward.  The
kernel's gradient is compared with (a) before anything is timed: the worst, over the candidates, of ``max|got - want| / max|want|``
within a candidate's ``g_x0`` / ``g_U``; a deviation above 1e-2 ends the run.  Needs a HIP device."""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import sampling_gpmpc_amd as sg                                              # noqa: E402
from bench_moments import BATCHES, WORKLOADS, TorchMoments, inputs, time_device   # noqa: E402
from sampling_gpmpc_amd.workloads import load_params                         # noqa: E402

F64 = torch.float64
LIMIT = 1e-2


def cotangents(M, P, seed):
    """Normal draws scaled per state dimension by 1 / max|M| and per step by 1 / max|P_t| (1 where the step's P is zero)."""
    g = torch.Generator().manual_seed(seed)
    gm = torch.randn(M.shape, dtype=F64, generator=g).to(M.device) / M.abs().amax(dim=(0, 2), keepdim=True)
    sc = P.abs().amax(dim=(0, 2, 3), keepdim=True)
    gp = torch.randn(P.shape, dtype=F64, generator=g).to(M.device) / torch.where(sc > 0, sc, torch.ones_like(sc))
    return gm, gp


def deviation(want, got):
    B = want.shape[0]
    sc = want.abs().reshape(B, -1).amax(1)
    return float(((got - want).abs().reshape(B, -1).amax(1) / torch.where(sc > 0, sc, torch.ones_like(sc))).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "moments_grad_bench.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_moments_grad.py needs a HIP device: a timing taken elsewhere says nothing about the kernel")
    name, cu, _ = sg._lib.device_info(0)
    rows = []
    for label, yaml_name, H in WORKLOADS:
        p = load_params(yaml_name)
        p["common"]["use_cuda"] = True
        p["agent"]["num_dyn_samples"] = 1
        agent = sg.Agent(p, sg.make_env(p))
        tm = TorchMoments(p, "cuda")
        for B in BATCHES:
            x0, U = inputs(p, B, H, "cuda")
            tube = sg.moment_rollout(agent, x0, U)
            gm, gp = cotangents(tube.mean, tube.cov, B + H)

            def torch_grad():
                xr, ur = x0.clone().requires_grad_(True), U.clone().requires_grad_(True)
                M, P = tm(xr, ur)
                return torch.autograd.grad((gm * M).sum() + (gp * P).sum(), [xr, ur])

            g_x0, g_U, _, info = sg.moment_rollout_vjp(agent, tube, x0, U, None, gm, gp)
            w_x0, w_U = torch_grad()
            torch.cuda.synchronize()
            d0, d1 = deviation(w_x0, g_x0), deviation(w_U, g_U)
            print(label, H, B, f"kernel against torch.autograd: g_x0 {d0:.1e}  g_U {d1:.1e}  info {int(info.max())}", flush=True)
            if not (d0 <= LIMIT and d1 <= LIMIT) or int(info.max()) != 0:
                sys.exit(f"the kernel's gradient differs from torch.autograd's by more than {LIMIT}: nothing is timed")
            del w_x0, w_U
            it = args.iters if B < 65536 else max(3, args.iters // 4)
            t_b = time_device(lambda: sg.moment_rollout_vjp(agent, tube, x0, U, None, gm, gp), it)
            t_f = time_device(lambda: sg.moment_rollout(agent, x0, U), it)
            t_a = time_device(torch_grad, max(2, it // 4))
            rows.append((label, H, B, t_b, t_f, t_b / t_f, t_a, t_a / (t_b + t_f), d0, d1))
            print(rows[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# gpmpc_moment_rollout_vjp: ms per launch\n\n")
        f.write(f"Device: {name} ({cu} CUs).  `python tools/bench_moments_grad.py --iters {args.iters}`; device times from events around "
                "back-to-back launches after three warm-up launches (each kernel figure includes its Python wrapper's output "
                "allocations).  VJP = `gpmpc_moment_rollout_vjp` with both cotangents, from a tube computed once; forward = "
                "`gpmpc_moment_rollout` alone; (a) = `torch.autograd` through the same arithmetic as batched torch operations on the "
                "device (hand-written Jacobian, one backward pass), forward plus backward; speed-up = (a) / (forward + VJP).  "
                "dev g_x0 / g_U: the kernel against (a), the worst over the candidates of max|diff| / max|gradient| within a "
                "candidate, taken before anything was timed.\n\n")
        f.write("| workload | H | B | VJP ms | forward ms | VJP / forward | (a) torch autograd ms | speed-up | dev g_x0 | dev g_U |\n")
        f.write("|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r[0]} | {r[1]} | {r[2]} | {r[3]:.4f} | {r[4]:.4f} | {r[5]:.2f} | {r[6]:.3f} | {r[7]:.1f} | {r[8]:.1e} | {r[9]:.1e} |\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
