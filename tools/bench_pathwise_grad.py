#!/usr/bin/env python3
"""Time ``gpmpc_pathwise_rollout_vjp`` (the reverse-mode gradient of the pathwise rollout of Ns samples, one launch) and write
profiles/pathwise_grad_bench.md.

    python tools/bench_pathwise_grad.py [--iters 20] [--rounds 7] [--out profiles/pathwise_grad_bench.md]

Two workloads (car Ns 4096 H 40 M 512; pendulum1D Ns 1024 H 30 M 256; the shipped training sets, feedback as shipped, one start state
and one input sequence shared by the samples: the planner's problem).  Per workload, ms per call of
  * the VJP with Y evaluated again (``pathwise_rollout_vjp(..., Y=None)``), and with the forward's Y given;
  * the forward alone, without and with Y;
  * ``torch.autograd`` through the same rollout as batched torch operations on the device (``pathwise.torch_rollout``), forward plus
    backward: what stands in for the kernel without it.
The kernel's gradient is compared with autograd's before anything is timed - ``max|got - want| / max|want|`` within ``g_x0`` and within
``g_U`` - and a deviation above the parity tolerance ends the run: 8 x the worst A-against-B figure the device test records for the
workload's shipped case (tests/test_pathwise_grad_host.py), times H / 5 for a horizon that is H / 5 of the test's.  Timing: device
events around ``iters`` back-to-back calls, every variant warmed up first, the variants alternated round by round in one process; the
median over the rounds and their lowest and highest value are reported.  Needs a HIP device."""
import argparse
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import sampling_gpmpc_amd as sg                                              # noqa: E402
from sampling_gpmpc_amd import _lib                                          # noqa: E402
from sampling_gpmpc_amd.pathwise import PathwiseSamples, torch_rollout       # noqa: E402
from sampling_gpmpc_amd.workloads import closed_loop_params, synthetic_u_ff  # noqa: E402
from tests.pathwise_reference import H as TEST_H                             # noqa: E402
from tests.test_pathwise_grad_host import WORST_AB                           # noqa: E402

F64 = torch.float64
WORKLOADS = (("car", "params_car_residual", "car_fb", 4096, 40, 512), ("pendulum1D", "params_pendulum1D_samples", "pend_fb", 1024, 30, 256))
VARIANTS = ("VJP, Y evaluated again", "VJP, Y given", "forward", "forward with Y", "torch.autograd forward + backward")


def block_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def deviation(want, got):
    return float((got - want).abs().max() / want.abs().max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pathwise_grad_bench.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_pathwise_grad.py needs a HIP device: a timing taken elsewhere says nothing about the kernel")
    name, cu, _ = _lib.device_info(0)
    rows = []
    for label, yaml_name, case, Ns, H, M in WORKLOADS:
        p = closed_loop_params(yaml_name, Ns, H, 1, 1)
        p["common"]["use_cuda"] = True
        p["agent"]["base_sample_generator"] = "counter"
        agent = sg.Agent(p, sg.make_env(p))
        env = agent.env_desc(None)
        x0 = torch.tensor(p["env"]["start"], dtype=F64)[:agent.nx].to("cuda")
        U = torch.as_tensor(synthetic_u_ff(agent.nu, H), dtype=F64).to("cuda")
        pw = PathwiseSamples.draw(agent, Ns, M, seed=7)
        X, Y = pw.rollout(x0, U, want_samples=True)
        g = torch.Generator().manual_seed(Ns + H + M)
        gX = torch.randn(X.shape, dtype=F64, generator=g).to("cuda") / X.abs().amax(dim=(0, 2), keepdim=True)

        def torch_grad():
            xr, ur = x0.clone().requires_grad_(True), U.clone().requires_grad_(True)
            return torch.autograd.grad((gX * torch_rollout(pw, xr, ur, env)).sum(), [xr, ur])

        g_x0, g_U, info = sg.pathwise_rollout_vjp(pw, X, x0, U, gX)
        y_x0, y_U, _ = sg.pathwise_rollout_vjp(pw, X, x0, U, gX, Y=Y)
        w_x0, w_U = torch_grad()
        torch.cuda.synchronize()
        limit = 8.0 * max(max(v.values()) for k, v in WORST_AB.items() if k[0] == case) * H / TEST_H
        d0, d1, bad = deviation(w_x0, g_x0), deviation(w_U, g_U), int((info != 0).sum()) + int((pw.last_info != 0).sum())
        same = bool(torch.equal(g_x0, y_x0) and torch.equal(g_U, y_U))
        print(label, Ns, H, M, f"kernel against torch.autograd: g_x0 {d0:.1e}  g_U {d1:.1e}  limit {limit:.1e}  non-finite {bad}  "
              f"Y given = Y evaluated again: {same}", flush=True)
        if not (d0 <= limit and d1 <= limit) or bad or not same:
            sys.exit(f"the kernel's gradient differs from torch.autograd's by more than {limit:.1e}: nothing is timed")
        del w_x0, w_U
        fns = (lambda: sg.pathwise_rollout_vjp(pw, X, x0, U, gX), lambda: sg.pathwise_rollout_vjp(pw, X, x0, U, gX, Y=Y),
               lambda: pw.rollout(x0, U), lambda: pw.rollout(x0, U, want_samples=True), torch_grad)
        iters = (args.iters,) * 4 + (max(2, args.iters // 5),)
        for fn in fns:                                                       # every shape once before anything is timed
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = [[] for _ in fns]
        for _ in range(args.rounds):                                         # the variants alternate: a drift of the clocks meets all of them
            for k, fn in enumerate(fns):
                ms[k].append(block_ms(fn, iters[k]))
        rows.append((label, Ns, H, M, [(statistics.median(v), min(v), max(v)) for v in ms], d0, d1))
        print(rows[-1], flush=True)
        del agent, pw
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# gpmpc_pathwise_rollout_vjp: ms per call\n\n")
        f.write(f"Device: {name} ({cu} CUs).  `python tools/bench_pathwise_grad.py --iters {args.iters} --rounds {args.rounds}`; device times "
                f"from events around {args.iters} back-to-back calls (torch.autograd: {max(2, args.iters // 5)}) after three warm-up calls of "
                "every variant, the variants alternated round by round in one process; median over the rounds (lowest - highest).  Every "
                "figure includes its Python wrapper: the output allocations and, for the VJP, the sum over the samples of the per-sample "
                "gradients (x0 and U are shared).  The VJP runs from a tube computed once.  dev g_x0 / g_U: the kernel against "
                "torch.autograd, max|diff| / max|gradient|, taken before anything was timed.\n\n")
        f.write("| workload | Ns | H | M | variant | ms median (lowest - highest) | against the forward | dev g_x0 | dev g_U |\n|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            fwd = r[4][2][0]
            for vname, (med, lo, hi) in zip(VARIANTS, r[4]):
                f.write(f"| {r[0]} | {r[1]} | {r[2]} | {r[3]} | {vname} | {med:.4f} ({lo:.4f} - {hi:.4f}) | {med / fwd:.2f} | {r[5]:.1e} | {r[6]:.1e} |\n")
        f.write("\n")
        for r in rows:
            t = [v[0] for v in r[4]]
            f.write(f"{r[0]}: forward + VJP (Y evaluated again) {t[2] + t[0]:.4f} ms, forward with Y + VJP (Y given) {t[3] + t[1]:.4f} ms, "
                    f"torch.autograd {t[4]:.3f} ms: {t[4] / (t[2] + t[0]):.1f} x and {t[4] / (t[3] + t[1]):.1f} x.\n\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
