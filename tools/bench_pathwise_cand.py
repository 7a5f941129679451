#!/usr/bin/env python3
"""Time the pathwise rollout of B candidate input sequences and its VJP (``gpmpc_pathwise_rollout_cand`` / ``_cand_vjp``, one launch
each) against the two ways the single-candidate kernels offer, and write profiles/pathwise_cand_bench.md.

    python tools/bench_pathwise_cand.py [--iters 20] [--rounds 7] [--out profiles/pathwise_cand_bench.md]

Two workloads (car Ns 1024 H 40 M 512; pendulum1D Ns 1024 H 30 M 256; the shipped training sets, feedback as shipped, one start state),
each at B = 1, 4, 16, 64 candidates: the synthetic input sequence plus 0.01 b.  Per workload and B, ms per evaluation of all B
candidates - a forward that keeps Y and a VJP that reads it, the sum over the samples of the gradients included - of
  (i)   the candidate kernels: one forward launch, one backward launch;
  (ii)  B calls of ``gpmpc_pathwise_rollout`` + ``gpmpc_pathwise_rollout_vjp``, one per candidate;
  (iii) one call of that pair over B Ns rows, the normals and update vectors replicated B times and U per row - where the replicas fit
        in ``--replica-gib`` (default 4) of device memory;
and the peak device memory of one evaluation: what torch's allocator holds at most above what was allocated before the evaluation
(every output of all B candidates alive at once), for (iii) plus its replicas (Z, V and the per-row U).  Before anything is timed the tubes, Y, info and per-pair gradients the kernels of (i) write are compared with those of (ii)
bit for bit; a difference ends the run.  Timing: device events around ``iters`` back-to-back evaluations, every variant warmed up first, the variants
alternated round by round in one process; the median over the rounds and their lowest and highest value are reported, and for the
ratio (i) / (ii) the interval [lowest (i) / highest (ii), highest (i) / lowest (ii)] is the run's own spread.  Needs a HIP device."""
import argparse
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import sampling_gpmpc_amd as sg                                              # noqa: E402
from sampling_gpmpc_amd import _lib                                          # noqa: E402
from sampling_gpmpc_amd.pathwise import PathwiseSamples, _rollout_backward, _rollout_cand_backward    # noqa: E402
from sampling_gpmpc_amd.workloads import closed_loop_params, synthetic_u_ff  # noqa: E402

F64 = torch.float64
WORKLOADS = (("car", "params_car_residual", 1024, 40, 512), ("pendulum1D", "params_pendulum1D_samples", 1024, 30, 256))
CANDIDATES = (1, 4, 16, 64)
VARIANTS = ("(i) candidate kernels", "(ii) B calls of the pair", "(iii) the pair on B Ns rows")
MIB = 1024.0 * 1024.0


def block_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def peak_mib(fn):
    """what one evaluation allocates at its peak, above what was allocated before it (torch's allocator)"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = (torch.cuda.max_memory_allocated() - before) / MIB
    del out
    return peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--replica-gib", type=float, default=4.0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pathwise_cand_bench.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_pathwise_cand.py needs a HIP device: a timing taken elsewhere says nothing about the kernel")
    name, cu, _ = _lib.device_info(0)
    rows = []
    for label, yaml_name, Ns, H, M in WORKLOADS:
        p = closed_loop_params(yaml_name, Ns, H, 1, 1)
        p["common"]["use_cuda"] = True
        p["agent"]["base_sample_generator"] = "counter"
        agent = sg.Agent(p, sg.make_env(p))
        x0 = torch.tensor(p["env"]["start"], dtype=F64)[:agent.nx].to("cuda")
        U1 = torch.as_tensor(synthetic_u_ff(agent.nu, H), dtype=F64).to("cuda")
        pw = PathwiseSamples.draw(agent, Ns, M, seed=7)
        for B in CANDIDATES:
            U = (U1[None] + 0.01 * torch.arange(B, dtype=F64, device="cuda")[:, None, None]).contiguous()
            X = pw.rollout_candidates(x0, U)
            g = torch.Generator().manual_seed(Ns + H + M + B)
            gX = (torch.randn(X.shape, dtype=F64, generator=g).to("cuda") / X.abs().amax(dim=(0, 1, 3), keepdim=True)).contiguous()
            del X

            def cand():
                X, Y = pw.rollout_candidates(x0, U, want_samples=True)
                return X, Y, sg.pathwise_rollout_cand_vjp(pw, X, x0, U, gX, Y=Y)

            def calls():
                out = []
                for b in range(B):
                    X, Y = pw.rollout(x0, U[b], want_samples=True)
                    out.append((X, Y, sg.pathwise_rollout_vjp(pw, X, x0, U[b], gX[b], Y=Y)))
                return out

            peaks = [peak_mib(cand), peak_mib(calls)]                        # before the replicas of (iii) exist
            replica_bytes = 8.0 * B * (pw.Z.numel() + pw.V.numel())
            fits = replica_bytes <= args.replica_gib * 1024.0 ** 3
            rep = None
            if fits:
                rep = PathwiseSamples(pw.plan, agent, pw.omega, pw.Z.repeat(B, 1), pw.V.repeat(B, 1, 1), pw.info.repeat(B), M)
                U_rows, gX_rows = U.repeat_interleave(Ns, dim=0), gX.flatten(0, 1)

            def rows_once():
                X, Y = rep.rollout(x0, U_rows, want_samples=True)
                g0, gU, info = sg.pathwise_rollout_vjp(rep, X, x0, U_rows, gX_rows, Y=Y)
                return X, Y, (g0, gU.reshape(B, Ns, H, -1).sum(1), info)

            # parity before anything is timed: what the kernels of (i) write has the bits of (ii), pair by pair (the sums over the
            # samples are torch's and may round by the shape they are taken in: their difference is printed)
            env = agent.env_desc(None)
            Xc, Yc, (g0c, gUc, infoc) = cand()
            pair_x0, pair_U, _ = _rollout_cand_backward(pw, env, x0, U, Xc, Yc, gX)
            same, sum_dev = True, 0.0
            for b in range(B):
                Xb, Yb = pw.rollout(x0, U[b], want_samples=True)
                one_x0, one_U, one_info = _rollout_backward(pw, env, x0, U[b], Xb, Yb, gX[b])
                same = same and all(torch.equal(p, q) for p, q in ((Xc[b], Xb), (Yc[b], Yb), (pair_x0[b], one_x0), (pair_U[b], one_U),
                                                                   (infoc[b], one_info)))
                sum_dev = max(sum_dev, float((gUc[b] - one_U.sum(0)).abs().max() / one_U.sum(0).abs().max()))
            bad = int((infoc != 0).sum()) + int((pw.last_info != 0).sum())
            print(label, f"Ns {Ns} H {H} M {M} B {B}: (i) has the bits of (ii): {same}, non-finite pairs {bad}, the summed gradients differ "
                  f"by {sum_dev:.1e} of the largest", flush=True)
            if not same or bad:
                sys.exit("the candidate kernels do not reproduce the single-candidate kernels: nothing is timed")
            del Xc, Yc, g0c, gUc, infoc, pair_x0, pair_U
            fns = [cand, calls] + ([rows_once] if fits else [])
            for fn in fns:                                                   # every shape once before anything is timed
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            ms = [[] for _ in fns]
            for _ in range(args.rounds):                                     # the variants alternate: a drift of the clocks meets all of them
                for k, fn in enumerate(fns):
                    ms[k].append(block_ms(fn, args.iters))
            torch.cuda.empty_cache()
            if fits:                                                         # (iii) also needs its replicas: counted with it
                peaks.append(peak_mib(rows_once) + 8.0 * (rep.Z.numel() + rep.V.numel() + U_rows.numel()) / MIB)
            stats = [(statistics.median(v), min(v), max(v)) for v in ms]
            rows.append((label, Ns, H, M, B, stats, peaks, replica_bytes / MIB))
            print(rows[-1], flush=True)
            del rep
            torch.cuda.empty_cache()
        del agent, pw
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# gpmpc_pathwise_rollout_cand + _cand_vjp: ms per evaluation of B candidates against Ns samples\n\n")
        f.write(f"Device: {name} ({cu} CUs).  `python tools/bench_pathwise_cand.py --iters {args.iters} --rounds {args.rounds}`; device times "
                f"from events around {args.iters} back-to-back evaluations after three warm-up evaluations of every variant, the variants "
                "alternated round by round in one process; median over the rounds (lowest - highest).  An evaluation is a forward that "
                "keeps Y plus a VJP that reads it, Python wrappers, output allocations and the sum of the gradients over the samples "
                "included.  Peak MiB: what torch's allocator holds at most during one evaluation above what was allocated before it (the "
                "outputs of all B candidates alive at once), for (iii) plus its B replicas of the normals and update vectors and its "
                "per-row U.  What the kernels of (i) write was compared with (ii) bit for bit before anything was timed.  "
                "(i) / (ii): the ratio of the medians and [lowest (i) / highest (ii), highest (i) / lowest (ii)], the run's own spread.\n\n")
        f.write("| workload | Ns | H | M | B | variant | ms median (lowest - highest) | peak MiB | (i) / (ii) |\n|---|---|---|---|---|---|---|---|---|\n")
        for label, Ns, H, M, B, stats, peaks, rep_mib in rows:
            (mi, li, hi_), (mii, lii, hii) = stats[0], stats[1]
            ratio = f"{mi / mii:.3f} [{li / hii:.3f}, {hi_ / lii:.3f}]"
            for k, vname in enumerate(VARIANTS):
                if k < len(stats):
                    med, lo, hi = stats[k]
                    f.write(f"| {label} | {Ns} | {H} | {M} | {B} | {vname} | {med:.4f} ({lo:.4f} - {hi:.4f}) | {peaks[k]:.0f} | "
                            f"{ratio if k == 0 else ''} |\n")
                else:
                    f.write(f"| {label} | {Ns} | {H} | {M} | {B} | {vname} | not run: the replicas are {rep_mib:.0f} MiB | | |\n")
        f.write("\n")
        for label, Ns, H, M, B, stats, peaks, _ in rows:
            if B in (1, 16):
                (mi, li, hi_), (mii, lii, hii) = stats[0], stats[1]
                f.write(f"{label}, B = {B}: (i) / (ii) = {mi / mii:.3f}, spread [{li / hii:.3f}, {hi_ / lii:.3f}].\n\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
