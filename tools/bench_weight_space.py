#!/usr/bin/env python3
"""Time ``gpmpc_ws_condition`` (conditioning the weight-space samples and their shared state on a block of k measurements) and write
profiles/weight_space_bench.md.

    python tools/bench_weight_space.py [--iters 20] [--rounds 7] [--out profiles/weight_space_bench.md]

Two workloads (car Ns 4096, M 512, g_ny 3; pendulum1D Ns 1024, M 256; the shipped training sets conditioned on first).  Per workload
and k = 1, 16, 64, ms per call of
  (i)   ``gpmpc_ws_condition`` (``WeightSpaceSamples._condition_block``: the seven launches and the wrapper's allocations), and the same
        call for the state alone (Ns = 0): the difference is the sample update, reported as its share of the call and as bytes per
        second against 2 Ns g_ny M 8 B;
  (ii)  the same arithmetic in torch operations on the device (``tests/weight_space_reference.py``, ``torch_condition``: ``addmm`` / ``cholesky`` /
        ``cholesky_solve``, rocBLAS and rocSOLVER behind them);
and once per workload
  (iii) re-conditioning from the prior on all data seen so far - what the reference does at every step (``train_BLR_multioutput`` +
        ``sample_weights``) - at the real data + 50 measurements: as one torch batch, and as blocks of at most 64 through (i).
The kernel's result is compared with the torch statement's before anything is timed - a deviation above 8 x the worst A-against-B
figure the device test records for the workload's shipped case ends the run.  Timing: device events around ``iters`` back-to-back
calls, every variant warmed up first, the variants alternated round by round in one process; the median over the rounds and their
lowest and highest value are reported.  The registers of the code object come from compiling csrc/weight_space.hip with the build's
flags (tools/isa.py).  Needs a HIP device."""
import argparse
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import isa                                                                   # noqa: E402
import sampling_gpmpc_amd as sg                                              # noqa: E402
from sampling_gpmpc_amd import _lib                                          # noqa: E402
from sampling_gpmpc_amd.weight_space import WeightSpaceSamples             # noqa: E402
from sampling_gpmpc_amd.workloads import closed_loop_params                  # noqa: E402
from tests.test_weight_space_host import WORST_AB                            # noqa: E402
from tests.weight_space_reference import torch_condition                     # noqa: E402

F64 = torch.float64
WORKLOADS = (("car", "params_car_residual", "car_fb", 4096, 512), ("pendulum1D", "params_pendulum1D_samples", "pend_fb", 1024, 256))
KS = (1, 16, 64)
N_SEEN = 50


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


def measurements(agent, n, seed):
    """n scattered GP inputs inside the training data's box and the plant's labels there: (X (n, D), Y (g_ny, n))"""
    X_r = agent.Dyn_gp_X_train.to("cuda")
    lo, hi = X_r.amin(0), X_r.amax(0)
    g = torch.Generator().manual_seed(seed)
    X = lo + (hi - lo) * torch.rand(n, X_r.shape[1], dtype=F64, generator=g).to("cuda")
    return X, agent.env_model.get_prior_data(X)[:, :, 0].to("cuda").contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "weight_space_bench.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_weight_space.py needs a HIP device: a timing taken elsewhere says nothing about the kernel")
    name, cu, _ = _lib.device_info(0)
    rows, refits = [], []
    for label, yaml_name, case, Ns, M in WORKLOADS:
        p = closed_loop_params(yaml_name, Ns, 10, 1, 1)
        p["common"]["use_cuda"] = True
        p["agent"]["base_sample_generator"] = "counter"
        agent = sg.Agent(p, sg.make_env(p))
        limit = 8.0 * max(max(v[q] for q in ("mu", "P", "W")) for k, v in WORST_AB.items() if k[0] == case)
        ws = WeightSpaceSamples.draw(agent, Ns, M, seed=7)
        state = WeightSpaceSamples.draw(agent, 0, M, seed=7)                 # the state alone
        d, s2 = ws.plan.desc, float(ws.plan.desc.noise[0])
        for k in KS:
            X, Y = measurements(agent, k, 100 + k)
            E = ws.measurement_normals(0, k)
            probe = WeightSpaceSamples.draw(agent, Ns, M, seed=7)            # a fresh state: the timed one has moved on
            want = torch_condition(probe.omega, probe.plan.hyper, s2, probe.mu, probe.P, probe.weights(), X, Y, E)
            probe._condition_block(X, Y, E)
            torch.cuda.synchronize()
            devs = [deviation(w, g) for w, g in zip(want[:3], (probe.mu, probe.P, probe.weights()))]
            bad = int((probe.last_condition_info != 0).sum()) + int((probe.last_info_state != 0).sum())
            print(label, Ns, M, k, "kernel against the torch statement: mu %.1e  P %.1e  W %.1e  limit %.1e  flagged %d" % (*devs, limit, bad),
                  flush=True)
            if max(devs) > limit or bad:
                sys.exit(f"the kernel's update differs from the torch statement's by more than {limit:.1e}: nothing is timed")
            del probe, want
            Wc = ws.weights().contiguous()
            fns = (lambda: ws._condition_block(X, Y, E), lambda: state._condition_block(X, Y, None),
                   lambda: torch_condition(ws.omega, ws.plan.hyper, s2, ws.mu, ws.P, Wc, X, Y, E))
            for fn in fns:
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            ms = [[] for _ in fns]
            for _ in range(args.rounds):                                     # the variants alternate: a drift of the clocks meets all of them
                for i, fn in enumerate(fns):
                    ms[i].append(block_ms(fn, args.iters))
            if int((ws.last_info_state != 0).sum()) or not bool(torch.isfinite(ws.P).all()):
                sys.exit("the timed state left the admissible range: the timings say nothing")
            rows.append((label, Ns, M, d.g_ny, k, [(statistics.median(v), min(v), max(v)) for v in ms], devs))
            print(rows[-1], flush=True)
        # (iii) from the prior on everything seen so far
        Xs, Ys = measurements(agent, N_SEEN, 999)
        X_all = torch.cat([ws.plan.X_r, Xs])
        Y_all = torch.cat([ws.plan.Y_r[:, :, 0], Ys], dim=1).contiguous()
        n_all = int(X_all.shape[0])
        prior = WeightSpaceSamples.draw(agent, Ns, M, seed=7, condition_on_real=False)
        Z0 = prior.Z.clone()
        E_all = torch.randn(Ns, d.g_ny, n_all, dtype=F64, generator=torch.Generator().manual_seed(5)).to("cuda")
        mu0, P0, W0 = prior.mu.clone(), prior.P.clone(), prior.weights().contiguous()

        def refit_kernel():
            prior.Z.copy_(Z0), prior.mu.zero_(), prior.P.copy_(P0)
            for j0 in range(0, n_all, 64):
                prior._condition_block(X_all[j0:j0 + 64], Y_all[:, j0:j0 + 64], E_all[:, :, j0:j0 + 64])

        fns = (refit_kernel, lambda: torch_condition(prior.omega, prior.plan.hyper, s2, mu0, P0, W0, X_all, Y_all, E_all))
        for fn in fns:
            for _ in range(3):
                fn()
        ms = [[] for _ in fns]
        for _ in range(args.rounds):
            for i, fn in enumerate(fns):
                ms[i].append(block_ms(fn, max(2, args.iters // 4)))
        refits.append((label, Ns, M, n_all, [(statistics.median(v), min(v), max(v)) for v in ms]))
        print(refits[-1], flush=True)
        del agent, ws, state, prior
        torch.cuda.empty_cache()

    meta = isa.metadata(open(isa.compile_to_isa("weight_space.hip")).read())
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    fmt = lambda t: f"{t[0]:.4f} ({t[1]:.4f} - {t[2]:.4f})"
    with open(args.out, "w") as f:
        f.write("# gpmpc_ws_condition: ms per call\n\n")
        f.write(f"Device: {name} ({cu} CUs).  `python tools/bench_weight_space.py --iters {args.iters} --rounds {args.rounds}`; device times "
                f"from events around {args.iters} back-to-back calls after three warm-up calls of every variant, the variants alternated "
                "round by round in one process; median over the rounds (lowest - highest).  Every figure includes its Python wrapper "
                "(output and workspace allocations).  (i) the call with the samples, (i0) the state alone (Ns = 0), (ii) the same arithmetic "
                "in torch operations (addmm / cholesky / cholesky_solve).  Sample update: (i) - (i0), its share of (i) and its rate against "
                "2 Ns g_ny M 8 B (W read and written once).  dev: the kernel against (ii), max|diff| / max|value| of mu, P, W, taken before "
                "anything was timed.\n\n")
        f.write("| workload | Ns | M | g_ny | k | (i) gpmpc_ws_condition | (i0) state alone | (ii) torch | (ii) / (i) | sample update ms | share | GB/s | dev mu / P / W |\n")
        f.write("|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for label, Ns, M, g_ny, k, t, devs in rows:
            upd = t[0][0] - t[1][0]
            gbs = 2.0 * Ns * g_ny * M * 8 / (upd * 1e-3) / 1e9 if upd > 0 else float("nan")
            f.write(f"| {label} | {Ns} | {M} | {g_ny} | {k} | {fmt(t[0])} | {fmt(t[1])} | {fmt(t[2])} | {t[2][0] / t[0][0]:.2f} | {upd:.4f} | "
                    f"{upd / t[0][0]:.0%} | {gbs:.0f} | {devs[0]:.1e} / {devs[1]:.1e} / {devs[2]:.1e} |\n")
        f.write("\n## (iii) re-conditioning from the prior on all data seen so far\n\nWhat the reference does before every solve, at the real "
                f"data + {N_SEEN} measurements: the kernel in blocks of at most 64 (the copies that reset the state included), and one torch "
                "batch.  Against it stands ONE call of (i) with the step's k from the table above.\n\n")
        f.write("| workload | Ns | M | points | gpmpc_ws_condition in blocks | torch, one batch |\n|---|---|---|---|---|---|\n")
        for label, Ns, M, n_all, t in refits:
            f.write(f"| {label} | {Ns} | {M} | {n_all} | {fmt(t[0])} | {fmt(t[1])} |\n")
        f.write("\n## The code object\n\ncsrc/weight_space.hip compiled with the build's flags (tools/isa.py):\n\n")
        f.write("| kernel | VGPRs | AGPRs | scratch bytes / lane | LDS bytes |\n|---|---|---|---|---|\n")
        for kname, m in sorted(meta.items()):
            if "ws_" in kname:
                f.write(f"| `{kname}` | {m.get('vgpr_count', '?')} | {m.get('agpr_count', '?')} | {m.get('private_segment_fixed_size', '?')} | "
                        f"{m.get('group_segment_fixed_size', '?')} |\n")
        f.write("\nThe sample update is the MFMA form (16 samples per workgroup on the tiles' independent axis).  A one-sample-per-wave VALU "
                "form was not built, so no number stands against it here: UNMEASURED.\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
