#!/usr/bin/env python3
"""Time the pathwise GP samples (``gpmpc_pathwise_fit`` / ``_eval`` / ``_rollout``) next to the re-conditioned paths they stand beside,
compare the tubes, and write profiles/pathwise_bench.md.

    python tools/bench_pathwise.py [--iters 20] [--out profiles/pathwise_bench.md] [--no-joint]

Per workload (pendulum1D Ns 1024 H 30, car Ns 4096 H 40, the shipped training sets, feedback as shipped) and M in {128, 512, 1024}:
ms per launch of fit, eval (H points per sample and output, value + gradient) and rollout; the same evaluation as plain torch operations
on the device (``pathwise.torch_evaluate``, a shared point set, against the kernel on the same set); ``gpmpc_rollout`` mode R of the same
shape; the closed loop's joint draw at k = 0..3 (the output of tools/bench_joint.py, run as a child process).  Then the tubes: per-step
``hull_area_ratio`` and ``tube_coverage`` of the pathwise tube against a mode-R tube of the same Ns, and of a second mode-R tube (another
seed) against the first - the yardstick for "differs by sampling noise only".  Mode R runs here WITHOUT the beta clip and with unbounded
normals, like the pathwise samples.  Needs a HIP device."""
import argparse
import os
import subprocess
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import sampling_gpmpc_amd as sg                                              # noqa: E402
from sampling_gpmpc_amd import _lib                                          # noqa: E402
from sampling_gpmpc_amd.pathwise import PathwiseSamples, torch_evaluate      # noqa: E402
from sampling_gpmpc_amd.rollout import rollout_device                        # noqa: E402
from sampling_gpmpc_amd.workloads import closed_loop_params, synthetic_u_ff  # noqa: E402

F64 = torch.float64
WORKLOADS = (("pendulum1D", "params_pendulum1D_samples", 1024, 30), ("car", "params_car_residual", 4096, 40))
FEATURES = (128, 512, 1024)


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


def mode_r(agent, u_ff, H, seed):
    """gpmpc_rollout mode R for the agent's samples with unbounded normals of ``seed``, no clip: (callable, z)"""
    T = 1 + agent.in_dim_x
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(H, agent.ns * agent.g_ny * T, dtype=F64, generator=g).to(agent.torch_device).contiguous()
    return lambda: rollout_device(agent, u_ff, z.reshape(-1), z.shape[1], H=H, mode=_lib.MODE_RECONDITIONED,
                                  use_model_without_derivatives=False, beta=float("inf"), var_zero_thr=-1.0)


def compare(X_a, X_b, dims=(0, 1)):
    """per-step area(hull a) / area(hull b), the fraction of a's states inside b's hulls per step, and of a's whole trajectories"""
    ha, hb = sg.convex_hulls(X_a, dims=dims, layout="tube"), sg.convex_hulls(X_b, dims=dims, layout="tube")
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = sg.hull_area_ratio(ha, hb)
    per_step, whole = sg.tube_coverage(hb, X_a, dims=dims)
    return ratio, per_step, whole


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    v = v[np.isfinite(v)]
    return "-" if v.size == 0 else f"{v.min():.3f} / {np.median(v):.3f} / {v.max():.3f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pathwise_bench.md"))
    ap.add_argument("--no-joint", action="store_true", help="skip the child process that runs tools/bench_joint.py")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_pathwise.py needs a HIP device: a timing taken elsewhere says nothing about the kernels")
    name, cu, _ = _lib.device_info(0)
    timing, tubes, yard = [], [], []
    for label, yaml_name, Ns, H in WORKLOADS:
        p = closed_loop_params(yaml_name, Ns, H, 1, 1)
        p["common"]["use_cuda"] = True
        p["agent"]["base_sample_generator"] = "counter"
        agent = sg.Agent(p, sg.make_env(p))
        u_ff = synthetic_u_ff(agent.nu, H)
        x0 = torch.tensor(p["env"]["start"], dtype=F64)[:agent.nx].to("cuda")
        U = torch.as_tensor(u_ff, dtype=F64).to("cuda")
        run_r, run_r2 = mode_r(agent, u_ff, H, 1), mode_r(agent, u_ff, H, 2)
        res_r, res_r2 = run_r(), run_r2()
        torch.cuda.synchronize()
        bad = int((res_r.info != 0).sum()), int((res_r2.info != 0).sum())
        t_r = time_device(run_r, args.iters)
        kernel_r = _lib.load().gpmpc_rollout_last_kernel()
        ratio, per_step, whole = compare(res_r2.X_traj, res_r.X_traj)
        yard.append((label, Ns, H, stats(ratio[2:]), stats(per_step[2:]), whole, bad))
        print("mode R", label, t_r, "kernel", kernel_r, yard[-1], flush=True)
        for M in FEATURES:
            pw = PathwiseSamples.draw(agent, Ns, M, seed=7)
            X, Y = pw.rollout(x0, U, want_samples=True)
            sel = 0 if agent.env_model.env_id == 0 else 2
            # the points the rollout visited, as the (Ns, g_ny, H, D) tensor the closed loop would hand over
            fbu = (U[None] + (X[:, :, :H].transpose(1, 2) - torch.tensor(p["env"]["goal_state"], dtype=F64, device="cuda")[:agent.nx])
                   @ torch.tensor(p["optimizer"]["terminal_tightening"]["K"], dtype=F64, device="cuda").reshape(agent.nu, agent.nx).T)
            u_in = fbu if p["agent"]["feedback"]["use"] else U[None].expand(Ns, -1, -1)
            xi = torch.stack([X[:, sel, :H], u_in[:, :, 0]], dim=-1)[:, None].expand(-1, agent.g_ny, -1, -1).contiguous()
            shared = xi[0, 0].contiguous()                                  # (H, D)
            torch.cuda.synchronize()
            n_bad = int((pw.info != 0).sum()) + int((pw.last_info != 0).sum())
            d_torch = float((pw.evaluate(shared) - torch_evaluate(pw, shared)).abs().max())
            t_fit = time_device(lambda: PathwiseSamples._fit(pw.plan, agent, pw.omega, pw.Z, M, 7, 0), args.iters)
            t_eval = time_device(lambda: pw.evaluate(xi), args.iters)
            t_eval_s = time_device(lambda: pw.evaluate(shared), args.iters)
            t_torch = time_device(lambda: torch_evaluate(pw, shared), max(2, args.iters // 4))
            t_roll = time_device(lambda: pw.rollout(x0, U, want_samples=True), args.iters)
            timing.append((label, Ns, H, M, t_fit, t_eval, t_eval_s, t_torch, d_torch, t_roll, t_r, kernel_r, n_bad))
            ratio, per_step, whole = compare(X, res_r.X_traj)
            tubes.append((label, Ns, H, M, stats(ratio[2:]), stats(per_step[2:]), whole))
            print(timing[-1], tubes[-1], flush=True)
        del agent
        torch.cuda.empty_cache()
    joint = "not run (--no-joint)"
    if not args.no_joint:                                                    # a fresh child process; its output is quoted as it is
        r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "bench_joint.py")], capture_output=True, text=True, cwd=REPO)
        lines = [ln for ln in r.stdout.splitlines() if "sample_gp" in ln]
        joint = "\n".join(lines) if r.returncode == 0 and lines else f"not measured: tools/bench_joint.py ended with status {r.returncode}"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# Pathwise GP samples: ms per launch, and the tubes against mode R\n\n")
        f.write(f"Device: {name} ({cu} CUs).  `python tools/bench_pathwise.py --iters {args.iters}`; device times from events around "
                "back-to-back launches after three warm-up launches (every figure includes the Python wrapper's output allocations).  "
                "fit: `gpmpc_pathwise_fit` for all Ns samples; eval: `gpmpc_pathwise_eval`, value + gradient at H points per sample and "
                "output (the tensor the closed loop hands over); eval shared / torch: the kernel and the same arithmetic as plain torch "
                "operations on the device at one shared set of H points (max |difference| between the two in the next column); "
                "rollout: `gpmpc_pathwise_rollout` with Y; mode R: `gpmpc_rollout` of the same Ns and H (re-conditioned, no clip; the "
                "kernel id is `gpmpc_rollout_last_kernel()`).  non-finite: samples with an info flag in fit, eval or rollout.\n\n")
        f.write("| workload | Ns | H | M | fit ms | eval ms | eval shared ms | torch shared ms | max diff | rollout ms | mode R rollout ms | mode R kernel | non-finite |\n")
        f.write("|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in timing:
            f.write(f"| {r[0]} | {r[1]} | {r[2]} | {r[3]} | {r[4]:.4f} | {r[5]:.4f} | {r[6]:.4f} | {r[7]:.3f} | {r[8]:.1e} | {r[9]:.4f} | {r[10]:.4f} | {r[11]} | {r[12]} |\n")
        f.write("\n## The closed loop's joint draw (tools/bench_joint.py, Ns 1024)\n\n```\n" + joint + "\n```\n")
        f.write("\n## Tubes: pathwise against mode R, and mode R against mode R\n\n"
                "State dimensions (0, 1), steps 2..H (at steps 0 and 1 the sets are degenerate); min / median / max over the steps.  area ratio = "
                "area(hull of the row's tube) / area(hull of the mode-R tube, seed 1); coverage = the fraction of the row's states inside "
                "that hull per step; whole = the fraction of the row's trajectories that never leave it.  Both tubes have Ns samples, no "
                "clip, unbounded normals.\n\n")
        f.write("| workload | Ns | H | tube | area ratio | coverage per step | whole |\n|---|---|---|---|---|---|---|\n")
        for y in yard:
            f.write(f"| {y[0]} | {y[1]} | {y[2]} | mode R, seed 2 (chains with an info flag: {y[6][0]} / {y[6][1]}) | {y[3]} | {y[4]} | {y[5]:.3f} |\n")
        for t in tubes:
            f.write(f"| {t[0]} | {t[1]} | {t[2]} | pathwise, M = {t[3]} | {t[4]} | {t[5]} | {t[6]:.3f} |\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
