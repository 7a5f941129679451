#!/usr/bin/env python3
"""Time ``gpmpc_robust_tube_rollout_vjp`` (the reverse-mode gradient of the robust ellipsoidal tube, one launch) and write
profiles/robust_tube_grad_bench.md.

    python tools/bench_robust_tube_grad.py --registers-only --registers regs.json        (no GPU: compiles two files with hipcc)
    python tools/bench_robust_tube_grad.py [--rounds 7] [--iters 20] [--registers regs.json] [--bit-identity note.md] [--out ...]

Shapes: those of tools/bench_robust_tube.py (pendulum1D and car, the shipped training sets, feedback as shipped, B = 1024, H = 10,
beta = 2, shared Lipschitz constants).  Per workload, medians over ``--rounds`` rounds that alternate between the measured calls (each
round times ``--iters`` back-to-back calls between two events), with the minimum and maximum over the rounds:

* the VJP against ``gpmpc_moment_rollout_vjp`` at the same shapes and cotangents - what the adjoint of the Q recursion costs on top
  of the GP passes both kernels share -, next to the same ratio of the two forward kernels measured in the same rounds;
* forward + VJP against ``torch.autograd`` through the batched-torch recursion of tools/bench_robust_tube.py (its forward with the
  two square roots guarded, so that the gradient is finite), forward plus backward, on the device.  The kernel's gradients are
  compared with autograd's before anything is timed.

The register table is read from the metadata of the code objects hipcc emits for ``robust_tube_grad.hip`` and ``moments_grad.hip``
with the flags of csrc/build.py through tools/isa.py (``--registers-only`` stores it as JSON, a timing run embeds that file or compiles itself);
``--bit-identity`` names a markdown file whose text is copied into the report (the record of the moment VJP's bit-for-bit check).
Timing needs a HIP device."""
import argparse
import json
import os
import re
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sampling_gpmpc_amd as sg                                              # noqa: E402
from sampling_gpmpc_amd.workloads import load_params                         # noqa: E402

F64 = torch.float64
B, BETA = 1024, 2.0
KERNELS = (("robust_tube_grad.hip", "robust_tube_vjp_kernel"), ("moments_grad.hip", "moment_rollout_vjp_kernel"))
FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_spill_count", ".vgpr_spill_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


# ---------------------------------------------------------------------------------------------------------------------
# registers and scratch from the code objects' metadata
# ---------------------------------------------------------------------------------------------------------------------
def register_table():
    """{kernel: {"<env, NRP, HG>": {field: value}}} for the two VJP kernels."""
    import isa
    out = {}
    for src, kernel in KERNELS:
        rows = {}
        for name, fields in isa.metadata(open(isa.compile_to_isa(src)).read()).items():
            m = re.search(kernel + r"ILi(\d+)ELi(\d+)ELb([01])EE", name)
            if m:
                key = f"<{m.group(1)}, {m.group(2)}, {'true' if m.group(3) == '1' else 'false'}>"
                rows[key] = {f: fields[f[1:]] for f in FIELDS}
        out[kernel] = rows
    return out


def write_registers(f, regs):
    f.write("## Registers and scratch\n\n"
            "From the metadata of the code objects (`tools/isa.py`: `hipcc -S` of the device side with the flags of `csrc/build.py`; the form of "
            "`profiles/moments_step_isa.md`): `<env, NRP, HG>` with env 0 = pendulum1D, 1 = car.  VGPR counts the AGPRs in (above 256 the "
            "excess lives in AGPRs, moved by `v_accvgpr` instead of going to memory); private B is the scratch (private segment) size.\n\n")
    rv, mv = regs["robust_tube_vjp_kernel"], regs["moment_rollout_vjp_kernel"]
    f.write("| instantiation | robust VJP: VGPR | AGPR | SGPR spills | VGPR spills | private B | LDS B | moment VJP: VGPR | AGPR | SGPR spills | VGPR spills | private B |\n")
    f.write("|---|---|---|---|---|---|---|---|---|---|---|---|\n")
    for key in sorted(rv, key=lambda k: [int(v) if v.isdigit() else v for v in re.findall(r"\w+", k)]):
        a, m = rv[key], mv[key]
        f.write(f"| `{key}` | {a['.vgpr_count']} | {a['.agpr_count']} | {a['.sgpr_spill_count']} | {a['.vgpr_spill_count']} | "
                f"{a['.private_segment_fixed_size']} | {a['.group_segment_fixed_size']} | {m['.vgpr_count']} | {m['.agpr_count']} | "
                f"{m['.sgpr_spill_count']} | {m['.vgpr_spill_count']} | {m['.private_segment_fixed_size']} |\n")
    car = rv["<1, 64, false>"]
    scratch = max(v[".private_segment_fixed_size"] for v in rv.values())
    spilled = {k: v[".vgpr_spill_count"] for k, v in rv.items() if v[".vgpr_spill_count"]}
    f.write(f"\nThe instantiation to watch, the car at `NRP = 64`: {car['.vgpr_count']} VGPRs of which {car['.agpr_count']} AGPRs, "
            f"{car['.private_segment_fixed_size']} B of scratch, {car['.vgpr_spill_count']} VGPR spills.  "
            + ("No instantiation of the robust VJP uses scratch." if scratch == 0 else f"The largest private segment is {scratch} B.")
            + (f"  VGPR spill counts above zero: {spilled} (the spill slots are AGPRs where private B is 0)." if spilled else "")
            + "  Every car instantiation is above 256 VGPRs, one wave per SIMD, whatever NRP is: the peak is not in the GP passes but in "
            "the unrolled 4 x 4 adjoint behind them (A, A Q, Qbar, its cotangent, Abar, the eigenvector block), which the moment VJP "
            "has half of.  At B = 1024 there are 16 waves for 1024 SIMDs, so occupancy does not enter the timings above; it would at "
            "B >= 65536.\n")


# ---------------------------------------------------------------------------------------------------------------------
# the recursion of tools/bench_robust_tube.py with the square roots guarded: autograd gives a finite gradient
# ---------------------------------------------------------------------------------------------------------------------
def torch_robust(tr, x0, U, l_mu, l_sigma, beta):
    """``TorchRobust.__call__`` of tools/bench_robust_tube.py without in-place writes and with sqrt(0) guarded."""
    Bn, H, nx = U.shape[0], U.shape[1], tr.nx
    dev = x0.device
    mu, Q = x0, torch.zeros(Bn, nx, nx, dtype=F64, device=dev)
    M, Qs = [mu], [Q]
    eye = torch.eye(nx, dtype=F64, device=dev)
    dxi = torch.zeros(2, nx, dtype=F64, device=dev)
    dxi[0, tr.sel] = 1.0
    dxi[1] = tr.K[0]
    W = torch.linalg.cholesky(eye + tr.K.T @ tr.K).T

    def gsqrt(v):
        pos = v > 0
        return torch.where(pos, torch.sqrt(torch.where(pos, v, torch.ones_like(v))), torch.zeros_like(v))

    def outer(X, Y):
        tx, ty = torch.diagonal(X, dim1=1, dim2=2).sum(1), torch.diagonal(Y, dim1=1, dim2=2).sum(1)
        ok = (tx != 0) & (ty != 0)
        c = torch.sqrt(torch.where(ok, tx, torch.ones_like(tx)) / torch.where(ok, ty, torch.ones_like(ty)))
        both = (1.0 + 1.0 / c)[:, None, None] * X + (1.0 + c)[:, None, None] * Y
        return torch.where((ty == 0)[:, None, None], X, torch.where((tx == 0)[:, None, None], Y, both))

    zero = torch.zeros(Bn, dtype=F64, device=dev)
    for t in range(H):
        u = U[:, t] + (mu - tr.xg) @ tr.K.T
        xi = torch.stack([mu[:, tr.sel], u[:, 0]], dim=1)
        r = xi[:, None, None, :] - tr.X[None, None]
        q = r * tr.u[None, :, None, :]
        k = tr.os[None, :, None] * torch.exp(-0.5 * (r * q).sum(-1))
        ka = k * tr.alpha[None]
        m = ka.sum(-1)
        dm = -(ka[..., None] * q).sum(2)
        v = torch.einsum("oij,boj->boi", tr.Linv, k)
        s = (tr.os[None] - (v * v).sum(-1)).clamp_min(tr.floor)
        dmx = dm @ dxi
        if tr.env_id == 0:
            A = torch.stack([(eye[0] + tr.dt * eye[1]).expand(Bn, nx), eye[1] + dmx[:, 0]], dim=1)
            nxt = torch.stack([mu[:, 0] + mu[:, 1] * tr.dt, mu[:, 1] + m[:, 0]], dim=1)
            gd = torch.stack([zero, s[:, 0]], dim=1)
        else:
            vel = mu[:, 3]
            top = eye[None, :3, :] + vel[:, None, None] * dmx + m[:, :, None] * eye[3][None, None, :]
            A = torch.cat([top, (eye[3] + tr.dt * tr.K[1])[None, None, :].expand(Bn, 1, nx)], dim=1)
            nxt = torch.cat([mu[:, :3] + vel[:, None] * m, (vel + u[:, 1] * tr.dt)[:, None]], dim=1)
            gd = torch.cat([(vel * vel)[:, None] * s, zero[:, None]], dim=1)
        lam = torch.linalg.eigvalsh(W @ Q @ W.T)[:, -1]
        r2 = torch.where(lam > 0, lam, torch.zeros_like(lam))
        ub = 0.5 * l_mu * r2[:, None]
        sb = beta * (gsqrt(gd) + l_sigma * gsqrt(r2)[:, None])
        Q = outer(outer(torch.diag_embed(nx * sb * sb), torch.diag_embed(nx * ub * ub)), A @ Q @ A.transpose(1, 2))
        mu = nxt
        M.append(mu), Qs.append(Q)
    return torch.stack(M, dim=2), torch.stack(Qs, dim=1)


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
    """{name: (median, min, max)} ms per call over ``rounds`` rounds, each round timing every function once in turn."""
    for fn, _ in fns.values():
        for _ in range(3):
            fn()
    samples = {k: [] for k in fns}
    for _ in range(rounds):
        for k, (fn, div) in fns.items():
            samples[k].append(timed(fn, max(1, iters // div)))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in samples.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--registers", default=None, help="JSON of the register table (written by --registers-only, read by a timing run)")
    ap.add_argument("--registers-only", action="store_true")
    ap.add_argument("--bit-identity", default=None, help="markdown file copied into the report")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "robust_tube_grad_bench.md"))
    args = ap.parse_args()
    if args.registers_only:
        if not args.registers:
            sys.exit("--registers-only needs --registers FILE")
        with open(args.registers, "w") as f:
            json.dump(register_table(), f, indent=1, sort_keys=True)
        print("wrote", args.registers)
        return
    if not torch.cuda.is_available():
        sys.exit("bench_robust_tube_grad.py needs a HIP device: a timing taken elsewhere says nothing about the kernels")
    from bench_moments import inputs
    from bench_robust_tube import WORKLOADS, TorchRobust
    regs = json.load(open(args.registers)) if args.registers else register_table()
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
        x0, U = inputs(p, B, H, "cuda")
        tube = sg.robust_tube_rollout(agent, x0, U, l_mu, l_sigma, BETA)
        mtube = sg.moment_rollout(agent, x0, U)
        g = torch.Generator().manual_seed(7)
        gm = (torch.randn(tube.mean.shape, dtype=F64, generator=g).to("cuda") / tube.mean.abs().amax(dim=(0, 2), keepdim=True)).contiguous()
        sc = tube.cov.abs().amax(dim=(0, 2, 3), keepdim=True)
        gq = (torch.randn(tube.cov.shape, dtype=F64, generator=g).to("cuda") / torch.where(sc > 0, sc, torch.ones_like(sc))).contiguous()

        def torch_fb():
            leaves = [t.detach().clone().requires_grad_(True) for t in (x0, U, l_mu.expand(B, -1), l_sigma.expand(B, -1))]
            M, Q = torch_robust(tr, leaves[0], leaves[1], leaves[2], leaves[3], BETA)
            return torch.autograd.grad((gm * M).sum() + (gq * Q).sum(), leaves)

        got = sg.robust_tube_rollout_vjp(agent, tube, x0, U, l_mu.expand(B, -1).contiguous(), l_sigma.expand(B, -1).contiguous(), BETA,
                                         g_mean=gm, g_cov=gq)
        want = torch_fb()
        torch.cuda.synchronize()
        assert int(got[5].abs().max()) == 0
        dev = []
        for a, w in zip((got[0], got[1], got[3], got[4]), want):
            d = (a - w).abs().reshape(B, -1).amax(1) / w.abs().reshape(B, -1).amax(1).clamp_min(1e-300)
            dev.append(float(d.max()))
        fns = {"rv": (lambda: sg.robust_tube_rollout_vjp(agent, tube, x0, U, l_mu, l_sigma, BETA, g_mean=gm, g_cov=gq), 1),
               "mv": (lambda: sg.moment_rollout_vjp(agent, mtube, x0, U, None, gm, gq), 1),
               "rf": (lambda: sg.robust_tube_rollout(agent, x0, U, l_mu, l_sigma, BETA), 1),
               "mf": (lambda: sg.moment_rollout(agent, x0, U), 1),
               "torch": (torch_fb, 10)}
        t = alternating(fns, args.rounds, args.iters)
        rows.append((label, H, t, dev))
        print(label, {k: f"{v[0]:.4f} [{v[1]:.4f}, {v[2]:.4f}]" for k, v in t.items()}, [f"{d:.1e}" for d in dev], flush=True)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# gpmpc_robust_tube_rollout_vjp: ms per call, registers, and the moment VJP's bits\n\n")
        f.write(f"Device: {name} ({cu} CUs).  `python tools/bench_robust_tube_grad.py --rounds {args.rounds} --iters {args.iters}`; B = {B}, "
                f"H = 10, beta = {BETA}, Q0 = 0, shared constants, cotangents on M and Q.  Device times from events around back-to-back "
                f"calls, three warm-up calls; {args.rounds} rounds alternate between the five calls, the table gives the median and "
                "[min, max] over the rounds (the figures include the Python wrappers' output allocations; the torch form runs a tenth "
                "of the iterations per round).\n\n## Timings\n\n")
        f.write("| workload | robust VJP ms | moment VJP ms | robust forward ms | moment forward ms | torch autograd forward + backward ms |\n")
        f.write("|---|---|---|---|---|---|\n")
        for label, H, t, _ in rows:
            f.write(f"| {label} | " + " | ".join(f"{t[k][0]:.4f} [{t[k][1]:.4f}, {t[k][2]:.4f}]" for k in ("rv", "mv", "rf", "mf", "torch")) + " |\n")
        f.write("\nThe two ratios (medians):\n\n| workload | robust VJP / moment VJP | robust forward / moment forward (same rounds) | "
                "torch autograd / (robust forward + robust VJP) | robust VJP / robust forward |\n|---|---|---|---|---|\n")
        for label, H, t, _ in rows:
            f.write(f"| {label} | {t['rv'][0] / t['mv'][0]:.2f} | {t['rf'][0] / t['mf'][0]:.2f} | "
                    f"{t['torch'][0] / (t['rf'][0] + t['rv'][0]):.0f} | {t['rv'][0] / t['rf'][0]:.2f} |\n")
        f.write("\nThe first column is what the adjoint of the Q recursion costs on top of the moment VJP (the GP passes, A_t and the tail "
                "are shared); the second is the same question for the forward kernels, which profiles/robust_tube_bench.md answered with "
                "13 - 27 %.  Where the first is larger than the second the backward pays more for Q than the forward does: it runs the "
                "Jacobi sweeps with the rotations accumulated and the forward's steps 2 - 6 again before their adjoints.\n\n")
        f.write("The kernel's gradients against autograd's before timing (worst candidate, max|diff| / max|autograd| within the "
                "candidate; x0, U, l_mu, l_sigma): "
                + "; ".join(f"{label}: " + ", ".join(f"{d:.1e}" for d in dev) for label, _, _, dev in rows) + ".\n\n")
        write_registers(f, regs)
        if args.bit_identity:
            f.write("\n" + open(args.bit_identity).read().rstrip() + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
