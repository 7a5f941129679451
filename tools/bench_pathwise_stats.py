#!/usr/bin/env python3
"""Time the fused tube statistics (``gpmpc_pathwise_tube_stats``) against the same answer from the existing path in chunks, and write
profiles/pathwise_stats_bench.md.

    python tools/bench_pathwise_stats.py [--repeats 5] [--budget-gib 2] [--out profiles/pathwise_stats_bench.md] [--small]

Runs: pendulum1D Ns = 2^20, H = 30, M = 256; car Ns = 2^18 and 2^20, H = 40, M = 512 (the shipped training sets, feedback as shipped,
three thresholds, ``sup`` not returned).  The yardstick is the chunked existing path on the same machine and commit:
``PathwiseSamples.draw`` (normals + fit), ``.rollout``, ``tube_stats_of`` (torch reductions) per chunk and ``merge_tube_stats``; the
chunk is the largest number of samples whose tensors fit the stated memory budget (``chunk_bytes_per_sample``).  Both sides are run
once to warm up (and their results compared bit for bit), then ``--repeats`` times in alternation; each run is timed with device events
around work that ends in a synchronise.  Reported: median and min .. max of the repeats, ``torch.cuda.max_memory_allocated`` of a run of
each side, and the fused kernel's VGPR / LDS / scratch figures read from the code object in libgpmpc_hip.so.  Needs a HIP device."""
import argparse
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import isa                                                                   # noqa: E402  (beside this script)
import sampling_gpmpc_amd as sg                                              # noqa: E402
from sampling_gpmpc_amd import _lib                                          # noqa: E402
from sampling_gpmpc_amd.pathwise import (PathwiseSamples, draw_omega, merge_tube_stats, pathwise_tube_stats,   # noqa: E402
                                         tube_stats_of)
from sampling_gpmpc_amd.workloads import closed_loop_params, synthetic_u_ff  # noqa: E402

F64 = torch.float64
RUNS = (("pendulum1D", "params_pendulum1D_samples", 1 << 20, 30, 256), ("car", "params_car_residual", 1 << 18, 40, 512),
        ("car", "params_car_residual", 1 << 20, 40, 512))
SMALL = (("pendulum1D", "params_pendulum1D_samples", 1 << 12, 30, 256), ("car", "params_car_residual", 1 << 12, 40, 512))
SEED, OFFSET = 7, 0
READELF = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf")


def kernel_figures(lib_path=_lib.LIB_PATH):
    """{kernel symbol: (vgpr, agpr, lds bytes, scratch bytes per lane, sgpr spills, vgpr spills)} of the fused kernels, from the AMDGPU
    metadata notes of the gfx950 code objects bundled in the library ({} when the tools to read them are missing)."""
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    out = {}
    try:
        blob = open(lib_path, "rb").read()
        at = blob.find(magic)
        while at >= 0:
            n = struct.unpack_from("<Q", blob, at + len(magic))[0]
            pos = at + len(magic) + 8
            for _ in range(n):
                off, size, tl = struct.unpack_from("<QQQ", blob, pos)
                triple = blob[pos + 24:pos + 24 + tl].decode()
                pos += 24 + tl
                if "gfx950" not in triple or b"pathwise_tube_stats" not in blob[at + off:at + off + size]:
                    continue
                with tempfile.NamedTemporaryFile(suffix=".co") as f:
                    f.write(blob[at + off:at + off + size])
                    f.flush()
                    notes = subprocess.run([READELF, "--notes", f.name], capture_output=True, text=True, check=True).stdout
                for name, m in isa.metadata(notes).items():
                    if "pathwise_tube_stats" in name:
                        out[name] = (m["vgpr_count"], m["agpr_count"], m["group_segment_fixed_size"], m["private_segment_fixed_size"],
                                     m["sgpr_spill_count"], m["vgpr_spill_count"])
            at = blob.find(magic, at + len(magic))
    except (OSError, subprocess.CalledProcessError, KeyError, struct.error):
        return {}
    return out


def chunk_bytes_per_sample(d, M, nx, H):
    """bytes the chunked path holds per sample at its peak: the row of normals, the update vectors and info words, the tube, and the
    reductions' temporaries of the tube's size (deviation, two masked copies, the comparison for the lowest index as int64, one spare)"""
    V = d.g_ny * (M + d.N_r)
    return 8 * V + 8 * d.g_ny * d.N_r + 8 + 8 * nx * (H + 1) * 6


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    res = fn()
    b.record()
    torch.cuda.synchronize()
    return res, a.elapsed_time(b)


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def same(a, b):
    return all(torch.equal(getattr(a, f), getattr(b, f)) for f in ("dev_max", "dev_arg", "box_lo", "box_hi", "n_within", "n_nonfinite"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--budget-gib", type=float, default=2.0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pathwise_stats_bench.md"))
    ap.add_argument("--small", action="store_true", help="Ns = 4096 per run: a rehearsal of the tool, not a measurement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_pathwise_stats.py needs a HIP device: a timing taken elsewhere says nothing about the kernels")
    name, cu, _ = _lib.device_info(0)
    budget = int(args.budget_gib * (1 << 30))
    rows = []
    for label, yaml_name, Ns, H, M in (SMALL if args.small else RUNS):
        p = closed_loop_params(yaml_name, 8, H, 1, 1)
        p["common"]["use_cuda"] = True
        p["agent"]["base_sample_generator"] = "counter"
        agent = sg.Agent(p, sg.make_env(p))
        plan = agent._plan(use_grad=(agent.in_dim_y != 1))
        d = plan.desc
        x0 = torch.tensor(p["env"]["start"], dtype=F64)[:agent.nx].to("cuda")
        U = torch.as_tensor(synthetic_u_ff(agent.nu, H), dtype=F64).to("cuda")
        omega = draw_omega(plan.hyper.ell, M, SEED).to("cuda")
        centre = PathwiseSamples.draw(agent, 1, M, SEED, omega=omega).mean_only().rollout(x0, U)[0].contiguous()
        probe = pathwise_tube_stats(agent, x0, U, 4096, M, SEED, OFFSET, omega=omega, centre=centre, want_sup=True)
        eps = tuple(float(v) for v in torch.quantile(probe.sup, torch.tensor([0.25, 0.5, 0.75], dtype=F64, device="cuda")))
        chunk = max(1, min(Ns, budget // chunk_bytes_per_sample(d, M, agent.nx, H)))

        def fused():
            return pathwise_tube_stats(agent, x0, U, Ns, M, SEED, OFFSET, omega=omega, centre=centre, eps=eps)

        def chunked():
            acc = None
            for lo in range(0, Ns, chunk):
                n = min(chunk, Ns - lo)
                X = PathwiseSamples.draw(agent, n, M, SEED, OFFSET + lo, omega=omega).rollout(x0, U)
                part = tube_stats_of(X, centre, OFFSET + lo, None, eps)
                acc = part if acc is None else merge_tube_stats([acc, part])
                del X, part
            return acc

        (a, _), (b, _) = timed(fused), timed(chunked)                       # warm-up of every shape, and the answers agree
        equal = same(a, b)
        tf, tc = [], []
        for _ in range(args.repeats):                                       # alternating: drift of the machine hits both sides alike
            tf.append(timed(fused)[1])
            tc.append(timed(chunked)[1])
        mem_f, mem_c = peak_of(fused), peak_of(chunked)
        rows.append((label, Ns, H, M, chunk, np.array(tf), np.array(tc), mem_f, mem_c, equal, int(a.n_nonfinite), a.n_within.tolist()))
        print(rows[-1], flush=True)
        del agent
        torch.cuda.empty_cache()
    figs = kernel_figures()
    sp = lambda t: f"{np.median(t):.1f} ({t.min():.1f} .. {t.max():.1f})"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# Tube statistics of pathwise samples: the fused call against the chunked existing path\n\n")
        f.write(f"Device: {name} ({cu} CUs).  `python tools/bench_pathwise_stats.py --repeats {args.repeats} --budget-gib {args.budget_gib:g}"
                f"{' --small' if args.small else ''}`.  fused: one call of `gpmpc_pathwise_tube_stats` (three thresholds, `sup` not returned, "
                "the library's grid).  chunked: `PathwiseSamples.draw` (normals + fit), `.rollout`, `tube_stats_of` (torch reductions) per "
                f"chunk and `merge_tube_stats`; the chunk is the largest number of samples whose tensors fit {args.budget_gib:g} GiB by "
                "`chunk_bytes_per_sample` (normals, update vectors, tube and five tube-sized temporaries of the reductions).  Each side "
                f"is run once to warm up, then {args.repeats} times in alternation; a run is timed with device events around the whole "
                "Python call, a synchronise after it.  ms: median (min .. max).  peak: `torch.cuda.max_memory_allocated` of one run above "
                "what was allocated before it.  equal: every output of the two sides has the same bits.\n\n")
        if args.small:
            f.write("**A rehearsal at Ns = 4096: these figures measure overheads, not the kernels.**\n\n")
        f.write("| workload | Ns | H | M | fused ms | chunked ms | chunked / fused | chunk | fused peak MiB | chunked peak MiB | equal | non-finite | n_within |\n")
        f.write("|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r[0]} | {r[1]} | {r[2]} | {r[3]} | {sp(r[5])} | {sp(r[6])} | {np.median(r[6]) / np.median(r[5]):.2f} | {r[4]} | "
                    f"{r[7] / 2 ** 20:.1f} | {r[8] / 2 ** 20:.1f} | {r[9]} | {r[10]} | {r[11]} |\n")
        f.write("\n## The fused kernels in the code object\n\n")
        if figs:
            f.write("| kernel | VGPRs | AGPRs | LDS bytes per workgroup | scratch bytes per lane | SGPR spills | VGPR spills |\n|---|---|---|---|---|---|---|\n")
            for k in sorted(figs):
                f.write(f"| `{k}` | " + " | ".join(str(v) for v in figs[k]) + " |\n")
        else:
            f.write("not read: no llvm-readelf next to the ROCm installation.\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
