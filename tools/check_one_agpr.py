#!/usr/bin/env python3
"""rollout_one_kernel keeps a chain's factor in AGPRs a[0:243] as C++ doubles that are only ever touched through asm operands with
PHYSICAL register constraints, and some of its writes are hidden from hipcc (EXEC-masked v_accvgpr_write under uniform branches,
declared afterwards by an instruction-free statement: csrc/rollout_one.hip).  That is only sound while hipcc itself
never touches those registers between the statements: no copy (v_accvgpr_mov / read / write of its own), no live-range split, no
AGPR used as a spill slot for a VGPR.  This script compiles rollout_one.hip exactly as csrc/build.py does (tools/isa.py) and scans the ISA of
every rollout_one_kernel instantiation and of rollout_one_steps_kernel (to the function's end: the static steps leave through
s_endpgm inside asm statements, one per step): ANY instruction outside an inline-asm statement (between ;;#ASMEND and the next
;;#ASMSTART) that names an AGPR, and any scratch spill inside the kernel, is reported.  A toolchain or flag change that makes the
compiler move a panel fails here (a CPU test runs it), not in a wrong trajectory.

    python tools/check_one_agpr.py [file.s]        exit code 0 = hipcc never touches an AGPR of the kernel itself
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))     # isa.py stands beside this file, however it is loaded
import isa                                                          # noqa: E402


def compile_to_isa():
    """the shipped flavour of rollout_one.hip"""
    return isa.compile_to_isa("rollout_one.hip")


def check(functions):
    """functions: (name, lines) as isa.functions yields them; those of another kernel are passed over"""
    n_asm, n_out = 0, 0
    problems = []
    for kernel, lines in functions:
        if "rollout_one_kernel" not in kernel and "rollout_one_steps_kernel" not in kernel:
            continue
        for ln, t, in_asm in lines:
            code = isa.instruction(t)
            if code is None:
                continue
            if in_asm:
                n_asm += 1
                continue
            n_out += 1
            if re.search(r"\ba\[\d+:\d+\]|\ba\d+\b", code) or code.startswith("v_accvgpr"):
                problems.append((kernel, ln, code, "an AGPR named by a compiler-generated instruction"))
            elif code.startswith("scratch_") or code.startswith("buffer_store_dword") and "offen" in code and "s[0:3]" in code:
                problems.append((kernel, ln, code, "scratch traffic (a spill) inside the kernel"))
    return n_asm, n_out, problems


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else compile_to_isa()
    n_asm, n_out, probs = check(isa.functions(open(path).read()))
    print(f"{path}: {n_asm} instructions inside asm statements, {n_out} compiler-generated; {len(probs)} of those touch an AGPR or spill")
    for k, ln, code, why in probs[:20]:
        print(f"  line {ln}: `{code}`: {why}")
    sys.exit(1 if probs or n_asm == 0 else 0)
