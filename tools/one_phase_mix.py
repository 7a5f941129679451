#!/usr/bin/env python3
"""Static instruction mix of rollout_one_kernel per epoch and phase of the step (CPU only: hipcc cross-compiles).

Compiles rollout_one.hip to assembly with the flags of csrc/build.py plus -DGPMPC_ONE_PHASE_MARKS, which turns the phase
timers' positions (OPH(i): the phase that ENDS there) and the bounds of the cold block into comments of the ISA, and counts the
instructions between the marks of the LEAN instantiation (--full: the other one) by class:

    VALU (every v_* but the MFMAs; v_cmp / v_cndmask / DPP / v_accvgpr_write are counted again in columns of their own),
    MFMA, SALU (s_* without branches, s_nop and s_waitcnt), branch, s_nop, LDS (ds_*), wait (s_waitcnt), mem (global / flat / SMEM)

The marks are asm statements: like the timers they fence the scheduler, so the counts are those of the marked build - a few
instructions off the shipped one.  The attribution is by position in the file: code between two marks belongs to the phase the
second one ends.  The step blocks of the append (one per step t) each carry their own marks; their counts are summed over
the blocks of the epoch, and `blocks` says how many there are - a step runs ONE of them.

    python tools/one_phase_mix.py [--full] [--src DIR]      DIR: another csrc directory (e.g. a checkout of the parent commit)
    python tools/one_phase_mix.py --steps                   rollout_one_steps_kernel: the mix of every static step's body (scan_steps)
"""
import collections
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))     # isa.py stands beside this file, however it is loaded
import isa                                                          # noqa: E402

CSRC = isa.CSRC
PHASES = {"0": "entries: LDS reads", "1": "entries: products + writes", "2": "solve", "3": "Gram + extract", "4": "sample",
          "5": "append: panel writes", "6": "append: diagonal tiles", "7": "state"}
COLS = ["VALU", "v_cmp", "v_cndmask", "DPP", "v_accvgpr_write", "MFMA", "SALU", "branch", "s_nop", "LDS", "wait", "mem"]
KFIRST = 2


def compile_to_isa(csrc=CSRC):
    """the marked flavour: the shared compile with the phase marks switched on"""
    return isa.compile_to_isa("rollout_one.hip", ("-DGPMPC_ONE_PHASE_MARKS",), csrc)


def classes(op, text):
    if op.startswith("v_mfma"):
        return ["MFMA"]
    if op.startswith("v_"):
        c = ["VALU"]
        if op.startswith("v_cmp"):
            c.append("v_cmp")
        if op.startswith("v_cndmask"):
            c.append("v_cndmask")
        if "_dpp" in op or " row_" in text or "quad_perm" in text:
            c.append("DPP")
        if op.startswith("v_accvgpr_write"):
            c.append("v_accvgpr_write")
        return c
    if op.startswith("ds_"):
        return ["LDS"]
    if op in ("s_branch", "s_setpc_b64") or op.startswith("s_cbranch"):
        return ["branch"]
    if op == "s_nop":
        return ["s_nop"]
    if op == "s_waitcnt":
        return ["wait"]
    if op.startswith(("global_", "flat_", "buffer_", "scratch_", "s_load", "s_buffer_load")):
        return ["mem"]
    if op.startswith("s_"):
        return ["SALU"]
    return []


def kernel_lines(path, want):
    """the lines (isa.functions) of the kernels of an .s whose mangled name `want` accepts"""
    for name, lines in isa.functions(open(path).read()):
        if want(name):
            yield from lines


def scan(path, lean=True):
    want = "ILi4ELi0ELb1EEE" if lean else "ILi4ELi0ELb0EEE"
    table = collections.OrderedDict()           # (epoch label, phase label) -> Counter
    blocks = collections.Counter()              # epoch label -> marks "1" seen (step blocks)
    epoch = "prologue"
    pending = collections.Counter()
    code_len = None

    def flush(key):
        nonlocal pending
        table.setdefault(key, collections.Counter()).update(pending)
        pending = collections.Counter()

    k = KFIRST
    for _, t, _ in kernel_lines(path, lambda name: "rollout_one_kernel" in name and want in name):
        if t.startswith("; codeLenInByte"):
            code_len = int(t.split("=")[1])
            continue
        m = re.match(r"^; one_phase_(\w+) (\w+)", t)
        if m:
            kind, what = m.groups()
            if kind == "end" and what == "prologue":
                flush(("prologue", "kernel entry .. step loop"))
                epoch = f"K = {k}"
            elif kind == "cold" and what == "begin":
                flush((epoch, "(between the marks: loop control, joins)"))
            elif kind == "cold" and what == "end":
                flush((epoch, "cold block (clip, repair)"))
            elif kind == "end":
                flush((epoch, PHASES[what]))
                if what == "1":
                    blocks[epoch] += 1
                if what == "7":
                    k += 1
                    epoch = f"K = {k}"
            continue
        code = isa.instruction(t)
        if code is None:
            continue
        op = code.split()[0]
        pending.update(classes(op, code))
        pending["all"] += 1
    flush(("epilogue", "behind the last mark (rare paths of the last epoch, epilogue)"))
    return table, blocks, code_len


def scan_steps(path, n_steps=30):
    """rollout_one_steps_kernel (one body per step index): its own marks are `; one_steps_head <t>` where the body of step t
    begins; the rare blocks (root retry, cold block, the launch's end with the epilogue) stand behind the last body.  Returns
    (per step t the Counter of the instructions between its head and the next one - the last body ends at its s_endpgm -,
    the Counter of what stands behind the bodies, codeLenInByte, spine) with spine = [(line number, code, step or None)] of
    everything from the prologue's end to the last body's end, for the checks on the spine's branches."""
    steps, tail, spine = collections.OrderedDict(), collections.Counter(), []
    cur, done, code_len, started = None, False, None, False
    for ln, t, _ in kernel_lines(path, lambda name: "rollout_one_steps_kernel" in name):
        if t.startswith("; codeLenInByte"):
            code_len = int(t.split("=")[1])
            continue
        if t.startswith("; one_phase_end prologue"):
            started = True
            continue
        m = re.match(r"^; one_steps_head (\d+)", t)
        if m:
            cur = int(m.group(1))
            steps[cur] = collections.Counter()
            continue
        code = isa.instruction(t)
        if code is None:
            continue
        if started and not done:
            spine.append((ln, code, cur))
        op = code.split()[0]
        c = tail if (done or cur is None) else steps[cur]
        c.update(classes(op, code))
        c["all"] += 1
        if op == "s_endpgm" and cur == n_steps - 1 and not done:
            done = True
    return steps, tail, code_len, spine


def main():
    if "--steps" in sys.argv:
        path = compile_to_isa()
        steps, tail, code_len, _ = scan_steps(path)
        print(f"{path}: rollout_one_steps_kernel<4, pendulum1D>, codeLenInByte = {code_len}\n")
        print("| step | all | " + " | ".join(COLS) + " |")
        print("|---|---|" + "---|" * len(COLS))
        for t, c in list(steps.items()) + [("behind the bodies", tail)]:
            print(f"| {t} | {c['all']} | " + " | ".join(str(c[k]) for k in COLS) + " |")
        return
    csrc = os.path.abspath(sys.argv[sys.argv.index("--src") + 1]) if "--src" in sys.argv else CSRC
    path = compile_to_isa(csrc)
    table, blocks, code_len = scan(path, lean="--full" not in sys.argv)
    print(f"{path}: rollout_one_kernel<4, pendulum1D, {'LEAN' if '--full' not in sys.argv else 'full'}>, codeLenInByte = {code_len}\n")
    print("| epoch | phase | all | " + " | ".join(COLS) + " |")
    print("|---|---|---|" + "---|" * len(COLS))
    last = None
    for (epoch, phase), c in table.items():
        if c["all"] == 0:
            continue
        label = epoch
        if epoch != last and blocks.get(epoch):
            label += f" ({blocks[epoch]} step block{'s' if blocks[epoch] > 1 else ''})"
        last = epoch
        print(f"| {label} | {phase} | {c['all']} | " + " | ".join(str(c[k]) for k in COLS) + " |")


if __name__ == "__main__":
    main()
