"""The ISA of rollout_one_steps_kernel - one body per step index, laid out as a straight line (csrc/rollout_one.hip).  CPU only:
hipcc cross-compiles rollout_one.hip (tools/isa.py: once per flavour and pytest process), as csrc/build.py ships it (resources, the AGPR and hazard checks) and with
-DGPMPC_ONE_PHASE_MARKS (tools/one_phase_mix.py: scan_steps reads the steps' own marks) for the shape of the spine:

  * the shipped build has exactly one rollout_one_steps_kernel, without scratch and without a spilled register, within
    252 VGPRs + 244 AGPRs; the two rollout_one_kernel instantiations are still there;
  * hipcc touches no AGPR of the new kernel itself and the distance rules hold in it (tools/check_one_agpr.py,
    tools/check_dpp_hazard.py);
  * thirty bodies, t = 0 .. 29 in order; from the prologue's end to the last body's end no branch goes backward, and a body holds
    at most ONE conditional branch - the shared entry of its rare blocks (root retry, cold block, the launch's end), which stand
    behind the last body.  The last body (t = 29) ends every launch that reaches it: its rare blocks are its tail, and the
    spine is read up to their entry;
  * a body's solve statement holds no branch at all, and no body compares against the row count.
"""
import re

import pytest

from tests.helpers import load_tool

STEPS_NAME = "rollout_one_steps_kernel"
isa = load_tool("isa")


@pytest.fixture(scope="module")
def shipped():
    return open(isa.compile_to_isa("rollout_one.hip")).read()


@pytest.fixture(scope="module")
def marked():
    mix = load_tool("one_phase_mix")
    path = mix.compile_to_isa()
    return path, mix.scan_steps(path)


def test_one_steps_kernel_without_scratch_or_spills(shipped):
    meta = isa.metadata(shipped)
    steps = [k for k in meta if STEPS_NAME in k]
    loops = [k for k in meta if "rollout_one_kernel" in k]
    print({k: (v["vgpr_count"], v["agpr_count"], v["private_segment_fixed_size"]) for k, v in meta.items()})
    assert len(steps) == 1 and len(loops) == 2
    assert not [k for k in steps if "rollout_one_kernel" in k]
    for k in steps + loops:
        assert meta[k]["private_segment_fixed_size"] == 0, k
        assert meta[k]["vgpr_spill_count"] == 0 and meta[k]["sgpr_spill_count"] == 0, k
    assert meta[steps[0]]["vgpr_count"] <= 252 + 244
    assert meta[steps[0]]["agpr_count"] <= 244


def test_compiler_leaves_the_panels_alone_and_distances_hold(shipped):
    alone = [f for f in isa.functions(shipped) if STEPS_NAME in f[0]]      # the new kernel alone
    assert len(alone) == 1
    n_asm, n_out, problems = load_tool("check_one_agpr").check(alone)
    print(f"{n_asm} instructions inside asm statements, {n_out} compiler-generated, {len(problems)} touch an AGPR or spill")
    assert n_asm > 10000 and n_out > 10000 and problems == []
    counts, hazards = load_tool("check_dpp_hazard").check(alone, "rollout_one.hip")
    print(f"{counts['dpp']} DPP reads and {counts['mfma']} MFMAs checked, {len(hazards)} hazard(s)")
    assert counts["mfma"] > 1000 and hazards == []


BR = re.compile(r"^(s_cbranch_\w+|s_branch)\s+(\S+)$")
FAR = re.compile(r"^s_add_u32 .*\((\.LBB\w+)-\.Lpost_getpc\d+\)")


def test_spine_is_a_straight_line(marked):
    path, (steps, tail, code_len, spine) = marked
    assert list(steps) == list(range(30))
    lines = [x for _, fl in isa.functions(open(path).read()) for x in fl]        # of every function of the file
    labels = {}
    for ln, tx, _ in lines:
        m = re.match(r"^(\.LBB\w+):", tx)
        if m:
            labels.setdefault(m.group(1), []).append(ln)
    lo, hi = spine[0][0], spine[-1][0]

    def target(name, ln):
        c = labels.get(name, [])
        assert len(c) == 1, name                                    # (the function's number is part of a label: unique in the file)
        return c[0]

    cond = {t: 0 for t in steps}
    backward, in_solve = [], []
    for ln, code, t in spine:
        if t == max(steps) and code.startswith("s_cbranch"):        # the last body's tail: its rare blocks and the epilogue
            hi = ln
            break
        m = BR.match(code) or FAR.match(code)
        if m:
            name = m.group(2) if m.re is BR else m.group(1)
            tl = target(name, ln)
            if tl <= ln:
                backward.append((ln, code))
        if code.startswith("s_cbranch") and t is not None:
            cond[t] += 1
    # a solve statement = the asm statement that holds the body's MFMAs with a panel operand: no control flow inside
    has_panel, ctrl = False, []
    for ln, tx, in_asm in lines:
        if not lo <= ln <= hi:
            continue
        if in_asm:
            if re.match(r"^v_mfma_f64_4x4x4_4b_f64 v\[\d+:\d+\], a\[", tx):
                has_panel = True
            if tx.startswith(("s_cbranch", "s_branch", "s_cmp", "s_setpc")) or re.match(r"^\.L\w+:", tx):
                ctrl.append(tx)
        else:                                                       # a statement's bounds, or what stands between two
            if has_panel and ctrl:
                in_solve.append(ctrl)
            has_panel, ctrl = False, []
    print(f"codeLenInByte = {code_len}; conditional branches per body: {sorted(set(cond.values()))}; "
          f"instructions per body {min(c['all'] for c in steps.values())} .. {max(c['all'] for c in steps.values())}, "
          f"{tail['all']} behind the bodies")
    assert backward == []
    assert max(cond.values()) <= 1, cond
    assert in_solve == []
    # the bodies' branch instructions in all (the one conditional branch and the long jump it skips): the loop form runs 13 per step
    assert max(c["branch"] for t, c in steps.items() if t < max(steps)) <= 2
