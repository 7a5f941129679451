"""rollout_one_kernel's prologue issues its global loads, writes the 244 panel registers (one_init needs the lane id alone) and only
then uses a loaded value: checked in the ISA hipcc emits (CPU only: hipcc cross-compiles; the marked build is the one of
tools/one_phase_mix.py, the shipped build that of csrc/build.py, both through tools/isa.py).  The pinned diagonal-tile state and
the one-instruction EXEC masks that were measured with it are not shipped (profiles/one_pinned_state.md,
tools/experiments/one_pinned_state_items_1_3.patch): their checks went with them."""
import os
import re

import pytest

from tests.helpers import load_tool

LEAN = "ILi4ELi0ELb1EEE"
isa = load_tool("isa")

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")


@pytest.fixture(scope="module")
def marked_isa():
    return open(load_tool("one_phase_mix").compile_to_isa()).read()


@pytest.fixture(scope="module")
def shipped_isa():
    return open(isa.compile_to_isa("rollout_one.hip")).read()


def _prologue(text, want, marked):
    """the kernel's instructions from its entry to the step loop: up to the prologue's mark, or (shipped build) up to the first
    MFMA - the step's solve statement"""
    for name, lines in isa.functions(text):
        if "rollout_one_kernel" in name and want in name:
            out = []
            for _, t, _ in lines[1:]:
                if t.startswith("; one_phase_end prologue") if marked else t.startswith("v_mfma"):
                    return out
                if t:
                    out.append(t)
    raise AssertionError("the prologue's end was not found in the ISA")


def test_prologue_waits_for_its_loads_behind_one_init(marked_isa, shipped_isa):
    """the LEAN instantiation - what the benchmark and RolloutRunner launch (with the optional outputs hipcc still waits for the
    start state in front of one_init: three loads are left in flight there)"""
    for flavour, text, marked in (("marked", marked_isa, True), ("shipped", shipped_isa, False)):
        pro = _prologue(text, LEAN, marked)
        loads = [i for i, t in enumerate(pro) if t.startswith("global_load")]
        writes = [i for i, t in enumerate(pro) if t.startswith("v_accvgpr_write")]
        waits = [i for i, t in enumerate(pro) if re.match(r"s_waitcnt\s+vmcnt\(\d+\)", t)]
        assert len(writes) == 244 and len(loads) >= 20 and waits, (len(writes), len(loads), len(waits))
        # every load is in flight before the first panel write, no wait for a load stands in front of the last one
        assert max(loads) < writes[0], (flavour, max(loads), writes[0])
        assert writes[-1] < waits[0], (flavour, writes[-1], waits[0])


def test_shipped_build_has_no_scratch_and_no_spills(shipped_isa):
    meta = isa.metadata(shipped_isa)
    ones = [k for k in meta if "rollout_one_kernel" in k]
    assert len(ones) == 2
    for name in ones:
        assert meta[name]["vgpr_count"] <= 512 and meta[name]["private_segment_fixed_size"] == 0, name
    for name, m in meta.items():                                    # every kernel of the file
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, name


def test_hazard_and_agpr_checks_report_nothing(shipped_isa):
    counts, problems = load_tool("check_dpp_hazard").check(isa.functions(shipped_isa), "rollout_one.hip")
    assert counts["mfma"] > 0 and counts["dpp"] > 0 and not problems, problems[:5]
    n_asm, _, problems = load_tool("check_one_agpr").check(isa.functions(shipped_isa))
    assert n_asm > 0 and not problems, problems[:5]
