"""rollout_one_kernel's prologue issues its global loads, writes the 244 panel registers (one_init needs the lane id alone) and only
then uses a loaded value: checked in the ISA hipcc emits (CPU only: hipcc cross-compiles; the marked build is the one of
tools/one_phase_mix.py, the shipped build that of csrc/build.py).  The pinned diagonal-tile state and the one-instruction EXEC
masks that were measured with it are not shipped (profiles/one_pinned_state.md, tools/experiments/one_pinned_state_items_1_3.patch):
their checks went with them."""
import importlib.util
import os
import re
import subprocess
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "sampling_gpmpc_amd", "csrc")
LEAN = "ILi4ELi0ELb1EEE"

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def marked_isa():
    return _load("one_phase_mix", os.path.join(REPO, "tools", "one_phase_mix.py")).compile_to_isa(CSRC)


@pytest.fixture(scope="module")
def shipped_isa():
    b = _load("gpmpc_build", os.path.join(CSRC, "build.py"))
    out = os.path.join(tempfile.mkdtemp(prefix="gpmpc_pinned_"), "rollout_one.s")      # (the name check_dpp_hazard.py relaxes rule M2-M4 for)
    cmd = [b.HIPCC, "-x", "hip", "-S", "--cuda-device-only", os.path.join(CSRC, "rollout_one.hip"), "-o", out] + \
        [f for f in b.FLAGS if f != "-fPIC"] + b.EXTRA_FLAGS.get("rollout_one.hip", [])
    subprocess.run(cmd, check=True, capture_output=True)
    return out


def _prologue(path, want, marked):
    """the kernel's instructions from its entry to the step loop: up to the prologue's mark, or (shipped build) up to the first
    MFMA - the step's solve statement"""
    out, inside = [], False
    for raw in open(path):
        t = raw.strip()
        m = re.match(r"^(_Z\w+):", t)
        if m:
            inside = "rollout_one_kernel" in m.group(1) and want in m.group(1)
            continue
        if not inside or not t:
            continue
        if t.startswith("; one_phase_end prologue") if marked else t.startswith("v_mfma"):
            return out
        out.append(t)
    raise AssertionError("the prologue's end was not found in the ISA")


def test_prologue_waits_for_its_loads_behind_one_init(marked_isa, shipped_isa):
    """the LEAN instantiation - what the benchmark and RolloutRunner launch (with the optional outputs hipcc still waits for the
    start state in front of one_init: three loads are left in flight there)"""
    for path, marked in ((marked_isa, True), (shipped_isa, False)):
        pro = _prologue(path, LEAN, marked)
        loads = [i for i, t in enumerate(pro) if t.startswith("global_load")]
        writes = [i for i, t in enumerate(pro) if t.startswith("v_accvgpr_write")]
        waits = [i for i, t in enumerate(pro) if re.match(r"s_waitcnt\s+vmcnt\(\d+\)", t)]
        assert len(writes) == 244 and len(loads) >= 20 and waits, (len(writes), len(loads), len(waits))
        # every load is in flight before the first panel write, no wait for a load stands in front of the last one
        assert max(loads) < writes[0], (path, max(loads), writes[0])
        assert writes[-1] < waits[0], (path, writes[-1], waits[0])


def test_shipped_build_has_no_scratch_and_no_spills(shipped_isa):
    text = open(shipped_isa).read()
    heads = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S)
    ones = [(n, b) for n, b in heads if "rollout_one_kernel" in n]
    assert len(ones) == 2
    for name, body in ones:
        f = lambda k: int(re.search(r"\.amdhsa_%s (\d+)" % k, body).group(1))
        assert f("next_free_vgpr") <= 512 and f("private_segment_fixed_size") == 0, name
    for k in ("vgpr", "sgpr"):
        counts = re.findall(r"\.%s_spill_count:\s+(\d+)" % k, text)
        assert counts and set(counts) == {"0"}, (k, counts)


def test_hazard_and_agpr_checks_report_nothing(shipped_isa):
    hz = _load("check_dpp_hazard", os.path.join(REPO, "tools", "check_dpp_hazard.py"))
    counts, problems = hz.check(shipped_isa)
    assert counts["mfma"] > 0 and counts["dpp"] > 0 and not problems, problems[:5]
    ag = _load("check_one_agpr", os.path.join(REPO, "tools", "check_one_agpr.py"))
    n_asm, _, problems = ag.check(shipped_isa)
    assert n_asm > 0 and not problems, problems[:5]
