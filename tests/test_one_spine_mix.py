"""The sample phase of rollout_one_kernel's step (between the marks "Gram + extract" and "sample" of tools/one_phase_mix.py) after
the bookkeeping left its spine (profiles/one_spine.md): one exponent formula for axis lanes and point lanes instead of two EXEC
regions, the INFO_VAR_CLAMPED test as a running minimum that is read once behind the step loop, the variance floor in the cold
block.  CPU only: hipcc cross-compiles rollout_one.hip with the phase marks (tools/isa.py: about a minute, once per pytest process
whichever test asks first).

Bounds: the counts of the commit before this change (profiles/one_append_steps.md, "change" table: 216 instructions in the
epoch K = 2, 207 in every later one); the phase has to stay below them.
"""
import re

import pytest

from tests.helpers import load_tool

PARENT_SAMPLE = {2: 216, 3: 207, 4: 207, 5: 207, 6: 207, 7: 207}
LEAN = "ILi4ELi0ELb1EEE"


@pytest.fixture(scope="module")
def sample_phases():
    """{epoch K: [instruction text, ...]} of the sample phase, by the attribution rule of one_phase_mix.scan: what stands between
    two marks belongs to the phase the second one ends; the epoch advances at every mark "7"."""
    mix, isa = load_tool("one_phase_mix"), load_tool("isa")
    phases, cur, started, k = {}, [], False, mix.KFIRST
    for _, t, _ in mix.kernel_lines(mix.compile_to_isa(), lambda name: "rollout_one_kernel" in name and LEAN in name):
        m = re.match(r"^; one_phase_(\w+) (\w+)", t)
        if m:
            kind, what = m.groups()
            if kind == "end" and what == "prologue":
                started = True
            elif kind == "end" and what == "4":
                assert k not in phases, f"two sample phases in epoch K = {k}"
                phases[k] = cur
            elif kind == "end" and what == "7":
                k += 1
            cur = []
            continue
        code = isa.instruction(t)
        if started and code is not None:
            cur.append(code)
    return phases


def test_every_epoch_has_a_sample_phase(sample_phases):
    assert sorted(sample_phases) == sorted(PARENT_SAMPLE)


@pytest.mark.parametrize("K", sorted(PARENT_SAMPLE))
def test_sample_phase_is_shorter_than_the_parents(sample_phases, K):
    n = len(sample_phases[K])
    print(f"K = {K}: {n} instructions in the sample phase (parent {PARENT_SAMPLE[K]})")
    assert n < PARENT_SAMPLE[K]


@pytest.mark.parametrize("K", sorted(PARENT_SAMPLE))
def test_sample_phase_has_no_exec_region(sample_phases, K):
    """the two-sided `lane < kPt0 ? ... : ...` of ent_a was s_and_saveexec / s_andn2_saveexec around 15 VALU instructions"""
    hits = [c for c in sample_phases[K] if c.startswith("s_and_saveexec")]
    assert not hits, hits


@pytest.mark.parametrize("K", sorted(PARENT_SAMPLE))
def test_sample_phase_has_no_canonicalising_maximum(sample_phases, K):
    """v_max_f64 x, y, y: the copies the library's fmax / fmin put in front of their operands"""
    hits = []
    for c in sample_phases[K]:
        m = re.match(r"^v_max_f64(?:_e\d+)?\s+([^,]+),\s*([^,]+),\s*([^,\s]+)", c)
        if m and m.group(2).strip() == m.group(3).strip():
            hits.append(c)
    assert not hits, hits
