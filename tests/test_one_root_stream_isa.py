"""The static bodies of rollout_one_steps_kernel after the two 3 x 3 roots became ONE stream and the selects on lane conditions that
are literals of the step became moves under literal EXEC masks (csrc/rollout_one.hip; profiles/one_root_stream.md).  CPU only: one
cross compile with csrc/build.py's flags and -DGPMPC_ONE_PHASE_MARKS, read by tools/one_phase_mix.py: scan_steps.

  * every body that appends (t = 0 .. 28) holds exactly four v_rsq_f64 on its spine - the two first pivots and ONE stream's second
    and third (six before: two streams).  The last body (t = 29) appends nothing, so nothing reads the root of S + noise and its
    first pivot is not computed either: three;
  * no body holds more v_cndmask_b32, v_cmp or VALU instructions than the parent's body of the same step.  PARENT is the table of
    `python tools/one_phase_mix.py --steps` on the parent commit (VALU, v_cmp, v_cndmask per step);
  * the marked build has no scratch, spills nothing and stays within 252 VGPRs + 244 AGPRs (tests/test_one_steps_isa.py checks the
    shipped build's resources, the AGPR rule and the DPP / MFMA distances).
"""
import pytest

from tests.helpers import load_tool

# the parent commit: (VALU, v_cmp, v_cndmask_b32) of the static body of step t
PARENT = [(279, 12, 27), (278, 12, 23), (291, 12, 23), (293, 12, 23), (288, 12, 23), (312, 12, 23), (324, 12, 23), (319, 12, 23),
          (326, 12, 23), (373, 12, 23), (350, 12, 23), (355, 12, 23), (354, 12, 23), (385, 12, 23), (413, 12, 23), (386, 12, 23),
          (390, 12, 23), (415, 12, 23), (424, 12, 23), (431, 12, 23), (425, 12, 23), (445, 12, 23), (459, 12, 23), (449, 12, 23),
          (458, 12, 23), (500, 12, 23), (489, 12, 23), (485, 12, 23), (474, 11, 22), (502, 22, 16)]


@pytest.fixture(scope="module")
def marked():
    mix = load_tool("one_phase_mix")
    path = mix.compile_to_isa()
    return path, mix.scan_steps(path)


def test_four_rsq_per_appending_body(marked):
    _, (steps, _, _, spine) = marked
    n = {t: 0 for t in steps}
    for _, code, t in spine:
        if t == max(steps) and code.startswith("s_cbranch"):       # the last body's rare blocks are its tail
            break
        if t is not None and code.startswith("v_rsq_f64"):
            n[t] += 1
    print(n)
    assert list(steps) == list(range(30))
    assert [n[t] for t in range(29)] == [4] * 29
    assert n[29] == 3


def test_no_body_holds_more_selects_compares_or_valu_than_the_parents(marked):
    _, (steps, _, _, _) = marked
    worse = []
    for t, c in steps.items():
        now = (c["VALU"], c["v_cmp"], c["v_cndmask"])
        print(t, "parent", PARENT[t], "now", now)
        if any(a > b for a, b in zip(now, PARENT[t])):
            worse.append((t, PARENT[t], now))
    assert worse == []


def test_marked_build_without_scratch_or_spills(marked):
    path, _ = marked
    meta = load_tool("isa").metadata(open(path).read())
    ks = [k for k in meta if "rollout_one_steps_kernel" in k]
    assert len(ks) == 1
    k = meta[ks[0]]
    print({x: k[x] for x in ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")})
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0
    assert k["vgpr_count"] <= 252 + 244 and k["agpr_count"] <= 244
