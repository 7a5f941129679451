"""The lanes of the static steps' ONE root stream (csrc/rollout_one.hip: one_chol_rest1; tools/gen_rollout_one.py: root_lanes,
root_draw_lane -> OneRootLanes<t> in rollout_one_gen.inc).  CPU only.

In static step t the lanes A_t factor S + noise - the factor C and 1 / diag(C) that the append's selects read there - and every
other lane factors S, the root of the draw; slots 1 and 2 of the draw are taken from lane r_t.  Here A_t is derived a second
time, from what the selects MEAN rather than from the patterns' formulas: a lane of a diagonal-tile register, of its two
inverse-diagonal registers or of the panel register of the next tile row receives a value of C exactly when the entry of the
factor it holds lies in the step's three new rows and, for an entry of L, in one of the new columns at or below the diagonal.

  * for every appending step t = 0 .. 28: A_t is that union, it is not empty, and r_t lies outside it;
  * the steps whose own point lane (kPt0 + t) lies INSIDE A_t exist - the hand-over of the draw from r_t is for them - and in
    all others r_t is the point's lane itself;
  * the committed rollout_one_gen.inc holds exactly these constants (the kernel static_asserts them against its patterns).
"""
import os
import re

from tests.helpers import REPO, load_tool

NKT, NTR, T_ROWS, KPT0 = 9, 22, 3, 13


def _gen():
    return load_tool("gen_rollout_one")


def _lane(kq, bm, jq):
    return 16 * kq + 4 * bm + jq


def _expected(t):
    """A_t from the meaning of the selects; appended rows are counted from 0, tile row r holds rows 4 r .. 4 r + 3, group K holds
    the unified tiles 4 K .. 4 K + 3 of which tile NKT + r is tile row r"""
    new = range(T_ROWS * t, T_ROWS * t + T_ROWS)
    tn = new[0] // 4                                               # the incomplete tile row
    K = (NKT + tn) // 4                                            # its group
    m = 0

    def group(G):
        nonlocal m
        org = 4 * (4 * G - NKT)                                    # appended row of the group's first row (may be negative)
        for kq in range(4):
            for bm in range(4):
                for jq in range(4):
                    row, col = org + 4 * bm + jq, org + 4 * bm + kq   # L^T in the natural map: lane (kq, jq) of block bm
                    if row in new and col in new and col <= row:      # an entry of C
                        m |= 1 << _lane(kq, bm, jq)
                    if col in new:                                     # 1 / diag along the rows of L^T
                        m |= 1 << _lane(kq, bm, jq)
                    if row in new:                                     # 1 / diag along its columns
                        m |= 1 << _lane(kq, bm, jq)

    group(K)
    last_group = (NKT + NTR - 1) // 4
    if new[-1] >= 4 * (4 * (K + 1) - NKT) and K < last_group:      # rows wrapped into the next group
        group(K + 1)
    if new[-1] // 4 == tn + 1 and tn + 1 < NTR:                    # rows reach into the next tile row: its panel against tile tn
        bt = (NKT + tn) % 4
        for kq in range(4):
            for jq in range(4):
                row, col = 4 * (tn + 1) + jq, 4 * tn + kq
                if row in new and col in new and col <= row:
                    m |= 1 << _lane(kq, bt, jq)
    return m


def test_root_lanes_are_the_union_of_the_applied_selects():
    g = _gen()
    assert (g.NKT, g.NTR, g.T_ROWS, g.KPT0, g.APPEND_STEPS) == (NKT, NTR, T_ROWS, KPT0, 29)
    inside = []
    for t in range(g.APPEND_STEPS):
        a, r = g.root_lanes(t), g.root_draw_lane(t)
        pats = g.root_patterns(t)
        u = 0
        for v in pats.values():
            u |= v
        assert a == u == _expected(t), (t, hex(a), hex(u), hex(_expected(t)))
        assert a != 0 and a < (1 << 64)
        assert 0 <= r < 64 and not (a >> r) & 1, (t, r)
        if (a >> (KPT0 + t)) & 1:
            inside.append(t)
            assert r == max(l for l in range(64) if not (a >> l) & 1)
        else:
            assert r == KPT0 + t
    print("steps whose point lane factors S + noise:", inside)
    assert inside != [] and 20 in inside                          # (step 20: drow is written in lanes 32 - 35, the point sits in 33)
    # the last static step appends nothing: no lane factors S + noise
    assert g.root_lanes(g.APPEND_STEPS) == 0 and g.root_draw_lane(g.APPEND_STEPS) == KPT0 + g.APPEND_STEPS


def test_committed_include_holds_the_constants():
    g = _gen()
    text = open(os.path.join(REPO, "sampling_gpmpc_amd", "csrc", "rollout_one_gen.inc")).read()
    found = {int(t): (int(v, 16), int(d)) for t, v, d in re.findall(
        r"template <> struct OneRootLanes<(\d+)> \{ static constexpr unsigned long long value = 0x([0-9a-f]{16})ull; "
        r"static constexpr int draw = (\d+); \};", text)}
    assert found == {t: (g.root_lanes(t), g.root_draw_lane(t)) for t in range(g.APPEND_STEPS + 1)}
