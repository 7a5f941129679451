"""The EXEC masks tools/gen_rollout_one.py writes into rollout_one_gen.inc as constants (append_row_masks) against a brute-force
evaluation, lane by lane, of the run-time rule they replace; and the steps of the epochs (CPU)."""
import os
import re

import pytest

from tests.helpers import REPO, load_tool


def _gen():
    return load_tool("gen_rollout_one")


def _rule(r, n_h, b):
    """what the kernel's row_masks computed per step from the run-time n_h"""
    m_base = m_last = 0
    for lane in range(64):
        bm, jq = (lane >> 2) & 3, lane & 3
        nw = n_h <= 4 * r + jq < n_h + 3
        if nw:
            m_base |= 1 << lane
        if nw and bm < b:
            m_last |= 1 << lane
    return m_base, m_last


def _candidate_rows(g, K):
    R0 = 4 * K - g.NKT
    return range(max(R0, 0), min(R0 + 5, g.NTR))


def test_epochs_cover_every_step_once():
    g = _gen()
    expect = {2: (0, 3), 3: (4, 9), 4: (10, 14), 5: (15, 19), 6: (20, 25), 7: (26, 29)}
    seen = []
    for K in g.Map().gd:
        s = g.epoch_steps(K)
        assert (s.start, s.stop - 1) == expect[K]
        for t in s:
            assert g.epoch_of(t) == K, (t, K)
        seen += list(s)
    assert seen == list(range(30))


@pytest.mark.parametrize("t", range(29))
def test_row_masks_are_the_lane_rule(t):
    g = _gen()
    n_h = 3 * t
    K = g.epoch_of(t)
    written = []
    for r in _candidate_rows(g, K):
        got = g.append_row_masks(r, n_h)
        assert got == _rule(r, n_h, (g.NKT + r) & 3), (t, r)
        if got[0]:
            written.append(r)
    # the rows that receive lanes are the ones the step's block writes, and together they take the three new rows
    assert written == g.append_rows(t)
    assert sum(bin(g.append_row_masks(r, n_h)[0]).count("1") for r in written) == 3 * 16


def test_committed_constants_are_the_functions_values():
    g = _gen()
    text = open(os.path.join(REPO, "sampling_gpmpc_amd", "csrc", "rollout_one_gen.inc")).read()
    found = {(int(r), int(nh)): (int(b, 16), int(l, 16)) for r, nh, b, l in
             re.findall(r"OneRowMask<(\d+), (\d+)> \{ static constexpr unsigned long long base = 0x([0-9a-f]+)ull, last = 0x([0-9a-f]+)ull", text)}
    expect = {(r, 3 * t): g.append_row_masks(r, 3 * t) for t in range(29) for r in g.append_rows(t)}
    assert found == expect
