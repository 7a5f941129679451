"""The inverse of group K's diagonal tiles inside one_solve<K> (tools/gen_rollout_one.py: solve_stmt, inverse_ops).  CPU only: the
generator's text of the statements K = 2 .. 7 is read, nothing is compiled.

For K = 3 .. 7 the three MFMAs of the inverse (M^T, M M, (I + M)(I + M^2): the statement's only MFMAs with C = 0 whose A operand
is an ordinary register and differs from B - a Gram product multiplies a register with itself) and the two v_accvgpr_write of
gd[K]'s register pair stand exactly once in the statement, in front of the first MFMA that reads gd[K] as its A operand: on
every path through the statement, because they stand in front of its first branch.  The statement of K = 2 holds none of them.
"""
import io
import re

import pytest

from tests.helpers import load_tool


def _gen():
    return load_tool("gen_rollout_one")


@pytest.fixture(scope="module")
def statements():
    """{K: (instruction lines of one_solve_<K>, first AGPR of gd[K])}"""
    g = _gen()
    m = g.Map()
    member = lambda r, gg: f"P.p[{m.idx[('p', r, gg)]}]"
    out = {}
    for K in m.gd:
        f = io.StringIO()
        g.solve_stmt(f, m, K, member)
        text = f.getvalue()
        body = text[text.index("asm volatile(") + len("asm volatile("):]
        body = body[:body.index("\n        : ")]                     # the template: everything in front of the operand lists
        lines = [re.sub(r'\\n\\t$', "", x.strip().strip('"')) for x in body.split("\n")]
        lines = [re.sub(r'\\n\\t"?$', "", x) for x in lines if x]
        out[K] = (lines, m.reg("gd", K, 0))
    assert sorted(out) == [2, 3, 4, 5, 6, 7]
    return out


MFMA = re.compile(r"^v_mfma_f64_4x4x4_4b_f64 (\S+), (\S+), (\S+), (\S+?)( neg:\[1,0,0\])?$")


def inverse_mfmas(lines):
    hits = []
    for i, x in enumerate(lines):
        mm = MFMA.match(x)
        if mm and not mm.group(2).startswith("a[") and mm.group(2) != mm.group(3) and mm.group(4) == "0" and not mm.group(5):
            hits.append(i)
    return hits


def gd_writes(lines, n):
    return [[i for i, x in enumerate(lines) if re.match(rf"^v_accvgpr_write_b32 a{r}, ", x)] for r in (n, n + 1)]


def first_gd_read(lines, n):
    for i, x in enumerate(lines):
        mm = MFMA.match(x)
        if mm and mm.group(2) == f"a[{n}:{n + 1}]":
            return i
    return None


def test_the_statements_parse(statements):
    for K, (lines, n) in statements.items():
        assert sum(1 for x in lines if MFMA.match(x)) >= 28, K
        assert first_gd_read(lines, n) is not None, K


@pytest.mark.parametrize("K", [3, 4, 5, 6, 7])
def test_inverse_and_write_pair_once_in_front_of_the_first_read(statements, K):
    lines, n = statements[K]
    inv = inverse_mfmas(lines)
    lo, hi = gd_writes(lines, n)
    first = first_gd_read(lines, n)
    first_branch = min(i for i, x in enumerate(lines) if x.startswith("s_cbranch") or x.startswith("s_branch"))
    print(f"K = {K}: inverse MFMAs at {inv}, writes of a{n} / a{n + 1} at {lo} / {hi}, first read of gd[{K}] at {first}, first branch at {first_branch}")
    assert len(inv) == 3
    assert len(lo) == 1 and len(hi) == 1
    assert inv[0] < inv[1] < inv[2] < lo[0] < hi[0] < first
    assert hi[0] < first_branch                                      # on every path through the statement
    # the chain: M^T = MFMA(M, I); M M = MFMA(M^T, M); the last product writes what the pair then copies
    a = [MFMA.match(lines[i]).groups() for i in inv]
    assert a[1][1] == a[0][0] and a[1][2] == a[0][1]
    assert a[2][1] == a[0][0] and a[2][2] == a[1][0]
    src = re.match(r"^v_accvgpr_write_b32 a\d+, v(\d+)$", lines[lo[0]]).group(1)
    assert a[2][0] == f"v[{src}:{int(src) + 1}]"


def test_epoch_two_keeps_the_inline_inverse(statements):
    lines, n = statements[2]
    assert inverse_mfmas(lines) == []
    assert not [x for x in lines if x.startswith("v_accvgpr_write")]
