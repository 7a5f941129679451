"""The static solve statements one_solve_t<t> (tools/gen_rollout_one.py: solve_stmt(..., nh = 3 t)) against the run-time statement of
the step's epoch.  CPU only: the generator's text is read, nothing is compiled.

For every t = 0 .. 29 the run-time statement one_solve<K(t)> is WALKED along the path it takes for n_h = 3 t - each s_cmp / s_cbranch
resolved with the known n_h - and the instructions it executes there, without the padding (s_nop), the compares, the branches and
the labels, are compared text for text with the static statement's: the same MFMAs, DPP moves, adds, multiplies and
v_accvgpr_write, in the same order with the same operands, the stages of the riding inverse (K >= 3) included.  The static
statements hold no branch, no compare and no label, and pass the distance rules of tools/check_dpp_hazard.py (a row reached by
fall-through drops the padded head the branched-to copy carries: the rules say whether what is left suffices).
"""
import io
import os
import re

import pytest

from tests.helpers import REPO, load_tool

STEPS = list(range(30))


def _lines(text):
    body = text[text.index("asm volatile(") + len("asm volatile("):]
    body = body[:body.index("\n        : ")]                         # the template: everything in front of the operand lists
    lines = [re.sub(r'\\n\\t$', "", x.strip().strip('"')) for x in body.split("\n")]
    return [re.sub(r'\\n\\t"?$', "", x) for x in lines if x]


@pytest.fixture(scope="module")
def gen():
    g = load_tool("gen_rollout_one")
    m = g.Map()
    member = lambda r, gg: f"P.p[{m.idx[('p', r, gg)]}]"
    run, static, operands = {}, {}, {}
    for K in m.gd:
        f = io.StringIO()
        g.solve_stmt(f, m, K, member)
        run[K] = _lines(f.getvalue())
    for t in STEPS:
        f = io.StringIO()
        g.solve_stmt(f, m, g.epoch_of(t), member, nh=g.T_ROWS * t)
        static[t] = _lines(f.getvalue())
        operands[t] = f.getvalue()[f.getvalue().index("\n        : "):]
    return g, run, static, operands


PAD = re.compile(r"^(s_nop|s_cmp|s_cbranch|s_branch)\b|:$")


def work(lines):
    return [x for x in lines if not PAD.search(x)]


def walk(lines, nh):
    """the instructions the run-time statement executes for n_h = nh, in order (padding, compares, branches and labels left out)"""
    label = {x[:-1]: i for i, x in enumerate(lines) if x.endswith(":")}
    out, pc, scc, n = [], 0, None, 0
    while pc < len(lines):
        n += 1
        assert n < 10 * len(lines), "the walk does not end"
        x = lines[pc]
        pc += 1
        m = re.match(r"^s_cmp_(eq|gt)_u32 %\d+, (\d+)$", x)
        if m:
            scc = (nh == int(m.group(2))) if m.group(1) == "eq" else (nh > int(m.group(2)))
        elif x.startswith("s_cbranch_scc"):
            m = re.match(r"^s_cbranch_scc([01]) (\S+)$", x)
            assert scc is not None
            if scc == (m.group(1) == "1"):
                pc = label[m.group(2)]
        elif x.startswith("s_branch"):
            pc = label[x.split()[1]]
        elif x.startswith("s_cmp") or x.startswith("s_cbranch"):
            raise AssertionError(f"unknown control instruction {x}")
        elif not PAD.search(x):
            out.append(x)
    return out


@pytest.mark.parametrize("t", STEPS)
def test_static_statement_is_the_run_time_path(gen, t):
    g, run, static, _ = gen
    K, nh = g.epoch_of(t), g.T_ROWS * t
    path = walk(run[K], nh)
    mine = work(static[t])
    n_rows = len([r for r in range(g.NTR) if 4 * r < nh and r < 4 * K - g.NKT + 4])
    print(f"t = {t}: epoch {K}, n_h = {nh}, {n_rows} tile rows, {len(path)} instructions on the run-time path, {len(mine)} in the static statement")
    assert len(path) >= 3 and mine == path
    # one cross-block sum and one merge per tile row: the rows with 4 r < n_h and no other
    assert sum(1 for x in mine if "row_ror:8" in x) == 2 * n_rows
    assert sum(1 for x in mine if "quad_perm:[0,1,2,3]" in x) == 2 * n_rows


@pytest.mark.parametrize("t", STEPS)
def test_static_statement_has_no_branch_label_or_row_count(gen, t):
    _, _, static, operands = gen
    for x in static[t]:
        assert not x.startswith(("s_cmp", "s_cbranch", "s_branch", "s_setpc")) and not x.endswith(":") and ".L" not in x, x
    assert '"s"(' not in operands[t] and "nh" not in operands[t] and '"scc"' not in operands[t]


def test_static_statements_pass_the_distance_rules(gen):
    _, _, static, _ = gen
    # each statement as a function of its own: (name, [(line number, text, inside an asm statement)])
    stmts = [(f"one_solve_t{t}", [(i, x, True) for i, x in enumerate(static[t], 1)]) for t in STEPS]
    counts, problems = load_tool("check_dpp_hazard").check(stmts, "rollout_one.hip")
    print(f"{counts['dpp']} DPP reads and {counts['mfma']} MFMAs checked, {len(problems)} hazard(s)")
    for k, ln, code, rule, rg in problems[:10]:
        print(f"  [{rule}] {k} line {ln}: `{code}` <- {rg}")
    assert counts["mfma"] > 1000 and counts["dpp"] > 1000
    assert problems == []


def test_build_writes_the_statements_file_and_depends_on_it(gen):
    """rollout_one_steps_gen.inc is not committed: csrc/build.py writes it when the module is loaded and before it compiles, and
    treats it as a header of rollout_one.hip"""
    g = gen[0]
    b = load_tool("isa").build
    assert list(b.BUILD_GENERATED) == ["rollout_one_steps_gen.inc"] and "rollout_one_steps_gen.inc" in b.HEADERS
    f = io.StringIO()
    g.emit_steps(f)
    text = open(os.path.join(b.HERE, "rollout_one_steps_gen.inc")).read()
    assert text.split("\n", 1)[1] == f.getvalue()                   # (behind the file's first line, the "GENERATED" note)
    assert '#include "rollout_one_steps_gen.inc"' in open(os.path.join(b.HERE, "rollout_one.hip")).read()
    ignored = open(os.path.join(REPO, ".gitignore")).read().split("\n")
    assert "sampling_gpmpc_amd/csrc/rollout_one_steps_gen.inc" in ignored
