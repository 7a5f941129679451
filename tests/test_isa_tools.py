"""tools/isa.py, which every ISA check goes through: the parser on a hand-written snippet, the compile command against
csrc/build.py's flags, and the one compile per process (CPU; the last test cross-compiles base_samples.hip, 58 lines)."""
import os

import pytest

from tests.helpers import TOOLS, load_tool

isa = load_tool("isa")

SNIPPET = """\t.text
\t.globl\t_Z5firstPd
_Z5firstPd:                             ; @_Z5firstPd
; %bb.0:
\ts_load_dwordx2 s[0:1], s[0:1], 0x0
\tv_mov_b32_e32 v2, 0                     ; a trailing comment
\t;;#ASMSTART
\tv_accvgpr_write_b32 a0, v2
\ts_nop 1
\t;;#ASMEND
.LBB0_1:                                ; %loop
\t.p2align\t6
\ts_cbranch_scc1 .LBB0_1
\ts_endpgm
.Lfunc_end0:
\t.size\t_Z5firstPd, .Lfunc_end0-_Z5firstPd
; codeLenInByte = 40
\t.globl\t_Z6secondPd
_Z6secondPd:
\tv_add_f64 v[0:1], v[0:1], v[2:3]
\ts_endpgm
.Lfunc_end1:
; codeLenInByte = 12
\t.amdgpu_metadata
---
amdhsa.kernels:
  - .agpr_count:     4
    .args:
      - .address_space:  global
        .name:           x
        .offset:         0
        .size:           8
        .value_kind:     global_buffer
    .group_segment_fixed_size: 512
    .name:           _Z5firstPd
    .private_segment_fixed_size: 0
    .sgpr_count:     10
    .sgpr_spill_count: 0
    .symbol:         _Z5firstPd.kd
    .vgpr_count:     8
    .vgpr_spill_count: 0
  - .agpr_count:     0
    .args:           []
    .group_segment_fixed_size: 0
    .name:           _Z6secondPd
    .private_segment_fixed_size: 16
    .sgpr_count:     6
    .sgpr_spill_count: 1
    .vgpr_count:     5
    .vgpr_spill_count: 2
amdhsa.target:   amdgcn-amd-amdhsa--gfx950
amdhsa.version:
  - 1
  - 2
...
\t.end_amdgpu_metadata
"""


def test_parser_on_a_hand_written_snippet():
    funcs = list(isa.functions(SNIPPET))
    assert [name for name, _ in funcs] == ["_Z5firstPd", "_Z6secondPd"]
    first, second = funcs[0][1], funcs[1][1]
    # from the label to the function's end, numbered by the line of the text (from 1), stripped
    assert first[0] == (3, "_Z5firstPd:                             ; @_Z5firstPd", False)
    assert [ln for ln, _, _ in first] == list(range(3, 18)) and first[-1][1] == "; codeLenInByte = 40"
    assert [ln for ln, _, _ in second] == list(range(19, 24))
    # inside an asm statement: the lines between the two marks, not the marks
    assert [ln for ln, _, in_asm in first if in_asm] == [8, 9]
    assert not any(in_asm for _, _, in_asm in second)
    # the instruction of a line, or nothing: comment stripped; label, directive, comment-only and mark lines hold none
    assert [(ln, isa.instruction(t)) for ln, t, _ in first if isa.instruction(t) is not None] == [
        (5, "s_load_dwordx2 s[0:1], s[0:1], 0x0"), (6, "v_mov_b32_e32 v2, 0"), (8, "v_accvgpr_write_b32 a0, v2"), (9, "s_nop 1"),
        (13, "s_cbranch_scc1 .LBB0_1"), (14, "s_endpgm")]
    assert [isa.instruction(t) for _, t, _ in second] == [None, "v_add_f64 v[0:1], v[0:1], v[2:3]", "s_endpgm", None, None]
    for none in ("", "; %bb.0:", ".LBB0_1:                                ; %loop", ".p2align\t6", ";;#ASMSTART", "_Z6secondPd:"):
        assert isa.instruction(none) is None, none
    # the kernels' own integer fields, each under its kernel - those in front of .name included -, none of an argument's
    meta = isa.metadata(SNIPPET)
    assert list(meta) == ["_Z5firstPd", "_Z6secondPd"]
    assert meta["_Z5firstPd"] == {"agpr_count": 4, "group_segment_fixed_size": 512, "private_segment_fixed_size": 0, "sgpr_count": 10,
                                  "sgpr_spill_count": 0, "vgpr_count": 8, "vgpr_spill_count": 0}
    assert meta["_Z6secondPd"] == {"agpr_count": 0, "group_segment_fixed_size": 0, "private_segment_fixed_size": 16, "sgpr_count": 6,
                                   "sgpr_spill_count": 1, "vgpr_count": 5, "vgpr_spill_count": 2}


def test_compile_command_is_the_shipped_builds():
    b = isa.build
    cmd = isa.command("rollout_one.hip", "out.s")
    assert b.EXTRA_FLAGS["rollout_one.hip"], "rollout_one.hip ships with flags of its own"
    for tok in b.EXTRA_FLAGS["rollout_one.hip"] + [f for f in b.FLAGS if f != "-fPIC"]:
        assert tok in cmd, tok
    assert cmd[0] == b.HIPCC and "-fPIC" not in cmd and "-S" in cmd
    assert isa.command("rollout_one.hip", "out.s", ("-DX",))[:-1] == cmd
    # the hazard tool carries no flags and no compile of its own
    hz = load_tool("check_dpp_hazard")
    assert not hasattr(hz, "EXTRA") and not hasattr(hz, "compile_to_isa")
    text = open(os.path.join(TOOLS, "check_dpp_hazard.py")).read()
    for word in ("-mllvm", "--offload-arch", "-O3", "subprocess", "hipcc\""):
        assert word not in text, word


@pytest.mark.skipif(not os.path.exists(isa.build.HIPCC), reason="hipcc not available")
def test_a_file_is_compiled_once_per_process(capfd):
    a = isa.compile_to_isa("base_samples.hip")
    b = isa.compile_to_isa("base_samples.hip")
    lines = [x for x in capfd.readouterr().err.split("\n") if x.startswith("tools/isa.py: hipcc") and "base_samples.hip" in x]
    assert a == b and os.path.getsize(a) > 0
    assert len(lines) == 1, lines
    # another flavour is another compile, and no other file's
    c = isa.compile_to_isa("base_samples.hip", ("-DGPMPC_ISA_TEST_FLAVOUR",))
    assert c != a and len(capfd.readouterr().err.strip().split("\n")) == 1
