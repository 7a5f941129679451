"""The gfx950 ISA of a kernel file, for the checks that read it (CPU only: hipcc cross-compiles): how it is obtained and how its text
splits into functions, asm statements, instructions and metadata.  The flags are those of csrc/build.py and nothing else - this
module knows none of its own -, so every check reads the ISA of the build that ships (or that build plus the defines it asks for).

    compile_to_isa(src, defines=(), csrc=CSRC)   path of the .s of csrc/<src>; compiled once per process and flavour
    functions(text)                              (mangled name, [(line number, stripped text, inside an asm statement), ...]) per function
    instruction(line)                            the instruction of a line, or None (comment, directive, label, empty)
    metadata(text)                               {kernel name: {key: int}} of the amdhsa.kernels notes
"""
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "sampling_gpmpc_amd", "csrc")

_spec = importlib.util.spec_from_file_location("gpmpc_build", os.path.join(CSRC, "build.py"))
build = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(build)

_compiled = {}              # (source path, defines) -> path of the .s


def command(src, out, defines=(), csrc=CSRC):
    """csrc/build.py's compile command for `src`, to assembly instead of an object (-fPIC is the host side's)"""
    return [build.HIPCC, "-x", "hip", "-S", "--cuda-device-only", os.path.join(csrc, src), "-o", out] + \
        [f for f in build.FLAGS if f != "-fPIC"] + build.EXTRA_FLAGS.get(src, []) + list(defines)


def compile_to_isa(src, defines=(), csrc=CSRC):
    """`csrc`: another csrc directory (a checkout of the parent commit); the quoted includes of a source are found beside it first"""
    key = (os.path.join(os.path.abspath(csrc), src), tuple(defines))
    if key not in _compiled:
        out = os.path.join(tempfile.mkdtemp(prefix="gpmpc_isa_"), src.replace(".hip", ".s"))
        print(f"tools/isa.py: hipcc -S {key[0]} {' '.join(defines)}".rstrip(), file=sys.stderr, flush=True)
        subprocess.run(command(src, out, defines, csrc), check=True, capture_output=True)
        _compiled[key] = out
    return _compiled[key]


def functions(text):
    """The functions of an ISA text, in order: (mangled name, lines) with lines = [(line number in `text` from 1, stripped text,
    True between ;;#ASMSTART and ;;#ASMEND), ...] from the function's label to its end (the `; codeLenInByte` comment hipcc puts
    behind .Lfunc_end; the next function's label or the text's end where there is none)."""
    name, lines, in_asm = None, [], False
    for ln, raw in enumerate(text.split("\n"), 1):
        t = raw.strip()
        m = re.match(r"^(_Z\w+):", t)
        if m:
            if name is not None:
                yield name, lines
            name, lines, in_asm = m.group(1), [], False
        if name is None:
            continue
        if t.startswith(";;#ASMEND"):
            in_asm = False
        lines.append((ln, t, in_asm))
        if t.startswith(";;#ASMSTART"):
            in_asm = True
        if t.startswith("; codeLenInByte"):
            yield name, lines
            name = None
    if name is not None:
        yield name, lines


def instruction(line):
    """the instruction of a line without its comment, or None: empty and comment-only lines, directives and labels hold none"""
    code = line.split(";")[0].strip()
    return None if not code or code.startswith(".") or code.endswith(":") else code


def metadata(text):
    """{kernel name: {key: int}} from the amdhsa.kernels notes (an .s file, or `llvm-readelf --notes` of a code object): the
    integer fields of each kernel's own entry - vgpr_count, agpr_count, sgpr_count, vgpr_spill_count, sgpr_spill_count,
    private_segment_fixed_size, group_segment_fixed_size, ... -, not those of its arguments."""
    out, entry, item, field = {}, None, None, None
    for raw in text.split("\n"):
        m = re.match(r"^(\s*)amdhsa\.kernels:\s*$", raw)
        if m:                                               # a kernel's entry opens with "  - .key:", its fields stand under the key
            item, field = m.group(1) + "  - .", m.group(1) + "    ."
            continue
        if item is None:
            continue
        if raw.startswith(item):
            entry = {}
        elif not raw.startswith(field):
            if raw.strip() and len(raw) - len(raw.lstrip()) < len(field) - 1:       # the list's end (amdhsa.target, amdhsa.version)
                item = entry = None
            continue
        m = re.match(r"^\.(\w+):\s+(\S+)$", raw[len(field) - 1:])
        if m and m.group(1) == "name":
            out[m.group(2)] = entry
        elif m and m.group(2).isdigit():
            entry[m.group(1)] = int(m.group(2))
    return out
