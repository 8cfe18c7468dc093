"""The binding of sde_sampler_lrds_amd/_lib.py is read from include/sdeng.h; this file holds that reading to the C compiler's (no GPU):
every structure's size, every field's offset and size and every constant's value as a compiled program prints them, nothing in the
header skipped, the built library against the binding, and the reader's refusals of what it does not know."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from sde_sampler_lrds_amd import _lib as L
from sde_sampler_lrds_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXT = open(os.path.join(ROOT, "include", "sdeng.h")).read()


def binding_lines(consts, structs):
    """What a binding holds, one line per fact, in the format compiler_lines prints."""
    lines = [f"const {name} {value}" for name, value in consts.items()]
    for cname, cls in structs.items():
        lines.append(f"struct {cname} {ctypes.sizeof(cls)}")
        lines += [f"field {cname}.{f} {getattr(cls, f).offset} {getattr(cls, f).size}" for f, _ in cls._fields_]
    return lines


def compiler_lines(tmp_path):
    """The same facts from the host C compiler: a program that includes the header and prints sizeof / offsetof / the values.  The reader
    only supplies the names to ask about (test_nothing_in_the_header_is_skipped counts them against the raw text)."""
    consts, structs, _ = L.read_header(TEXT)
    out = [f'  printf("const {n} %lld\\n", (long long)(SDENG_{n}));' for n in consts]
    for cname, cls in structs.items():
        out.append(f'  printf("struct {cname} %zu\\n", sizeof({cname}));')
        out += [f'  printf("field {cname}.{f} %zu %zu\\n", offsetof({cname}, {f}), sizeof((({cname}*)0)->{f}));' for f, _ in cls._fields_]
    src, exe = tmp_path / "abi_probe.c", tmp_path / "abi_probe"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "sdeng.h"\nint main(void) {\n' + "\n".join(out) + "\n  return 0;\n}\n")
    cc = [shutil.which("cc"), "-x", "c"] if shutil.which("cc") else [build.HIPCC, "-x", "c++"]  # host code only, either way
    subprocess.run([*cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    return subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()


def test_layout_and_constants_equal_the_compilers(tmp_path):
    consts, structs, _ = L.read_header(TEXT)
    mine = binding_lines({n: getattr(L, n) for n in consts}, {c: getattr(L, cls.__name__) for c, cls in structs.items()})  # the module's own
    theirs = compiler_lines(tmp_path)
    assert len(theirs) > len(consts) + len(structs)
    assert mine == theirs, [pair for pair in zip(mine, theirs) if pair[0] != pair[1]]


def test_nothing_in_the_header_is_skipped():
    """Plain counts over the raw text, not through the reader."""
    consts, structs, protos = L.read_header(TEXT)
    assert len(re.findall(r"^#define SDENG_\w+[ \t]+\S", TEXT, re.M)) == len(consts) > 0
    assert TEXT.count("typedef struct") == len(structs) > 0
    assert len(re.findall(r"^(?:int|size_t|const char\*) sdeng_\w+\(", TEXT, re.M)) == len(protos) == len(L.EXPORTS) > 0
    assert L.EXPORTS == list(protos)
    assert structs["sdeng_time_embed"].__name__ == "TimeEmbed" and L.TimeEmbed._fields_ == structs["sdeng_time_embed"]._fields_


def test_library_exports_every_declared_symbol():
    declared = set(re.findall(r"\b(sdeng_[a-z0-9_]+)\s*\(", TEXT))
    assert declared, "no declarations parsed"
    lib = ctypes.CDLL(L.LIB_PATH)
    for sym in sorted(declared | set(L.EXPORTS)):
        assert hasattr(lib, sym), f"{sym} declared in include/sdeng.h but not exported"
    assert set(L.EXPORTS) <= declared
    lib.sdeng_abi_version.restype = ctypes.c_int
    assert lib.sdeng_abi_version() == L.ABI_VERSION == L.lib().sdeng_abi_version()


@pytest.mark.parametrize("old,new,message", [
    ("typedef struct sdeng_ref {", "typedef struct sdeng_ref {\n  unsigned long x;", "unknown type 'unsigned long'"),
    ("typedef struct sdeng_ref {", "typedef struct sdeng_ref {\n  int32_t x : 3;", "cannot parse the declarator"),
    ("#define SDENG_NCOEF 16", "#define SDENG_NCOEF 16\n#define SDENG_X 1.5f", "not an integer expression: '#define SDENG_X 1.5f'"),
    ("#define SDENG_NCOEF 16", "#define SDENG_NCOEF", "not an integer expression"),
    ("#define SDENG_NCOEF 16", "#define OTHER_NCOEF 16", "unknown directive"),
    ("int sdeng_simulate(", "float sdeng_simulate(", "unknown return type"),
    ("int sdeng_simulate(", "extern int sdeng_calls;\nint sdeng_simulate(", "cannot parse the declaration"),
])
def test_reader_refuses_what_it_does_not_know(old, new, message):
    assert TEXT.count(old) == 1
    with pytest.raises(ImportError, match=re.escape(message)):
        L.read_header(TEXT.replace(old, new))
