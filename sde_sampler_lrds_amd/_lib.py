"""ctypes binding of libsdeng.so, derived from include/sdeng.h (the C ABI) when this module is imported.

There is no CPU fallback: if the HIP library is missing or fails to load, importing this module's
``lib()`` raises.  ``python -m sde_sampler_lrds_amd.build`` (or ``__graft_entry__.build()``) builds it.
"""
from __future__ import annotations

import ctypes as C
import os
import re

SPLIT_TILES_MAX_B = 8192  # SDENG_FLAG_SPLIT_TILES is honoured up to this batch size (sdeng.h, sdeng_api.hip split_eligible)

_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
            "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t}
_RETURNS = {"int": C.c_int, "size_t": C.c_size_t, "const char*": C.c_char_p}
_DIRECTIVE = re.compile(r"#(?:ifndef SDENG_H|include <\w+\.h>|endif|define SDENG_(\w+)(.*))\s*")
_DECLARATION = re.compile(r"\s*(?:typedef\s+struct\s+(sdeng_\w+)\s*\{(.*?)\}\s*\1\s*;"  # a structure ...
                          r"|([\w\s*]+?)\b(sdeng_\w+)\s*\(([^()]*)\)\s*;)", re.S)  # ... or a prototype


def _refuse(what, text):
    raise ImportError(f"include/sdeng.h: {what}: {' '.join(text.split())[:120]!r}")


def _declarators(decl, structs, param=False):
    """``[(name, ctype)]`` of one field declaration or of one parameter: a base type, then declarators that each carry their own ``*``
    and ``[n]``.  A pointer is a c_void_p (device pointers travel as integers) unless it is a parameter that points to a structure."""
    head, rest = re.fullmatch(r"([\w\s]*)(.*)", decl, re.S).groups()
    words = [w for w in head.split() if w != "const"]
    if words and not rest.startswith("*"):
        rest = words.pop() + rest  # no star before the first name: the head's last word is that name, not part of the type
    base = " ".join(words)
    out = []
    for piece in rest.split(","):
        m = re.fullmatch(r"\s*(\*?)\s*(\w+)\s*(?:\[(\d+)\])?\s*", piece)
        if m is None or (param and m[3]):
            _refuse(f"cannot parse the declarator {piece.strip()!r}", decl)
        if m[1]:
            ctype = C.POINTER(structs[base]) if param and base in structs else C.c_void_p
        else:
            ctype = _SCALARS.get(base) or structs.get(base) or _refuse(f"unknown type {base!r}", decl)
        out.append((m[2], ctype * int(m[3]) if m[3] else ctype))
    return out


def read_header(text: str):
    """The declarations of include/sdeng.h, each kind in header order: constants ``{NAME: int}`` (the SDENG_ prefix dropped), structures
    ``{sdeng_name: ctypes.Structure}`` and prototypes ``{sdeng_name: (restype, argtypes)}``.  Not a C parser: it knows the constructs the
    header uses and raises ImportError, quoting the text, on anything else -- a declaration skipped in silence would be a binding that
    disagrees with the library."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)  # comments first: they hold prototype-like text
    text = re.sub(r"^#ifdef __cplusplus\n.*?^#endif\n", "", text, flags=re.S | re.M)  # the two halves of extern "C" { }
    consts, structs, protos = {}, {}, {}
    for line in re.findall(r"^[ \t]*#.*$", text, re.M):
        m = _DIRECTIVE.fullmatch(line) or _refuse("unknown directive", line)
        if m[1] and (m[1], m[2].strip()) != ("H", ""):  # SDENG_H without a value is the include guard
            expr = re.sub(r"\b(\d+)(?:ull|u)\b", r"\1", m[2])
            try:  # decimal literals, parentheses, unary minus and <<: nothing else reaches eval
                consts[m[1]] = int(eval(re.fullmatch(r"(?:\d+|<<|[\s()-])+", expr)[0]))
            except (SyntaxError, TypeError):  # TypeError: no match, or an empty pair of parentheses
                _refuse("not an integer expression", line)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    pos = 0
    while text[pos:].strip():
        m = _DECLARATION.match(text, pos) or _refuse("cannot parse the declaration", text[pos:])
        pos = m.end()
        if m[1]:
            fields = [f for decl in m[2].split(";") if decl.strip() for f in _declarators(decl, structs)]
            camel = "".join(part.capitalize() for part in m[1].split("_")[1:])  # sdeng_time_embed -> TimeEmbed
            structs[m[1]] = type(camel, (C.Structure,), {"_fields_": fields})
        else:
            restype = _RETURNS.get(" ".join(m[3].split())) or _refuse("unknown return type", m[0])
            params = [] if m[5].strip() == "void" else [_declarators(p, structs, param=True)[0] for p in m[5].split(",")]
            protos[m[4]] = (restype, [ctype for _, ctype in params])
    return consts, structs, protos


with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "sdeng.h")) as _f:
    _CONSTS, _STRUCTS, _PROTOS = read_header(_f.read())  # once per process
globals().update(_CONSTS)  # ABI_VERSION, NCOEF, FORM_*, FLAG_*, DIST_*, CTRL_*, REF_*, TILT_*, E_*, ...
globals().update({cls.__name__: cls for cls in _STRUCTS.values()})  # Dist, TimeEmbed, Net, Ref, Desc, Adjoint, CmcdAdjoint, ...
EXPORTS = list(_PROTOS)


class EngineError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"sdeng error {code}: {msg}")
        self.code = code


_LIB = None
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libsdeng.so")


def lib() -> C.CDLL:
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python -m sde_sampler_lrds_amd.build` "
                          "(there is no CPU fallback for the simulate path)")
    import torch  # noqa: F401 -- before the library: libsdeng.so then binds to the HIP runtime torch has loaded (its own copy), instead
    #                          of bringing /opt/rocm's into the process first; with two runtimes the library's launches find no device
    L = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in _PROTOS.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    if L.sdeng_abi_version() != ABI_VERSION:
        raise ImportError(f"libsdeng.so ABI {L.sdeng_abi_version()} != binding ABI {ABI_VERSION}")
    _LIB = L
    return L


def check(rc: int):
    if rc != 0:
        raise EngineError(rc, lib().sdeng_last_error().decode())


class HipEvents:
    """A pair of raw hipEvent_t for timing the step-loop kernel alone (bench.py roofline leg)."""

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.start, self.stop = C.c_void_p(), C.c_void_p()
        for ev in (self.start, self.stop):
            if self.hip.hipEventCreate(C.byref(ev)) != 0:
                raise RuntimeError("hipEventCreate failed")

    def elapsed_ms(self) -> float:
        if self.hip.hipEventSynchronize(self.stop) != 0:
            raise RuntimeError("hipEventSynchronize failed")
        ms = C.c_float()
        if self.hip.hipEventElapsedTime(C.byref(ms), self.start, self.stop) != 0:
            raise RuntimeError("hipEventElapsedTime failed")
        return ms.value
