"""ctypes binding of libfsnerf_hip.so, read from its C-ABI header (include/fsnerf_hip.h) once per process: the
header is the only place an entry point, an argument struct or an FSN_* constant is written down.  `parse_header`
gives, per symbol, every parameter's name, ctype and pointee; `SIGNATURES`, the argument structs and the FSN_*
attributes are derived from that.  The parser is strict: a type outside its table, a statement outside its grammar or
a non-integer FSN_* #define raises at import and quotes the text - nothing falls back to a void pointer.

There is no CPU fallback: if the library is missing or a call fails, a RuntimeError
is raised.  PyTorch is only used for device memory and streams."""
import ctypes as C
import os
import re
import subprocess
from typing import NamedTuple, Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
HEADER = os.path.join(_HERE, "..", "include", "fsnerf_hip.h")  # where csrc/Makefile looks for it
LIB_PATH = os.environ.get("FSN_LIB_PATH", os.path.join(CSRC, "libfsnerf_hip.so"))  # override: A/B builds


class Param(NamedTuple):
    """A parameter, a return value (name "") or a struct field.  pointee: None for a value, else what the pointer
    points at: a scalar type's name, "void", "char", a struct's name, or "<scalar>*" for a pointer to pointers."""
    name: str
    ctype: Optional[type]
    pointee: Optional[str]


# the whole type map: scalars by value (and as pointees), plus void / char pointees, structs and opaque handles
_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
            "uint8_t": C.c_uint8, "float": C.c_float, "double": C.c_double}
_DECL = re.compile(r"(?:const\s+)?(\w+)\s*((?:\*\s*(?:const\s*)?)*)(\w*)\s*(?:\[(\d+)\])?")
_STMT = re.compile(r"\s*(typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)|typedef\s+void\s*\*\s*(\w+)|[^;{}]+?)\s*;")
_FUNC = re.compile(r"([^()]+?[\s*])(\w+)\s*\(([^()]*)\)")
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(FSN_\w+)[ \t]+(.*?)[ \t]*$", re.M)


def _param(text: str, structs: dict, handles: set, field: bool = False) -> Param:
    m = _DECL.fullmatch(text.strip())
    if not m:
        raise ValueError(f"C-ABI header: cannot parse the declarator {text.strip()!r}")
    base, stars, name, dim = m.group(1), m.group(2).count("*"), m.group(3), m.group(4)
    if dim is not None and not (field and stars == 0 and base in _SCALARS):
        raise ValueError(f"C-ABI header: array outside a struct's scalar fields in {text.strip()!r}")
    if stars == 0 and base in _SCALARS:
        return Param(name, _SCALARS[base] * int(dim) if dim else _SCALARS[base], None)
    if stars == 0 and base in handles:
        return Param(name, C.c_void_p, None)
    if stars == 1 and base == "char":
        return Param(name, C.c_char_p, "char")
    if stars == 1 and base in structs and not field:
        return Param(name, C.POINTER(structs[base]), base)
    if stars == 1 and (base in _SCALARS or base == "void"):
        return Param(name, C.c_void_p, base)
    if stars == 2 and base in _SCALARS:
        return Param(name, C.c_void_p, base + "*")
    raise ValueError(f"C-ABI header: unknown type in {text.strip()!r}")


def _fields(body: str, structs: dict, handles: set) -> list:
    out = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        first, *more = decl.split(",")  # `float near, far`: the later names share the first one's value type
        f = _param(first, structs, handles, field=True)
        if not f.name or (more and f.pointee is not None):
            raise ValueError(f"C-ABI header: a field without a name, or several pointers in one declaration: {decl!r}")
        base = first.strip()[:first.strip().rindex(f.name)]
        out += [f] + [_param(base + n, structs, handles, field=True) for n in more]
    return out


def parse_header(text: str):
    """-> (functions: name -> (return Param, [Param]), structs: name -> ctypes.Structure with `.fields` = [Param],
    defines: FSN_* name -> the #define's text)."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    defines = dict(_DEFINE.findall(text))
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    text, wrapped = re.subn(r'extern\s+"C"\s*\{', "", text)
    text = text.rstrip()
    if wrapped:
        if not text.endswith("}"):
            raise ValueError('C-ABI header: extern "C" { is not closed')
        text = text[:-1].rstrip()
    functions, structs, handles, pos = {}, {}, set(), 0
    while pos < len(text):
        m = _STMT.match(text, pos)
        if not m:
            raise ValueError(f"C-ABI header: no statement ends here: {text[pos:pos + 80].strip()!r}")
        pos = m.end()
        stmt, tag, body, name, handle = m.groups()
        if handle:
            handles.add(handle)
            continue
        fn = None if body is not None else _FUNC.fullmatch(stmt)
        if body is None and not fn:
            raise ValueError(f"C-ABI header: neither a declaration nor a typedef: {stmt[:80]!r}")
        name = name if fn is None else fn.group(2)
        if name in functions or name in structs or (fn is None and tag != name):
            raise ValueError(f"C-ABI header: {name!r} is declared twice (or its struct tag differs)")
        if fn is None:
            fields = _fields(body, structs, handles)
            structs[name] = type(name, (C.Structure,), {"_fields_": [(f.name, f.ctype) for f in fields], "fields": fields})
        else:
            params = [] if fn.group(3).strip() == "void" else [_param(p, structs, handles) for p in fn.group(3).split(",")]
            if any(not p.name for p in params):
                raise ValueError(f"C-ABI header: a parameter of {name} has no name: {stmt[:80]!r}")
            functions[name] = (_param(fn.group(1), structs, handles), params)
    return functions, structs, defines


def define_int(defines: dict, name: str) -> int:
    m = re.fullmatch(r"\(?\s*(-?\d+)[uU]?\s*\)?", defines[name])
    if not m:
        raise ValueError(f"C-ABI header: #define {name} {defines[name]!r} is not an integer")
    return int(m.group(1))


with open(HEADER) as _f:
    FUNCTIONS, STRUCTS, DEFINES = parse_header(_f.read())
MlpDesc, RenderArgs, OccRenderArgs = STRUCTS["fsn_mlp_desc"], STRUCTS["fsn_render_args"], STRUCTS["fsn_occ_render_args"]
UnseenDist = STRUCTS["fsn_unseen_dist"]
# name -> (restype, argtypes); every symbol declared in include/fsnerf_hip.h
SIGNATURES = {name: (ret.ctype, [p.ctype for p in params]) for name, (ret, params) in FUNCTIONS.items()}
globals().update({name: define_int(DEFINES, name) for name in DEFINES})  # FSN_PREC_*, FSN_STATUS_*, FSN_SCAN_*, ...

_lib = None


def build(force: bool = False) -> str:
    """Compile the HIP sources for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC, "-j4"] + (["-B"] if force else [])
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("building libfsnerf_hip.so failed:\n" + r.stdout[-4000:] + r.stderr[-4000:])
    return LIB_PATH


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(there is no CPU fallback for the HIP path)")
        l = C.CDLL(LIB_PATH)
        # FSN_LIB_PARTIAL: the library may export a subset - the sanitizer build of the host side, and an older
        # build loaded for an A/B timing (tools/bench_occ_cone.py loads the parent commit's library this way)
        partial = os.environ.get("FSN_LIB_PARTIAL") == "1"
        for name, (res, args) in SIGNATURES.items():
            if partial and not hasattr(l, name):
                continue
            fn = getattr(l, name)
            fn.restype, fn.argtypes = res, args
        _lib = l
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().fsn_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{what} failed (code {rc}): {msg}")
