"""ctypes binding of libseg3d_hip.so, derived from the C ABI's one declaration: include/seg3d_hip.h.

The header is parsed once, when this module is imported (plain ``re``, a few milliseconds), into
  SIGNATURES      {entry point: (restype, [argtypes])}, bound to the library by load();
  the constants   every ``#define SEG3D_<NAME> <int>`` as ``_lib.<NAME>`` (OK, EINVAL, REDUCE_SUM, ABI_VERSION, ...);
  struct(name)    one ctypes.Structure per ``typedef struct { ... } seg3d_<name>;``; ``np.dtype(struct(name))`` is the
                  record dtype of a device table of them.
To add an entry point, a constant or a table record, declare it in the header: there is nothing to repeat here.  The
grammar the parser takes is stated at the top of the header; what falls outside it (an unknown type, a struct by value,
a function pointer, a define or an array bound that is no integer, anything else at file scope) raises HeaderError with the
declaration's text instead of being skipped.  Type rules: anything with a ``*`` is c_void_p (a ``const char*`` return is
c_char_p); int / int32_t, int64_t, uint64_t, size_t, float, double map to the ctypes type of the same width.

There is no fallback: if the shared object is missing or a symbol does not resolve, loading
raises.  Build it with ``python __graft_entry__.py`` (hipcc --offload-arch=gfx950).
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libseg3d_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "seg3d_hip.h")

_SCALARS = {"int": ctypes.c_int32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
            "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double}
_DECLARATOR = r"[A-Za-z_]\w*(?:\s*\[[^\]]*\])?"


class HeaderError(ValueError):
    """include/seg3d_hip.h holds a declaration outside the grammar this binding derives itself from."""


def _scalar(words, decl):
    """ctypes type of a non-pointer type given as its words (const dropped)"""
    words = [w for w in words if w != "const"]
    if len(words) != 1 or words[0] not in _SCALARS:
        raise HeaderError(f"unknown type '{' '.join(words)}' in: {decl}")
    return _SCALARS[words[0]]


def _struct_class(name, body, defines, structs):
    fields = []
    for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
        m = re.fullmatch(rf"(.*?[\s*])({_DECLARATOR}(?:\s*,\s*{_DECLARATOR})*)", decl)
        if "(" in decl or not m:
            raise HeaderError(f"{name}: cannot parse the field: {decl}")
        words = [w for w in m.group(1).split() if w != "const"]
        if "*" in m.group(1):
            base = ctypes.c_void_p
        elif len(words) == 1 and words[0] in structs:  # a struct declared earlier in the header
            base = structs[words[0]]
        else:
            base = _scalar(words, f"{name}: {decl}")
        for item in m.group(2).split(","):
            field, _, bound = item.strip().partition("[")
            ctype = base
            if bound:
                bound = bound.rstrip("] ").strip()
                count = int(bound) if bound.isdigit() else defines.get(bound[len("SEG3D_"):]) if bound.startswith("SEG3D_") else None
                if count is None or count <= 0:
                    raise HeaderError(f"{name}: cannot resolve the array bound [{bound}] in: {decl}")
                ctype = base * count
            fields.append((field.strip(), ctype))
    return type(name, (ctypes.Structure,), {"_fields_": fields, "__doc__": f"{name} of include/seg3d_hip.h"})


def _signature(decl, structs):
    m = re.fullmatch(r"([\w\s*]+?)\b(seg3d_\w+)\s*\((.*)\)", decl)
    if not m:
        raise HeaderError(f"cannot parse the declaration: {decl}")
    ret, name, params = m.group(1).split(), m.group(2), m.group(3).strip()
    if "(" in params or ")" in params:
        raise HeaderError(f"{name}: function-pointer parameters are not supported: {decl}")
    if "*" in m.group(1):
        if "".join(ret) != "constchar*":
            raise HeaderError(f"{name}: the only pointer an entry may return is const char*: {decl}")
        restype = ctypes.c_char_p
    else:
        restype = _scalar(ret, decl)
    argtypes = []
    for param in ([] if params == "void" else params.split(",")):
        if "*" in param:
            argtypes.append(ctypes.c_void_p)
            continue
        words = [w for w in param.split() if w != "const"]
        if words and words[0] in structs:
            raise HeaderError(f"{name}: {words[0]} is passed by value; pass a pointer to it: {decl}")
        if "[" in param or not 1 <= len(words) <= 2:
            raise HeaderError(f"{name}: cannot parse the parameter '{param.strip()}' of: {decl}")
        argtypes.append(_scalar(words[:1], decl))
    return name, (restype, argtypes)


def parse_header(text):
    """(defines, structs, signatures) of a header written in the grammar stated at the top of include/seg3d_hip.h."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^[ \t]*#[ \t]*ifdef[ \t]+__cplusplus\b.*?^[ \t]*#[ \t]*endif\b[^\n]*", " ", text, flags=re.S | re.M)
    defines, guards = {}, set(re.findall(r"^[ \t]*#[ \t]*ifndef[ \t]+(\w+)", text, flags=re.M))
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)(.*)$", text, flags=re.M):
        value = value.strip()
        if not value and name in guards:
            continue  # the include guard
        m = re.fullmatch(r"-?\d+|\(\s*-?\d+\s*\)", value)
        if not name.startswith("SEG3D_") or not m:
            raise HeaderError(f"cannot resolve the define to an integer: #define {name}{' ' + value if value else ''}")
        defines[name[len("SEG3D_"):]] = int(value.strip("() "))
    for line in re.findall(r"^[ \t]*#[^\n]*", text, flags=re.M):
        if not re.match(r"\s*#\s*(define|include|ifndef|endif)\b", line):
            raise HeaderError(f"unsupported preprocessor line: {line.strip()}")
    text = re.sub(r"^[ \t]*#[^\n]*", " ", text, flags=re.M)
    structs, signatures = {}, {}
    # a struct body holds no braces, so the typedefs can be cut out first; what is left splits into declarations at ';'
    for m in re.finditer(r"\btypedef\s+struct\s*\{([^{}]*)\}\s*(\w+)\s*;", text):
        structs[m.group(2)] = _struct_class(m.group(2), m.group(1), defines, structs)
    text = re.sub(r"\btypedef\s+struct\s*\{[^{}]*\}\s*\w+\s*;", " ", text)
    for decl in filter(None, (" ".join(d.split()) for d in text.split(";"))):
        name, sig = _signature(decl, structs)
        signatures[name] = sig
    return defines, structs, signatures


with open(HEADER_PATH) as _f:
    DEFINES, STRUCTS, SIGNATURES = parse_header(_f.read())
globals().update(DEFINES)  # OK, EINVAL, EWORKSPACE, ELAUNCH, REDUCE_*, ATTN_*, OPTIM_*, CRITERION_*, ABI_VERSION, ...


def struct(name):
    """The ctypes.Structure class of the header's `typedef struct { ... } name;` (np.dtype(struct(name)) for a record table)."""
    return STRUCTS[name]


_ERR = {EINVAL: "SEG3D_EINVAL (bad argument)", EWORKSPACE: "SEG3D_EWORKSPACE (workspace too small)",  # noqa: F821
        ELAUNCH: "SEG3D_ELAUNCH (HIP launch/runtime error)"}  # noqa: F821

_lib = None


class Seg3dError(RuntimeError):
    pass


def header_symbols():
    """Function names declared in include/seg3d_hip.h (a plain name search, independent of parse_header)."""
    with open(HEADER_PATH) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(seg3d_[a-z0-9_]+)\s*\(", text)))


def load():
    """Load the shared object and bind every entry point; raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise Seg3dError(
            f"{LIB_PATH} not found: the HIP library is required (no CPU fallback). "
            "Build it with `python __graft_entry__.py`.")
    # torch first: its bundled HIP runtime must be the one this library binds to (the streams and device pointers
    # handed over come from it); loading the library before torch would pull in a second runtime from /opt/rocm
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.seg3d_abi_version() != ABI_VERSION:  # noqa: F821
        raise Seg3dError(f"libseg3d_hip.so ABI {lib.seg3d_abi_version()} != header {ABI_VERSION}")  # noqa: F821
    _lib = lib
    return lib


def call(name, *args):
    """Invoke an int-returning entry point; negative return codes raise Seg3dError."""
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != OK:  # noqa: F821
        detail = ""
        if rc == ELAUNCH:  # noqa: F821  the runtime's own words (hipGetErrorString) for the failure behind SEG3D_ELAUNCH
            text = lib.seg3d_last_error()
            detail = f": {text.decode(errors='replace')}" if text else ""
        raise Seg3dError(f"{name} failed: {_ERR.get(rc, rc)}{detail}")


def query(name, *args):
    """Invoke a size_t-returning *_bytes query."""
    return int(getattr(load(), name)(*args))
