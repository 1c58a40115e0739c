"""The Python binding is derived from include/seg3d_hip.h (openseg3d_amd/_lib.py: parse_header).  CPU-only checks of the
parser on small synthetic headers, of the derived struct layouts against the host C compiler, of every literal call site's
argument count against the derived table, and of the built library against the header's ABI version."""
import ast
import ctypes
import glob
import os
import re
import shutil
import subprocess

import pytest

from openseg3d_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I32, I64, U64, SZ, F, D = (ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_size_t,
                              ctypes.c_float, ctypes.c_double)


def test_signatures_from_a_synthetic_header():
    defines, structs, sigs = _lib.parse_header("""
        #ifndef SEG3D_FAKE_H
        #define SEG3D_FAKE_H
        #include <stdint.h>
        #ifdef __cplusplus
        extern "C" {
        #endif
        #define SEG3D_OK 0
        #define SEG3D_EBAD (-3)   /* negative defines stand in parentheses */
        #define SEG3D_ALSO_BAD ( -4 )
        /* prose that mentions a call: seg3d_fake(int x); must not become an entry */
        int seg3d_version(void);
        const char* seg3d_text(void);
        size_t seg3d_bytes(int64_t n, int32_t c /* channels */, uint64_t seed, int flag);
        // a line comment with seg3d_other(float y);
        int32_t seg3d_run(const float* x /*or NULL*/, float * const * y, const void* const p, void** q,
                          const int32_t* shape /* [m, cout] rows, (z, y, x) */, float eps, double tol, const int64_t n,
                          void* stream);
        double seg3d_unnamed(int32_t, const float*);
        #ifdef __cplusplus
        }
        #endif
        #endif
    """)
    assert defines == {"OK": 0, "EBAD": -3, "ALSO_BAD": -4} and structs == {}
    assert sigs == {"seg3d_version": (I32, []),
                    "seg3d_text": (ctypes.c_char_p, []),
                    "seg3d_bytes": (SZ, [I64, I32, U64, I32]),
                    "seg3d_run": (I32, [P, P, P, P, P, F, D, I64, P]),
                    "seg3d_unnamed": (D, [I32, P])}


def test_structs_from_a_synthetic_header():
    _, structs, sigs = _lib.parse_header("""
        #define SEG3D_MAX_VIEWS 3
        typedef struct {
          float scale, cos_a;      /* several names per declaration */
          int32_t a, b;
        } seg3d_view;
        typedef struct {
          const float* src;        /* pointers of any constness */
          void* dst;
          int32_t n_views;
          double w[2], bias;       /* a literal bound */
          int64_t ids[SEG3D_MAX_VIEWS];
          seg3d_view views[SEG3D_MAX_VIEWS];
          seg3d_view one;
        } seg3d_table;
        int seg3d_use(const seg3d_table* t);
    """)
    view, table = structs["seg3d_view"], structs["seg3d_table"]
    assert issubclass(view, ctypes.Structure) and view.__name__ == "seg3d_view"
    assert view._fields_ == [("scale", F), ("cos_a", F), ("a", I32), ("b", I32)] and ctypes.sizeof(view) == 16
    assert [n for n, _ in table._fields_] == ["src", "dst", "n_views", "w", "bias", "ids", "views", "one"]
    kinds = dict(table._fields_)
    assert kinds["src"] is P and kinds["dst"] is P and kinds["n_views"] is I32 and kinds["bias"] is D
    assert (kinds["w"]._type_, kinds["w"]._length_) == (D, 2) and (kinds["ids"]._type_, kinds["ids"]._length_) == (I64, 3)
    assert (kinds["views"]._type_, kinds["views"]._length_) == (view, 3) and kinds["one"] is view
    assert [getattr(table, n).offset for n, _ in table._fields_] == [0, 8, 16, 24, 40, 48, 72, 120]
    assert ctypes.sizeof(table) == 136
    assert sigs == {"seg3d_use": (I32, [P])}
    t = table()
    t.views[2].b = 7
    assert t.views[2].b == 7 and t.one.a == 0


STRUCT = "typedef struct { int32_t n; } seg3d_rec;\n"
REFUSED = [
    ("unknown parameter type", "int seg3d_f(int32_t n, unsigned flag);", "seg3d_f"),
    ("unknown return type", "void seg3d_g(int32_t n);", "seg3d_g"),
    ("unknown two-word type", "int seg3d_h(long long n);", "seg3d_h"),
    ("unknown field type", "typedef struct { uint8_t tag; } seg3d_bad_rec;", "seg3d_bad_rec"),
    ("struct used before its typedef", "typedef struct { seg3d_later x; } seg3d_early;", "seg3d_early"),
    ("struct by value", STRUCT + "int seg3d_by_value(seg3d_rec r, int32_t n);", "seg3d_by_value"),
    ("const struct by value", STRUCT + "int seg3d_by_cvalue(const seg3d_rec r);", "seg3d_by_cvalue"),
    ("function-pointer parameter", "int seg3d_cb(void (*done)(int32_t, void*), void* arg);", "seg3d_cb"),
    ("function-pointer field", "typedef struct { int (*cb)(void); } seg3d_cb_rec;", "seg3d_cb_rec"),
    ("array parameter", "int seg3d_arr(int32_t shape[3]);", "seg3d_arr"),
    ("pointer return other than const char*", "float* seg3d_ptr(void);", "seg3d_ptr"),
    ("declaration it cannot fully parse", "int seg3d_broken(int32_t n;", "seg3d_broken"),
    ("declaration with a body", "static inline int seg3d_inline(int32_t n) { return n; }", "seg3d_inline"),
    ("something else at file scope", "int seg3d_ok(void);\nextern int counter;", "counter"),
    ("define that is no integer", "#define SEG3D_SCALE 1.5f", "SEG3D_SCALE"),
    ("define built from another", "#define SEG3D_A 1\n#define SEG3D_B (SEG3D_A + 1)", "SEG3D_B"),
    ("function-like define", "#define SEG3D_MAX(a, b) ((a) > (b) ? (a) : (b))", "SEG3D_MAX"),
    ("pragma that changes layout", "#pragma pack(1)\ntypedef struct { int32_t n; double x; } seg3d_packed;", "#pragma pack(1)"),
    ("conditional declaration", "#if SEG3D_WIDE\nint seg3d_wide(void);\n#endif", "#if SEG3D_WIDE"),
    ("array bound that is no define", "typedef struct { float v[SEG3D_NOWHERE]; } seg3d_vec;", "SEG3D_NOWHERE"),
    ("array bound by expression", "#define SEG3D_N 4\ntypedef struct { float v[SEG3D_N * 2]; } seg3d_vec2;", "seg3d_vec2"),
    ("zero array bound", "typedef struct { float v[0]; } seg3d_vec0;", "seg3d_vec0"),
    ("two-dimensional array", "typedef struct { double m[3][4]; } seg3d_mat;", "seg3d_mat"),
]


@pytest.mark.parametrize("text,named", [r[1:] for r in REFUSED], ids=[r[0] for r in REFUSED])
def test_parser_refuses_by_name(text, named):
    with pytest.raises(_lib.HeaderError, match=re.escape(named)):
        _lib.parse_header(text)


def test_the_header_itself():
    """What the package exports is what the header says, under the spellings callers use."""
    with open(_lib.HEADER_PATH) as f:
        text = f.read()
    defines, structs, sigs = _lib.parse_header(text)
    assert sigs == _lib.SIGNATURES and defines == _lib.DEFINES and sorted(structs) == sorted(_lib.STRUCTS)
    assert sorted(sigs) == _lib.header_symbols()
    assert sorted(structs) == sorted(re.findall(r"^\}\s*(seg3d_\w+)\s*;", text, flags=re.M)) and len(structs) >= 16
    plain = dict((n, int(v.strip("()"))) for n, v in re.findall(r"^#define SEG3D_(\w+) (\(?-?\d+\)?)", text, flags=re.M))
    assert plain == defines and len(defines) >= 30
    for name, value in defines.items():
        assert getattr(_lib, name) == value
    assert (_lib.OK, _lib.EINVAL, _lib.EWORKSPACE, _lib.ELAUNCH) == (0, -1, -2, -3)
    assert _lib.struct("seg3d_tta_table") is _lib.STRUCTS["seg3d_tta_table"]
    with pytest.raises(KeyError):
        _lib.struct("seg3d_no_such_record")
    import numpy as np
    for name, size in (("seg3d_pack_job", 48), ("seg3d_reduce_job", 56), ("seg3d_optim_tensor", 64), ("seg3d_instance_cluster", 56)):
        dt = np.dtype(_lib.struct(name))  # the record dtype of a device table
        assert dt.itemsize == size == ctypes.sizeof(_lib.struct(name))
        assert list(dt.names) == [n for n, _ in _lib.struct(name)._fields_]
        assert [dt.fields[n][1] for n in dt.names] == [getattr(_lib.struct(name), n).offset for n in dt.names]
    assert np.dtype(_lib.struct("seg3d_pack_job"))["dst"] == np.dtype("<u8")


def _host_cc():
    for cand in ("cc", "/opt/rocm/llvm/bin/clang", "/opt/rocm/lib/llvm/bin/clang"):
        path = shutil.which(cand)
        if path:
            return path
    return None


def test_struct_layouts_against_the_c_compiler(tmp_path):
    """The host C compiler is the judge of layout: a C program (C, not C++: the header claims to be plain C) that includes
    the header prints sizeof and every offsetof; the derived ctypes classes must say the same."""
    cc = _host_cc()
    if cc is None:
        pytest.skip("no host C compiler (cc, or the clang of the ROCm tree)")
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "seg3d_hip.h"', 'int main(void) {']
    expected = []
    for name, cls in _lib.STRUCTS.items():
        lines.append(f'  printf("{name} sizeof %zu\\n", sizeof({name}));')
        expected.append(f"{name} sizeof {ctypes.sizeof(cls)}")
        for field, _ in cls._fields_:
            lines.append(f'  printf("{name} {field} %zu %zu\\n", offsetof({name}, {field}), sizeof((({name}*)0)->{field}));')
            expected.append(f"{name} {field} {getattr(cls, field).offset} {getattr(cls, field).size}")
    lines += ['  printf("abi %d\\n", SEG3D_ABI_VERSION);', '  return 0;', '}']
    expected.append(f"abi {_lib.ABI_VERSION}")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-x", "c", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(_lib.HEADER_PATH), str(src),
                    "-o", str(exe)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(expected) > 100
    assert out == expected


def _call_sites():
    """(file, line, entry name or None, positional count or None) of every _lib.call / _lib.query in the package"""
    sites = []
    for path in sorted(glob.glob(os.path.join(ROOT, "openseg3d_amd", "*.py"))):
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        for node in ast.walk(tree):
            if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in ("call", "query")
                    and isinstance(node.func.value, ast.Name) and node.func.value.id == "_lib"):
                continue
            first = node.args[0] if node.args else None
            literal = isinstance(first, ast.Constant) and isinstance(first.value, str)
            starred = any(isinstance(a, ast.Starred) for a in node.args) or node.keywords
            sites.append((os.path.basename(path), node.lineno, first.value if literal else None,
                          None if starred or not literal else len(node.args) - 1))
    return sites


def test_call_sites_pass_as_many_arguments_as_the_header_declares():
    sites = _call_sites()
    checked = [s for s in sites if s[3] is not None]
    skipped = [s for s in sites if s[3] is None]
    print(f"{len(sites)} call sites, {len(checked)} checked, {len(skipped)} skipped (computed name or *args): "
          f"{[s[:2] for s in skipped]}")
    wrong = [(f, line, name, n, len(_lib.SIGNATURES[name][1])) for f, line, name, n in checked
             if name not in _lib.SIGNATURES or n != len(_lib.SIGNATURES[name][1])]
    assert not wrong, wrong
    for f, line, name, _ in skipped:  # a literal name with *args still has to exist
        assert name is None or name in _lib.SIGNATURES, (f, line, name)
    # When this test was written the package had 169 sites, 16 of them (9.5 %) with a computed name or *args (the list is
    # printed above).  The cap leaves room for a few more of those, not for the check to empty out.
    assert len(checked) >= 100
    assert len(skipped) <= 0.15 * len(sites)


def test_library_matches_the_header_version():
    with open(_lib.HEADER_PATH) as f:
        define = re.search(r"^#define SEG3D_ABI_VERSION (\d+)$", f.read(), flags=re.M)
    assert define and int(define.group(1)) == _lib.ABI_VERSION
    assert _lib.load().seg3d_abi_version() == _lib.ABI_VERSION
