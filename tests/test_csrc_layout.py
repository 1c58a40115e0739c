"""Source-text checks of csrc/: the split-bf16 arithmetic is defined once, in split_bf16.hpp, and
only the attention kernels reach for attn_common.hpp; the fixed-order wave / workgroup sums, the instance recipes, the
prototypes of functions shared between .hip files and the readers of the environment have one home each as well."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openseg3d_amd", "csrc")
HOME = "split_bf16.hpp"

HELPERS = ("pack_bf16", "split1", "split2", "split3", "split8", "split_frag", "split_frag2", "mfma2", "mfma3",
           "frag_from_bf16_rows", "load_frag")
VECTOR_TYPES = ("f32x4", "f32x2", "bf16x8", "bf16x2", "u32x4")
# not MFMA kernels: each keeps its own single-line typedefs of the float vectors it loads and stores with
OWN_FLOAT_TYPEDEFS = {"spconv.hip": {"f32x4"}, "pointops.hip": {"f32x4"}, "sa_gate.hip": {"f32x4"},
                      "knn_attention.hip": {"f32x4", "f32x2"}}
ATTENTION = {"attention.hip", "attention_small.hip", "attention_fused.hip", "attention_fused_bwd.hip", "attn_fused.hpp",
             "attn_dropout.hpp"}


def _sources():
    out = {}
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".hpp")):
            text = open(os.path.join(CSRC, f)).read()
            text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
            out[f] = re.sub(r"//[^\n]*", "", text)  # comments may name a helper
    return out


def _defined_in(name, sources):
    """files with `<type> name(<parameters>) {`: a definition, not a call (a call has no type in front) or a declaration"""
    pat = re.compile(r"[\w>&*]\s+" + name + r"\s*\([^;{}()]*\)\s*\{")
    return {f for f, text in sources.items() if pat.search(text)}


def test_split_helpers_are_defined_once():
    sources = _sources()
    assert HOME in sources
    for name in HELPERS:
        where = _defined_in(name, sources)
        assert where == {HOME},f"{name} is defined in {sorted(where)}, expected only {HOME}"


def test_vector_typedefs_live_in_the_split_header():
    sources = _sources()
    for name in VECTOR_TYPES:
        pat = re.compile(r"typedef[^;]*\b" + name + r"\b[^;]*ext_vector_type[^;]*;")
        where = {f for f, text in sources.items() if pat.search(text)}
        allowed = {HOME} | {f for f, names in OWN_FLOAT_TYPEDEFS.items() if name in names}
        assert HOME in where, name
        assert where <= allowed, f"{name} is declared in {sorted(where - allowed)}"


def test_only_attention_includes_attn_common():
    users = {f for f, text in _sources().items() if re.search(r'#\s*include\s*"attn_common\.hpp"', text)}
    assert users and users <= ATTENTION, sorted(users - ATTENTION)


# ---- the other shared recipes ("Where the other shared recipes are defined")
SHARED_HELPERS = {
    "wave_ops.hpp": ("wave_sum", "wave_scan_inclusive", "block_sum", "block_scan_inclusive"),
    "instance_geom.hpp": ("closer", "dist3", "block_sum3", "block_max", "sum3_host", "label_at"),
}
PROTOTYPE_HEADERS = ("common.hpp", "attn_common.hpp")
# Full-wave xor sums that stay written out, by file: through the helper the compiler assembles their kernel with other
# instructions than before (tools/isa_diff.py: `different instructions`), or, in the attention files, which carry the
# step's time, with any difference at all.
#   criterion_device.hpp     lovasz_chunk_count and the dot of lovasz_chunk_grad (an extra exec-mask instruction / the keys
#                            loaded as two dwords instead of one qword)
#   loss_select.hip          select_finalize_kernel (a branch comes out inverted)
#   attention_small.hip      pass Q's tau gradient; tau_reduce_small
#   attention_fused_bwd.hip  pass Q's tau gradient; tau_reduce_fused: the same kernel as tau_reduce_small, and still a copy,
#                            because one shared body renumbers the registers of both
XOR_SUMS_LEFT = {"criterion_device.hpp": 2, "loss_select.hip": 1, "attention_small.hip": 2, "attention_fused_bwd.hip": 2}


def _includes(f, sources, seen=None):
    """f and every csrc header it includes, directly or through another"""
    seen = {f} if seen is None else seen
    for h in re.findall(r'#\s*include\s*"(\w+\.hpp)"', sources[f]):
        if h in sources and h not in seen:
            seen.add(h)
            _includes(h, sources, seen)
    return seen


def test_shared_helpers_are_defined_once():
    sources = _sources()
    for home, names in SHARED_HELPERS.items():
        assert home in sources
        for name in names:
            where = _defined_in(name, sources)
            assert where == {home}, f"{name} is defined in {sorted(where)}, expected only {home}"


def test_environment_is_read_in_common_only():
    where = {f for f, text in _sources().items() if "getenv(" in text}
    assert where == {"common.hpp"}, sorted(where)


def test_cross_file_functions_are_declared_once():
    sources = _sources()
    head = r"^(?:int|size_t|bool|void)\s+"
    checked = 0
    for header in PROTOTYPE_HEADERS:
        for name in re.findall(head + r"(\w+)\s*\([^;{}]*\)\s*;", sources[header], flags=re.M):
            copies = {f for f, text in sources.items()
                      if f != header and re.search(head + name + r"\s*\([^;{}]*\)\s*;", text, flags=re.M)}
            assert not copies, f"{name} is declared again in {sorted(copies)}"
            defs = {f for f, text in sources.items() if re.search(head + name + r"\s*\([^;{}]*\)\s*\{", text, flags=re.M)}
            assert len(defs) == 1 and next(iter(defs)).endswith(".hip"), f"{name} is defined in {sorted(defs)}"
            assert header in _includes(next(iter(defs)), sources), f"{defs} defines {name} without seeing {header}"
            checked += 1
    assert checked >= 22  # 11 attention launchers / queries, 11 of the conv, weight-gradient, group, scan and error files


def test_full_wave_sums_come_from_wave_ops():
    loop = re.compile(r"off = 32; off > 0; off >>= 1\)[^;]*__shfl_xor")
    found = {f: len(loop.findall(text)) for f, text in _sources().items() if loop.search(text)}
    assert found.pop("wave_ops.hpp", 0) > 0
    assert found == XOR_SUMS_LEFT
