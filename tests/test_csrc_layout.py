"""Source-text checks of csrc/: the split-bf16 arithmetic is defined once, in split_bf16.hpp, and
only the attention kernels reach for attn_common.hpp."""
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
