// a19-a21: C-ABI entry points of the ragged sparse-window cosine attention (include/seg3d_hip.h) and the choice of
// kernels behind them.  Reference: flat2window -> CosineMultiheadAttention -> window2flat (swformer_utils.py:34-85,
// point_transformer_layer.py:233-258, cosine_msa.py:115-177).
//   forward   attention_fused.hip      persistent fused kernel, every head width (dh 6 / 12 / 24 / 48), dropout-capable
//             attention_small.hip      exact-fp32 vector-ALU kernel, dh 6 with dropout (round 4: 101 / 96 -> 86 / 73 us per layer)
//   backward  attention_fused_bwd.hip  two flash-style passes, dh 12 / 24 / 48
//             attention_small.hip      exact-fp32 vector-ALU passes, dh 6 (windows of ~15 voxels: 360 vs 475 us per layer)
// Every kernel above is instantiated for three attention modes (attn_common.hpp): the shared tau of seg3d_window_attn_fwd /
// _bwd, and per-head tau and scaled dot product behind seg3d_window_attn_fwd_modes / _bwd_modes (cosine_msa.py:156-165).
// Both entry sets are thin: each fills the argument record of attn_common.hpp from its parameters and calls attn_forward /
// attn_backward / attn_workspace_bytes below, where the validation, the choice of kernels, the workspace check and the launch
// are written once.  What the two sets answer differently on purpose is spelled out in EntryRules.
// Head geometries these kernels do not take (narrow heads whose count is not a multiple of 4, head widths other than the
// four the reference builds -- pointtransformer.py:143-155: 8 heads of 6 / 12 / 24 / 48 channels) are refused with
// SEG3D_EINVAL; seg3d_window_attn_supported says so up front.  The round-1 / round-2 fallbacks (prepare pass + core,
// three-launch backward with prepared operands through HBM, vector-ALU forward) were removed in round 3: nothing on the
// reference's path reached them and their workspace demand (gigabytes on a 2 M-point scene) leaked into every call.
#include "attn_common.hpp"

namespace {

// backward kernels for a head geometry: 0 fused (two flash-style passes), 1 vector-ALU (dh 6), -1 none
int bwd_path(int heads, int dh) {
    if (!attn_fused_supported(heads, dh)) return -1;
    if (attn_fused_bwd_supported(heads, dh)) return 0;
    if (attn_small_supported(heads, dh)) return 1;
    return -1;
}

// dh 6 (stage 1: windows of ~15 voxels) WITH dropout: exact fp32 on the vector ALUs, like its backward -- one hash per key
// pair and thread instead of the MFMA kernel's per-fragment mask: 101 -> 86 / 96 -> 73 us per layer (shift 0 / 1).  Without
// dropout the two forms tie (84 / 67 against 72 / 66 us) and the fused kernel stays.  SEG3D_ATTN_SMALL_FWD=0 | 1 | 2 (A/B):
// never / with dropout (default) / always.  (The vector-ALU kernel always writes the LSE: a caller that passes none stays
// on the fused one.)
bool small_fwd_runs(int heads, int dh, float dropout_p, bool has_lse) {
    static const int small_fwd = env_int("SEG3D_ATTN_SMALL_FWD", 1);
    return (small_fwd == 2 || (small_fwd == 1 && dropout_p > 0.f)) && attn_small_supported(heads, dh) && has_lse;
}

// kernel instantiation (attn_common.hpp: kShared / kPerHead / kDot) for a mode of the header and a count of tau values;
// -1 for a pair the entries refuse: cosine takes 1 or `heads` values, dot none
int attn_kernel_mode(int mode, int n_tau, int heads) {
    if (mode == SEG3D_ATTN_DOT) return n_tau == 0 ? attn::kDot : -1;
    if (mode != SEG3D_ATTN_COSINE) return -1;
    if (n_tau == 1) return attn::kShared;
    return n_tau == heads && heads > 1 ? attn::kPerHead : -1;
}

bool rows_misaligned(const void* a, const void* b, const void* c, int lda, int ldb, int ldc) {
    return ((lda | ldb | ldc) & 3) ||
           ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15);
}

// bytes the backward kernels of `path` use: one tau-gradient partial per wave plus <dO, O> per (token, head) between the
// two passes (fused), or one partial per tile -- per (tile, head) with per-head tau -- (vector-ALU)
size_t bwd_workspace_bytes(int path, int64_t m, int n_tiles, int n_chunks, int heads, int dh, int n_tau) {
    return path == 0 ? attn_fused_bwd_workspace_bytes(m, n_tiles, n_chunks, heads, dh)
                     : attn_small_blocks(n_tiles) * (n_tau > 1 ? n_tau : 1) * sizeof(float);
}

size_t attn_workspace_bytes(int64_t m, int n_tiles, int heads, int dh, int mode, int n_tau) {
    const int path = bwd_path(heads, dh);
    if (m < 0 || heads <= 0 || n_tiles < 0 || attn_kernel_mode(mode, n_tau, heads) < 0 || path < 0) return 0;
    return bwd_workspace_bytes(path, m, n_tiles, n_tiles, heads, dh, n_tau) + 256;  // chunks <= tiles
}

// Where the shared-tau entries and the _modes entries differ on purpose; everything else is one path.  (Three more
// differences need no rule, they follow from (mode, n_tau): per-head tau at dh 6 takes the vector-ALU forward without
// dropout too, an empty backward zeroes n_tau floats of dtau, and dot mode takes no dtau where cosine mode needs one.)
struct EntryRules {
    bool empty_before_tau;  // an empty problem is SEG3D_OK even without a tau (shared); _modes refuses a cosine call
                            // without tau, or any (mode, n_tau) it does not know, before it looks at the sizes
    bool fwd_without_bwd;   // the forward takes every geometry attn_fused_supported takes, 12 heads x dh 6 included,
                            // which has no backward (shared); _modes requires seg3d_window_attn_supported
};
constexpr EntryRules kSharedEntry{true, true}, kModesEntry{false, false};

bool dropout_in_range(float p) { return p >= 0.f && p < 1.f; }

int attn_forward(AttnArgs a, float* out, float* lse, int mode, int n_tau, int n_windows, float dropout_p, EntryRules rules) {
    a.am = attn_kernel_mode(mode, n_tau, a.heads);
    const bool tau_fits = a.am >= 0 && (mode == SEG3D_ATTN_DOT) == (a.tau == nullptr);
    if (!rules.empty_before_tau && !tau_fits) return SEG3D_EINVAL;
    if (a.m == 0 || n_windows == 0 || a.n_tiles == 0 || a.n_chunks == 0) return SEG3D_OK;
    if (!a.q || !a.k || !a.v || !a.tok || !a.win_start || !a.win_count || !a.tile_item || !a.chunk_item || a.m < 0 ||
        n_windows < 0 || a.n_tiles < 0 || a.n_chunks < 0 || a.heads <= 0 || a.heads > 16 || !tau_fits || !out ||
        !dropout_in_range(dropout_p))
        return SEG3D_EINVAL;
    if (!(rules.fwd_without_bwd ? attn_fused_supported(a.heads, a.dh) : seg3d_window_attn_supported(a.heads, a.dh) != 0))
        return SEG3D_EINVAL;
    if (rows_misaligned(a.q, a.k, a.v, a.ldq, a.ldk, a.ldv)) return SEG3D_EINVAL;  // rows are gathered in 16-B pieces
    // Per-head tau at dh 6 takes the exact-fp32 vector-ALU forward without dropout too: a head near tau_min has scores of 72 -
    // 144 log2 units, and over 6 channels the split-bf16 score product (2^-18 per operand) puts the forward of such a head at
    // 1.3 x its per-head bar (6.7e-4 against 5.3e-4 at tau 0.02); in fp32 it stands at a tenth of it.  The two forms tie on
    // time without dropout (see small_fwd_runs).
    if ((a.am == attn::kPerHead && attn_small_supported(a.heads, a.dh) && lse != nullptr) ||
        small_fwd_runs(a.heads, a.dh, dropout_p, lse != nullptr))
        return attn_small_fwd_launch(a, out, lse);
    return attn_fused_fwd_launch(a, out, lse);
}

int attn_backward(AttnBwdArgs a, int mode, int n_tau, int n_windows, float dropout_p, size_t workspace_bytes, EntryRules rules) {
    if (!dropout_in_range(dropout_p)) return SEG3D_EINVAL;
    a.am = attn_kernel_mode(mode, n_tau, a.heads);
    const bool dot = mode == SEG3D_ATTN_DOT;
    const bool tau_fits = a.am >= 0 && dot == (a.tau == nullptr) && !(dot && a.dtau);
    if (!rules.empty_before_tau && !tau_fits) return SEG3D_EINVAL;
    if (a.m == 0 || n_windows == 0 || a.n_tiles == 0 || a.n_chunks == 0) {
        if (a.dtau) SEG3D_CHECK_HIP(hipMemsetAsync(a.dtau, 0, (size_t)n_tau * sizeof(float), a.st));
        return SEG3D_OK;
    }
    if (!a.q || !a.k || !a.v || !a.out || !a.dout || !a.lse || !a.tok || !a.win_start || !a.win_count || !a.tile_item ||
        !a.chunk_item || a.m < 0 || n_windows < 0 || a.n_tiles < 0 || a.n_chunks < 0 || a.heads <= 0 || a.heads > 16 ||
        !tau_fits || !a.dq || !a.dk || !a.dv || (!dot && !a.dtau) || !a.workspace)
        return SEG3D_EINVAL;
    if (rows_misaligned(a.q, a.k, a.v, a.ldq, a.ldk, a.ldv) || rows_misaligned(a.dq, a.dk, a.dv, a.lddq, a.lddk, a.lddv))
        return SEG3D_EINVAL;  // rows are gathered / stored in 16-B pieces
    const int path = bwd_path(a.heads, a.dh);
    if (path < 0) return SEG3D_EINVAL;
    if (workspace_bytes < bwd_workspace_bytes(path, a.m, a.n_tiles, a.n_chunks, a.heads, a.dh, n_tau)) return SEG3D_EWORKSPACE;
    return path == 0 ? attn_fused_bwd_launch(a) : attn_small_bwd_launch(a);
}

// The record from an entry's own parameters: the four entries name them alike, so every field is filled from the parameter
// of its name (qg_item is the kernels' chunk list).  The dropout pair becomes the mask parameters here, once: forward and
// backward of a layer get the same mask from the same two values.
#define SEG3D_ATTN_ARGS(a)                                                                                            \
    a.q = q, a.k = k, a.v = v, a.ldq = ldq, a.ldk = ldk, a.ldv = ldv;                                                 \
    a.tok = tok, a.win_start = win_start, a.win_count = win_count;                                                    \
    a.tile_item = reinterpret_cast<const int4*>(tile_item), a.n_tiles = n_tiles;                                      \
    a.chunk_item = reinterpret_cast<const int4*>(qg_item), a.n_chunks = n_qgroups;                                    \
    a.m = m, a.heads = heads, a.dh = dh, a.tau = tau, a.tau_min = tau_min, a.am = -1;                                 \
    a.drop = make_dropout(dropout_p, dropout_seed), a.st = as_stream(stream)
#define SEG3D_ATTN_BWD_ARGS(a)                                                                                        \
    SEG3D_ATTN_ARGS(a);                                                                                               \
    a.out = out, a.dout = dout, a.lse = lse, a.dq = dq, a.dk = dk, a.dv = dv, a.lddq = lddq, a.lddk = lddk, a.lddv = lddv; \
    a.dtau = dtau, a.workspace = workspace

}  // namespace

extern "C" {

int seg3d_window_attn_supported(int32_t heads, int32_t dh) {
    return heads > 0 && heads <= 16 && bwd_path(heads, dh) >= 0 ? 1 : 0;
}

// Bytes for the kernels seg3d_window_attn_fwd / _bwd take with these arguments: nothing in the forward, one tau-gradient
// partial per wave (fused) or per tile (vector-ALU) in the backward, plus <dO, O> per (token, head) between its two passes.
size_t seg3d_window_attn_workspace_bytes(int64_t m, int32_t n_tiles, int32_t heads, int32_t dh) {
    return attn_workspace_bytes(m, n_tiles, heads, dh, SEG3D_ATTN_COSINE, 1);
}

// Host only (no launch): the kernels and grids seg3d_window_attn_fwd (given an lse) / _bwd take for these counts, from the
// same functions the launchers call.
int seg3d_window_attn_schedule(int32_t n_tiles, int32_t n_chunks, int32_t heads, int32_t dh, float dropout_p, int32_t* out) {
    if (!out || n_tiles < 0 || n_chunks < 0 || n_chunks > n_tiles || !(dropout_p >= 0.f && dropout_p < 1.f) ||
        !seg3d_window_attn_supported(heads, dh))
        return SEG3D_EINVAL;
    if (small_fwd_runs(heads, dh, dropout_p, true)) {  // one workgroup per tile: no cap, no walk, no XCD blocks
        const int blocks = (int)attn_small_blocks(n_tiles);
        out[0] = 1, out[1] = 0, out[2] = blocks, out[3] = blocks > 0 ? 1 : 0, out[4] = 1;
    } else {
        int cap = 0, grid = 0, walked = 0, xb = 0;
        const int rc = attn_fused_fwd_schedule(n_tiles, n_chunks, heads, dh, dropout_p > 0.f, &cap, &grid, &walked, &xb);
        if (rc != SEG3D_OK) return rc;
        out[0] = 0, out[1] = cap, out[2] = grid, out[3] = walked, out[4] = xb;
    }
    out[5] = (int32_t)(bwd_path(heads, dh) == 0 ? attn_fused_bwd_blocks(n_tiles, n_chunks, heads, dh) : attn_small_blocks(n_tiles));
    return SEG3D_OK;
}

int seg3d_window_attn_fwd(const float* q, const float* k, const float* v, int32_t ldq, int32_t ldk, int32_t ldv,
                          const int32_t* tok, const int32_t* win_start, const int32_t* win_count,
                          const int32_t* win_tile0, const int32_t* tile_item, int32_t n_tiles, const int32_t* qg_item,
                          int32_t n_qgroups, int64_t m, int32_t n_windows, int32_t heads, int32_t dh, const float* tau,
                          float tau_min, float dropout_p, uint64_t dropout_seed, float* out, float* lse, void* workspace,
                          size_t workspace_bytes, void* stream) {
    (void)win_tile0;
    (void)workspace;
    (void)workspace_bytes;
    AttnArgs a;
    SEG3D_ATTN_ARGS(a);
    return attn_forward(a, out, lse, SEG3D_ATTN_COSINE, 1, n_windows, dropout_p, kSharedEntry);
}

int seg3d_window_attn_bwd(const float* q, const float* k, const float* v, int32_t ldq, int32_t ldk, int32_t ldv,
                          const float* out, const float* dout, const float* lse, const int32_t* tok,
                          const int32_t* win_start, const int32_t* win_count, const int32_t* win_tile0,
                          const int32_t* tile_item, int32_t n_tiles, const int32_t* qg_item, int32_t n_qgroups, int64_t m,
                          int32_t n_windows, int32_t heads, int32_t dh, const float* tau, float tau_min, float dropout_p,
                          uint64_t dropout_seed, float* dq, float* dk, float* dv, int32_t lddq, int32_t lddk, int32_t lddv,
                          float* dtau, void* workspace, size_t workspace_bytes, void* stream) {
    (void)win_tile0;
    AttnBwdArgs a;
    SEG3D_ATTN_BWD_ARGS(a);
    return attn_backward(a, SEG3D_ATTN_COSINE, 1, n_windows, dropout_p, workspace_bytes, kSharedEntry);
}

// ---- per-head tau and scaled-dot-product modes (cosine_msa.py:156-160 with non_shared_tau=True; :163-165).  The same
// path as the entries above with (mode, n_tau) from the caller and the stricter rules of kModesEntry; (cosine, 1) runs the
// shared-tau kernels.
size_t seg3d_window_attn_workspace_bytes_modes(int64_t m, int32_t n_tiles, int32_t heads, int32_t dh, int32_t mode,
                                               int32_t n_tau) {
    return attn_workspace_bytes(m, n_tiles, heads, dh, mode, n_tau);
}

int seg3d_window_attn_fwd_modes(const float* q, const float* k, const float* v, int32_t ldq, int32_t ldk, int32_t ldv,
                                const int32_t* tok, const int32_t* win_start, const int32_t* win_count,
                                const int32_t* tile_item, int32_t n_tiles, const int32_t* qg_item, int32_t n_qgroups, int64_t m,
                                int32_t n_windows, int32_t heads, int32_t dh, int32_t mode, const float* tau, int32_t n_tau,
                                float tau_min, float dropout_p, uint64_t dropout_seed, float* out, float* lse, void* workspace,
                                size_t workspace_bytes, void* stream) {
    (void)workspace;
    (void)workspace_bytes;
    AttnArgs a;
    SEG3D_ATTN_ARGS(a);
    return attn_forward(a, out, lse, mode, n_tau, n_windows, dropout_p, kModesEntry);
}

int seg3d_window_attn_bwd_modes(const float* q, const float* k, const float* v, int32_t ldq, int32_t ldk, int32_t ldv,
                                const float* out, const float* dout, const float* lse, const int32_t* tok,
                                const int32_t* win_start, const int32_t* win_count, const int32_t* tile_item, int32_t n_tiles,
                                const int32_t* qg_item, int32_t n_qgroups, int64_t m, int32_t n_windows, int32_t heads,
                                int32_t dh, int32_t mode, const float* tau, int32_t n_tau, float tau_min, float dropout_p,
                                uint64_t dropout_seed, float* dq, float* dk, float* dv, int32_t lddq, int32_t lddk,
                                int32_t lddv, float* dtau, void* workspace, size_t workspace_bytes, void* stream) {
    AttnBwdArgs a;
    SEG3D_ATTN_BWD_ARGS(a);
    return attn_backward(a, mode, n_tau, n_windows, dropout_p, workspace_bytes, kModesEntry);
}

}  // extern "C"
