// a19-a21: C-ABI entry points of the ragged sparse-window cosine attention (include/seg3d_hip.h) and the choice of
// kernels behind them.  Reference: flat2window -> CosineMultiheadAttention -> window2flat (swformer_utils.py:34-85,
// point_transformer_layer.py:233-258, cosine_msa.py:115-177).
//   forward   attention_fused.hip      persistent fused kernel, every head width (dh 6 / 12 / 24 / 48), dropout-capable
//             attention_small.hip      exact-fp32 vector-ALU kernel, dh 6 with dropout (round 4: 101 / 96 -> 86 / 73 us per layer)
//   backward  attention_fused_bwd.hip  two flash-style passes, dh 12 / 24 / 48
//             attention_small.hip      exact-fp32 vector-ALU passes, dh 6 (windows of ~15 voxels: 360 vs 475 us per layer)
// Every kernel above is instantiated for three attention modes (attn_common.hpp): the shared tau of seg3d_window_attn_fwd /
// _bwd, and per-head tau and scaled dot product behind seg3d_window_attn_fwd_modes / _bwd_modes (below; cosine_msa.py:156-165).
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

}  // namespace

extern "C" {

int seg3d_window_attn_supported(int32_t heads, int32_t dh) {
    return heads > 0 && heads <= 16 && bwd_path(heads, dh) >= 0 ? 1 : 0;
}

// Bytes for the kernels seg3d_window_attn_fwd / _bwd take with these arguments: nothing in the forward, one tau-gradient
// partial per wave (fused) or per tile (vector-ALU) in the backward, plus <dO, O> per (token, head) between its two passes.
size_t seg3d_window_attn_workspace_bytes(int64_t m, int32_t n_tiles, int32_t heads, int32_t dh) {
    if (m < 0 || heads <= 0 || n_tiles < 0) return 0;
    size_t bwd = 0;
    switch (bwd_path(heads, dh)) {
        case 0: bwd = attn_fused_bwd_workspace_bytes(m, n_tiles, n_tiles, heads, dh); break;  // chunks <= tiles
        case 1: bwd = attn_small_blocks(n_tiles) * sizeof(float); break;
        default: return 0;
    }
    return bwd + 256;
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
    if (m == 0 || n_windows == 0 || n_tiles == 0 || n_qgroups == 0) return SEG3D_OK;
    if (!q || !k || !v || !tok || !win_start || !win_count || !tile_item || !qg_item || m < 0 || n_windows < 0 ||
        n_tiles < 0 || n_qgroups < 0 || heads <= 0 || heads > 16 || !tau || !out || !(dropout_p >= 0.f && dropout_p < 1.f))
        return SEG3D_EINVAL;
    if (!attn_fused_supported(heads, dh)) return SEG3D_EINVAL;
    if (rows_misaligned(q, k, v, ldq, ldk, ldv)) return SEG3D_EINVAL;  // rows are gathered in 16-B pieces
    if (small_fwd_runs(heads, dh, dropout_p, lse != nullptr))
        return attn_small_fwd_launch(q, k, v, ldq, ldk, ldv, tok, win_start, win_count, tile_item, n_tiles, heads, dh, tau, tau_min,
                                     out, lse, make_dropout(dropout_p, dropout_seed), as_stream(stream), attn::kShared);
    return attn_fused_fwd_launch(q, k, v, ldq, ldk, ldv, tok, win_start, win_count, tile_item, n_tiles, qg_item, n_qgroups,
                                 heads, dh, tau, tau_min, out, lse, dropout_p, dropout_seed, as_stream(stream), attn::kShared);
}

int seg3d_window_attn_bwd(const float* q, const float* k, const float* v, int32_t ldq, int32_t ldk, int32_t ldv,
                          const float* out, const float* dout, const float* lse, const int32_t* tok,
                          const int32_t* win_start, const int32_t* win_count, const int32_t* win_tile0,
                          const int32_t* tile_item, int32_t n_tiles, const int32_t* qg_item, int32_t n_qgroups, int64_t m,
                          int32_t n_windows, int32_t heads, int32_t dh, const float* tau, float tau_min, float dropout_p,
                          uint64_t dropout_seed, float* dq, float* dk, float* dv, int32_t lddq, int32_t lddk, int32_t lddv,
                          float* dtau, void* workspace, size_t workspace_bytes, void* stream) {
    (void)win_tile0;
    if (!(dropout_p >= 0.f && dropout_p < 1.f)) return SEG3D_EINVAL;
    const DropoutParams drop = make_dropout(dropout_p, dropout_seed);  // same mask as the forward, given the same two values
    if (m == 0 || n_windows == 0 || n_tiles == 0 || n_qgroups == 0) {
        if (dtau) SEG3D_CHECK_HIP(hipMemsetAsync(dtau, 0, sizeof(float), as_stream(stream)));
        return SEG3D_OK;
    }
    if (!q || !k || !v || !out || !dout || !lse || !tok || !win_start || !win_count || !tile_item || !qg_item || m < 0 ||
        n_windows < 0 || n_tiles < 0 || n_qgroups < 0 || heads <= 0 || heads > 16 || !tau || !dq || !dk || !dv || !dtau ||
        !workspace)
        return SEG3D_EINVAL;
    if (rows_misaligned(q, k, v, ldq, ldk, ldv) || rows_misaligned(dq, dk, dv, lddq, lddk, lddv))
        return SEG3D_EINVAL;  // rows are gathered / stored in 16-B pieces
    const int path = bwd_path(heads, dh);
    if (path < 0) return SEG3D_EINVAL;
    if (path == 0) {
        if (workspace_bytes < attn_fused_bwd_workspace_bytes(m, n_tiles, n_qgroups, heads, dh)) return SEG3D_EWORKSPACE;
        return attn_fused_bwd_launch(q, k, v, ldq, ldk, ldv, out, dout, lse, tok, win_start, win_count, tile_item, n_tiles,
                                     qg_item, n_qgroups, m, heads, dh, tau, tau_min, dq, dk, dv, lddq, lddk, lddv, dtau,
                                     workspace, drop, as_stream(stream), attn::kShared);
    }
    if (workspace_bytes < attn_small_blocks(n_tiles) * sizeof(float)) return SEG3D_EWORKSPACE;
    return attn_small_bwd_launch(q, k, v, ldq, ldk, ldv, out, dout, lse, tok, win_start, win_count, tile_item, n_tiles, heads,
                                 dh, tau, tau_min, dq, dk, dv, lddq, lddk, lddv, dtau, workspace, drop, as_stream(stream),
                                 attn::kShared);
}

// ---- per-head tau and scaled-dot-product modes (cosine_msa.py:156-160 with non_shared_tau=True; :163-165).  The head
// geometries, the choice of kernels (small_fwd_runs, bwd_path) and the schedule are those of the entries above; one tau
// through these entries runs the shared-tau kernels themselves.
size_t seg3d_window_attn_workspace_bytes_modes(int64_t m, int32_t n_tiles, int32_t heads, int32_t dh, int32_t mode,
                                               int32_t n_tau) {
    if (m < 0 || heads <= 0 || n_tiles < 0 || attn_kernel_mode(mode, n_tau, heads) < 0) return 0;
    size_t bwd = 0;
    switch (bwd_path(heads, dh)) {
        case 0: bwd = attn_fused_bwd_workspace_bytes(m, n_tiles, n_tiles, heads, dh); break;  // one tau slot per wave in every mode
        case 1: bwd = attn_small_blocks(n_tiles) * (n_tau > 1 ? n_tau : 1) * sizeof(float); break;  // per (tile, head)
        default: return 0;
    }
    return bwd + 256;
}

int seg3d_window_attn_fwd_modes(const float* q, const float* k, const float* v, int32_t ldq, int32_t ldk, int32_t ldv,
                                const int32_t* tok, const int32_t* win_start, const int32_t* win_count,
                                const int32_t* tile_item, int32_t n_tiles, const int32_t* qg_item, int32_t n_qgroups, int64_t m,
                                int32_t n_windows, int32_t heads, int32_t dh, int32_t mode, const float* tau, int32_t n_tau,
                                float tau_min, float dropout_p, uint64_t dropout_seed, float* out, float* lse, void* workspace,
                                size_t workspace_bytes, void* stream) {
    (void)workspace;
    (void)workspace_bytes;
    const int am = attn_kernel_mode(mode, n_tau, heads);
    if (am < 0 || (mode == SEG3D_ATTN_DOT) != (tau == nullptr)) return SEG3D_EINVAL;
    if (m == 0 || n_windows == 0 || n_tiles == 0 || n_qgroups == 0) return SEG3D_OK;
    if (!q || !k || !v || !tok || !win_start || !win_count || !tile_item || !qg_item || m < 0 || n_windows < 0 ||
        n_tiles < 0 || n_qgroups < 0 || heads <= 0 || heads > 16 || !out || !(dropout_p >= 0.f && dropout_p < 1.f))
        return SEG3D_EINVAL;
    if (!seg3d_window_attn_supported(heads, dh)) return SEG3D_EINVAL;
    if (rows_misaligned(q, k, v, ldq, ldk, ldv)) return SEG3D_EINVAL;  // rows are gathered in 16-B pieces
    // Per-head tau at dh 6 takes the exact-fp32 vector-ALU forward without dropout too: a head near tau_min has scores of 72 -
    // 144 log2 units, and over 6 channels the split-bf16 score product (2^-18 per operand) puts the forward of such a head at
    // 1.3 x its per-head bar (6.7e-4 against 5.3e-4 at tau 0.02); in fp32 it stands at a tenth of it.  The two forms tie on
    // time without dropout (see small_fwd_runs).
    if ((am == attn::kPerHead && attn_small_supported(heads, dh) && lse != nullptr) ||
        small_fwd_runs(heads, dh, dropout_p, lse != nullptr))
        return attn_small_fwd_launch(q, k, v, ldq, ldk, ldv, tok, win_start, win_count, tile_item, n_tiles, heads, dh, tau, tau_min,
                                     out, lse, make_dropout(dropout_p, dropout_seed), as_stream(stream), am);
    return attn_fused_fwd_launch(q, k, v, ldq, ldk, ldv, tok, win_start, win_count, tile_item, n_tiles, qg_item, n_qgroups,
                                 heads, dh, tau, tau_min, out, lse, dropout_p, dropout_seed, as_stream(stream), am);
}

int seg3d_window_attn_bwd_modes(const float* q, const float* k, const float* v, int32_t ldq, int32_t ldk, int32_t ldv,
                                const float* out, const float* dout, const float* lse, const int32_t* tok,
                                const int32_t* win_start, const int32_t* win_count, const int32_t* tile_item, int32_t n_tiles,
                                const int32_t* qg_item, int32_t n_qgroups, int64_t m, int32_t n_windows, int32_t heads,
                                int32_t dh, int32_t mode, const float* tau, int32_t n_tau, float tau_min, float dropout_p,
                                uint64_t dropout_seed, float* dq, float* dk, float* dv, int32_t lddq, int32_t lddk,
                                int32_t lddv, float* dtau, void* workspace, size_t workspace_bytes, void* stream) {
    const int am = attn_kernel_mode(mode, n_tau, heads);
    if (am < 0 || !(dropout_p >= 0.f && dropout_p < 1.f)) return SEG3D_EINVAL;
    if ((mode == SEG3D_ATTN_DOT) != (tau == nullptr) || (mode == SEG3D_ATTN_DOT && dtau)) return SEG3D_EINVAL;
    const DropoutParams drop = make_dropout(dropout_p, dropout_seed);  // same mask as the forward, given the same two values
    if (m == 0 || n_windows == 0 || n_tiles == 0 || n_qgroups == 0) {
        if (dtau) SEG3D_CHECK_HIP(hipMemsetAsync(dtau, 0, (size_t)n_tau * sizeof(float), as_stream(stream)));
        return SEG3D_OK;
    }
    if (!q || !k || !v || !out || !dout || !lse || !tok || !win_start || !win_count || !tile_item || !qg_item || m < 0 ||
        n_windows < 0 || n_tiles < 0 || n_qgroups < 0 || heads <= 0 || heads > 16 || !dq || !dk || !dv ||
        (mode == SEG3D_ATTN_COSINE && !dtau) || !workspace)
        return SEG3D_EINVAL;
    if (rows_misaligned(q, k, v, ldq, ldk, ldv) || rows_misaligned(dq, dk, dv, lddq, lddk, lddv))
        return SEG3D_EINVAL;  // rows are gathered / stored in 16-B pieces
    const int path = bwd_path(heads, dh);
    if (path < 0 || !seg3d_window_attn_supported(heads, dh)) return SEG3D_EINVAL;
    const size_t need = path == 0 ? attn_fused_bwd_workspace_bytes(m, n_tiles, n_qgroups, heads, dh)
                                  : attn_small_blocks(n_tiles) * (n_tau > 1 ? n_tau : 1) * sizeof(float);
    if (workspace_bytes < need) return SEG3D_EWORKSPACE;
    if (path == 0)
        return attn_fused_bwd_launch(q, k, v, ldq, ldk, ldv, out, dout, lse, tok, win_start, win_count, tile_item, n_tiles,
                                     qg_item, n_qgroups, m, heads, dh, tau, tau_min, dq, dk, dv, lddq, lddk, lddv, dtau,
                                     workspace, drop, as_stream(stream), am);
    return attn_small_bwd_launch(q, k, v, ldq, ldk, ldv, out, dout, lse, tok, win_start, win_count, tile_item, n_tiles, heads,
                                 dh, tau, tau_min, dq, dk, dv, lddq, lddk, lddv, dtau, workspace, drop, as_stream(stream), am);
}

}  // extern "C"
