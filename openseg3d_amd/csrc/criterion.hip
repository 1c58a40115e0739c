// The training criterion of tools/train.py:71-110 in one call: up to four heads (point, voxel, auxiliary voxel logits),
// each with the 'ce' / 'ohem_ce' term (loss.hip) and / or the 'lovasz' term (lovasz.hip) of build_criterion, summed with
// their MODEL.LOSSES weights into one scalar.  Per head and term it computes what the per-term entries compute, with the
// same expressions (criterion_device.hpp) in the same order, so loss and gradients carry the same bits; what is saved is
// the work in between: the per-term path runs 2 + 5 kernels and one device sort per head and term, evaluates the softmax
// of every row twice each way, and leaves the weighted sum and the sum of the two gradients to ~25 elementwise launches.
//
//   criterion_rows_kernel      a workgroup belongs to one head (<= 1024 per head, grid-stride): a thread reads its row,
//                              takes max and sum ONCE, writes lse and the CE partials, and the (key, value) pair of every
//                              class:  key = (head * c + class) << 30 | bits(error)   (errors are in [0, 1]: < 2^30)
//                                      val = row in the concatenated numbering | [label == class] << 31
//   rocprim::radix_sort_pairs_desc   ONE sort over 30 + log2(heads * c) bits: segment (head, class) is contiguous, errors
//                              descending inside it, ties in row order (stable sort, rows ascending in the input)
//   criterion_count / _offsets / _grad   one launch each over all (segment, 2048-element chunk) pairs, chunks aligned to
//                              their segment; coef is one [sum n, c] buffer
//   criterion_finalize_kernel  CE mean per head, Lovasz class selection and mean per head, then the total in the order
//                              compute_loss adds it: for every head in turn, ce then lovasz, each (head weight * term) *
//                              term weight, starting from 0
//   criterion_bwd_kernel       one pass over all heads: dlogits = CE gradient + Lovasz gradient, each rounded as its own
//                              backward kernel rounds it
// No atomics, no memsets of ours: every workspace word that is read was written by an earlier kernel of the same call.
#include <rocprim/device/device_radix_sort.hpp>

#include "criterion_device.hpp"

namespace {

using crit::class_bits;
using crit::kChunk;
using crit::kMaxBlocks;
using crit::kMaxClasses;
using crit::kThreads;
using Key = unsigned long long;

constexpr int kMaxHeads = SEG3D_CRITERION_MAX_HEADS;
constexpr int kErrBits = 30;
constexpr uint32_t kErrMask = (1u << kErrBits) - 1u;
constexpr int kStatsStride = SEG3D_CRITERION_STATS_STRIDE;  // {ce mean, ce count, lovasz loss, classes averaged, cscale[64]}

struct Head {
    const float* x;
    const int64_t* y;
    float* dx;        // backward only
    int n;
    int row0;         // first row in the concatenated numbering (lse, coef, values)
    int blk0, nblk;   // row pass: first workgroup and number of workgroups
    int bblk0;        // backward: first workgroup (bwd_tile_rows rows each)
    int nchunks;      // sorted chunks per segment
    int chunk0;       // first (segment, chunk) pair = c * chunks of the heads in front
    int64_t sorted0;  // first sorted element: the sort is descending, so the LAST head comes first
    float weight;
};

struct Heads {
    int nh;
    Head h[kMaxHeads];
};

struct Plan {
    Heads hd;
    int64_t rows, total;  // sum n, sum n * c
    int row_blocks, bwd_blocks, pairs;  // grid sizes
    int sort_bits;
    size_t sort_bytes;
};

__device__ __forceinline__ int head_of(const Heads& hd, int idx, int Head::*first) {
    int h = 0;
    for (int i = 1; i < hd.nh; ++i)
        if (idx >= hd.h[i].*first) h = i;
    return h;
}

__global__ __launch_bounds__(kThreads) void criterion_rows_kernel(Heads hd, int c, int terms, int64_t ignore_index,
                                                                  float keep_thresh, float* __restrict__ lse,
                                                                  float* __restrict__ ce_part /*[row blocks][2]*/,
                                                                  Key* __restrict__ keys, uint32_t* __restrict__ vals) {
    const int hi = head_of(hd, (int)blockIdx.x, &Head::blk0);
    const Head& H = hd.h[hi];
    const int n = H.n;
    const int64_t in0 = (int64_t)H.row0 * c;
    const int blk = (int)blockIdx.x - H.blk0;
    // (the table's pointers carry no __restrict__: without these the compiler orders every load of the row behind the
    // stores of the pairs in front of it)
    const float* __restrict__ x = H.x;
    const int64_t* __restrict__ label = H.y;
    float loss = 0.f, cnt = 0.f;
    for (int64_t r = (int64_t)blk * kThreads + threadIdx.x; r < n; r += (int64_t)H.nblk * kThreads) {
        const float* __restrict__ row = x + r * c;
        float m, s;
        crit::softmax_stats(row, c, &m, &s);
        const int64_t y = label[r];
        if (terms & SEG3D_CRITERION_CE) {
            float l;
            const bool counted = crit::ce_row(row, c, y, ignore_index, keep_thresh, m, s, &l);
            lse[H.row0 + r] = counted ? l : INFINITY;
            if (counted) {
                loss += l - row[y];
                cnt += 1.f;
            }
        }
        if (terms & SEG3D_CRITERION_LOVASZ) {
            const bool valid = y != ignore_index;
            for (int j = 0; j < c; ++j) {
                const bool fg = valid && y == j;
                const int64_t at = in0 + (int64_t)j * n + r;
                // (errors are in [0, 1]: the mask changes nothing.  It keeps the error of a NaN logit, whose bits reach past
                // 2^30, out of the segment id: the loss of such an input is undefined here -- NaN from the per-term entry --
                // but every segment keeps its n elements)
                keys[at] = ((Key)(hi * c + j) << kErrBits) | (crit::lovasz_err_bits(row, j, m, s, valid, fg) & kErrMask);
                vals[at] = (uint32_t)(H.row0 + r) | (fg ? 0x80000000u : 0u);
            }
        }
    }
    if (terms & SEG3D_CRITERION_CE) {
        block_sum<kThreads>(loss, cnt);
        if (threadIdx.x == 0) {
            ce_part[2 * blockIdx.x] = loss;
            ce_part[2 * blockIdx.x + 1] = cnt;
        }
    }
}

__global__ __launch_bounds__(kThreads) void criterion_count_kernel(Heads hd, const uint32_t* __restrict__ vals,
                                                                   int* __restrict__ chunk_cnt) {
    const Head& H = hd.h[head_of(hd, (int)blockIdx.x, &Head::chunk0)];
    const int local = (int)blockIdx.x - H.chunk0;
    const int seg = local / H.nchunks, chunk = local - seg * H.nchunks;
    const int t = crit::lovasz_chunk_count(vals + H.sorted0 + (int64_t)seg * H.n, H.n, chunk);
    if (threadIdx.x == 0) chunk_cnt[blockIdx.x] = t;
}

// one wave per (head, sorted segment)
__global__ __launch_bounds__(64) void criterion_offsets_kernel(Heads hd, int c, const int* __restrict__ chunk_cnt,
                                                               int* __restrict__ chunk_off, int* __restrict__ total) {
    const int hi = (int)blockIdx.x / c, seg = (int)blockIdx.x - hi * c;
    const Head& H = hd.h[hi];
    const int at = H.chunk0 + seg * H.nchunks;
    const int t = crit::lovasz_segment_offsets(chunk_cnt + at, H.nchunks, chunk_off + at);
    if (threadIdx.x == 0) total[blockIdx.x] = t;
}

__global__ __launch_bounds__(kThreads) void criterion_grad_kernel(Heads hd, int c, const Key* __restrict__ keys,
                                                                  const uint32_t* __restrict__ vals,
                                                                  const int* __restrict__ chunk_off,
                                                                  const int* __restrict__ total, float* __restrict__ coef,
                                                                  float* __restrict__ part) {
    const int hi = head_of(hd, (int)blockIdx.x, &Head::chunk0);
    const Head& H = hd.h[hi];
    const int local = (int)blockIdx.x - H.chunk0;
    const int seg = local / H.nchunks, chunk = local - seg * H.nchunks;
    const int64_t seg0 = H.sorted0 + (int64_t)seg * H.n;
    const float t = crit::lovasz_chunk_grad(keys + seg0, vals + seg0, kErrMask, H.n, c, c - 1 - seg, chunk,
                                            chunk_off[blockIdx.x], total[hi * c + seg], coef);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

__global__ __launch_bounds__(kThreads) void criterion_finalize_kernel(Heads hd, int c, int terms, float w_ce, float w_lovasz,
                                                                      const float* __restrict__ ce_part,
                                                                      const float* __restrict__ part,
                                                                      const int* __restrict__ total,
                                                                      float* __restrict__ stats, float* __restrict__ out) {
    for (int hi = 0; hi < hd.nh; ++hi) {
        const Head& H = hd.h[hi];
        float* st = stats + hi * kStatsStride;
        if (terms & SEG3D_CRITERION_CE) {
            float mean, count;
            crit::ce_mean(ce_part + 2 * H.blk0, H.nblk, &mean, &count);
            if (threadIdx.x == 0) {
                st[0] = mean;
                st[1] = count;
            }
            __syncthreads();  // the reduction's shared words are used again for the next head
        }
        if (terms & SEG3D_CRITERION_LOVASZ) {
            crit::lovasz_head_finalize(part + H.chunk0, total + hi * c, c, H.nchunks, 0, nullptr, nullptr, st + 2);
            __syncthreads();
        }
    }
    if (threadIdx.x == 0) {
        // compute_loss: loss = 0; per head, per term: loss = loss + (head weight * term) * term weight
        float loss = 0.f;
        for (int hi = 0; hi < hd.nh; ++hi) {
            const float* st = stats + hi * kStatsStride;
            if (terms & SEG3D_CRITERION_CE) loss = loss + hd.h[hi].weight * st[0] * w_ce;
            if (terms & SEG3D_CRITERION_LOVASZ) loss = loss + hd.h[hi].weight * st[2] * w_lovasz;
        }
        out[0] = loss;
    }
}

// A workgroup owns `tile` consecutive rows of one head.  The rows' logits (and coef) lie back to back in memory, so the
// workgroup copies them to LDS with coalesced loads, every thread works on its own row there (row stride c | 1 words: odd,
// so the lanes of a wave spread over the banks), writes the gradient over the logits in place, and the tile goes out
// with coalesced stores.  (One row per thread straight from memory, as lovasz_bwd does it, makes every load and store of
// a wave touch 64 rows 4 c bytes apart, one element per trip: 378 us against 190 us for the three per-term passes.)
__global__ __launch_bounds__(kThreads) void criterion_bwd_kernel(Heads hd, int c, int terms, int tile, float w_ce,
                                                                 float w_lovasz, const float* __restrict__ lse,
                                                                 const float* __restrict__ coef,
                                                                 const float* __restrict__ stats,
                                                                 const float* __restrict__ gout) {
    extern __shared__ float tile_mem[];
    const int hi = head_of(hd, (int)blockIdx.x, &Head::bblk0);
    const Head& H = hd.h[hi];
    const bool ce = terms & SEG3D_CRITERION_CE, lov = terms & SEG3D_CRITERION_LOVASZ;
    const int stride = c | 1;
    float* xs = tile_mem;
    float* cs = tile_mem + tile * stride;  // (Lovasz term only)
    const int r0 = ((int)blockIdx.x - H.bblk0) * tile;
    const int nrows = H.n - r0 < tile ? H.n - r0 : tile;
    const int count = nrows * c;
    const float* __restrict__ xg = H.x + (int64_t)r0 * c;
    const float* __restrict__ cg = coef + (int64_t)(H.row0 + r0) * c;
    for (int e = threadIdx.x; e < count; e += kThreads) {
        const int rr = e / c, at = rr * stride + (e - rr * c);
        xs[at] = xg[e];
        if (lov) cs[at] = cg[e];
    }
    __syncthreads();
    if ((int)threadIdx.x < nrows) {
        const int r = r0 + (int)threadIdx.x;
        const float* st = stats + hi * kStatsStride;
        float* row = xs + threadIdx.x * stride;
        const float* cf = cs + threadIdx.x * stride;
        // autograd's chain for one term: d(loss + (hw * f) * w) / df = (g * w) * hw
        float scale = 0.f, l = INFINITY, m = 0.f, s = 1.f, g = 0.f, dot = 0.f;
        int64_t y = -1;
        if (ce) {
            const float cnt = st[1];
            scale = cnt > 0.f ? gout[0] * w_ce * H.weight / cnt : 0.f;
            l = lse[H.row0 + r];
            y = H.y[r];
        }
        if (lov) {
            crit::softmax_stats(row, c, &m, &s);
            g = gout[0] * w_lovasz * H.weight;
            dot = crit::lovasz_row_dot(row, cf, st + 4, c, m, s, g);
        }
        for (int j = 0; j < c; ++j) {
            const float x = row[j];
            const float a = ce ? crit::ce_grad(x, l, j == y, scale) : 0.f;
            const float b = lov ? crit::lovasz_grad_elem(x, cf[j], st[4 + j], m, s, g, dot) : 0.f;
            row[j] = ce && lov ? a + b : (ce ? a : b);
        }
    }
    __syncthreads();
    float* __restrict__ og = H.dx + (int64_t)r0 * c;
    for (int e = threadIdx.x; e < count; e += kThreads) {
        const int rr = e / c;
        og[e] = xs[rr * stride + (e - rr * c)];
    }
}

// rows per workgroup of the backward pass: as many as threads where the tiles (logits, and coef with the Lovasz term) fit
// in 64 KB of LDS, else the largest multiple of 64 that does (64 rows at c = 64 with both tiles)
int bwd_tile_rows(int c, int terms) {
    const int tiles = (terms & SEG3D_CRITERION_LOVASZ) ? 2 : 1;
    int rows = (64 * 1024) / (tiles * (c | 1) * (int)sizeof(float)) / 64 * 64;
    return rows > kThreads ? kThreads : rows;
}

// EINVAL checks and the launch geometry; no device is touched
int make_plan(const seg3d_criterion_table* tab, int c, int terms, Plan* pl) {
    if (!tab || tab->n_heads < 1 || tab->n_heads > kMaxHeads || c <= 0 || c > kMaxClasses) return SEG3D_EINVAL;
    if (terms < 1 || terms > (SEG3D_CRITERION_CE | SEG3D_CRITERION_LOVASZ)) return SEG3D_EINVAL;
    const int nh = tab->n_heads;
    int64_t rows = 0;
    for (int i = 0; i < nh; ++i) {
        const int64_t n = tab->heads[i].n;
        if (n < 0 || n >= (int64_t)1 << 31) return SEG3D_EINVAL;
        rows += n;
        if (rows * c >= (int64_t)1 << 31) return SEG3D_EINVAL;
        if (n > 0 && (!tab->heads[i].logits || !tab->heads[i].labels)) return SEG3D_EINVAL;
    }
    Heads& hd = pl->hd;
    hd.nh = nh;
    int row0 = 0, blk0 = 0, bblk0 = 0, chunk0 = 0;
    const int tile = bwd_tile_rows(c, terms);
    for (int i = 0; i < nh; ++i) {
        Head& H = hd.h[i];
        const int64_t n = tab->heads[i].n;
        H.x = tab->heads[i].logits;
        H.y = tab->heads[i].labels;
        H.dx = nullptr;
        H.n = (int)n;
        H.weight = tab->heads[i].weight;
        H.row0 = row0;
        H.blk0 = blk0;
        H.nblk = (int)(ceil_div64(n, kThreads) > kMaxBlocks ? kMaxBlocks : ceil_div64(n, kThreads));
        H.bblk0 = bblk0;
        H.nchunks = (int)ceil_div64(n, kChunk);
        H.chunk0 = chunk0;
        row0 += (int)n;
        blk0 += H.nblk;
        bblk0 += (int)ceil_div64(n, tile);
        chunk0 += c * H.nchunks;
    }
    int64_t behind = 0;
    for (int i = nh - 1; i >= 0; --i) {
        hd.h[i].sorted0 = behind;
        behind += (int64_t)hd.h[i].n * c;
    }
    pl->rows = rows;
    pl->total = rows * c;
    pl->row_blocks = blk0;
    pl->bwd_blocks = bblk0;
    pl->pairs = chunk0;
    pl->sort_bits = kErrBits + class_bits(nh * c);
    pl->sort_bytes = 0;
    return SEG3D_OK;
}

// the sort's scratch size into pl->sort_bytes: asked of rocPRIM, which sizes it for the current device
int plan_sort_scratch(int terms, Plan* pl) {
    if (!(terms & SEG3D_CRITERION_LOVASZ) || pl->total == 0) return SEG3D_OK;
    rocprim::double_buffer<Key> k(nullptr, nullptr);
    rocprim::double_buffer<uint32_t> v(nullptr, nullptr);
    size_t bytes = 0;
    if (rocprim::radix_sort_pairs_desc(nullptr, bytes, k, v, (size_t)pl->total, 0u, (unsigned)pl->sort_bits) != hipSuccess)
        return SEG3D_ELAUNCH;
    pl->sort_bytes = bytes;
    return SEG3D_OK;
}

// everything but the sort's own scratch
size_t fixed_bytes(const Plan& pl, int c, int terms) {
    size_t b = align_up((size_t)(pl.row_blocks > 0 ? pl.row_blocks : 1) * 2 * sizeof(float), 256);
    if (terms & SEG3D_CRITERION_LOVASZ) {
        const size_t t = (size_t)pl.total, cc = (size_t)pl.pairs;
        b += 2 * align_up(t * sizeof(Key), 256) + 2 * align_up(t * sizeof(uint32_t), 256) + 2 * align_up(cc * sizeof(int), 256) +
             align_up(cc * sizeof(float), 256) + align_up((size_t)pl.hd.nh * c * sizeof(int), 256);
    }
    return b + 256;
}

}  // namespace

// 0 when the arguments are invalid or (with the lovasz term) no device is visible
extern "C" size_t seg3d_criterion_workspace_bytes(const seg3d_criterion_table* heads, int32_t c, int32_t terms) {
    Plan pl;
    if (make_plan(heads, c, terms, &pl) != SEG3D_OK || plan_sort_scratch(terms, &pl) != SEG3D_OK) return 0;
    return fixed_bytes(pl, c, terms) + align_up(pl.sort_bytes, 256);
}

extern "C" int seg3d_criterion_fwd(const seg3d_criterion_table* heads, int32_t c, int32_t terms, int64_t ignore_index,
                                   float keep_thresh, float w_ce, float w_lovasz, float* lse, float* coef, float* stats,
                                   float* loss, void* workspace, size_t workspace_bytes, void* stream) {
    Plan pl;
    int rc = make_plan(heads, c, terms, &pl);
    if (rc != SEG3D_OK) return rc;
    const bool ce = terms & SEG3D_CRITERION_CE, lov = terms & SEG3D_CRITERION_LOVASZ;
    if (!stats || !loss || (pl.rows > 0 && ((ce && !lse) || (lov && !coef)))) return SEG3D_EINVAL;
    // (the part that needs no device first: a short workspace is refused before rocPRIM is asked for its scratch size)
    if (!workspace || workspace_bytes < fixed_bytes(pl, c, terms)) return SEG3D_EWORKSPACE;
    rc = plan_sort_scratch(terms, &pl);
    if (rc != SEG3D_OK) return rc;
    if (workspace_bytes < fixed_bytes(pl, c, terms) + align_up(pl.sort_bytes, 256)) return SEG3D_EWORKSPACE;
    hipStream_t st = as_stream(stream);
    WsCarver ws(workspace);
    float* ce_part = ws.take<float>((size_t)(pl.row_blocks > 0 ? pl.row_blocks : 1) * 2);
    Key *k0 = nullptr, *k1 = nullptr;
    uint32_t *v0 = nullptr, *v1 = nullptr;
    int *chunk_cnt = nullptr, *chunk_off = nullptr, *total = nullptr;
    float* part = nullptr;
    void* sort_tmp = nullptr;
    if (lov) {
        const size_t t = (size_t)pl.total, cc = (size_t)pl.pairs;
        k0 = ws.take<Key>(t);
        k1 = ws.take<Key>(t);
        v0 = ws.take<uint32_t>(t);
        v1 = ws.take<uint32_t>(t);
        chunk_cnt = ws.take<int>(cc);
        chunk_off = ws.take<int>(cc);
        part = ws.take<float>(cc);
        total = ws.take<int>((size_t)pl.hd.nh * c);
        sort_tmp = ws.take<char>(pl.sort_bytes);
    }
    const Key* ks = k0;
    const uint32_t* vs = v0;
    if (pl.row_blocks > 0) {
        hipLaunchKernelGGL(criterion_rows_kernel, dim3((unsigned)pl.row_blocks), dim3(kThreads), 0, st, pl.hd, c, terms,
                           ignore_index, keep_thresh, lse, ce_part, k0, v0);
        SEG3D_CHECK_LAUNCH();
    }
    if (lov) {
        if (pl.total > 0) {
            rocprim::double_buffer<Key> kb(k0, k1);
            rocprim::double_buffer<uint32_t> vb(v0, v1);
            size_t bytes = pl.sort_bytes;
            SEG3D_CHECK_HIP(rocprim::radix_sort_pairs_desc(sort_tmp, bytes, kb, vb, (size_t)pl.total, 0u,
                                                           (unsigned)pl.sort_bits, st));
            ks = kb.current();
            vs = vb.current();
            hipLaunchKernelGGL(criterion_count_kernel, dim3((unsigned)pl.pairs), dim3(kThreads), 0, st, pl.hd, vs, chunk_cnt);
            SEG3D_CHECK_LAUNCH();
        }
        hipLaunchKernelGGL(criterion_offsets_kernel, dim3((unsigned)(pl.hd.nh * c)), dim3(64), 0, st, pl.hd, c, chunk_cnt,
                           chunk_off, total);
        SEG3D_CHECK_LAUNCH();
        if (pl.total > 0) {
            hipLaunchKernelGGL(criterion_grad_kernel, dim3((unsigned)pl.pairs), dim3(kThreads), 0, st, pl.hd, c, ks, vs,
                               chunk_off, total, coef, part);
            SEG3D_CHECK_LAUNCH();
        }
    }
    hipLaunchKernelGGL(criterion_finalize_kernel, dim3(1), dim3(kThreads), 0, st, pl.hd, c, terms, w_ce, w_lovasz, ce_part,
                       part, total, stats, loss);
    SEG3D_CHECK_LAUNCH();
    return SEG3D_OK;
}

extern "C" int seg3d_criterion_bwd(const seg3d_criterion_table* heads, int32_t c, int32_t terms, float w_ce, float w_lovasz,
                                   const float* lse, const float* coef, const float* stats, const float* grad_out,
                                   float* const* dlogits, void* stream) {
    Plan pl;
    const int rc = make_plan(heads, c, terms, &pl);
    if (rc != SEG3D_OK) return rc;
    const bool ce = terms & SEG3D_CRITERION_CE, lov = terms & SEG3D_CRITERION_LOVASZ;
    if (!stats || !grad_out || !dlogits) return SEG3D_EINVAL;
    if (pl.rows == 0) return SEG3D_OK;
    if ((ce && !lse) || (lov && !coef)) return SEG3D_EINVAL;
    for (int i = 0; i < pl.hd.nh; ++i) {
        if (pl.hd.h[i].n > 0 && !dlogits[i]) return SEG3D_EINVAL;
        pl.hd.h[i].dx = dlogits[i];
    }
    const int tile = bwd_tile_rows(c, terms);
    const size_t lds = (size_t)(lov ? 2 : 1) * tile * (c | 1) * sizeof(float);
    hipLaunchKernelGGL(criterion_bwd_kernel, dim3((unsigned)pl.bwd_blocks), dim3(kThreads), lds, as_stream(stream), pl.hd, c,
                       terms, tile, w_ce, w_lovasz, lse, coef, stats, grad_out);
    SEG3D_CHECK_LAUNCH();
    return SEG3D_OK;
}
