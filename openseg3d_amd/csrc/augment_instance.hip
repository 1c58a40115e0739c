// Instance copy-paste augmentation on the device.
// Reference: seg3d/datasets/transforms/instance_augmentation.py:25-186 (InstanceAugmentation.__call__, instance_flip,
// check, rotate_origin, local_transform, radius_instance), called at seg3d/datasets/waymo_dataset.py:314-315, :321.
//
// MI355X design: every random number of the class is independent of the data, so the host draws them all and hands
// them over as one seg3d_aug_instance_plan per instance.  What is left is, per instance, (1) a tiny rigid transform of
// a few hundred bank rows (one workgroup), (2) ONE pass over the frame plus the rows pasted so far that evaluates all
// candidate rotations at once -- per candidate an `occluded` bit and the lexicographic minimum (ground distance, row),
// reduced per wave64 with shuffles, per workgroup through LDS, per grid through one record per workgroup and
// candidate -- and (3) a one-workgroup decision and append.  The instances depend on each other (instance k sees what
// 0 .. k-1 pasted), so the chain is 2 K + 1 launches for K instances: step(0) scan(0) step(1) ... scan(K-1) step(K),
// where step(k) decides and pastes instance k-1 and prepares instance k.  The number of rows pasted so far lives in
// device memory (counts[0]); the host reads nothing until the whole chain is enqueued.  The lexicographic minimum and
// the OR are exact and order-independent and the two means use one fixed summation order, so the result is a pure
// function of the inputs; the host twin below shares every recipe and gives the same bits.  All arithmetic is double.
#include <string.h>

#include "instance_geom.hpp"

// fixed sequences of IEEE products and sums, as numpy rounds them; no fused multiply-add (see augment.hip)
#pragma clang fp contract(off)

namespace {

constexpr int kWaves = kThreads / SEG3D_WAVE;
constexpr int kMaxDim = 16;
constexpr int kMaxAngles = SEG3D_AUG_MAX_ANGLES;
constexpr int kMaxScanBlocks = 256;  // 65 536 threads: a 175 k-row frame is three rows per thread
constexpr int32_t kNoRow = INT32_MAX;

struct GroundSet {
    uint8_t is_ground[256];
};

// instance_augmentation.py:35-43: 0 = label 255 (skipped), 1 = ground, 2 = object
__host__ __device__ __forceinline__ int row_kind(const GroundSet& g, const void* labels, int label_bytes, int64_t i) {
    const int64_t l = label_at(labels, label_bytes, i);
    if (l == 255) return 0;
    return (l >= 0 && l < 256 && g.is_ground[l]) ? 1 : 2;
}

// what the decision needs of a prepared instance
struct InstState {
    double cand[kMaxAngles][3];  // rotate_origin(center, r) per candidate (:79); unused slots are zeros
    double radius;               // radius_instance (:74, :179-186)
    double center_z;
};

// one workgroup's (or, on the host, the whole frame's) result for one candidate
struct ScanRec {
    double d;      // smallest ground distance, +inf without a ground row
    double z;      // z of that ground row
    int32_t row;   // its row in [frame; pasted rows], kNoRow without one
    int32_t occ;   // 1: an object row within `radius`
};

// closer (np.argmin, :149) and dist3 (np.linalg.norm, :137, :144, :184) are instance_geom.hpp's

// flip over the short axis (:63-64, :121-125): the 2 x 2 matrix of the axes through center0
__host__ __device__ __forceinline__ void flip_matrix(const double* c0, double* m) {
    const double nrm = sqrt(c0[0] * c0[0] + c0[1] * c0[1]);
    const double lx = c0[0] / nrm, ly = c0[1] / nrm;
    const double a = -ly, b = lx;  // the short axis
    m[0] = b * b - a * a;
    m[1] = (-2.0 * a) * b;
    m[2] = a * a - b * b;
}

// one bank row through local_transform (:166-177) and the flip (:67-69, :109-129), both about center0
__host__ __device__ __forceinline__ void inst_point(const seg3d_aug_instance_plan& p, const double* c0, const double* m,
                                                    const double* row, double* o) {
    double x = row[0], y = row[1], z = row[2];
    if (p.local_on) {
        const double px = x - c0[0], py = y - c0[1], pz = z - c0[2];
        const double rx = px * p.rot_cos + py * p.rot_sin;
        const double ry = (-px) * p.rot_sin + py * p.rot_cos;
        x = (rx + p.loc_noise[0]) + c0[0];
        y = (ry + p.loc_noise[1]) + c0[1];
        z = (pz + p.loc_noise[2]) + c0[2];
    }
    if (p.flip) {
        const double px = x - c0[0], py = y - c0[1];
        x = (m[0] * px + m[1] * py) + c0[0];
        y = (m[1] * px + m[2] * py) + c0[1];
    }
    o[0] = x;
    o[1] = y;
    o[2] = z;
}

// rotate_origin (:157-164)
__host__ __device__ __forceinline__ void rotate_origin(double x, double y, double c, double s, double* o) {
    o[0] = x * c + y * s;
    o[1] = (-x) * s + y * c;
}

// the accepted instance's row j: z adjusted to the ground (:150-152), then rotated to the free place (:87)
__host__ __device__ __forceinline__ void paste_row(const seg3d_aug_instance_plan& p, int choice, double dz, const double* xyz,
                                                   const double* bank_row, int dim, double* out) {
    rotate_origin(xyz[0], xyz[1], p.ang_cos[choice], p.ang_sin[choice], out);
    out[2] = xyz[2] + dz;
    for (int c = 3; c < dim; ++c) out[c] = bank_row[c];
}

__host__ __device__ __forceinline__ void write_label(void* labels, int label_bytes, int64_t i, int32_t label) {
    if (label_bytes == 1)
        static_cast<uint8_t*>(labels)[i] = (uint8_t)label;
    else
        static_cast<int64_t*>(labels)[i] = (int64_t)label;
}

// the first candidate that is free of occlusion and on the ground (:78-84, :138-148); -1: the instance is skipped
__host__ __device__ __forceinline__ bool candidate_passes(const ScanRec& r, double radius) {
    return !r.occ && r.d < 1.2 * radius;
}

// ------------------------------------------------------------------------------------------ device
// the two means are summed in the one order of block_sum3 (instance_geom.hpp)
// :47-74 for one instance: transformed xyz -> xyz [m, 3], candidate centres / radius -> st
__device__ void prepare_block(const seg3d_aug_instance_plan& p, const double* __restrict__ bank, int dim,
                              double* __restrict__ xyz, InstState* __restrict__ st, double* lds) {
    const int t = threadIdx.x, m = p.n_rows;
    const double* rows = bank + p.row_begin * dim;
    double c0[3] = {0.0, 0.0, 0.0};
    for (int j = t; j < m; j += kThreads)
        for (int c = 0; c < 3; ++c) c0[c] += rows[(int64_t)j * dim + c];
    block_sum3(c0, lds);
    for (int c = 0; c < 3; ++c) c0[c] /= (double)m;
    double fm[3] = {0.0, 0.0, 0.0};
    if (p.flip) flip_matrix(c0, fm);
    double ctr[3] = {0.0, 0.0, 0.0};
    for (int j = t; j < m; j += kThreads) {
        double o[3];
        inst_point(p, c0, fm, rows + (int64_t)j * dim, o);
        for (int c = 0; c < 3; ++c) {
            xyz[(int64_t)j * 3 + c] = o[c];
            ctr[c] += o[c];
        }
    }
    block_sum3(ctr, lds);
    for (int c = 0; c < 3; ++c) ctr[c] /= (double)m;
    double r = 0.0;
    for (int j = t; j < m; j += kThreads) {  // the rows this thread wrote itself
        const double d = dist3(xyz[(int64_t)j * 3], xyz[(int64_t)j * 3 + 1], xyz[(int64_t)j * 3 + 2], ctr);
        if (d > r) r = d;
    }
    r = block_max(r, lds);
    if (t < kMaxAngles) {
        double o[2] = {0.0, 0.0};
        if (t < p.n_angles) rotate_origin(ctr[0], ctr[1], p.ang_cos[t], p.ang_sin[t], o);
        st->cand[t][0] = o[0];
        st->cand[t][1] = o[1];
        st->cand[t][2] = t < p.n_angles ? ctr[2] : 0.0;
    }
    if (t == 0) {
        st->radius = r;
        st->center_z = ctr[2];
    }
}

// step(k): decide and paste instance k - 1 (from the records its scan left), then prepare instance k
__global__ __launch_bounds__(kThreads) void inst_step_kernel(int has_prev, seg3d_aug_instance_plan prev, int k_prev, int has_next,
                                                             seg3d_aug_instance_plan next, const double* __restrict__ bank,
                                                             int dim, int label_bytes, int nb_prev,
                                                             const ScanRec* __restrict__ recs,
                                                             const InstState* __restrict__ st_prev,
                                                             InstState* __restrict__ st_next,
                                                             const double* __restrict__ xyz_prev, double* __restrict__ xyz_next,
                                                             double* __restrict__ add_points, void* __restrict__ add_labels,
                                                             int32_t* __restrict__ decisions, int32_t* __restrict__ counts) {
    __shared__ double lds[3 * kThreads];
    __shared__ int s_pass[kMaxAngles];
    __shared__ double s_gz[kMaxAngles];
    __shared__ int s_choice, s_base;
    __shared__ double s_dz;
    const int t = threadIdx.x;
    if (!has_prev) {
        if (t < 4) counts[t] = 0;
    } else {
        if (t < kMaxAngles) {
            ScanRec best = {INFINITY, 0.0, kNoRow, 0};
            for (int b = 0; b < nb_prev; ++b) {
                const ScanRec r = recs[b * kMaxAngles + t];
                best.occ |= r.occ;
                if (closer(r.d, r.row, best.d, best.row)) {
                    best.d = r.d;
                    best.z = r.z;
                    best.row = r.row;
                }
            }
            s_pass[t] = t < prev.n_angles && candidate_passes(best, st_prev->radius);
            s_gz[t] = best.z;
        }
        __syncthreads();
        if (t == 0) {
            int choice = -1;
            for (int c = kMaxAngles - 1; c >= 0; --c)
                if (s_pass[c]) choice = c;
            decisions[k_prev] = choice;
            s_choice = choice;
            s_base = counts[0];
            s_dz = choice >= 0 ? (s_gz[choice] + prev.height) - st_prev->center_z : 0.0;
        }
        __syncthreads();
        const int choice = s_choice;
        if (choice >= 0) {
            const int64_t base = s_base;
            const double dz = s_dz;
            for (int j = t; j < prev.n_rows; j += kThreads) {
                paste_row(prev, choice, dz, xyz_prev + (int64_t)j * 3, bank + (prev.row_begin + j) * dim, dim,
                          add_points + (base + j) * dim);
                write_label(add_labels, label_bytes, base + j, prev.label);
            }
            if (t == 0) {
                counts[0] = (int32_t)(base + prev.n_rows);
                counts[1] += 1;
            }
        }
    }
    if (has_next) prepare_block(next, bank, dim, xyz_next, st_next, lds);
}

// scan(k): every row of [frame; rows pasted so far] once, against all candidates of instance k
template <typename T>
__global__ __launch_bounds__(kThreads) void inst_scan_kernel(const T* __restrict__ pts, int64_t n, int dim,
                                                             const void* __restrict__ labels, int label_bytes, GroundSet gs,
                                                             const double* __restrict__ add_points,
                                                             const void* __restrict__ add_labels,
                                                             const int32_t* __restrict__ counts,
                                                             const InstState* __restrict__ st, ScanRec* __restrict__ recs) {
    __shared__ double s_d[kWaves][kMaxAngles];
    __shared__ int32_t s_row[kWaves][kMaxAngles];
    __shared__ uint32_t s_occ[kWaves];
    const int t = threadIdx.x;
    const int64_t total = n + counts[0];
    const double radius = st->radius;
    double cand[kMaxAngles][3], bd[kMaxAngles];
    int32_t brow[kMaxAngles];
    uint32_t occ = 0u;
#pragma unroll
    for (int c = 0; c < kMaxAngles; ++c) {
        cand[c][0] = st->cand[c][0];
        cand[c][1] = st->cand[c][1];
        cand[c][2] = st->cand[c][2];
        bd[c] = INFINITY;
        brow[c] = kNoRow;
    }
    for (int64_t i = (int64_t)blockIdx.x * kThreads + t; i < total; i += (int64_t)gridDim.x * kThreads) {
        double x, y, z;
        int kind;
        if (i < n) {
            const T* row = pts + i * dim;
            x = (double)row[0];
            y = (double)row[1];
            z = (double)row[2];
            kind = row_kind(gs, labels, label_bytes, i);
        } else {
            const double* row = add_points + (i - n) * dim;
            x = row[0];
            y = row[1];
            z = row[2];
            kind = row_kind(gs, add_labels, label_bytes, i - n);
        }
        if (kind == 0) continue;
#pragma unroll
        for (int c = 0; c < kMaxAngles; ++c) {
            const double d = dist3(x, y, z, cand[c]);
            if (kind == 1) {
                if (closer(d, (int32_t)i, bd[c], brow[c])) {
                    bd[c] = d;
                    brow[c] = (int32_t)i;
                }
            } else if (d <= radius) {
                occ |= 1u << c;
            }
        }
    }
    // wave64: xor butterflies; (distance, row) minima and ORs are exact, so the order does not show in the result
    for (int off = SEG3D_WAVE / 2; off > 0; off >>= 1) {
        occ |= (uint32_t)__shfl_xor((int)occ, off, SEG3D_WAVE);
#pragma unroll
        for (int c = 0; c < kMaxAngles; ++c) {
            const double od = __shfl_xor(bd[c], off, SEG3D_WAVE);
            const int32_t orow = __shfl_xor(brow[c], off, SEG3D_WAVE);
            if (closer(od, orow, bd[c], brow[c])) {
                bd[c] = od;
                brow[c] = orow;
            }
        }
    }
    const int wave = t / SEG3D_WAVE;
    if (t % SEG3D_WAVE == 0) {
        s_occ[wave] = occ;
#pragma unroll
        for (int c = 0; c < kMaxAngles; ++c) {
            s_d[wave][c] = bd[c];
            s_row[wave][c] = brow[c];
        }
    }
    __syncthreads();
    if (t < kMaxAngles) {
        ScanRec r = {s_d[0][t], 0.0, s_row[0][t], 0};
        uint32_t o = s_occ[0];
        for (int w = 1; w < kWaves; ++w) {
            o |= s_occ[w];
            if (closer(s_d[w][t], s_row[w][t], r.d, r.row)) {
                r.d = s_d[w][t];
                r.row = s_row[w][t];
            }
        }
        r.occ = (int32_t)((o >> t) & 1u);
        if (r.row != kNoRow)
            r.z = r.row < n ? (double)pts[(int64_t)r.row * dim + 2] : add_points[((int64_t)r.row - n) * dim + 2];
        recs[(int64_t)blockIdx.x * kMaxAngles + t] = r;
    }
}

struct InstWs {
    ScanRec* recs;
    InstState* st;   // [2]: instance k uses slot k & 1
    double* xyz[2];  // [max_rows, 3] each
};

InstWs inst_carve(void* ws, int64_t max_rows, size_t* bytes) {
    WsCarver c(ws);
    InstWs w;
    w.recs = c.take<ScanRec>((size_t)kMaxScanBlocks * kMaxAngles);
    w.st = c.take<InstState>(2);
    w.xyz[0] = c.take<double>((size_t)max_rows * 3 + 1);
    w.xyz[1] = c.take<double>((size_t)max_rows * 3 + 1);
    if (bytes) *bytes = c.off;
    return w;
}

bool inst_args_ok(const void* points, int64_t n, int32_t dim, int32_t point_bytes, const void* labels, int32_t label_bytes,
                  const uint8_t* ground_ids, int32_t n_ground, const double* bank, int64_t bank_rows,
                  const seg3d_aug_instance_plan* plans, int32_t k, int64_t cap_add, const double* add_points,
                  const void* add_labels, const int32_t* decisions, const int32_t* counts, GroundSet* gs, int64_t* max_rows) {
    if (n < 0 || dim < 3 || dim > kMaxDim || (point_bytes != 4 && point_bytes != 8)) return false;
    if ((label_bytes != 1 && label_bytes != 8) || n_ground < 0 || n_ground > 256 || (n_ground > 0 && !ground_ids)) return false;
    if (k < 0 || bank_rows < 0 || cap_add < 0 || !counts) return false;
    if (n > INT32_MAX - 1 || cap_add > INT32_MAX - 1 - n) return false;  // rows of [frame; pasted] are indexed in int32
    if (n > 0 && (!points || !labels)) return false;
    if (k > 0 && (!plans || !decisions || !bank)) return false;
    if (cap_add > 0 && (!add_points || !add_labels)) return false;
    memset(gs->is_ground, 0, sizeof(gs->is_ground));
    for (int g = 0; g < n_ground; ++g) gs->is_ground[ground_ids[g]] = 1;
    int64_t sum = 0, mx = 0;
    for (int i = 0; i < k; ++i) {
        const seg3d_aug_instance_plan& p = plans[i];
        if (p.n_rows < 1 || p.row_begin < 0 || p.row_begin > bank_rows - p.n_rows) return false;
        if (p.label < 0 || p.label > 255 || p.n_angles < 0 || p.n_angles > kMaxAngles) return false;
        if ((p.flip != 0 && p.flip != 1) || (p.local_on != 0 && p.local_on != 1)) return false;
        sum += p.n_rows;
        mx = p.n_rows > mx ? p.n_rows : mx;
    }
    if (sum > cap_add) return false;
    *max_rows = mx;
    return true;
}

template <typename T>
int inst_launch(const T* pts, int64_t n, int dim, const void* labels, int label_bytes, const GroundSet& gs, const double* bank,
                const seg3d_aug_instance_plan* plans, int k, double* add_points, void* add_labels, int32_t* decisions,
                int32_t* counts, const InstWs& w, hipStream_t st) {
    const seg3d_aug_instance_plan none = {};
    int64_t rows = n;  // upper bound of the rows instance i has to see
    int nb_prev = 0;
    for (int i = 0; i <= k; ++i) {
        const int has_prev = i > 0, has_next = i < k;
        hipLaunchKernelGGL(inst_step_kernel, dim3(1), dim3(kThreads), 0, st, has_prev, has_prev ? plans[i - 1] : none, i - 1,
                           has_next, has_next ? plans[i] : none, bank, dim, label_bytes, nb_prev, w.recs,
                           w.st + ((i + 1) & 1), w.st + (i & 1), w.xyz[(i + 1) & 1], w.xyz[i & 1], add_points, add_labels,
                           decisions, counts);
        SEG3D_CHECK_LAUNCH();
        if (!has_next) break;
        int64_t nb = ceil_div64(rows > 0 ? rows : 1, kThreads);
        nb = nb > kMaxScanBlocks ? kMaxScanBlocks : nb;
        hipLaunchKernelGGL(inst_scan_kernel<T>, dim3((unsigned)nb), dim3(kThreads), 0, st, pts, n, dim, labels, label_bytes, gs,
                           add_points, add_labels, counts, w.st + (i & 1), w.recs);
        SEG3D_CHECK_LAUNCH();
        nb_prev = (int)nb;
        rows += plans[i].n_rows;
    }
    return SEG3D_OK;
}

// ------------------------------------------------------------------------------------------ host twin
void prepare_host(const seg3d_aug_instance_plan& p, const double* bank, int dim, double* xyz, InstState* st) {
    const int m = p.n_rows;
    const double* rows = bank + p.row_begin * dim;
    std::vector<double> part(3 * kThreads, 0.0);
    for (int j = 0; j < m; ++j)
        for (int c = 0; c < 3; ++c) part[c * kThreads + j % kThreads] += rows[(int64_t)j * dim + c];
    double c0[3], ctr[3], fm[3] = {0.0, 0.0, 0.0};
    sum3_host(part, c0);
    for (int c = 0; c < 3; ++c) c0[c] /= (double)m;
    if (p.flip) flip_matrix(c0, fm);
    part.assign(3 * kThreads, 0.0);
    for (int j = 0; j < m; ++j) {
        inst_point(p, c0, fm, rows + (int64_t)j * dim, xyz + (int64_t)j * 3);
        for (int c = 0; c < 3; ++c) part[c * kThreads + j % kThreads] += xyz[(int64_t)j * 3 + c];
    }
    sum3_host(part, ctr);
    for (int c = 0; c < 3; ++c) ctr[c] /= (double)m;
    double r = 0.0;
    for (int j = 0; j < m; ++j) {
        const double d = dist3(xyz[(int64_t)j * 3], xyz[(int64_t)j * 3 + 1], xyz[(int64_t)j * 3 + 2], ctr);
        if (d > r) r = d;
    }
    memset(st->cand, 0, sizeof(st->cand));
    for (int c = 0; c < p.n_angles; ++c) {
        rotate_origin(ctr[0], ctr[1], p.ang_cos[c], p.ang_sin[c], st->cand[c]);
        st->cand[c][2] = ctr[2];
    }
    st->radius = r;
    st->center_z = ctr[2];
}

template <typename T>
void inst_host(const T* pts, int64_t n, int dim, const void* labels, int label_bytes, const GroundSet& gs, const double* bank,
               const seg3d_aug_instance_plan* plans, int k, int64_t max_rows, double* add_points, void* add_labels,
               int32_t* decisions, int32_t* counts) {
    std::vector<double> xyz((size_t)max_rows * 3 + 1);
    int64_t added = 0;
    int32_t placed = 0;
    for (int i = 0; i < k; ++i) {
        const seg3d_aug_instance_plan& p = plans[i];
        InstState st;
        prepare_host(p, bank, dim, xyz.data(), &st);
        ScanRec rec[kMaxAngles];
        for (int c = 0; c < kMaxAngles; ++c) rec[c] = ScanRec{INFINITY, 0.0, kNoRow, 0};
        for (int64_t r = 0; r < n + added; ++r) {
            double x, y, z;
            int kind;
            if (r < n) {
                x = (double)pts[r * dim];
                y = (double)pts[r * dim + 1];
                z = (double)pts[r * dim + 2];
                kind = row_kind(gs, labels, label_bytes, r);
            } else {
                const double* row = add_points + (r - n) * dim;
                x = row[0];
                y = row[1];
                z = row[2];
                kind = row_kind(gs, add_labels, label_bytes, r - n);
            }
            if (kind == 0) continue;
            for (int c = 0; c < p.n_angles; ++c) {
                const double d = dist3(x, y, z, st.cand[c]);
                if (kind == 1) {
                    if (closer(d, (int32_t)r, rec[c].d, rec[c].row)) {
                        rec[c].d = d;
                        rec[c].z = z;
                        rec[c].row = (int32_t)r;
                    }
                } else if (d <= st.radius) {
                    rec[c].occ = 1;
                }
            }
        }
        int choice = -1;
        for (int c = p.n_angles - 1; c >= 0; --c)
            if (candidate_passes(rec[c], st.radius)) choice = c;
        decisions[i] = choice;
        if (choice < 0) continue;
        const double dz = (rec[choice].z + p.height) - st.center_z;
        for (int j = 0; j < p.n_rows; ++j) {
            paste_row(p, choice, dz, xyz.data() + (int64_t)j * 3, bank + (p.row_begin + j) * dim, dim,
                      add_points + (added + j) * dim);
            write_label(add_labels, label_bytes, added + j, p.label);
        }
        added += p.n_rows;
        placed += 1;
    }
    counts[0] = (int32_t)added;
    counts[1] = placed;
    counts[2] = counts[3] = 0;
}

}  // namespace

extern "C" {

size_t seg3d_aug_instance_workspace_bytes(int64_t n, int64_t max_instance_rows, int32_t k) {
    (void)n;  // the partial records are one per workgroup and candidate, and the grid is capped
    (void)k;  // instance k reuses the buffers of instance k - 2
    size_t bytes = 0;
    inst_carve(nullptr, max_instance_rows > 0 ? max_instance_rows : 0, &bytes);
    return bytes;
}

int seg3d_aug_instance_paste(const void* points, int64_t n, int32_t dim, int32_t point_bytes, const void* labels,
                             int32_t label_bytes, const uint8_t* ground_ids, int32_t n_ground, const double* bank,
                             int64_t bank_rows, const seg3d_aug_instance_plan* plans, int32_t k, int64_t cap_add,
                             double* add_points, void* add_labels, int32_t* decisions, int32_t* counts, void* workspace,
                             size_t workspace_bytes, void* stream) {
    GroundSet gs;
    int64_t max_rows = 0;
    if (!inst_args_ok(points, n, dim, point_bytes, labels, label_bytes, ground_ids, n_ground, bank, bank_rows, plans, k,
                      cap_add, add_points, add_labels, decisions, counts, &gs, &max_rows) ||
        !workspace)
        return SEG3D_EINVAL;
    if (workspace_bytes < seg3d_aug_instance_workspace_bytes(n, max_rows, k)) return SEG3D_EWORKSPACE;
    const InstWs w = inst_carve(workspace, max_rows, nullptr);
    hipStream_t st = as_stream(stream);
    if (point_bytes == 4)
        return inst_launch<float>(static_cast<const float*>(points), n, dim, labels, label_bytes, gs, bank, plans, k,
                                  add_points, add_labels, decisions, counts, w, st);
    return inst_launch<double>(static_cast<const double*>(points), n, dim, labels, label_bytes, gs, bank, plans, k, add_points,
                               add_labels, decisions, counts, w, st);
}

int seg3d_aug_instance_paste_host(const void* points, int64_t n, int32_t dim, int32_t point_bytes, const void* labels,
                                  int32_t label_bytes, const uint8_t* ground_ids, int32_t n_ground, const double* bank,
                                  int64_t bank_rows, const seg3d_aug_instance_plan* plans, int32_t k, int64_t cap_add,
                                  double* add_points, void* add_labels, int32_t* decisions, int32_t* counts) {
    GroundSet gs;
    int64_t max_rows = 0;
    if (!inst_args_ok(points, n, dim, point_bytes, labels, label_bytes, ground_ids, n_ground, bank, bank_rows, plans, k,
                      cap_add, add_points, add_labels, decisions, counts, &gs, &max_rows))
        return SEG3D_EINVAL;
    if (point_bytes == 4)
        inst_host<float>(static_cast<const float*>(points), n, dim, labels, label_bytes, gs, bank, plans, k, max_rows,
                         add_points, add_labels, decisions, counts);
    else
        inst_host<double>(static_cast<const double*>(points), n, dim, labels, label_bytes, gs, bank, plans, k, max_rows,
                          add_points, add_labels, decisions, counts);
    return SEG3D_OK;
}

}  // extern "C"
