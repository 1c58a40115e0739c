/*
 * seg3d_hip.h -- C ABI of libseg3d_hip.so, the MI355X (gfx950) implementation of the
 * OpenSeg3D sparse-voxel segmentation hot path.
 *
 * Boundary: the reference exposes this path as Python callables
 * backed by pybind11/CUDA extension modules and by the third-party spconv /
 * torch_scatter packages.  This header is what a binding for that path binds instead:
 * plain pointers and sizes, explicit stream, no torch types, no allocation inside
 * (callers pass workspaces sized by the *_workspace_bytes queries), no exceptions.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the parameter comment says "host";
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing
 *     synchronises, so every entry point is hipGraph-capturable;
 *   - return value: 0 = ok, <0 = SEG3D_E* below (checked before anything is enqueued);
 *   - row-major, float32 features, int32 indices; -1 marks "none";
 *   - coordinates are rows [batch, z, y, x] (spconv order), spatial shapes are (z, y, x);
 *   - kernel offset k = (kz*3 + ky)*3 + kx, neighbour site = site + (kz-1, ky-1, kx-1).
 *
 * Each entry cites the reference interface (path:line under /root/reference) it replaces.
 *
 * This file is also the ONLY description of the ABI the Python binding has: openseg3d_amd/_lib.py parses it when the
 * package is imported and derives every argtypes row, constant and ctypes.Structure from it, and refuses, naming the
 * declaration, whatever falls outside this grammar (plain C; block and line comments are dropped first):
 *   - #define SEG3D_<NAME> <decimal integer>, negative ones in parentheses: (-3);
 *   - typedef struct { <fields> } seg3d_<name>;  a field is <type> <name>[, <name>...]; each name may carry one array
 *     bound [<integer or SEG3D_ define>]; <type> is a scalar below, any pointer, or a struct typedef'd EARLIER;
 *   - <return type> seg3d_<name>(<parameters>);  a parameter is a pointer (anything with a '*') or a scalar with an
 *     optional name, or the list is `void`; no struct by value, no function pointer, no array parameter;
 *   - scalars: int, int32_t, int64_t, uint64_t, size_t, float, double; the return type may also be const char*;
 *   - the include guard, #include lines and every #ifdef __cplusplus ... #endif block are skipped; nothing else may
 *     stand at file scope.
 */
#ifndef SEG3D_HIP_H
#define SEG3D_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SEG3D_OK 0
#define SEG3D_EINVAL (-1)     /* bad argument (null pointer, unsupported size, ...) */
#define SEG3D_EWORKSPACE (-2) /* workspace smaller than the *_workspace_bytes query */
#define SEG3D_ELAUNCH (-3)    /* hipGetLastError() after a launch */

#define SEG3D_REDUCE_SUM 0
#define SEG3D_REDUCE_MEAN 1
#define SEG3D_REDUCE_MAX 2

/* ABI version; bumped whenever a signature below changes.  seg3d_abi_version() returns the value the library was built
 * with: a binding that read another one from this file is looking at a stale build. */
#define SEG3D_ABI_VERSION 59
int seg3d_abi_version(void);

/* Text of the HIP runtime error behind the calling thread's most recent SEG3D_ELAUNCH
 * ("<hipGetErrorString> (<hipGetErrorName>) at <file>:<line>"), "" if none yet.  The reference
 * surfaces argument failures as Python exceptions through TORCH_CHECK
 * (seg3d/ops/ingroup_inds/src/ingroup_inds.cpp:6-12) and checks nothing after its kernel launches
 * (ingroup_inds_cuda.cu:35-49); a C ABI that returns codes needs an accessor for the runtime's text.
 * The pointer stays valid for the life of the thread. */
const char* seg3d_last_error(void);

/* ------------------------------------------------------------------------------------------
 * a2  VoxelGenerator.__init__  -- seg3d/core/voxel/voxel_generator.py:11-22
 * grid = round((hi - lo) / voxel_size) evaluated in float32 (host helper, no GPU work).
 * voxel_size: host float[3] (x,y,z); range: host float[6] (xyz min, xyz max); grid_xyz: host int32[3].
 */
int seg3d_grid_size(const float* voxel_size, const float* range, int32_t* grid_xyz);

/* ------------------------------------------------------------------------------------------
 * a1 + a4  points_to_voxel / _points_to_voxel_reverse_kernel -- voxel_generator.py:55-153,
 *          batch id column + cumulative voxel-id offset of WaymoDataset.collate_batch --
 *          seg3d/datasets/waymo_dataset.py:339-365.
 * Hard voxelisation with first-seen voxel order, on device, for a whole collated batch:
 * c_j = floor((p_j - lo_j) / vs_j) with an IEEE subtract and true divide in the dtype of
 * `points`; a point is rejected (id -1) if any c_j is outside [0, grid_j).  A point with a
 * non-finite coordinate (NaN, +Inf, -Inf) is rejected in the same way, like the reference's
 * out-of-range points.
 *   points     [n, row_stride] row-major; xyz at columns xyz_col..xyz_col+2;
 *               batch id (stored as a float, as the reference collates it) at batch_col, or
 *               batch_col < 0 for a single sample (batch id 0)
 *   voxel_size, range: host float[3], float[6]  (float32 constants, widened for the f64 entry)
 *   voxel_coords      out [>= n, 4]  rows [b, z, y, x] in first-seen order
 *   point_voxel_ids   out [n]        batch-global voxel row of each point, -1 if rejected
 *   n_voxels          out device int32[1]
 */
size_t seg3d_voxelize_workspace_bytes(int64_t n_points);
int seg3d_voxelize_f32(const float* points, int64_t n_points, int32_t row_stride, int32_t xyz_col,
                       int32_t batch_col, const float* voxel_size, const float* range,
                       int32_t* voxel_coords, int32_t* point_voxel_ids, int32_t* n_voxels,
                       void* workspace, size_t workspace_bytes, void* stream);
int seg3d_voxelize_f64(const double* points, int64_t n_points, int32_t row_stride, int32_t xyz_col,
                       int32_t batch_col, const float* voxel_size, const float* range,
                       int32_t* voxel_coords, int32_t* point_voxel_ids, int32_t* n_voxels,
                       void* workspace, size_t workspace_bytes, void* stream);

/* (b) The CPU entry of VoxelGenerator.generate -- seg3d/core/voxel/voxel_generator.py:24-26 (-> points_to_voxel :55-95,
 * _points_to_voxel_reverse_kernel :98-153), called by DataLoader workers (seg3d/datasets/waymo_dataset.py:275) and
 * test-time augmentation (test_time_aug.py:33): forked processes WITHOUT a GPU context, which SURVEY 8(b) says must keep
 * a CPU voxelizer.  Same contract as seg3d_voxelize_f32 / _f64 with every pointer a HOST pointer and no stream: the
 * reference's serial first-seen loop, the dense 531 MB lookup grid replaced by an open-addressing table in the caller's
 * workspace.  Plain host code: makes no HIP call (safe after fork, runs on a machine without a GPU).  n_voxels: host
 * int32[1]; voxel_coords host [>= n_points, 4] rows (b, z, y, x). */
size_t seg3d_voxelize_host_workspace_bytes(int64_t n_points);
int seg3d_voxelize_host_f32(const float* points, int64_t n_points, int32_t row_stride, int32_t xyz_col,
                            int32_t batch_col, const float* voxel_size, const float* range,
                            int32_t* voxel_coords, int32_t* point_voxel_ids, int32_t* n_voxels,
                            void* workspace, size_t workspace_bytes);
int seg3d_voxelize_host_f64(const double* points, int64_t n_points, int32_t row_stride, int32_t xyz_col,
                            int32_t batch_col, const float* voxel_size, const float* range,
                            int32_t* voxel_coords, int32_t* point_voxel_ids, int32_t* n_voxels,
                            void* workspace, size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------
 * a3  cart2polar -- seg3d/utils/pointops_utils.py:8-11, wired into the cylinder configs at
 *     seg3d/datasets/waymo_dataset.py:270-273: rows [.., x, y, z, f..] -> [.., rho, phi, z, x, y, f..]
 *     (row_stride + 2 columns; the `xyz_col` columns in front -- the batch index of a collated tensor -- are
 *     copied).  rho = sqrt(x*x + y*y) in the point dtype, bit-identical to numpy; phi = atan2(y, x): float32 rows
 *     get the double-precision result rounded once, float64 rows the device library's atan2 (numpy takes the host
 *     libm's atan2f / atan2, documented at 1 ulp: that column of the reference is machine-dependent in its last bit).
 */
int seg3d_cart2polar_f32(const float* points, int64_t n_points, int32_t row_stride, int32_t xyz_col,
                         float* out /* [n_points, row_stride + 2] */, void* stream);
int seg3d_cart2polar_f64(const double* points, int64_t n_points, int32_t row_stride, int32_t xyz_col,
                         double* out /* [n_points, row_stride + 2] */, void* stream);

/* ------------------------------------------------------------------------------------------
 * a14  ingroup_inds_ext.forward(group_inds, out_inds) -- seg3d/ops/ingroup_inds/src/
 *      ingroup_inds.cpp:28-48, ingroup_inds_cuda.cu:12-25 (+ the CSR the callers rebuild from it).
 * Rank of every element inside its group.  The reference hands ranks out in atomic arrival
 * order; this build's canonical order is ascending element index (deterministic).
 *   group_ids [n] in [0, n_groups), or -1 = not in any group
 *   rank      out [n] or NULL   (-1 for skipped elements)
 *   order     out [n] or NULL   element indices grouped by group id, ascending inside a group
 *   offsets   out [n_groups+1] or NULL   CSR offsets into `order`
 */
size_t seg3d_group_index_workspace_bytes(int64_t n, int64_t n_groups);
int seg3d_group_index(const int32_t* group_ids, int64_t n, int64_t n_groups, int32_t* rank,
                      int32_t* order, int32_t* offsets, void* workspace, size_t workspace_bytes,
                      void* stream);

/* ------------------------------------------------------------------------------------------
 * a8-a11  spconv indice generation (third-party spconv, call sites seg3d/utils/spconv_utils.py:13-32,
 *         seg3d/models/backbones/pointtransformer.py:26-34,73-81,159-166,184-189).
 * Coordinate hash (open addressing, 64-bit linear site key -> row) and the neighbour tables
 * ("rulebooks") built from it.  Tables are offset-major int32 [27][m_rows], -1 = inactive.
 */
size_t seg3d_coord_hash_bytes(int64_t m);
int seg3d_coord_hash_build(const int32_t* coords, int64_t m, const int32_t* shape_zyx /*host[3]*/,
                           void* table, size_t table_bytes, void* stream);
/* SubMConv3d(k=3, padding=1): nbr[k][i] = row of the active site at coords[i] + offset(k). */
int seg3d_rulebook_subm(const int32_t* coords, int64_t m, const int32_t* shape_zyx /*host[3]*/,
                        const void* table, size_t table_bytes, int32_t* nbr, void* stream);
/* SparseConv3d(k=3, stride=2, padding=1) output sites, ascending (b,z,y,x).
 * shape_out = floor((shape_in + 2 - 3) / 2) + 1.  coords_out must hold cap_out >= min(8*m_in, cells) rows. */
size_t seg3d_downsample_workspace_bytes(int32_t batch_size, const int32_t* shape_in_zyx /*host[3]*/);
int seg3d_downsample_coords(const int32_t* coords_in, int64_t m_in,
                            const int32_t* m_in_dev /* or NULL: exact row count on the DEVICE when m_in is only an upper
                               bound -- lets the three strided levels be chained without reading a count back */,
                            int32_t batch_size, const int32_t* shape_in_zyx /*host[3]*/, int32_t* coords_out,
                            int64_t cap_out, int32_t* m_out /*device*/, void* workspace, size_t workspace_bytes,
                            void* stream);
/* nbr_fwd[k][o] = fine row at 2*coords_out[o] + k - 1; nbr_inv[k][i] = coarse row o with
 * 2*o + k - 1 == coords_in[i] (the table SparseInverseConv3d reuses under the same indice_key). */
int seg3d_rulebook_strided(const int32_t* coords_out, int64_t m_out, int64_t m_in,
                           const int32_t* shape_in_zyx /*host[3]*/, const void* table_in,
                           size_t table_bytes, int32_t* nbr_fwd, int32_t* nbr_inv, void* stream);

/* ------------------------------------------------------------------------------------------
 * a9-a11  spconv SubMConv3d / SparseConv3d / SparseInverseConv3d forward + backward
 *         (same call sites as above).  One output-stationary gather-GEMM kernel serves all three:
 *             y[r] = bias + sum_k x[nbr[k][r]] . W_k
 *   weight      [cout, 27, cin]  (= [Cout,3,3,3,Cin], the layout the modules keep)
 *   w_packed    seg3d_spconv_packed_bytes(cin, cout, flags) bytes written by seg3d_spconv_pack_weight;
 *               cin/cout there are those of `weight`; flags bit0: operand is W_k^T (dgrad), bit1: offsets
 *               reversed (k -> 26-k), bit2: split-bf16 pack -- every fp32 weight stored as bf16 hi + bf16 lo and
 *               the product evaluated as 3 bf16 MFMAs (hi*hi + hi*lo + lo*hi, fp32 accumulate, ~2^-16
 *               relative; 16/3 the fp32-MFMA rate).  Without bit2 the exact-fp32 MFMA path is used.
 *               seg3d_spconv_fwd must be given the same flags the pack was made with.
 * dgrad: seg3d_spconv_fwd over the transposed pair list with a W^T pack and cin/cout swapped:
 *        subm: same table, flags=3;  strided conv: the inverse table, flags=1;  inverse conv: the
 *        forward table, flags=1.
 * wgrad: dw[co][k][ci] = sum_r x[nbr[k][r]][ci] * dy[r][co].
 * cin and cout must be multiples of 16 (cin multiple of 4 for fwd).
 */
size_t seg3d_spconv_packed_bytes(int32_t cin, int32_t cout, int32_t flags);
int seg3d_spconv_pack_weight(const float* weight, int32_t cin, int32_t cout, int32_t flags,
                             void* w_packed, void* stream);
int seg3d_spconv_fwd(const float* x, const int32_t* nbr, int64_t m_out, int64_t m_in,
                     const void* w_packed, int32_t pack_flags, const float* bias /*or NULL*/,
                     int32_t cin, int32_t cout, float* y,
                     const int32_t* row_order /* [m_out] permutation: processing order of the output rows, or NULL.
                        Results do not depend on it; strided / inverse tables run ~2x faster when rows are grouped by
                        coordinate parity (same active offsets per tile).  Ignored by the exact-fp32 path. */,
                     void* stream);
/* Inference form of a conv block -- conv -> BatchNorm1d(eval) -> (+ residual) -> ReLU (ConvModule spconv_utils.py:13-32,
 * SparseBasicBlock pointtransformer.py:47-66 / spconv_unet.py:46-66): the caller folds the BatchNorm affine into the
 * weights before packing (W' = W * gamma * rstd per output channel) and into the bias (beta - mean * gamma * rstd
 * (+ conv bias * gamma * rstd)); the block is then ONE launch, y = act(conv_W'(x) + bias (+ addend [m_out, cout])).
 * Split-bf16 packs (flags bit2) only. */
int seg3d_spconv_fwd_act(const float* x, const int32_t* nbr, int64_t m_out, int64_t m_in, const void* w_packed,
                         int32_t pack_flags, const float* bias /*or NULL*/, const float* addend /*or NULL*/,
                         int32_t relu, int32_t cin, int32_t cout, float* y, const int32_t* row_order /*or NULL*/,
                         void* stream);
/* The same block with the sparse-conv feature maps STORED in bf16 (opt-in storage mode, BASELINE configs[4]; the
 * reference's only reduced-precision hook is seg3d/ops/voxel_pooling/voxel_pooling.py:12): x holds float32 (x_bf16 = 0)
 * or bf16 (x_bf16 = 1) rows, y and the residual addend are bf16 [m_out, cout]; accumulation, bias and activation stay
 * float32, the weights stay split-bf16 hi + lo.  A bf16 row is its own hi part: its products take two MFMAs instead of
 * three and its gather moves half the bytes.  Inference only (no backward entry point takes bf16 rows). */
int seg3d_spconv_fwd_act_bf16(const void* x, int32_t x_bf16, const int32_t* nbr, int64_t m_out, int64_t m_in,
                              const void* w_packed, int32_t pack_flags, const float* bias,
                              const void* addend_bf16, int32_t relu, int32_t cin, int32_t cout, void* y_bf16,
                              const int32_t* row_order, void* stream);
/* a9 "row image" schedule of the same gather-GEMM for submanifold tables (spconv.SubMConv3d, call sites
 * seg3d/utils/spconv_utils.py:15-17, seg3d/models/backbones/pointtransformer.py:26-34,47-66,88-113; spconv builds the
 * equivalent "indice pairs" once per indice_key and reuses them in every layer that names the key).  A TILE PLAN is built
 * once per neighbour table (site level): output rows in Morton order of their coordinates, 128 per tile, inside a tile
 * sorted by neighbour mask; per tile the list of DISTINCT input rows (<= 512, else the tile runs offset by offset) and,
 * per (offset, row), the LDS slot of the neighbour's row.  seg3d_spconv_fwd_tiled then loads and splits every distinct
 * input row of a tile ONCE per 32-channel slice into an LDS image and feeds all 27 offsets from it (spconv_split gathers and
 * splits per (row, offset) pair: 6.5 - 17 times per row).  Results are bit-identical to seg3d_spconv_fwd_act on the same
 * operands (same products in the same order per output row) for cout a multiple of 96 or 128.  EXCEPTION: cout 32 / 48
 * (and therefore cin 32 / 48 of the input-gradient conv, whose cout is the forward's cin) run the offset-split layouts --
 * the four waves of a workgroup take a quarter of a tile's 27 offsets each and their partial tiles are summed through LDS
 * in a fixed order: deterministic run to run, but ANOTHER summation order than seg3d_spconv_fwd_act's ascending offsets,
 * so the two entry points agree there to fp32 round-off (a few 1e-7 relative), not bit for bit.  coords [m_out, 4] (b, z, y, x) int32 are the sites the
 * table's rows belong to; nbr [27][m_out] may gather from any row set (m_in rows).  cout a multiple of 96 or 128, or 32 / 48
 * (seg3d_spconv_tiled_supported), split-bf16 packs only; forward and dgrad (W^T pack, flipped offsets) share one plan. */
size_t seg3d_conv_plan_bytes(int64_t m_out);
size_t seg3d_conv_plan_workspace_bytes(int64_t m_out);
int seg3d_conv_plan_build(const int32_t* coords, const int32_t* nbr, int64_t m_out, void* plan, void* workspace,
                          size_t workspace_bytes, void* stream);
int32_t seg3d_spconv_tiled_supported(int32_t cin, int32_t cout);
int seg3d_spconv_fwd_tiled(const float* x, const int32_t* nbr, const void* plan, int64_t m_out, int64_t m_in,
                           const void* w_packed, int32_t pack_flags, const float* bias /*or NULL*/,
                           const float* addend /*or NULL*/, int32_t relu, int32_t cin, int32_t cout, float* y, void* stream);
/* The tiled schedule with the feature maps STORED in bf16 -- seg3d_spconv_fwd_act_bf16's contract (opt-in storage mode,
 * BASELINE configs[4]): x float32 (x_bf16 = 0) or bf16 (x_bf16 = 1) rows, y and the residual addend bf16 [m_out, cout].  bf16
 * rows stage only a hi image (half the bytes) and take two MFMAs per product. */
int seg3d_spconv_fwd_tiled_bf16(const void* x, int32_t x_bf16, const int32_t* nbr, const void* plan, int64_t m_out,
                                int64_t m_in, const void* w_packed, int32_t pack_flags, const float* bias /*or NULL*/,
                                const void* addend_bf16 /*or NULL*/, int32_t relu, int32_t cin, int32_t cout, void* y_bf16,
                                void* stream);
/* Test hook: force the column-block width (x16 columns) of the split-bf16 gather-GEMM so that every kernel
 * instantiation can be pinned against the oracle at any row count (0 = automatic choice; 1, 2, 3, 4, 6, 12).
 * Same effect as the SEG3D_CONV_NBT environment variable, which is read once when the library loads.
 * The reference has no counterpart (spconv chooses its own tiles). */
int seg3d_debug_set_conv_nbt(int32_t nbt);
size_t seg3d_spconv_wgrad_workspace_bytes(int64_t m_out, int32_t cin, int32_t cout);
int seg3d_spconv_wgrad(const float* x, const float* dy, const int32_t* nbr, int64_t m_out,
                       int64_t m_in, int32_t cin, int32_t cout, int32_t flags /* bit2: split-bf16 */,
                       float* dw, void* workspace, size_t workspace_bytes, void* stream);

/* The first half of seg3d_spconv_wgrad alone (split-bf16 arithmetic): partial blocks part[chunks][27 * cin * cout] stay in the
 * workspace, *chunks (host) = their count (0 for m_out == 0: the sum then writes zeros); the fixed-order sum is queued by the
 * caller with the other parameter-gradient sums of the backward pass (seg3d_reduce_partials_batched).  spconv has no
 * counterpart: it accumulates weight gradients with atomics inside its own kernels (call sites spconv_utils.py:13-32). */
int seg3d_spconv_wgrad_partials(const float* x, const float* dy, const int32_t* nbr, int64_t m_out, int64_t m_in,
                                int32_t cin, int32_t cout, void* workspace, size_t workspace_bytes, int32_t* chunks,
                                void* stream);
/* The same with the layer's input rows stored as bf16 [m_in, cin] -- BASELINE configs[4] names bf16, the reference has no
 * reduced-precision mode, so the mode is build-defined and OPT-IN (SEG3D_TRAIN_STORAGE=bf16): the sparse-conv /
 * Linear autograd functions (call sites spconv_utils.py:13-32, point_transformer_layer.py:260-298) keep a bf16 COPY of their
 * input for the backward pass instead of the fp32 tensor; every tensor of the graph, and therefore every gradient, stays
 * fp32.  A bf16 row is its own high half: 8-byte gathers, no split of x, two MFMAs per product; dy stays fp32 / split. */
int seg3d_spconv_wgrad_partials_xbf16(const uint16_t* x_bf16, const float* dy, const int32_t* nbr, int64_t m_out,
                                      int64_t m_in, int32_t cin, int32_t cout, void* workspace, size_t workspace_bytes,
                                      int32_t* chunks, void* stream);

/* a6, a22  weight gradient of the dense per-point / per-voxel Linear layers (segformer.py:21-32,58-76,
 * point_transformer_layer.py:260-276, cosine_msa.py:58-63,403):  dw[cout][cin] = dy^T . x  over m rows.
 * Split-bf16 tall-skinny GEMM (rows = MFMA K dimension), workgroup-tiled; partial blocks per row chunk go to
 * the workspace and are summed in a fixed order, so dw/db are bit-reproducible and need no memset.
 * db (nullable) receives the bias gradient = column sums of dy.  cin, cout multiples of 4. */
size_t seg3d_linear_wgrad_workspace_bytes(int64_t m, int32_t cin, int32_t cout);
int seg3d_linear_wgrad(const float* x, const float* dy, int64_t m, int32_t cin, int32_t cout, float* dw,
                       float* db /* [cout] or NULL */, void* workspace, size_t workspace_bytes, void* stream);
/* The two halves of seg3d_linear_wgrad apart (same kernels): seg3d_linear_wgrad_partials leaves the per-chunk partial
 * blocks part[chunks][cin*cout + cout] in the workspace and reports the chunk count through *chunks (host memory; 0 when
 * m == 0); seg3d_reduce_partials sums part[chunks][n] in a fixed order into dw[0, nw) and db[0, n - nw) (db nullable; n, nw
 * multiples of 4; chunks == 0 writes zeros).  seg3d_reduce_partials_batched runs many such sums in ONE launch: jobs =
 * device array of { const float* part; float* dw; float* db; int64_t n, nw; int32_t chunks, reserved; int64_t first_block }
 * (56 bytes) sorted by first_block, a job owning ceil(n / 256) blocks; total_blocks = their sum.  A training step's
 * ~160 parameter-gradient sums (Linear weights / biases, LayerNorm gamma / beta) become one launch at the end of the
 * backward pass (openseg3d_amd/ops.py, deferred join).  The reference has no counterpart: torch.autograd sums inside each
 * layer's own GEMM / reduction kernels (point_transformer_layer.py:260-298). */
int seg3d_linear_wgrad_partials(const float* x, const float* dy, int64_t m, int32_t cin, int32_t cout, int32_t with_bias,
                                void* workspace, size_t workspace_bytes, int32_t* chunks, void* stream);
/* ... with x stored as bf16 [m, cin] (the opt-in training copies, see seg3d_spconv_wgrad_partials_xbf16) */
int seg3d_linear_wgrad_partials_xbf16(const uint16_t* x_bf16, const float* dy, int64_t m, int32_t cin, int32_t cout,
                                      int32_t with_bias, void* workspace, size_t workspace_bytes, int32_t* chunks,
                                      void* stream);
/* ... with x = max(x_pre * scale_in[ch] + shift_in[ch], 0) formed on operand load: the training-mode BatchNorm1d + ReLU in
 * front of the Linear, from its pre-activation x_pre [m, cin] fp32 and its folded affine (seg3d_batchnorm_stats rows 4, 5).
 * The plan of seg3d_linear_wgrad_partials: the same chunks and summation order, hence the same bits as seg3d_affine_act +
 * seg3d_linear_wgrad_partials.  seg3d_linear_wgrad_bnrelu_fits = 1 for the shapes the entry takes (EINVAL otherwise). */
int seg3d_linear_wgrad_bnrelu_fits(int64_t m, int32_t cin, int32_t cout);
int seg3d_linear_wgrad_partials_bnrelu(const float* x_pre, const float* scale_in, const float* shift_in, const float* dy,
                                       int64_t m, int32_t cin, int32_t cout, int32_t with_bias, void* workspace,
                                       size_t workspace_bytes, int32_t* chunks, void* stream);
int seg3d_reduce_partials(const float* part, int32_t chunks, int64_t n, int64_t nw, float* dw, float* db, void* stream);
/* One record of seg3d_reduce_partials_batched's `jobs`: a DEVICE array of n_jobs records sorted by first_block; job i
 * covers blocks [first_block_i, first_block_{i+1}), ceil(n / 256) of them. */
typedef struct {
  const float* part;    /* [chunks][n] partial blocks */
  float* dw;            /* [nw] */
  float* db;            /* [n - nw], or NULL */
  int64_t n, nw;
  int32_t chunks, reserved;
  int64_t first_block;
} seg3d_reduce_job;     /* 56 bytes */
int seg3d_reduce_partials_batched(const void* jobs, int32_t n_jobs, int64_t total_blocks, void* stream);
/* a6  exact-fp32 variant for the per-point MLPs (segformer.py:21-32,58-76), whose split-bf16 forward error would land
 * directly on the logits: the same contract as seg3d_linear_* on v_mfma_f32_16x16x4_f32;
 * cin, cout multiples of 16.  Forward: transpose = 0; input gradient: transpose = 1 with cin/cout swapped. */
size_t seg3d_linear_packed_bytes_f32(int32_t cin, int32_t cout);
int seg3d_linear_pack_weight_f32(const float* weight, int32_t cin, int32_t cout, int32_t transpose,
                                 void* w_packed, void* stream);
int seg3d_linear_fwd_f32(const float* x, int64_t m, const void* w_packed, const float* bias /*or NULL*/,
                         int32_t cin, int32_t cout, float* y, void* stream);
/* a6  fp32-GRADE variant on the bf16 matrix pipe (round 5; the default of the per-point MLPs, segformer.py:21-32,58-76):
 * every operand split three ways (x = h + m + l, bf16 each: exact), six v_mfma_f32_16x16x32_bf16 per product keep every
 * term down to 2^-16 of the leading one, the dropped ones are <= 2^-24 -- the error of an fp32 sum, at 6/16 of the fp32
 * MFMA's time (openseg3d_amd/csrc/linear_x6.hip).  cin a multiple of 32, cout of 64 (packed_bytes = 0 otherwise: the
 * caller takes seg3d_linear_fwd_f32).  Optional epilogue y * scale[col] + shift[col] (both or neither) and ReLU: the eval
 * form of the BatchNorm1d + ReLU behind these layers (seg3d/models/segmentors/segformer.py:21-32). */
size_t seg3d_linear_packed_bytes_x6(int32_t cin, int32_t cout);
int seg3d_linear_pack_weight_x6(const float* weight, int32_t cin, int32_t cout, int32_t transpose, void* w_packed,
                                void* stream);
int seg3d_linear_fwd_x6(const float* x, int64_t m, const void* w_packed, const float* bias /*or NULL*/,
                        const float* scale /*or NULL*/, const float* shift /*or NULL*/, int32_t relu, int32_t cin,
                        int32_t cout, float* y, void* stream);
/* ... on the output of a training-mode BatchNorm1d + ReLU formed on operand load: y = max(x_pre * scale_in + shift_in, 0)
 * W^T (+ bias), x_pre [m, cin] the pre-activation, scale_in / shift_in [cin] the folded affine; cin <= 2048.  The
 * activated tensor is never written; the result is bit-identical to seg3d_affine_act(relu) + seg3d_linear_fwd_x6. */
int seg3d_linear_fwd_x6_bnrelu(const float* x_pre, const float* scale_in, const float* shift_in, int64_t m,
                               const void* w_packed, const float* bias /*or NULL*/, int32_t cin, int32_t cout, float* y,
                               void* stream);

/* Batched split-bf16 packing: one launch for every conv / Linear weight whose pack is stale (in training all of
 * them, twice: W for forward, W^T for the input gradient).  `jobs` is a DEVICE array of n_jobs records sorted by
 * first_block; job i covers blocks [first_block_i, first_block_{i+1}) of 256 work items each, one item = 16 packed
 * elements (ceil(packed_bytes / 32 / 256) blocks); dst as for seg3d_spconv_pack_weight (flags bit2 set) /
 * seg3d_linear_pack_weight.  kk = 27 (conv, weight [Cout,27,Cin]) or 1 (Linear, weight [Cout,Cin]). */
typedef struct {
  const float* src;     /* weight in the reference layout */
  void* dst;            /* packed stream */
  int32_t cin, cout;    /* of the weight as stored */
  int32_t kk, transpose, flip, reserved;
  int64_t first_block;
} seg3d_pack_job;       /* 48 bytes */
int seg3d_pack_weights_batched(const void* jobs, int32_t n_jobs, int64_t total_blocks, void* stream);

/* a6, a22  forward / input gradient of the same layers: y[m, cout] = x[m, cin] . W^T + bias, as the
 * single-offset case of the split-bf16 gather-GEMM kernel (W fragments staged through LDS once per
 * 128-row tile).  weight is torch's [cout, cin]; transpose=1 packs W itself as the operand, i.e.
 * dx[m, cin] = dy[m, cout] . W is seg3d_linear_fwd(dy, ..., cin_of_call = cout, cout_of_call = cin).
 * Operand rows (cin of the call) must be a multiple of 8, columns (cout of the call) a multiple of 16. */
size_t seg3d_linear_packed_bytes(int32_t cin, int32_t cout, int32_t transpose);
int seg3d_linear_pack_weight(const float* weight, int32_t cin, int32_t cout, int32_t transpose,
                             void* w_packed, void* stream);
int seg3d_linear_fwd(const float* x, int64_t m, const void* w_packed, const float* bias /*or NULL*/,
                     const float* addend /* [m, cout] added in the epilogue, or NULL */, int32_t cin, int32_t cout,
                     float* y, void* stream);
/* y = (x + x_add) W^T + b without writing x + x_add: the q | k half of the cosine attention's in-projection reads
 * x + pos (cosine_msa.py:58-63 via point_transformer_layer.py:289-291).  Inference path; same kernel, the sum is taken on
 * the A operand's way into the bf16 split. */
int seg3d_linear_fwd_sum(const float* x, const float* x_add, int64_t m, const void* w_packed, const float* bias,
                         int32_t cin, int32_t cout, float* y, void* stream);
/* y = res + LayerNorm(x W^T + b) in ONE launch (inference path): the encoder layer's out-projection + norm1 + residual and
 * fc2 + norm2 + residual (point_transformer_layer.py:289-298; the reference runs Linear, LayerNorm and the add as three
 * kernels).  The normalised row must fit one workgroup: cout in {16, 32, 48, 64, 96, 128, 192}, SEG3D_EINVAL otherwise
 * (the caller then runs seg3d_linear_fwd + seg3d_layernorm_fwd).  res nullable.  Statistics as seg3d_layernorm_fwd takes
 * them: two-pass mean / biased variance in float32, rstd = rsqrt(var + eps). */
int seg3d_linear_layernorm_fwd(const float* x, int64_t m, const void* w_packed, const float* bias, const float* res,
                               const float* gamma, const float* beta, float eps, int32_t cin, int32_t cout, float* y,
                               void* stream);
/* y = (x W^T) * factor, elementwise ([m, cout] factor, no bias): the input gradient of the MLP's fc2 times the GELU
 * derivative saved by the training forward (point_transformer_layer.py:260-276; torch runs a gelu_backward pass there). */
int seg3d_linear_fwd_mul(const float* x, int64_t m, const void* w_packed, const float* factor, int32_t cin, int32_t cout,
                         float* y, void* stream);

/* ------------------------------------------------------------------------------------------
 * a13, a15, a16, a18  get_window_coors / batching_single_shift / get_flat2win_inds /
 *      make_continuous_inds -- seg3d/utils/swformer_utils.py:8-31,108-171,
 *      seg3d/models/layers/point_transformer_layer.py:71-87,141-149,209-220.
 * One call per (stage, shift).  Window id = b*Wx*Wy*Wz + wx*(Wy*Wz) + wy*Wz + wz with
 * w* = (c* + shift*) / win* (floor), in-window coordinate = (c* + shift*) % win*.
 *   win_xyz, nwin_xyz, shift_xyz : host int32[3]  (nwin = ceil(S/win)+1, swformer_utils.py:119-121)
 *   level_lo/level_hi/level_cap  : host int32[n_levels]  batching_range and max_tokens per level
 * Outputs (each [m] unless noted; any of win_id..slot may be NULL):
 *   win_id   batch_win_inds            in_win [m,3]  coors_in_win as (z,y,x)
 *   rank     in-window rank (ascending voxel row)    level  batching level, -1 if no range matches
 *   slot     flat2window index = compact_window_in_level * max_tokens + rank; -1 if rank >= max_tokens
 *            or level is -1 (such a window takes no compact index in any level)
 *   tok      voxel rows grouped by window (ascending window id, ascending row inside)
 *   win_start/win_count [<= min(m, canvas)]  CSR of the non-empty windows into tok
 *   win_tile0 [<= min(m, canvas)]  first 32-token tile of each window in the 32-padded token space
 *   tile_item [<= m/32 + windows][4]  {window, 32-token tile, win_start, win_count}: work items of the attention kernels, each
 *                                     a whole descriptor (one 16-byte read; no dependent win_start / win_count reads in front
 *                                     of a workgroup's first gather)
 *   qg_item   [<= m/16 + windows][4]  {window, 128-token chunk = 4 tiles, win_start, win_count}: items of the wide-head kernels
 *   counts   device int32[4]: {non-empty windows, voxels with slot == -1, 32-token tiles, 128-query chunks}
 */
size_t seg3d_window_partition_workspace_bytes(int64_t m, int32_t batch_size, const int32_t* nwin_xyz);
int seg3d_window_partition(const int32_t* coords, int64_t m, int32_t batch_size,
                           const int32_t* win_xyz, const int32_t* nwin_xyz, const int32_t* shift_xyz,
                           int32_t n_levels, const int32_t* level_lo, const int32_t* level_hi,
                           const int32_t* level_cap, int32_t* win_id, int32_t* in_win, int32_t* rank,
                           int32_t* level, int32_t* slot, int32_t* tok, int32_t* win_start,
                           int32_t* win_count, int32_t* win_tile0, int32_t* tile_item,
                           int32_t* qg_item, int32_t* counts, void* workspace,
                           size_t workspace_bytes, void* stream);

/* a17  SparseWindowPartitionLayer.get_pos_embed -- point_transformer_layer.py:151-203
 * pos[i] = cat_{d in x,y,z} interleave(sin(v_d / f[0::2]), cos(v_d / f[1::2])), v_d = in_win_d - win_d/2,
 * f = inv_freq [c/3] (device; the caller evaluates 1000**(2*(j//2)/(c/3)) exactly as torch does). */
int seg3d_pos_embed(const int32_t* in_win, int64_t m, const int32_t* win_xyz /*host[3]*/,
                    const float* inv_freq, int32_t c, float* pos, void* stream);

/* ------------------------------------------------------------------------------------------
 * a19-a21  flat2window -> CosineMultiheadAttention core -> window2flat --
 *      swformer_utils.py:34-85, point_transformer_layer.py:233-258,
 *      seg3d/models/layers/cosine_msa.py:115-177 (_scaled_cosine_attention).
 * Variable-length (CSR) form: no padded [W,T,C] tensors are materialised.  For every window w,
 * head h and query token i:  out_i = softmax_j( <q_i/|q_i|, k_j/|k_j|> / max(tau, tau_min) ) . v_j
 * over the tokens j of the same window.  q, k, v are the in-projection outputs in flat voxel
 * order with row strides ldq/ldk/ldv (floats); head h occupies columns [h*dh, (h+1)*dh).
 *   out [m, heads*dh] flat voxel order (input of the out-projection); lse [m, heads] or NULL
 *   (log-sum-exp per query row, kept for the backward).  m = number of voxel rows; dh in {6,12,24,48}
 *   (8 heads on 48/96/192/384 channels, pointtransformer.py:141-157).
 * Forward runs on the matrix cores in split-bf16 arithmetic (q, k, v, P as bf16 hi + lo, three
 * v_mfma_f32_16x16x32_bf16 per product, fp32 accumulate and softmax) in ONE launch per layer of PERSISTENT workgroups:
 * each walks its share of the work items -- (32-query tile, 4 heads) for dh 6 / 12 (tile_item), (128-query chunk, head)
 * for dh 24 / 48 (qg_item: the second field counts 128-token chunks, four 32-token tiles) -- gathers, normalises and
 * splits the item's query rows and the window's k / v rows itself, 32 keys at a time, through LDS, and requests the next
 * item's rows while the current one is multiplied; n_tiles / n_qgroups are counts[2..3] of seg3d_window_partition.
 * dropout_p / dropout_seed: attention-probability dropout of training mode (cosine_msa.py:172-174); 0 = none.
 * The mask is a function of (seed, window, head, query, key) only -- the backward is given the same two values
 * and regenerates it.  Drop probability is rounded to a multiple of 1/256 and compensated exactly.
 * Backward takes the forward's out and lse, returns gradients w.r.t. the raw q, k, v (through the
 * normalisation) and stores the tau gradient in dtau[0] (per-wave partials in the workspace, summed in a
 * fixed order: the whole backward is free of atomics and identical from run to run).
 * Head geometries: dh 6 with 4 / 8 / 16 heads, dh 12 with 4 / 8 / 12 / 16 heads, dh 24 / 48 with 1 .. 16 heads
 * (the reference builds 8 heads of 6 / 12 / 24 / 48 channels, pointtransformer.py:143-155); seg3d_window_attn_supported
 * returns 1 for those, everything else is refused with SEG3D_EINVAL.  win_tile0 is accepted and ignored (it served
 * kernels removed in ABI 30); the forward needs no workspace, seg3d_window_attn_workspace_bytes sizes the backward's.
 */
int seg3d_window_attn_supported(int32_t heads, int32_t dh);
size_t seg3d_window_attn_workspace_bytes(int64_t m, int32_t n_tiles, int32_t heads, int32_t dh);
/* Host only, no launch: the schedule seg3d_window_attn_fwd (called with an lse) and _bwd take for a window index with
 * n_tiles 32-token tiles and n_chunks 128-token chunks (counts[2..3] of seg3d_window_partition), computed by the functions
 * the launchers themselves call.  out[0] forward kernel: 0 fused persistent, 1 vector-ALU (one workgroup per tile);
 * out[1] forward grid cap = CUs x resident workgroups per CU (0 for the vector-ALU kernel, which has none; with zero items
 * the cap is still reported); out[2] forward grid; out[3] the most work units -- (item, head group) -- any forward workgroup
 * walks (1 = the persistent loop is not iterated); out[4] items per XCD block of the forward's item order (the fused backward
 * deals its blocks the same way; 1 for the vector-ALU kernel); out[5] workgroups of each backward pass, padding included.
 * SEG3D_EINVAL for a null out, negative counts, n_chunks > n_tiles, dropout_p outside [0, 1) or a head geometry
 * seg3d_window_attn_supported refuses. */
int seg3d_window_attn_schedule(int32_t n_tiles, int32_t n_chunks, int32_t heads, int32_t dh, float dropout_p, int32_t* out);
int seg3d_window_attn_fwd(const float* q, const float* k, const float* v, int32_t ldq, int32_t ldk,
                          int32_t ldv, const int32_t* tok, const int32_t* win_start,
                          const int32_t* win_count, const int32_t* win_tile0,
                          const int32_t* tile_item, int32_t n_tiles, const int32_t* qg_item,
                          int32_t n_qgroups, int64_t m, int32_t n_windows, int32_t heads, int32_t dh,
                          const float* tau, float tau_min, float dropout_p, uint64_t dropout_seed, float* out,
                          float* lse, void* workspace, size_t workspace_bytes, void* stream);
int seg3d_window_attn_bwd(const float* q, const float* k, const float* v, int32_t ldq, int32_t ldk,
                          int32_t ldv, const float* out, const float* dout, const float* lse,
                          const int32_t* tok, const int32_t* win_start, const int32_t* win_count,
                          const int32_t* win_tile0, const int32_t* tile_item, int32_t n_tiles,
                          const int32_t* qg_item, int32_t n_qgroups, int64_t m, int32_t n_windows,
                          int32_t heads, int32_t dh, const float* tau,
                          float tau_min, float dropout_p, uint64_t dropout_seed, float* dq, float* dk,
                          float* dv, int32_t lddq, int32_t lddk,
                          int32_t lddv, float* dtau, void* workspace, size_t workspace_bytes,
                          void* stream);

/* The two constructor options of the reference's attention layer the entries above do not take --
 *      seg3d/models/layers/cosine_msa.py:413-432 (non_shared_tau), :156-160 (tau [1, H, 1, 1] clamped per head),
 *      :163-165 (cosine=False: scores q.k / sqrt(dh), no normalisation, no tau),
 *      point_transformer_layer.py:222-231 (WindowAttention(..., cosine, tau_min)).
 * mode SEG3D_ATTN_COSINE: n_tau = 1 (the shared tau: the kernels and the bits of seg3d_window_attn_fwd / _bwd) or
 *   n_tau = heads: head h uses max(tau[h], tau_min).  The forward takes the fixed or the running softmax maximum head by
 *   head; the backward stores dtau[h] for every head (per-wave / per-tile partials of ONE head each in the workspace, summed
 *   in a fixed order, no atomics: identical from run to run), exactly 0 while tau[h] <= tau_min.
 * mode SEG3D_ATTN_DOT: n_tau = 0, tau = NULL, dtau = NULL, tau_min is ignored.  out_i = softmax_j(<q_i, k_j> / sqrt(dh)) . v_j;
 *   scores are unbounded, so every query row keeps a running maximum and lse is the true log-sum-exp; the backward goes
 *   straight to q and k.
 * Everything else -- operands, window index, dropout, head geometries (seg3d_window_attn_supported), schedule
 * (seg3d_window_attn_schedule) -- is as above, except that per-head tau at dh 6 runs the vector-ALU forward (exact fp32
 * scores) whenever an lse is given, with or without dropout; the ignored win_tile0 is gone.  SEG3D_EINVAL: a mode other than the two,
 * n_tau that is neither 1 nor heads (cosine) or not 0 (dot), tau given in dot mode or missing in cosine mode, a dtau that does
 * not match the mode (missing in cosine, given in dot), rows that are not 16-byte aligned, a refused head geometry.
 * SEG3D_EWORKSPACE: the backward's workspace is smaller than seg3d_window_attn_workspace_bytes_modes says (0 = refused
 * arguments).  Empty inputs (m, windows, tiles or chunks = 0) return SEG3D_OK; dtau[0 .. n_tau) is zeroed when given. */
#define SEG3D_ATTN_COSINE 0
#define SEG3D_ATTN_DOT 1
size_t seg3d_window_attn_workspace_bytes_modes(int64_t m, int32_t n_tiles, int32_t heads, int32_t dh, int32_t mode,
                                               int32_t n_tau);
int seg3d_window_attn_fwd_modes(const float* q, const float* k, const float* v, int32_t ldq, int32_t ldk, int32_t ldv,
                                const int32_t* tok, const int32_t* win_start, const int32_t* win_count,
                                const int32_t* tile_item, int32_t n_tiles, const int32_t* qg_item, int32_t n_qgroups,
                                int64_t m, int32_t n_windows, int32_t heads, int32_t dh, int32_t mode, const float* tau,
                                int32_t n_tau, float tau_min, float dropout_p, uint64_t dropout_seed, float* out, float* lse,
                                void* workspace, size_t workspace_bytes, void* stream);
int seg3d_window_attn_bwd_modes(const float* q, const float* k, const float* v, int32_t ldq, int32_t ldk, int32_t ldv,
                                const float* out, const float* dout, const float* lse, const int32_t* tok,
                                const int32_t* win_start, const int32_t* win_count, const int32_t* tile_item,
                                int32_t n_tiles, const int32_t* qg_item, int32_t n_qgroups, int64_t m, int32_t n_windows,
                                int32_t heads, int32_t dh, int32_t mode, const float* tau, int32_t n_tau, float tau_min,
                                float dropout_p, uint64_t dropout_seed, float* dq, float* dk, float* dv, int32_t lddq,
                                int32_t lddk, int32_t lddv, float* dtau, void* workspace, size_t workspace_bytes,
                                void* stream);

/* ------------------------------------------------------------------------------------------
 * a12, a22  row-wise normalisation layers on [m, c] features (c multiple of 4).
 * LayerNorm of the post-norm encoder layer (point_transformer_layer.py:289-298), fused with the residual:
 *     y = res + rowscale_row * ((x - mean_row) * rstd_row * gamma + beta)
 * res may be NULL; rowscale [m] (the per-row DropPath factor, seg3d/models/layers/drop.py:6-19) may be NULL = 1;
 * mean/rstd [m] are kept for the backward pass.
 * backward: dx, and dgamma/dbeta [c] (per-block partial sums in the workspace, summed in a fixed order: deterministic);
 * the residual's gradient is dy itself.
 * BatchNorm1d (+ residual) (+ ReLU) of the conv blocks / point MLPs (spconv_utils.py:13-32,
 * pointtransformer.py:47-66, segformer.py:21-76):
 *     seg3d_colstats   sums[0..c) = sum_r (x - x[0]), sums[c..2c) = sum_r (x - x[0])^2   (shifted, cancellation-free)
 *                      per-block partial sums in the workspace (seg3d_batchnorm_workspace_bytes), summed in a fixed
 *                      order: no atomics, results are identical from run to run
 *     seg3d_batchnorm_stats  colstats + one finalize pass: stats [6][c] = {scratch, scratch, mean, rstd (biased
 *                      variance), scale = gamma*rstd, shift = beta - mean*scale}; running_mean / running_var (may be
 *                      NULL) updated in place with `momentum` (unbiased variance), as torch.nn.BatchNorm1d does
 *     seg3d_affine_act y = act(x * scale + shift (+ res)), scale/shift [c] as produced above (or folded from the
 *                      running statistics by the caller in eval mode)
 *     seg3d_batchnorm_bwd  g = dy masked by (y > 0) when relu; dres = g (may be NULL);
 *                      dx = gamma*rstd*(g - mean_r(g) - xhat*mean_r(g*xhat)); sums = {dbeta, dgamma}
 */
int seg3d_layernorm_fwd(const float* x, const float* res, const float* gamma, const float* beta,
                        const float* rowscale, float eps, int64_t m, int32_t c, float* y, float* mean,
                        float* rstd, void* stream);
size_t seg3d_layernorm_bwd_workspace_bytes(int64_t m, int32_t c);
int seg3d_layernorm_bwd(const float* dy, const float* x, const float* mean, const float* rstd,
                        const float* gamma, const float* rowscale, int64_t m, int32_t c, float* dx,
                        float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, void* stream);
/* seg3d_layernorm_bwd without its final sum: dx now, the per-block partial sums of dgamma / dbeta left in the workspace as
 * part[*nblocks][2][c] -- a seg3d_reduce_partials job with n = 2 c, nw = c, dw = dgamma, db = dbeta. */
int seg3d_layernorm_bwd_partials(const float* dy, const float* x, const float* mean, const float* rstd,
                                 const float* gamma, const float* rowscale, int64_t m, int32_t c, float* dx,
                                 void* workspace, size_t workspace_bytes, int32_t* nblocks, void* stream);
size_t seg3d_batchnorm_workspace_bytes(int64_t m, int32_t c);
int seg3d_colstats(const float* x, int64_t m, int32_t c, float* sums, void* workspace, size_t workspace_bytes,
                   void* stream);
/* seg3d_colstats about a shift [c] of the caller's instead of x[0] (NULL = x[0]): sums[0..c) = sum_r (x - shift),
 * sums[c..2c) = sum_r (x - shift)^2.  The relative error of the variance formed from them grows with
 * 1 + ((shift - mean) / sigma)^2, so a shift near the column mean (the mean of a few rows) keeps it at rounding level
 * whatever row 0 holds; SyncBatchNorm's per-rank moments use it. */
int seg3d_colstats_about(const float* x, const float* shift, int64_t m, int32_t c, float* sums, void* workspace,
                         size_t workspace_bytes, void* stream);
int seg3d_batchnorm_stats(const float* x, int64_t m, int32_t c, float eps, const float* gamma, const float* beta,
                          float momentum, float* running_mean, float* running_var, float* stats, void* workspace,
                          size_t workspace_bytes, void* stream);
/* GELU, erf form (torch.nn.GELU default, point_transformer_layer.py:265): g = h Phi(h); gp (nullable) = d g / d h =
 * Phi(h) + h phi(h), written in the same pass by the training forward.  n = number of elements, a multiple of 4. */
int seg3d_gelu_fwd(const float* h, int64_t n, float* g, float* gp, void* stream);
int seg3d_affine_act(const float* x, const float* res, const float* scale, const float* shift, int32_t relu,
                     int64_t m, int32_t c, float* y, void* stream);
int seg3d_batchnorm_bwd(const float* dy, const float* y, const float* x, const float* mean, const float* rstd,
                        const float* gamma, int32_t relu, int64_t m, int32_t c, float* dx, float* dres,
                        float* sums, void* workspace, size_t workspace_bytes, void* stream);
/* seg3d_batchnorm_bwd for relu = 1 without a residual, from the pre-activation alone: the ReLU mask is formed as
 * x * scale + shift > 0 (scale / shift as seg3d_batchnorm_stats left them, rounded as seg3d_affine_act rounds), which is
 * y > 0 bit for bit; two row reads per pass instead of three, and y need not be kept for the backward. */
int seg3d_batchnorm_bwd_pre(const float* dy, const float* x, const float* scale, const float* shift, const float* mean,
                            const float* rstd, const float* gamma, int64_t m, int32_t c, float* dx, float* sums,
                            void* workspace, size_t workspace_bytes, void* stream);
/* torch.nn.SyncBatchNorm (tools/train.py:246-247, --sync_bn): the two halves of seg3d_batchnorm_bwd as separate
 * entries.  _reduce writes the rank-local sums = {sum g, sum g*xhat} (= dbeta, dgamma of this rank, which is what
 * torch's SyncBatchNorm hands DDP); the caller all-reduces a copy over the ranks and passes it to _apply together
 * with inv_count = device float[1] holding 1 / (rows of all ranks); mean / rstd are the synchronised statistics. */
int seg3d_batchnorm_bwd_reduce(const float* dy, const float* y, const float* x, const float* mean,
                               const float* rstd, int32_t relu, int64_t m, int32_t c, float* sums,
                               void* workspace, size_t workspace_bytes, void* stream);
int seg3d_batchnorm_bwd_apply(const float* dy, const float* y, const float* x, const float* mean,
                              const float* rstd, const float* gamma, const float* sums, const float* inv_count,
                              int32_t relu, int64_t m, int32_t c, float* dx, float* dres, void* stream);

/* ------------------------------------------------------------------------------------------
 * a7, a25, a26  torch_scatter.scatter(src, index, dim=0, reduce='mean'|'max') at
 *      seg3d/models/voxel_encoders/vfe.py:24-25, seg3d/models/layers/se_layer.py:24-28, and
 *      voxel_pooling_ext.voxel_pooling_{forward,backward}_* -- seg3d/ops/voxel_pooling/src/
 *      voxel_pooling.cpp:5-43, voxel_pooling_cuda.cu:10-79.
 * Segmented reduce over a CSR (order, offsets) built by seg3d_group_index: deterministic, no
 * float atomics.  Empty segments give 0.  argmax [n_seg, c] (MAX only, may be NULL) records the
 * source row (first maximum in ascending row order), -1 for empty segments.
 */
int seg3d_segment_reduce_fwd(const float* x, int32_t c, const int32_t* order, const int32_t* offsets,
                             int64_t n_seg, int32_t mode, float* out, int32_t* argmax, void* stream);
/* dx [n, c] must be zero-filled by the caller for MAX; fully written for SUM/MEAN (seg_of_row = group ids; rows
 * whose id is outside [0, n_seg), which seg3d_group_index left out of the CSR, get 0). */
int seg3d_segment_reduce_bwd(const float* dout, int32_t c, const int32_t* seg_of_row, int64_t n,
                             const int32_t* offsets, const int32_t* argmax, int64_t n_seg,
                             int32_t mode, float* dx, void* stream);

/* SURVEY 8(f) rank 1  DeepFusionBlock's cross attention over the kNN rows -- seg3d/models/layers/deep_fusion.py:26-45:
 *     out_i = sum_j dropout(nan_to_num(softmax_j(<q_i, k_{idx[i][j]}> * scale, -inf where invalid[idx[i][j]]))) . v_{idx[i][j]}
 * q [n, d], k / v [n_src, d], idx int32 [n, n_neighbors] (rows of k / v), d = 32, n_neighbors <= 16, scale = 1 / sqrt(d).
 * invalid uint8 [n_src] (1 = the source row has no image feature: torch.sum(image_features, 1) == 0) or NULL;
 * keep float [n, n_neighbors] = the dropout factors F.dropout would multiply with (0 or 1 / (1 - p)) or NULL;
 * prob [n, n_neighbors] receives the softmax (before dropout) for the backward, may be NULL.  Nothing of size
 * [n, n_neighbors, d] is materialised.  Backward: dq, and dk / dv by a fixed-order sum over the inverse neighbour
 * lists -- pair_order / pair_offsets = seg3d_group_index of the flattened idx table over the n_src rows -- so it is
 * free of float atomics and bit-reproducible; scratch holds 2 * n * n_neighbors floats. */
int seg3d_knn_attention_fwd(const float* q, const float* k, const float* v, const int32_t* idx,
                            const uint8_t* invalid, const float* keep, int64_t n, int64_t n_src,
                            int32_t n_neighbors, int32_t d, float scale, float* out, float* prob, void* stream);
int seg3d_knn_attention_bwd(const float* q, const float* k, const float* v, const int32_t* idx, const float* keep,
                            const float* prob, const float* dout, const int32_t* pair_order,
                            const int32_t* pair_offsets, int64_t n, int64_t n_src, int32_t n_neighbors, int32_t d,
                            float scale, float* dq, float* dk, float* dv, float* scratch, void* stream);

/* SURVEY 8(f) rank 3  OCR's SpatialGatherModule -- seg3d/models/layers/ocr.py:10-36: per sample b (a span of rows:
 * offsets [batch] = cumulative row counts, the stride-8 level is sorted by batch index) and class k,
 *     context[b, k, :] = sum_{r in b} softmax_r(scale * probs[r, k]) * feats[r, :]
 * instead of a Python loop over the samples with boolean masks.  feats [m, c], probs [m, classes <= 32];
 * chunks [n_chunks][2] = (sample, first row) of every 128-row chunk in sample order, chunk_offsets [batch] = cumulative
 * chunk counts.  weights [m, classes] (kept for the backward), partials [n_chunks, classes, c] and stats
 * [batch, classes, 2] are caller-provided scratch; sums run in a fixed order (no atomics).  Backward returns d feats
 * [m, c] and d probs [m, classes]; scratch = m * classes + n_chunks * classes floats.  offsets must not decrease and
 * must not exceed m (the caller checks: they are host integers there); rows at or behind offsets[batch - 1] are in no
 * sample: they add nothing to the context, their weights are left unwritten and both their gradients are 0. */
int seg3d_class_context_fwd(const float* feats, const float* probs, const int32_t* offsets, const int32_t* chunks,
                            const int32_t* chunk_offsets, int32_t n_chunks, int32_t batch, int64_t m,
                            int32_t classes, int32_t c, float scale, float* weights, float* partials, float* stats,
                            float* context, void* stream);
int seg3d_class_context_bwd(const float* feats, const float* weights, const float* dcontext,
                            const int32_t* offsets, const int32_t* chunks, const int32_t* chunk_offsets,
                            int32_t n_chunks, int32_t batch, int64_t m, int32_t classes, int32_t c, float scale,
                            float* dfeats, float* dprobs, float* scratch, void* stream);

/* a24  VoxelToPoint.__call__ -- seg3d/ops/voxel_to_point/voxel_to_point.py:4-17
 * out[i] = feats[ids[i]] (zeros where ids[i] == -1).  Its backward is
 * seg3d_segment_reduce_fwd(dout, SUM) over the CSR of ids. */
int seg3d_gather_rows(const float* feats, const int32_t* ids, int64_t n, int32_t c, float* out,
                      void* stream);

/* ------------------------------------------------------------------------------------------
 * SURVEY 8(f) rank 1  knn_query_ext.knn_query_cuda -- seg3d/ops/knn_query/src/knn_query_cuda.cu:67-133,
 *      wrapper seg3d/ops/knn_query/knn_query.py:7-24 (callers: DeepFusionBlock deep_fusion.py:31, tools/train.py:103).
 * For every query row of new_xyz [m,3] the k nearest rows of xyz [n,3] inside the same batch segment
 * (offset / new_offset: cumulative int32 counts per sample), ascending squared distance; ties by ascending
 * candidate index; slots beyond the segment size hold (1e10, segment start) as in the reference.  k <= 64.
 */
int seg3d_knn_query(const float* xyz, int64_t n, const float* new_xyz, int64_t m, const int32_t* offset,
                    const int32_t* new_offset, int32_t batch_size, int32_t k, int32_t* idx, float* dist2,
                    void* stream);

/* Grid-accelerated exact kNN (same results and tie rule as seg3d_knn_query) for large clouds.  Nothing here reads a
 * device value on the host: a whole query is a fixed sequence of launches.
 *   seg3d_knn_level_build  one grid level over xyz [n,3]: key = (batch << 48 | cx << 32 | cy << 16 | cz), c* =
 *                          floor(p / cell) + 32768 (clamped); device radix sort of (key, row); sorted_xyz [n,3] = points
 *                          in cell order, src_index [n] = their original rows; for the first point of every cell
 *                          (sorted position s): cell_end[s] = end of the cell's run, and key -> s goes into the
 *                          open-addressing table (capacity: power of two >= 2 n; table_keys capacity x 8 B,
 *                          table_vals capacity x 4 B).  Workspace: seg3d_knn_level_workspace_bytes(n) (0 = invalid n or
 *                          no device visible -- the sort's scratch size comes from rocPRIM).
 *   seg3d_knn_query_order  order [m] = query rows sorted by their cell key on a grid of the given cell size (neighbouring
 *                          lanes then walk the same cells); same workspace query with n = m.
 *   seg3d_knn_grid_query   per query: cube shells around its cell until the k-th distance is below the shell bound; up to
 *                          four grids, fine to coarse (lidar density falls as 1/r^2): a query still open after a level's
 *                          max_ring shells restarts on the next level, and scans its whole segment after the last one.
 *                          When every level's cell is exactly 8x the previous one, a coarse cell holding > 128 points is
 *                          searched through its sub-cells, pruned by box distance against the current k-th distance.
 *                          batch_size <= 255.  `levels` is a HOST array. */
size_t seg3d_knn_level_workspace_bytes(int64_t n);
int seg3d_knn_level_build(const float* xyz, int64_t n, const int32_t* offset, int32_t batch_size, float cell,
                          float* sorted_xyz, int32_t* src_index, int32_t* cell_end, void* table_keys, int32_t* table_vals,
                          int64_t capacity, void* workspace, size_t workspace_bytes, void* stream);
int seg3d_knn_query_order(const float* new_xyz, int64_t m, const int32_t* new_offset, int32_t batch_size, float cell,
                          int32_t* order, void* workspace, size_t workspace_bytes, void* stream);
/* a10/a11 scheduling aid: order [m] = rows of coords [m,4] (b,z,y,x) grouped by the parity of (z, y, x), original order
 * kept inside a group (stable 3-bit device radix sort).  Under SparseConv3d(k=3, s=2, p=1) the kernel offsets that can
 * reach a fine site are fixed by its parity, so 128-row tiles of same-parity rows of the inverse table visit 1-8 of
 * the 27 offsets (row_order of seg3d_spconv_fwd).  Workspace: seg3d_knn_level_workspace_bytes(m). */
int seg3d_parity_order(const int32_t* coords, int64_t m, int32_t* order, void* workspace, size_t workspace_bytes,
                       void* stream);
typedef struct {
  const float* sorted_xyz;     /* [n,3] points in this level's cell order */
  const int32_t* src_index;    /* [n] original row of each sorted point */
  const int32_t* cell_end;     /* [n] valid at the first sorted position of every cell */
  const void* table_keys;      /* capacity x 8 B */
  const int32_t* table_vals;   /* capacity x 4 B: first sorted position of the cell */
  int64_t capacity;
  float cell;                  /* metres */
  int32_t max_ring;            /* shells walked on this level (<= 16) */
} seg3d_knn_level;
int seg3d_knn_grid_query(const seg3d_knn_level* levels, int32_t n_levels, const float* new_xyz,
                         const int32_t* query_order /* queries in level-0 cell order, or NULL */, int64_t m,
                         const int32_t* offset, const int32_t* new_offset, int32_t batch_size, int32_t k,
                         int32_t* idx, float* dist2, void* stream);

/* ------------------------------------------------------------------------------------------
 * sampling_ext.furthestsampling_cuda -- seg3d/ops/sampling/src/sampling_cuda.cu:19-134, wrappers
 *      seg3d/ops/sampling/sampling.py:7-86 (furthestsampling, sectorized_fps).
 * Furthest-point sampling per segment: rows offset[i-1]:offset[i] of xyz [n,3] (contiguous float32), output slots
 * new_offset[i-1]:new_offset[i] of idx (cumulative int32 counts, as in seg3d_knn_query).
 *   - the first pick is the segment's first row; every further pick is the row with the largest
 *     tmp[k] = fminf(tmp[k], d(k, last pick)), tmp starting at 1e10,
 *     d = ((x2-x1)*(x2-x1) + (y2-y1)*(y2-y1)) + (z2-z1)*(z2-z1) in float32, every operation rounded, no FMA;
 *   - ties go to the lowest row of the segment (the reference's winner among exactly equal distances falls out of its
 *     shared-memory tree and changes with the block size); without exact ties both rules select the same rows;
 *   - a segment with 0 slots writes nothing (the reference writes idx[start] unconditionally); a segment with 0 rows
 *     and more than 0 slots gets -1 in its slots; a segment asked for more picks than it has rows keeps producing its
 *     lowest row of distance 0;
 *   - order (int32 [n], nullable): row k of a segment is xyz[order[k]] and the value stored is order[k]; "lowest row"
 *     then means lowest k.  Entries must lie in [0, n): one outside is never used as an address (its row counts as
 *     a point of running distance 0), but it can still be returned once every distance of the segment is 0.
 *     idx holds rows of xyz, int32.
 * One workgroup per segment, tier chosen on the device from the segment length (registers up to 16384 rows, four
 * float planes x, y, z, tmp in the workspace above).  No allocation, no sync, capturable.  The workspace (16 bytes per
 * row, 16-byte aligned) is required whatever the lengths.  _host: the same arithmetic and tie rule in serial C++,
 * no HIP call. */
size_t seg3d_furthest_sampling_workspace_bytes(int64_t n);
int seg3d_furthest_sampling(const float* xyz, int64_t n, const int32_t* order, const int32_t* offset,
                            const int32_t* new_offset, int32_t n_segments, int32_t* idx, void* workspace,
                            size_t workspace_bytes, void* stream);
int seg3d_furthest_sampling_host(const float* xyz, int64_t n, const int32_t* order, const int32_t* offset,
                                 const int32_t* new_offset, int32_t n_segments, int32_t* idx);
/* The sector partition of sectorized_fps (sampling.py:49-55).
 *   seg3d_sector_angles  angle [n] = atan2(x, y), x first as the reference writes it, evaluated in double and rounded
 *                        once (the CUDA atan2f it replaces is not correctly rounded); minmax [batch_size, 2] = min and
 *                        max of every sample's angles, NaN when one of them is NaN (as torch.min / torch.max: the caller
 *                        refuses such a sample, so NaN rows are reported rather than skipped) or the sample has no row.
 *   seg3d_sector_assign  sector_id [n] = sector_offset[b] + the first s with edge[s] <= angle < edge[s+1], or -1 (NaN
 *                        angles); sample b has sector_offset[b+1] - sector_offset[b] sectors (sector_offset
 *                        [batch_size + 1], cumulative) and one edge more, starting at edges[sector_offset[b] + b].
 * seg3d_group_index over sector_id then gives the `order` and the segment offsets of seg3d_furthest_sampling. */
int seg3d_sector_angles(const float* xyz, int64_t n, const int32_t* offset, int32_t batch_size, float* angle,
                        float* minmax, void* stream);
int seg3d_sector_angles_host(const float* xyz, int64_t n, const int32_t* offset, int32_t batch_size, float* angle,
                             float* minmax);
int seg3d_sector_assign(const float* angle, int64_t n, const int32_t* offset, int32_t batch_size, const float* edges,
                        const int32_t* sector_offset, int32_t* sector_id, void* stream);
int seg3d_sector_assign_host(const float* angle, int64_t n, const int32_t* offset, int32_t batch_size,
                             const float* edges, const int32_t* sector_offset, int32_t* sector_id);

/* ------------------------------------------------------------------------------------------
 * query_and_group / interpolation -- seg3d/utils/pointops_utils.py:25-44 and :47-61 (torch indexing in the reference,
 * no extension behind them).  xyz [n,3], new_xyz [m,3], feat [n,c], idx int32 [m,k] (rows of xyz / feat), dist float32
 * [m,k] (seg3d_knn_query's second result after the square root); everything float32, contiguous.  1 <= k <= 64,
 * 1 <= c <= 2^31 - 4 (a row of 3 + c floats is addressed with an int32 column; element offsets are 64-bit),
 * m * k < 0x7F000000 (seg3d_group_index's limit); anything else is SEG3D_EINVAL.  m = 0 or n = 0: OK, nothing written.
 *
 * Grouping (pair p = r * k + i):
 *     out[p, 0:3]   = xyz[idx[p]] - new_xyz[r]     one float32 subtraction per component
 *     out[p, 3:3+c] = feat[idx[p]]                 bit copy
 *   out is [m, k, 3 + c] -- what the reference's code returns (its docstring says (m, c+3, nsample) and promises a second
 *   result that is never returned).  xyz = NULL: without coordinates, out is [m, k, c] and new_xyz is not read.
 * Interpolation:
 *     rcp[r,i] = 1.0f / (dist[r,i] + 1e-8f);  norm[r] = ((rcp[r,0] + rcp[r,1]) + ...) left to right;
 *     weight[r,i] = rcp[r,i] / norm[r];  out[r,:] = ((0 + feat[idx[r,0]] * weight[r,0]) + feat[idx[r,1]] * weight[r,1]) + ...
 *   left to right, product and sum rounded separately, every operation in float32.  weight [m,k] (nullable) is written
 *   for the backward.  dist and idx carry no gradient.
 * An index outside [0, n) (-1 included; the reference would fault or wrap) is defined and never used as an address:
 *   grouping writes zeros to the whole slot of 3 + c values; interpolation leaves the slot out of the sum while its
 *   reciprocal stays in norm; neither passes a gradient through it.  The slots seg3d_knn_query fills beyond a short
 *   segment, (1e10, segment start), arrive here as an ordinary row at distance 1e5 and are treated as one, like in the
 *   reference: reciprocal 1e-5, i.e. weight 1e-5 / norm -- about 1e-5 * d beside a real neighbour at distance d, and 1 / k
 *   in a row made of nothing else.
 * Backward.  pair_order / pair_offsets = `order` / `offsets` of seg3d_group_index over the flattened, sanitised idx (m * k
 *   ids, n groups; entries outside [0, n) set to -1 first, so they are in no list), as for seg3d_knn_attention_bwd.
 *     grouping:      dfeat[j] = sum of dout[p, 3:] and dxyz[j] = sum of dout[p, 0:3] over the pairs p with idx[p] = j, both
 *                    from one launch and one read of the dout rows; dnew_xyz[r] = -(((0 + dout[r,0,0:3]) + dout[r,1,0:3])
 *                    + ...) over the slots with an inside index.  NULL = not wanted (not computed, columns not read);
 *                    with_xyz = 0: dout is [m, k, c] and dxyz / dnew_xyz must be NULL.
 *     interpolation: dfeat[j] = sum of dout[r] * weight[p] over the pairs p = r * k + i with idx[p] = j.
 *   ORDER OF SUMMATION (part of the contract): per source row j over its list in ascending pair index, starting from 0.
 *   A list longer than SEG3D_POINTOPS_CHUNK = 512 entries is cut into chunks of 512 consecutive entries; every chunk is
 *   summed on its own from 0 in ascending pair index, and the chunk sums are then added left to right in chunk order:
 *   ((chunk 0 + chunk 1) + chunk 2) + ...  A row nobody reads gets exactly 0.  No float atomics: results are
 *   bit-reproducible, and the _host twins (plain C++, no HIP call, host pointers, same order) return the same bits.
 *   scratch: seg3d_pointops_scratch_bytes(m, k, width) bytes for the chunk sums, width = floats per dout row (3 + c or c
 *   for grouping, c for interpolation); required by the device backward entries whatever the list lengths. */
#define SEG3D_POINTOPS_CHUNK 512
size_t seg3d_pointops_scratch_bytes(int64_t m, int32_t k, int32_t width);
int seg3d_group_points_fwd(const float* xyz, const float* new_xyz, const float* feat, const int32_t* idx, int64_t n,
                           int64_t m, int32_t k, int32_t c, float* out, void* stream);
int seg3d_group_points_fwd_host(const float* xyz, const float* new_xyz, const float* feat, const int32_t* idx, int64_t n,
                                int64_t m, int32_t k, int32_t c, float* out);
int seg3d_group_points_bwd(const float* dout, const int32_t* idx, const int32_t* pair_order, const int32_t* pair_offsets,
                           int64_t n, int64_t m, int32_t k, int32_t c, int32_t with_xyz, float* dxyz, float* dnew_xyz,
                           float* dfeat, void* scratch, size_t scratch_bytes, void* stream);
int seg3d_group_points_bwd_host(const float* dout, const int32_t* idx, const int32_t* pair_order,
                                const int32_t* pair_offsets, int64_t n, int64_t m, int32_t k, int32_t c,
                                int32_t with_xyz, float* dxyz, float* dnew_xyz, float* dfeat);
int seg3d_knn_interpolate_fwd(const float* feat, const int32_t* idx, const float* dist, int64_t n, int64_t m, int32_t k,
                              int32_t c, float* out, float* weight, void* stream);
int seg3d_knn_interpolate_fwd_host(const float* feat, const int32_t* idx, const float* dist, int64_t n, int64_t m,
                                   int32_t k, int32_t c, float* out, float* weight);
int seg3d_knn_interpolate_bwd(const float* dout, const float* weight, const int32_t* idx, const int32_t* pair_order,
                              const int32_t* pair_offsets, int64_t n, int64_t m, int32_t k, int32_t c, float* dfeat,
                              void* scratch, size_t scratch_bytes, void* stream);
int seg3d_knn_interpolate_bwd_host(const float* dout, const float* weight, const int32_t* idx, const int32_t* pair_order,
                                   const int32_t* pair_offsets, int64_t n, int64_t m, int32_t k, int32_t c,
                                   float* dfeat);

/* ------------------------------------------------------------------------------------------
 * One-output-channel submanifold convolution with an optional fused sigmoid gate (csrc/sa_gate.hip) -- SALayer,
 * seg3d/models/layers/sa_layer.py:8-25: SubMConv3d(planes, 1, 3, padding=1, bias=False) -> sigmoid -> x * gate; without
 * the gate, the plain C -> 1 conv that the MFMA paths (out_channels % 16 == 0) do not cover.
 *   x    float32 [M, C] contiguous          nbr  int32 [27][M], -1 = inactive, as seg3d_rulebook_subm writes it
 *   w    float32 [27, C] = weight[0] of a [1, 3, 3, 3, C] parameter viewed flat, same offset index k as the table
 *   bias DEVICE pointer (host pointer for the _host twins) to one float, or NULL
 *   C % 4 == 0, 4 <= C <= 1024, 0 <= M < 2^31 - 1; anything else is SEG3D_EINVAL.  M = 0: OK, nothing is written (the
 *   backward still writes dw = 0 and dbias = 0 when asked for them).
 *   ALIGNMENT: x, w, y_out (forward) and dy, x (seg3d_subm_dot_bwd_ds) are read and written as 16-byte vectors and must
 *   be 16-byte aligned: a pointer that is not is SEG3D_EINVAL, nothing is launched.  seg3d_subm_dot_bwd has no
 *   requirement beyond float alignment.
 *   THE TABLE MUST BE A SUBMANIFOLD TABLE: nbr[13][i] == i, and nbr[k][i] == j exactly when nbr[26 - k][j] == i.  The
 *   backward RELIES on this mirror property (it is what lets it gather scalars instead of rows) and does not check it;
 *   with any other table its gradients are not the gradients of the forward.  An entry outside [0, M) is treated as -1
 *   and never used as an address.
 * Math:  s_i = bias + sum_k [nbr[k][i] >= 0] dot(x[nbr[k][i]], w[k]);  g_i = sigmoid(s_i);  y_i = x_i g_i
 *   sigmoid(s): e = expf(-|s|), then 1 / (1 + e) for s >= 0 and e / (1 + e) for s < 0 -- expf never overflows, no NaN for
 *   any finite s; g is exactly 1 from s >= 17 on (1 + e rounds to 1) and exactly 0 from s <= -104 on (expf underflows to
 *   0; between -87.4 and -104 it is the denormal the exact sigmoid rounds to).
 * Backward, given dy:  dg_i = dot(dy_i, x_i);  ds_i = (dg_i g_i) (1 - g_i)   [seg3d_subm_dot_bwd_ds; g from s again]
 *   dx_j = dy_j g_j + sum_k [nbr[k][j] >= 0] ds[nbr[k][j]] w[26 - k]
 *   dw[k] = sum_j [nbr[26 - k][j] >= 0] ds[nbr[26 - k][j]] x_j;   dbias = sum_j ds_j
 *   -- 27 scalars of ds per row, x and dy streamed once, no second gather of feature rows.
 * seg3d_subm_dot_fwd: one launch; writes s [M]; with y_out != NULL also y [M, C] (the fused layer).
 * seg3d_subm_dot_bwd_ds: ds [M] from dy, x, s.  The plain conv has ds = dout and skips it.
 * seg3d_subm_dot_bwd: dy == NULL is the plain conv (no dy g term; s is not read).  dx, dw, dbias: NULL = not wanted, not
 *   computed (dx == NULL: dy, w not read; dw == dbias == NULL: x not read, no scratch needed).  scratch:
 *   seg3d_subm_dot_scratch_bytes(M, C) bytes for the per-block partial weight gradients, else SEG3D_EWORKSPACE.
 * ORDER OF SUMMATION (part of the contract; every product and every sum is rounded to float32 on its own, no fused
 * multiply-add; no float atomics; the _host twins -- plain C++, host pointers, no HIP call -- use the same order and
 * return the same bits wherever no expf is involved, i.e. s, and dx / dw / dbias of the plain conv):
 *   channel reduction (s and dg).  The row is cut into groups of 4 consecutive floats, group c4 = channels 4 c4 .. 4 c4 + 3.
 *     p(c4, k) = ((a0 b0 + a1 b1) + a2 b2) + a3 b3, in component order.  Per group the neighbours are summed in ascending
 *     k from 0: A(c4) = ((0 + p(c4, k1)) + p(c4, k2)) + ... over the offsets present.  With L = the power of two >= C / 4,
 *     at most 64, lane l of L sums its groups c4 = l, l + L, l + 2L, ... (< C / 4) in ascending order starting from the
 *     first, Q(l) = (A(l) + A(l + L)) + ...; a lane without a group has Q = 0.  Then the fixed tree
 *     for off = L / 2, L / 4, ..., 1: Q(l) = Q(l) + Q(l + off) for l < off;  the row's sum is Q(0), and s = Q(0) + bias (no
 *     addition without a bias).  The shape depends on C alone, not on M or on the launch.
 *   backward.  d(k, j) = ds[nbr[k][j]], and 0 where row j has no neighbour at offset k: such an offset is not skipped,
 *     its products (+-0) are added like any other (the loop has no branch).
 *   dx.  T = ((0 + d(0, j) w[26]) + d(1, j) w[25]) + ... + d(26, j) w[0], per channel; dx = dy g + T, or T alone for the
 *     plain conv.
 *   dw, dbias.  Rows are cut into blocks of SEG3D_SUBM_DOT_ROWS consecutive rows.  Per block every (k, c) is summed from
 *     0 over the block's rows j in ascending order, dw[26 - k][c] += d(k, j) x[j][c], and so is ds for dbias; the block
 *     partials are then added from 0 left to right: ((0 + block 0) + block 1) + ... */
#define SEG3D_SUBM_DOT_ROWS 128
size_t seg3d_subm_dot_scratch_bytes(int64_t M, int32_t C);
int seg3d_subm_dot_fwd(const float* x, const int32_t* nbr, const float* w, const float* bias, int64_t M, int32_t C,
                       float* s_out, float* y_out, void* stream);
int seg3d_subm_dot_fwd_host(const float* x, const int32_t* nbr, const float* w, const float* bias, int64_t M, int32_t C,
                            float* s_out, float* y_out);
int seg3d_subm_dot_bwd_ds(const float* dy, const float* x, const float* s, int64_t M, int32_t C, float* ds_out,
                          void* stream);
int seg3d_subm_dot_bwd_ds_host(const float* dy, const float* x, const float* s, int64_t M, int32_t C, float* ds_out);
int seg3d_subm_dot_bwd(const float* dy, const float* x, const float* s, const float* ds, const int32_t* nbr,
                       const float* w, int64_t M, int32_t C, float* dx, float* dw, float* dbias, void* scratch,
                       size_t scratch_bytes, void* stream);
int seg3d_subm_dot_bwd_host(const float* dy, const float* x, const float* s, const float* ds, const int32_t* nbr,
                            const float* w, int64_t M, int32_t C, float* dx, float* dw, float* dbias);

/*
 * SURVEY 8(f) rank 2  WaymoDataset.prepare_voxel_labels (seg3d/datasets/waymo_dataset.py:213-246): label of a voxel =
 * most frequent label (uint8, 0..255, the ignore label counted like any other) among its points, ties to the smallest
 * label, ignore_index for voxels without a point.  order / offsets: the point->voxel CSR of seg3d_group_index
 * (points with id -1 -- dropped or history-sweep points -- are in no segment).
 */
int seg3d_voxel_majority_labels(const uint8_t* point_labels, const int32_t* order, const int32_t* offsets,
                                int64_t n_voxels, int32_t ignore_index, uint8_t* voxel_labels, void* stream);

/*
 * SURVEY 8(f) rank 4  'ce' / 'ohem_ce' terms of build_criterion (seg3d/models/builder.py:26-40) on logits [n, c] with
 * int64 labels; rows whose label is ignore_index (or outside [0, c)) contribute nothing.
 *   keep_thresh <= 0 : nn.CrossEntropyLoss(ignore_index), mean over the counted rows
 *   keep_thresh  > 0 : OHEMCrossEntropyLoss(keep_thresh) (seg3d/models/losses/ohem_cross_entropy_loss.py:23-38): only
 *                      rows with softmax(logits)[label] < keep_thresh are counted
 * forward: lse [n] kept for backward (log-sum-exp on counted rows, +inf on the others), stats = {mean loss, count}
 * (mean = 0 when nothing is counted; torch returns NaN there); backward: dlogits = (softmax - onehot) * grad_out / count
 * on counted rows, 0 elsewhere.  Deterministic (per-block partials, fixed-order finalize).
 */
size_t seg3d_cross_entropy_workspace_bytes(int64_t n);
int seg3d_cross_entropy_fwd(const float* logits, const int64_t* labels, int64_t n, int32_t c, int64_t ignore_index,
                            float keep_thresh, float* lse, float* stats, void* workspace, size_t workspace_bytes,
                            void* stream);
int seg3d_cross_entropy_bwd(const float* logits, const int64_t* labels, const float* lse, const float* stats,
                            const float* grad_out, int64_t n, int32_t c, float* dlogits, void* stream);

/*
 * SURVEY 8(f) rank 4  Lovasz-softmax term: LovaszLoss(ignore_index) as build_criterion makes it (multi_class, per_image
 * False; seg3d/models/losses/lovasz_loss.py:13-26 lovasz_grad, :118-158 lovasz_softmax_flat, :268-290 forward) on logits
 * [n, c <= 64] with int64 labels, n * c < 2^31.  All classes go through ONE device radix sort of (class, error) keys
 * instead of c separate sorts; the jaccard differences use the reference's float32 arithmetic.
 *   classes_mode 0 = 'present' (classes without a label in the batch are skipped), 1 = 'all'; include (nullable int32
 *   [c], non-zero = averaged) is the explicit class list of the reference and overrides the presence test; class_weight
 *   nullable float [c].  Rows with label == ignore_index take no part.
 * forward : coef [n, c] (d loss_class / d prob, kept for backward), stats [2 + c] = {loss, classes averaged,
 *           d loss / d loss_class per class}
 * backward: dlogits [n, c] = softmax backward of coef * stats[2 + class] * grad_out[0]
 * seg3d_lovasz_workspace_bytes asks rocPRIM for the sort's scratch size on the current device: 0 = invalid arguments or
 * no device visible.
 */
size_t seg3d_lovasz_workspace_bytes(int64_t n, int32_t c);
int seg3d_lovasz_softmax_fwd(const float* logits, const int64_t* labels, int64_t n, int32_t c, int64_t ignore_index,
                             int32_t classes_mode, const int32_t* include, const float* class_weight, float* coef,
                             float* stats, void* workspace, size_t workspace_bytes, void* stream);
int seg3d_lovasz_softmax_bwd(const float* logits, const float* coef, const float* stats, const float* grad_out,
                             int64_t n, int32_t c, float* dlogits, void* stream);

/*
 * The whole criterion of tools/train.py:71-110 in one call: up to four heads (point, voxel, auxiliary voxel logits, each
 * [n_h, c <= 64] with int64 labels; sum n_h * c < 2^31), the 'ce' / 'ohem_ce' term and / or the 'lovasz' term as the two
 * entries above compute them ('present' classes, no class weights), and
 *   loss = sum over the heads in table order, per head ce then lovasz, of (head weight * term) * term weight
 * in float32, starting from 0: the sequence compute_loss runs.  Loss and gradients carry the bits of the per-term entries;
 * one row pass, ONE device sort of (head, class, error) keys and one finalize replace theirs.
 *   terms    SEG3D_CRITERION_CE | SEG3D_CRITERION_LOVASZ (at least one)
 *   forward  lse [sum n] and coef [sum n, c] (rows of the heads one after the other; kept for backward, lse only with the
 *            CE term, coef only with the Lovasz term), stats [n_heads][SEG3D_CRITERION_STATS_STRIDE] = per head {ce mean,
 *            ce count, lovasz loss, classes averaged, d lovasz / d loss_class [64]}, loss [1]
 *   backward dlogits[h] [n_h, c] = d loss / d logits of head h for the upstream gradient grad_out[0]: the float32 sum of the
 *            two terms' gradients, each rounded as its own backward rounds it
 * Logits must not be NaN: the per-term Lovasz entry then returns NaN, this one an undefined (possibly finite) loss; all
 * accesses stay in bounds either way.
 * seg3d_criterion_workspace_bytes: 0 = invalid arguments, or (Lovasz term) no device visible.  Invalid arguments and a
 * workspace too small for the call's own buffers are refused before anything is enqueued.
 */
#define SEG3D_CRITERION_MAX_HEADS 4
#define SEG3D_CRITERION_CE 1
#define SEG3D_CRITERION_LOVASZ 2
#define SEG3D_CRITERION_STATS_STRIDE 68
typedef struct {
    const float* logits;   /* [n, c] */
    const int64_t* labels; /* [n] */
    int64_t n;
    float weight;          /* head weight (MODEL.AUX_LOSS_WEIGHT on the auxiliary head, 1 elsewhere) */
} seg3d_criterion_head;
typedef struct {
    int32_t n_heads;
    seg3d_criterion_head heads[SEG3D_CRITERION_MAX_HEADS];
} seg3d_criterion_table;
size_t seg3d_criterion_workspace_bytes(const seg3d_criterion_table* heads, int32_t c, int32_t terms);
int seg3d_criterion_fwd(const seg3d_criterion_table* heads, int32_t c, int32_t terms, int64_t ignore_index,
                        float keep_thresh, float w_ce, float w_lovasz, float* lse, float* coef, float* stats, float* loss,
                        void* workspace, size_t workspace_bytes, void* stream);
int seg3d_criterion_bwd(const seg3d_criterion_table* heads, int32_t c, int32_t terms, float w_ce, float w_lovasz,
                        const float* lse, const float* coef, const float* stats, const float* grad_out,
                        float* const* dlogits, void* stream);

/*
 * FocalLoss (seg3d/models/losses/focal_loss.py:51-92) on logits [n, c <= 64] with int64 labels, sigmoid focal loss against
 * the one-hot label.  Valid rows: label != ignore_index; a label outside [0, c) is skipped and not counted either, as in
 * seg3d_cross_entropy_fwd (the reference's one_hot raises there -- the one deviation).  Per element of a valid row, with
 * t = [j == label]:  bce = max(x, 0) - x t + log1p(exp(-|x|)),  q = 1 - p_t (sigmoid(-x) for t = 1, sigmoid(x) for t = 0),
 *   loss = alpha_t * bce * q^gamma * class_weight[j],  alpha_t = alpha t + (1 - alpha)(1 - t), left out when alpha < 0.
 * gamma >= 0 (0, 1, 2 without powf); class_weight nullable float [c]; reduction SEG3D_REDUCE_SUM or SEG3D_REDUCE_MEAN
 * (sum / (n_valid * c); 0, not NaN, when no row is valid).  The reference's 'none' has a data-dependent shape and stays
 * with the caller.
 * forward : stats [2] = {loss, n_valid}, kept for backward.
 * backward: recomputes every term from logits (nothing [n, c] is kept); dlogits [n, c] written for every element, exactly
 *           0 on rows that are not valid.
 * Deterministic (per-workgroup partials, fixed-order finalize, no floating-point atomics).  seg3d_pointwise_loss_workspace_bytes
 * serves the focal and the dice forward.
 */
size_t seg3d_pointwise_loss_workspace_bytes(int64_t n);
int seg3d_focal_loss_fwd(const float* logits, const int64_t* labels, int64_t n, int32_t c, int64_t ignore_index, float gamma,
                         float alpha, const float* class_weight, int32_t reduction, float* stats, void* workspace,
                         size_t workspace_bytes, void* stream);
int seg3d_focal_loss_bwd(const float* logits, const int64_t* labels, const float* stats, const float* grad_out, int64_t n,
                         int32_t c, int64_t ignore_index, float gamma, float alpha, const float* class_weight,
                         int32_t reduction, float* dlogits, void* stream);

/*
 * DiceLoss (seg3d/models/losses/dice_loss.py:9-43 dice_loss / binary_dice_loss, :84-114 forward;
 * seg3d/utils/loss_utils.py:43-73 weight_reduce_loss) on logits [n, c <= 64] with int64 labels.  On [n, c] rows the
 * reference reduces to, with p = softmax(x_r), t = onehot(clamp(y_r, 0, c - 1)), v_r = [y_r != ignore_index]:
 *   loss = loss_weight / c * sum_{i != ignore_index} class_weight[i] / n * sum_r (1 - (2 p_ri t_ri v_r + smooth) /
 *                                                                                  (p_ri^exponent + t_ri^exponent + smooth))
 * The mean runs over ALL n rows and v masks the numerator only, so rows with the ignore label have a gradient (through
 * the denominator, with the clamped label's one-hot in it).  avg_factor >= 0: the scalar is divided by avg_factor +
 * FLT_EPSILON (reduction 'mean' with avg_factor, loss_utils.py:65-69); avg_factor < 0: none.  exponent 1 and 2 run
 * without powf.  class_weight nullable float [c].  n = 0 gives 0.
 * forward : loss [1].   backward: recomputes the row softmax, dlogits_rj = p_rj (g_j - sum_i g_i p_ri) with
 *           g_i = d loss / d p_ri, times grad_out[0].  Deterministic as above.
 */
int seg3d_dice_loss_fwd(const float* logits, const int64_t* labels, int64_t n, int32_t c, int64_t ignore_index, float smooth,
                        float exponent, const float* class_weight, float loss_weight, float avg_factor, float* loss,
                        void* workspace, size_t workspace_bytes, void* stream);
int seg3d_dice_loss_bwd(const float* logits, const int64_t* labels, const float* grad_out, int64_t n, int32_t c,
                        int64_t ignore_index, float smooth, float exponent, const float* class_weight, float loss_weight,
                        float avg_factor, float* dlogits, void* stream);

/*
 * The options of the cross-entropy family that need more than a per-row pass: nn.CrossEntropyLoss(weight=, ignore_index=)
 * and OHEMCrossEntropyLoss(keep_ratio=, keep_thresh=, class_weight=) (seg3d/models/losses/ohem_cross_entropy_loss.py:23-38)
 * on logits [n <= INT32_MAX, c <= 4096] with int64 labels.  Valid rows: label != ignore_index and in [0, c).  Per valid row
 *   l = w[label] * (lse - x[label]),  w = 1 when class_weight (float [c]) is NULL.
 *   SEG3D_CE_SELECT_MEAN_WEIGHTED  sum l / sum w[label]                                   (nn.CrossEntropyLoss(weight=w))
 *   SEG3D_CE_SELECT_MEAN_ALL       sum l / n_valid                                        (the OHEM module, no selector)
 *   SEG3D_CE_SELECT_THRESH         plain mean of l over the valid rows with softmax(x)[label] < keep_thresh (> 0)
 *   SEG3D_CE_SELECT_RATIO          plain mean of the kept largest l, kept = (int64)((double)n_valid * keep_ratio) clamped
 *                                  to n_valid (Python's int(n_valid * keep_ratio), hence the double; keep_ratio > 0)
 * RATIO is an exact selection on the device (a radix select over an order-preserving integer key of l, no sort, no host
 * read-back): descending by l, NaN above +inf, -0 = +0; among rows equal to the kept-th value the lowest row indices
 * are taken, the order of torch.sort(descending=True, stable=True).  A row's l does not depend on its position.
 * forward : lse [n] (log-sum-exp on counted rows, +inf on all others), stats [2] = {loss, denominator} (sum of weights,
 *           count, or kept); a denominator of 0 (n = 0, kept = 0, nothing below the threshold, a zero weight sum) gives
 *           loss 0 where torch gives NaN.  Invalid arguments are refused before anything is enqueued.
 * backward: dlogits = w[label] * (softmax - onehot) * grad_out[0] / denominator on counted rows, exactly 0 elsewhere and
 *           everywhere when the denominator is 0.
 * Bit-reproducible: integer atomics only (histogram counts), float64 partial sums folded in a fixed order.
 */
#define SEG3D_CE_SELECT_MEAN_WEIGHTED 0
#define SEG3D_CE_SELECT_MEAN_ALL 1
#define SEG3D_CE_SELECT_THRESH 2
#define SEG3D_CE_SELECT_RATIO 3
size_t seg3d_ce_select_workspace_bytes(int64_t n);
int seg3d_ce_select_fwd(const float* logits, const int64_t* labels, int64_t n, int32_t c, int64_t ignore_index,
                        const float* class_weight, int32_t mode, float keep_thresh, double keep_ratio, float* lse,
                        float* stats, void* workspace, size_t workspace_bytes, void* stream);
int seg3d_ce_select_bwd(const float* logits, const int64_t* labels, const float* class_weight, const float* lse,
                        const float* stats, const float* grad_out, int64_t n, int32_t c, int32_t mode, float* dlogits,
                        void* stream);

/* ------------------------------------------------------------------------------------------
 * Evaluation path (csrc/eval.hip): tools/eval.py:35-64 with --tta, test_time_aug.py:15-35 (MultiScaleFlipAug),
 * seg3d/core/evaluation/iou_metric.py:21-53 (IOUMetric.fast_hist / add).  None of the three allocates.
 *
 * seg3d_tta_views_f32: the views of ONE frame (points [n, dim] float32, no batch column, 3 <= dim <= 16) written as
 * collated rows out [n_views * n, 1 + dim], views in table order: column 0 = view index (v % batch_period when
 * batch_period > 0, so that a slice of K consecutive views is a batch 0..K-1 when batch_period = K), then per point, in
 * float32 without fused multiply-add, the reference's recipe (test_time_aug.py:26-31, transform_utils.py:11-32):
 *   xyz *= scale;  x' = x*cos + y*(-sin);  y' = x*sin + y*cos;  z unchanged;  flip_x: y' = -y';  flip_y: x' = -x'
 * and the other columns copied.  cos / sin are the caller's float32 constants (the reference takes torch.cos / torch.sin
 * of the float32 angle).  `table` is a HOST pointer; the kernel receives the table by value among its arguments.
 * n_views in [1, 64], flips 0 / 1, n_views * n <= INT32_MAX: SEG3D_EINVAL otherwise.
 * seg3d_tta_views_host_f32: the same contract on HOST pointers, plain C++ (no HIP call, runs without a GPU context, as
 * seg3d_voxelize_host_f32 does); bit-identical to the device kernel.
 */
#define SEG3D_TTA_MAX_VIEWS 64
typedef struct {
  float scale, cos_a, sin_a;
  int32_t flip_x, flip_y; /* 0 / 1 */
} seg3d_tta_view;
typedef struct {
  int32_t n_views;
  int32_t batch_period; /* 0 = column 0 holds the view index itself */
  seg3d_tta_view views[SEG3D_TTA_MAX_VIEWS];
} seg3d_tta_table;
int seg3d_tta_views_f32(const float* points, int64_t n_points, int32_t dim, const seg3d_tta_table* table, float* out,
                        void* stream);
int seg3d_tta_views_host_f32(const float* points, int64_t n_points, int32_t dim, const seg3d_tta_table* table,
                             float* out);

/* seg3d_softmax_accumulate_f32: logits [n_views * n_points, c] of one forward over n_views consecutive views (view-major,
 * as seg3d_tta_views_f32 lays them out), acc [n_points, c] float32.  Per point, view by view in order:
 *   m = max_c l;  e_c = expf(l_c - m);  s = sum_c e_c (fixed c order);  p_c = e_c / s (correctly rounded);
 *   acc_c = acc_c + p_c  (first = 1: the first view of this call overwrites acc instead)
 * -- F.softmax(point_out, dim=1) per view (eval.py:49) and the running sum behind torch.stack + torch.mean (:51-52).
 * One rounded add per view in view order: for the same logits the result is bit-identical however the views are split
 * into calls.  n_views in [1, 64], 1 <= c <= 64, n_views * n_points <= INT32_MAX.
 */
int seg3d_softmax_accumulate_f32(const float* logits, int64_t n_points, int32_t n_views, int32_t c, int32_t first,
                                 float* acc, void* stream);

/* seg3d_argmax_confusion: eval.py:55-58 (torch.argmax of point_out or of the mean probabilities) + IOUMetric.add
 * (iou_metric.py:21-37, 50-56) on the device.  Predictions come from exactly one of
 *   scores  [n, c] float32: pred = argmax_c score; with n_views > 0 the argmax is taken of score / n_views (the
 *           correctly rounded quotient torch.mean forms, not a product with 1/n_views: two distinct sums may tie);
 *           ties: the first maximum wins; NaN counts as the maximum and the first NaN wins (torch.argmax's rule)
 *   pred_in [n] int64: predictions already made ("labels in, hist out"; pred and n_views must then be 0 / NULL)
 * pred  nullable out [n] int64;
 * hist  nullable in/out int64 [c * c], hist[gt * c + pred] += 1, ACCUMULATED (never cleared here); needs labels:
 *       labels [n] uint8 (label_bytes 1, as the loader delivers them) or int64 (label_bytes 8, after load_data_to_gpu);
 *       labels outside [0, c) -- the ignore index 255 among them -- are skipped (iou_metric.py:33), as are predictions
 *       outside [0, c).  Per-workgroup LDS histogram of 32-bit counters, one 64-bit atomic per non-zero bin: integer-
 *       exact and independent of the order of the points.
 * 1 <= c <= 64 (SEG3D_EINVAL above), at least one of pred / hist.
 */
#define SEG3D_ARGMAX_MAX_CLASSES 64
int seg3d_argmax_confusion(const float* scores, const int64_t* pred_in, int64_t n_points, int32_t c, int32_t n_views,
                           const void* labels, int32_t label_bytes, int64_t* pred, int64_t* hist, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training augmentation (csrc/augment.hip): what the reference does once per training frame between the disk and the
 * voxelizer -- PolarMix (seg3d/datasets/transforms/polarmix.py:4-111, called at seg3d/datasets/waymo_dataset.py:307-323)
 * and the composed transforms (transforms.py:79-258, transform_utils.py:11-138, composed at waymo_dataset.py:44-50).
 * Every stage selects / reorders rows or maps x, y, z of a row, so the stages build an int32 SOURCE MAP and one kernel
 * touches the rows.  A source row s addresses the concatenation [frame1; frame2] (s < n1: frame1[s], else
 * frame2[s - n1]); the frames are never concatenated in memory.  Device entries neither allocate nor synchronise; every
 * *_host twin takes HOST pointers, is plain C++ without a HIP call (runs in a DataLoader worker or on a machine without
 * a GPU) and gives the same bits / the same integers as its device entry.
 */
#define SEG3D_AUG_MAX_PASTE 8
typedef struct {
  double paste_cos[SEG3D_AUG_MAX_PASTE]; /* np.cos / np.sin of PolarMix's rot_angle_range (polarmix.py:48-51) */
  double paste_sin[SEG3D_AUG_MAX_PASTE];
  double offset[3];       /* RandomGlobalTranslation's three float64 draws (transform_utils.py:68-94) */
  float rot_cos, rot_sin; /* torch.cos / torch.sin of the float32 angle (transform_utils.py:21-22) */
  float scale;            /* float32(noise_scale) (transforms.py:86-87); 1 when the transform is skipped (:84-85) */
  int32_t n_paste;        /* angles in use, 0 .. 8 */
  int32_t flip_x, flip_y; /* 0 / 1: random_flip_along_x / _y */
  int32_t global_on;      /* 0: stop after the float32 rounding (PolarMix alone); 1: the whole chain */
  int32_t batch_col;      /* 1: out rows are [batch_id, row] (WaymoDataset.collate_batch, waymo_dataset.py:347-352) */
  float batch_id;
} seg3d_aug_params;

/* seg3d_aug_polarmix_map -- PolarMix.__call__ (polarmix.py:72-111) as a row map.  points1 [n1, dim], points2 [n2, dim]
 * float32 (point_bytes 4) or float64 (8), 3 <= dim <= 16; labels2 [n2] uint8 (label_bytes 1) or int64 (8).
 * Rows, in the reference's order:
 *   frame-1 rows NOT in the sector, then frame-2 rows in the sector (swap, :4-25; with swap = 0 all of frame 1 and
 *   nothing of frame 2), both in original order; sector test yaw = -atan2(y, x) in double, yaw > alpha && yaw < beta;
 *   then the instance block of frame 2 -- class-major in the order of instance_classes (host uint8[n_classes], no class
 *   twice), ascending row inside a class (:31-41) -- written 1 + n_paste times: op 0, then op 1 .. n_paste (:44-58).
 * src [cap] int32 / op [cap] uint8 (0 = copy, r = rotate by paste angle r); cap >= n1 + n2 * (2 + n_paste).
 * counts: int32[4] = {n_out, rows before the instance block, rows of one instance block, 0} (device memory for the
 * device entry: the caller reads it once, as it reads the voxel count of seg3d_voxelize_f32).  flags -> scan -> emit;
 * the class-major order from a per-block class histogram, a scan and a stable in-block rank: no sort, no float atomics. */
size_t seg3d_aug_polarmix_workspace_bytes(int64_t n1, int64_t n2);
int seg3d_aug_polarmix_map(const void* points1, int64_t n1, const void* points2, int64_t n2, int32_t dim,
                           int32_t point_bytes, const void* labels2, int32_t label_bytes, int32_t swap, double alpha,
                           double beta, const uint8_t* instance_classes, int32_t n_classes, int32_t n_paste, int64_t cap,
                           int32_t* src, uint8_t* op, int32_t* counts, void* workspace, size_t workspace_bytes,
                           void* stream);
int seg3d_aug_polarmix_map_host(const void* points1, int64_t n1, const void* points2, int64_t n2, int32_t dim,
                                int32_t point_bytes, const void* labels2, int32_t label_bytes, int32_t swap, double alpha,
                                double beta, const uint8_t* instance_classes, int32_t n_classes, int32_t n_paste,
                                int64_t cap, int32_t* src, uint8_t* op, int32_t* counts);

/* seg3d_aug_far_near -- the far / near lists points_random_sampling draws from (transform_utils.py:120-134).  Row i of
 * the transformed, shuffled frame is source row src[idx[i]] with op[idx[i]] (idx NULL: i itself; src NULL: the identity
 * map over n_map <= n1 + n2 rows; op NULL: copies); its x, y go through the recipe of seg3d_aug_apply_f32 and
 * dist = sqrt(x*x + y*y) in float32 (two rounded products, a rounded sum, IEEE sqrt: np.linalg.norm, :122) is tested
 * dist >= sample_range.  far_flag [n] uint8 (nullable); far_idx / near_idx [n] int32 (both or neither): the rows i with
 * and without the flag, ascending, counts int32[2] = {n_far, n_near}.  The workspace is needed for the lists only. */
size_t seg3d_aug_far_near_workspace_bytes(int64_t n);
int seg3d_aug_far_near(const void* frame1, int64_t n1, const void* frame2, int64_t n2, int32_t dim, int32_t point_bytes,
                       const int32_t* src, const uint8_t* op, int64_t n_map, const int32_t* idx, int64_t n,
                       const seg3d_aug_params* params /* host */, float sample_range, uint8_t* far_flag, int32_t* far_idx,
                       int32_t* near_idx, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream);
int seg3d_aug_far_near_host(const void* frame1, int64_t n1, const void* frame2, int64_t n2, int32_t dim, int32_t point_bytes,
                            const int32_t* src, const uint8_t* op, int64_t n_map, const int32_t* idx, int64_t n,
                            const seg3d_aug_params* params, float sample_range, uint8_t* far_flag, int32_t* far_idx,
                            int32_t* near_idx, int32_t* counts);

/* seg3d_aug_sample_device -- PointShuffle + PointSample (transforms.py:141-146, :211-217, transform_utils.py:117-134)
 * without host random numbers: out [n_samples] = distinct rows of [0, n), far rows (far_flag != 0; NULL = none) kept
 * before near rows, a uniform subset of the set that does not fit, in uniform order -- the reference's distribution,
 * not its draws.  Keys are a counter-based hash of (seed, stream, row) with the row in the low 32 bits (unique keys):
 * one radix sort on (near bit, hash) selects, one on a fresh hash orders.  A pure function of (seed, n, far_flag);
 * the host twin sorts the same keys. */
size_t seg3d_aug_sample_workspace_bytes(int64_t n);
int seg3d_aug_sample_device(const uint8_t* far_flag, int64_t n, int64_t n_samples, uint64_t seed, int32_t* out,
                            void* workspace, size_t workspace_bytes, void* stream);
int seg3d_aug_sample_host(const uint8_t* far_flag, int64_t n, int64_t n_samples, uint64_t seed, int32_t* out);

/* seg3d_aug_cur_map -- PointShuffle / PointSample.get_shuffled_indices (transforms.py:165-177, :237-249), both dict
 * loops at once: src [m] = source point of every output row, cur_point_indices [n_cur] = the points of the current
 * sweep among n_points (a point listed twice keeps its later slot, as the dict does).  cur_pos [<= m] = the output rows
 * whose source is a current-sweep point, ascending (the new cur_point_indices); cur_gather = that point's slot (the
 * gather list for labels and image features, which are sized to the current sweep, :152-161, :224-233);
 * count int32[1]. */
size_t seg3d_aug_cur_map_workspace_bytes(int64_t m, int64_t n_points);
int seg3d_aug_cur_map(const int32_t* src, int64_t m, const int32_t* cur_point_indices, int64_t n_cur, int64_t n_points,
                      int32_t* cur_pos, int32_t* cur_gather, int32_t* count, void* workspace, size_t workspace_bytes,
                      void* stream);
int seg3d_aug_cur_map_host(const int32_t* src, int64_t m, const int32_t* cur_point_indices, int64_t n_cur, int64_t n_points,
                           int32_t* cur_pos, int32_t* cur_gather, int32_t* count);

/* seg3d_aug_apply_f32 / _f64in -- the rows themselves, each source row read once and each output row written once:
 * out [n_out, dim] float32 (or [n_out, 1 + dim] with params->batch_col).  Per output row g, source src[g] (NULL: g),
 * op[g] (NULL: 0), without fused multiply-add:
 *   1. op = r > 0: x' = x*cos_r + y*(-sin_r), y' = x*sin_r + y*cos_r in DOUBLE (np.dot, polarmix.py:48-53)
 *   2. x, y, z and the other columns rounded to float32 (the .float() of transform_utils.py:7)
 *   3. x' = x*c + y*(-s), y' = x*s + y*c in float32 (points @ [[c, s, 0], [-s, c, 0], [0, 0, 1]], :25-30)
 *   4. xyz *= scale (transforms.py:87)
 *   5. x = float32(double(x) + offset[0]), likewise y, z (numpy adds the float64 draw in double, :69, :81, :93)
 *   6. flip_x: y = -y, then flip_y: x = -x (:35-58)
 * (3-6 only with params->global_on).  A source outside [0, n1 + n2) reads as a row of zeros.  `params` is a HOST
 * pointer; the kernel receives it by value.  dim outside [3, 16]: SEG3D_EINVAL. */
int seg3d_aug_apply_f32(const float* frame1, int64_t n1, const float* frame2, int64_t n2, int32_t dim, const int32_t* src,
                        const uint8_t* op, int64_t n_out, const seg3d_aug_params* params, float* out, void* stream);
int seg3d_aug_apply_f64in(const double* frame1, int64_t n1, const double* frame2, int64_t n2, int32_t dim,
                          const int32_t* src, const uint8_t* op, int64_t n_out, const seg3d_aug_params* params, float* out,
                          void* stream);
int seg3d_aug_apply_host_f32(const float* frame1, int64_t n1, const float* frame2, int64_t n2, int32_t dim,
                             const int32_t* src, const uint8_t* op, int64_t n_out, const seg3d_aug_params* params,
                             float* out);
int seg3d_aug_apply_host_f64in(const double* frame1, int64_t n1, const double* frame2, int64_t n2, int32_t dim,
                               const int32_t* src, const uint8_t* op, int64_t n_out, const seg3d_aug_params* params,
                               float* out);

/* seg3d_aug_gather -- labels, image features and composed maps through a map (polarmix.py:17-22, :33-36;
 * transforms.py:157-161, :229-233): out row g = row idx[g] of the concatenation [a (na rows); b (nb rows)] of rows of
 * row_bytes bytes (1 for uint8 labels, 8 for int64, 4 * F for features, 4 for an int32 map: src2 = src[perm][choices]),
 * zeros for an index outside it.  16-byte accesses when pointers and row_bytes allow. */
int seg3d_aug_gather(const void* a, int64_t na, const void* b, int64_t nb, int64_t row_bytes, const int32_t* idx, int64_t m,
                     void* out, void* stream);
int seg3d_aug_gather_host(const void* a, int64_t na, const void* b, int64_t nb, int64_t row_bytes, const int32_t* idx,
                          int64_t m, void* out);

/* ------------------------------------------------------------------------------------------
 * Instance copy-paste augmentation (csrc/augment_instance.hip): InstanceAugmentation.__call__
 * (seg3d/datasets/transforms/instance_augmentation.py:25-107, called at waymo_dataset.py:314-315, :321) without its
 * random draws, which are independent of the data and arrive in the plans.
 *
 * seg3d_aug_instance_plan -- one instance to paste, a HOST struct (the kernels receive it by value):
 *   row_begin, n_rows   its rows in the packed bank (`cluster_points`, :47-48); n_rows >= 1
 *   label               the label its rows get (:97), 0 .. 255
 *   height              `cluster_height` (:49)
 *   local_on            1: local_transform (:57-58, :166-177) with loc_noise (normal(scale=0.25), :169) and
 *                       rot_cos / rot_sin = np.cos / np.sin of rot_noise (uniform(-pi/20, pi/20), :171)
 *   flip                1: flip_type == 3 was drawn (:66-69), the flip over the short axis through the PRE-transform
 *                       centre (:63-64, :121-127); every other flip_type does nothing in the reference
 *   n_angles            candidate rotations (:77), 0 .. SEG3D_AUG_MAX_ANGLES, in draw order, with
 *   ang_cos / ang_sin   np.cos / np.sin of each
 */
#define SEG3D_AUG_MAX_ANGLES 20
typedef struct {
  int64_t row_begin;
  int32_t n_rows;
  int32_t label;
  double height;
  double loc_noise[3];
  double rot_cos, rot_sin;
  int32_t local_on;
  int32_t flip;
  int32_t n_angles;
  int32_t reserved;
  double ang_cos[SEG3D_AUG_MAX_ANGLES];
  double ang_sin[SEG3D_AUG_MAX_ANGLES];
} seg3d_aug_instance_plan;

/* seg3d_aug_instance_paste -- the k planned instances, one after the other; instance i is checked against the frame
 * plus the rows instances 0 .. i-1 pasted (:35-45 are re-run per instance in the reference).
 * In:  points [n, dim] float32 (point_bytes 4) or float64 (8), converted exactly to double, 3 <= dim <= 16 (outside:
 *      SEG3D_EINVAL); labels [n] uint8 (label_bytes 1) or int64 (8); ground_ids host uint8 [n_ground]: rows with label
 *      255 are skipped, rows with a ground label are ground points, all other rows -- pasted ones included -- are
 *      object points (:38-43); bank double [bank_rows, dim], device memory for the device entry: xyz and the feature
 *      columns as they are pasted (the caller applies :52-53 once when it packs the bank); plans host [k].
 * Per instance, all in double and without fused multiply-add (IEEE add / mul / div / sqrt / compare only):
 *   center0 = mean(xyz) (:56); xyz = rotate_origin(xyz - center0) + loc_noise + center0 (local_on); flip about center0;
 *   center = mean(xyz), radius = max ||xyz - center|| (:73-74).  Both means in one fixed order: partial sum t adds rows
 *   t, t + 256, ..., then the 256 partial sums fold by halving.  Per candidate r, in order: c = rotate_origin(center, r)
 *   (x' = x cos + y sin, y' = -x sin + y cos, :157-164), d = sqrt((dx*dx + dy*dy) + dz*dz) to every row;
 *   no_occlusion = no object row with d <= radius (:138); on_ground = the smallest ground d < 1.2 * radius (:145).  The
 *   first candidate with both wins (:78-84); ground_z = z of the ground row with the smallest d, LOWEST ROW on equal d
 *   (np.argmin, :149); z += (ground_z + height) - center_z (:150-152); then rotate_origin by r (:87).  No candidate
 *   wins: nothing is appended (:86).  No ground row: nothing can be placed (the reference raises at :45); no object
 *   row: no_occlusion holds.
 * Out: add_points double [cap_add, dim] / add_labels [cap_add] in the labels' own width: the accepted instances' rows
 *      [xyz, bank columns 3 ..] in processing order (:95-98); cap_add >= the sum of the plans' n_rows, otherwise
 *      SEG3D_EINVAL.  decisions int32 [k]: the accepted candidate index or -1.  counts int32 [4] = {rows added,
 *      instances placed, 0, 0}; device memory for the device entry, which the caller reads once (counts[0] is also the
 *      running row count the kernels read: the host cannot know whether instance i-1 was accepted).  The frame's own
 *      rows are not copied: the result frame is [points; add_points[:counts[0]]].
 * Device: 2 k + 1 launches -- step(0) scan(0) step(1) ... scan(k-1) step(k); scan(i): one pass over the rows for all
 * candidates of instance i at once (per candidate an occluded bit and the minimum (d, row), wave64 shuffles -> LDS ->
 * one record per workgroup; the candidate centres are read from the workspace, where step(i) left them, through
 * uniform loads); step(i): one workgroup that folds the records, decides and appends instance i-1 and prepares
 * instance i.  No allocation, no host synchronisation, no float atomics; (d, row) minima and ORs are exact, so the
 * result does not depend on the launch geometry.  The *_host twin takes host pointers, makes no HIP call and returns
 * the same bits and the same integers.  workspace_bytes: sized by max_instance_rows = the largest n_rows of the plans
 * (n and k are accepted for the caller's convenience and do not change the size: the grid, hence the record list, is
 * capped, and instance i reuses the buffers of instance i-2). */
size_t seg3d_aug_instance_workspace_bytes(int64_t n, int64_t max_instance_rows, int32_t k);
int seg3d_aug_instance_paste(const void* points, int64_t n, int32_t dim, int32_t point_bytes, const void* labels,
                             int32_t label_bytes, const uint8_t* ground_ids, int32_t n_ground, const double* bank,
                             int64_t bank_rows, const seg3d_aug_instance_plan* plans, int32_t k, int64_t cap_add,
                             double* add_points, void* add_labels, int32_t* decisions, int32_t* counts, void* workspace,
                             size_t workspace_bytes, void* stream);
int seg3d_aug_instance_paste_host(const void* points, int64_t n, int32_t dim, int32_t point_bytes, const void* labels,
                                  int32_t label_bytes, const uint8_t* ground_ids, int32_t n_ground, const double* bank,
                                  int64_t bank_rows, const seg3d_aug_instance_plan* plans, int32_t k, int64_t cap_add,
                                  double* add_points, void* add_labels, int32_t* decisions, int32_t* counts);

/* ------------------------------------------------------------------------------------------
 * Instance bank extraction (csrc/instance_extract.hip): the per-frame body of tools/extract_instances.py:46-76 -- DBSCAN
 * over the xy of each target label's rows, then centre, radius and height above the nearest ground row per cluster --
 * for ALL target labels of a frame in one call.
 *
 * In:  points [n, dim] float32 (point_bytes 4) or float64 (8), converted exactly to double, 3 <= dim <= 16; labels [n]
 *      uint8 (label_bytes 1) or int64 (8), after load_label (:19-23); target_ids host uint8 [k] (distinct) with
 *      min_points host int32 [k] >= 1 (TARGET_LABEL_ID / TARGET_MIN_POINT_NUM, :10-11), 1 <= k <= 8; ground_ids host
 *      uint8 [g], 1 <= g <= 8 (:37); eps > 0 (:56); cap_clusters >= 0; n <= INT32_MAX - 1.  Outside: SEG3D_EINVAL.
 * DBSCAN, as sklearn's result on `DBSCAN(eps, min_samples).fit(target_points[:, :2])` is defined (not its code): rows i, j
 *      of one target label are neighbours iff (dx*dx + dy*dy) <= eps*eps in double without fused multiply-add, a row
 *      being its own neighbour; a row with >= min_points neighbours is core; a cluster is a connected component of core
 *      rows, clusters of a label numbered by ascending lowest core row; a non-core row with a core neighbour joins the
 *      LOWEST-NUMBERED cluster among its core neighbours, any other non-core row is noise.  Rows of different labels
 *      never neighbour each other.  Global cluster ids: by position of the label in target_ids, then that order.
 * Out: point_cluster int32 [n]: the row's global cluster id, -1 for noise and non-target rows (true ids even beyond
 *      cap_clusters).  cluster_rows int32 [n]: the clustered rows grouped by cluster, ascending row inside a cluster
 *      (the row order of `target_points[cluster_ids == c]`, :65), -1 behind the counts[2] used entries.
 *      clusters [cap_clusters]: per cluster label, begin / rows into cluster_rows, center = mean xyz (:66; partial sum
 *      t adds the cluster's rows t, t + 256, ..., the 256 partial sums fold by halving, then one division), radius =
 *      max sqrt((dx*dx + dy*dy) + dz*dz) to the centre (:26-33, :67), kept = 1 iff a ground row has that distance d to
 *      the centre < 1.2 * radius (:70, strict), height = center z - z of the ground row with the smallest (d, row) (:74-75,
 *      np.argmin's tie rule), 0 when not kept.  A frame without ground rows keeps nothing (the reference raises, :50).
 *      counts int32 [4] = {clusters found, clusters kept among the first cap_clusters, clustered rows, target rows}.
 *      More clusters than cap_clusters: the first cap_clusters entries are complete, counts[0] is the true number and
 *      nothing is written behind clusters[cap_clusters - 1].
 * Device: rows are binned on a grid of side eps (one 64-bit key label | floor cell x | floor cell y per row, rocPRIM
 *      radix sort; the 3 x 3 neighbouring cells of a row are three contiguous key ranges found by bisection), the core
 *      count, a lock-free union-find over the core rows that always hooks the larger root under the smaller (integer
 *      compare-and-swap only; every find walks strictly downward, so all loops terminate and the root of a component
 *      is its lowest core row), the border rule, a second stable sort by (label position, root row) that yields
 *      cluster_rows and the numbering, one workgroup per cluster for centre and radius, and one sweep over the frame
 *      for the nearest ground row of eight clusters at a time (wave64 shuffles -> LDS -> one record per workgroup -> a
 *      fold).  No allocation, no host synchronisation, no float atomics; every reduction is an integer, an exact
 *      lexicographic minimum or a fixed-order sum, so the result does not depend on the launch geometry or the
 *      schedule.  counts and every output are device memory; the *_host twin takes host pointers, makes no HIP call
 *      and returns the same integers and the same double bits.
 */
typedef struct {
  int32_t label; /* the target label id */
  int32_t begin; /* first entry in cluster_rows */
  int32_t rows;
  int32_t kept; /* 0 / 1 */
  double center[3];
  double radius;
  double height;
} seg3d_instance_cluster;
size_t seg3d_instance_extract_workspace_bytes(int64_t n, int32_t cap_clusters);
int seg3d_instance_extract(const void* points, int64_t n, int32_t dim, int32_t point_bytes, const void* labels,
                           int32_t label_bytes, const uint8_t* target_ids, const int32_t* min_points, int32_t k,
                           const uint8_t* ground_ids, int32_t g, double eps, int32_t cap_clusters, int32_t* point_cluster,
                           int32_t* cluster_rows, seg3d_instance_cluster* clusters, int32_t* counts, void* workspace,
                           size_t workspace_bytes, void* stream);
int seg3d_instance_extract_host(const void* points, int64_t n, int32_t dim, int32_t point_bytes, const void* labels,
                                int32_t label_bytes, const uint8_t* target_ids, const int32_t* min_points, int32_t k,
                                const uint8_t* ground_ids, int32_t g, double eps, int32_t cap_clusters,
                                int32_t* point_cluster, int32_t* cluster_rows, seg3d_instance_cluster* clusters,
                                int32_t* counts);

/* ------------------------------------------------------------------------------------------
 * Frame assembly (csrc/frame.hip): what WaymoDataset does on the host between np.load and the voxelizer, and what the
 * test path does after the head.
 *
 * seg3d_frame_assemble -- load_points (seg3d/datasets/waymo_dataset.py:145-154) and load_points_from_sweeps (:156-202)
 * for ALL sweeps of one frame in one launch.  `table` is a HOST pointer; the kernel receives it by value.  Sweep s holds
 * n_rows raw rows of `stride` elements (stride >= dim: a raw [N, 15] file or its [:, :dim] copy) of float32
 * (point_bytes 4) or float64 (8), a row-major 3 x 4 double matrix [R | t], a double time lag and a transform flag.
 * Output rows [sum_{<s} n, sum_{<=s} n) belong to sweep s, in order; a sweep of 0 rows is legal.  Per row, T the rows'
 * dtype, in the reference's order:
 *   col 3 = T(lag)                      (:151, :160 zero the range column, :198 stores ts - sweep_ts; current sweep: 0)
 *   col 4 = tanh(col 4) evaluated in T  (:153)
 *   transform = 1:  x' = T((double(x) * m00 + double(y) * m01) + double(z) * m02);  x' = T(double(x') + m03);  likewise
 *                   y, z with rows 1, 2 of the matrix (:196-197: numpy stores the product, then adds)
 *   transform = 0:  x, y, z copied bit for bit (the reference never multiplies the current sweep by an identity)
 *   cols 5 .. dim-1 copied.
 * Outputs, any subset (NULL = not wanted): out_rows [sum n, dim] in T; out_f32 [sum n, dim] = float(value), round to
 * nearest (load_data_to_gpu's .float(), data_utils.py:6-15); out_collated [sum n, 1 + dim] float32 with batch_id in
 * column 0 (collate_batch, waymo_dataset.py:347-352).  1 <= n_sweeps <= 8, 5 <= dim <= 16, sum n <= INT32_MAX:
 * SEG3D_EINVAL otherwise.  inv(T_cur) @ T_sweep (:193) stays with the caller.
 * seg3d_frame_assemble_host: the same contract on HOST pointers, plain C++ without a HIP call; every column but col 4
 * (two tanh libraries) is bit-identical to the device entry.
 */
#define SEG3D_FRAME_MAX_SWEEPS 8
typedef struct {
  const void* rows;
  int64_t n_rows;
  int64_t stride;    /* elements between two rows */
  double matrix[12]; /* row-major [R | t], 3 x 4 */
  double lag;
  int32_t transform; /* 0 / 1 */
  int32_t reserved;
} seg3d_sweep;
typedef struct {
  int32_t n_sweeps;
  int32_t reserved;
  seg3d_sweep sweeps[SEG3D_FRAME_MAX_SWEEPS];
} seg3d_sweep_table;
int seg3d_frame_assemble(const seg3d_sweep_table* table, int32_t dim, int32_t point_bytes, void* out_rows,
                         float* out_f32, float* out_collated, float batch_id, void* stream);
int seg3d_frame_assemble_host(const seg3d_sweep_table* table, int32_t dim, int32_t point_bytes, void* out_rows,
                              float* out_f32, float* out_collated, float batch_id);

/* seg3d_range_image_labels -- construct_seg_frame's loop (seg3d/utils/submission.py:27-41).  pred [n] uint8
 * (pred_bytes 1) or int64 (8); points_ri int32 [n, 3] as (col, row, return index); image1 / image2 int32
 * [rows, cols, 2], both written in full: channel 0 = 0; channel 1 of image1 at [row, col] = pred + 1 for return index 0,
 * of image2 for return index 1, 0 where no point lands.  Any other return index is skipped (the parser writes -1 for
 * the side lidars).  Several points on one pixel: the HIGHEST point index wins (the reference's loop lets the last
 * point win) -- an integer atomic max of (index + 1) << 8 | (pred + 1), then an unpack pass; independent of the launch
 * geometry.  A point with return index 0 / 1 whose row / col is outside the image, or whose pred is outside
 * [0, n_classes), is not written and counted in n_outside (int32 [1], device memory for the device entry; the reference
 * raises IndexError there).  1 <= n_classes <= 254 so that pred + 1 fits the packing.  workspace: 16 B per pixel.
 * The *_host twin: host pointers, no HIP call, the same integers.
 */
size_t seg3d_range_image_workspace_bytes(int32_t rows, int32_t cols);
int seg3d_range_image_labels(const void* pred, int32_t pred_bytes, const int32_t* points_ri, int64_t n, int32_t rows,
                             int32_t cols, int32_t n_classes, int32_t* image1, int32_t* image2, int32_t* n_outside,
                             void* workspace, size_t workspace_bytes, void* stream);
int seg3d_range_image_labels_host(const void* pred, int32_t pred_bytes, const int32_t* points_ri, int64_t n, int32_t rows,
                                  int32_t cols, int32_t n_classes, int32_t* image1, int32_t* image2, int32_t* n_outside);

/* ------------------------------------------------------------------------------------------------------------------
 * Per-point image features (csrc/image_features.hip): the producer of `point_image_features`, the input of
 * DeepFusionBlock.
 *
 * seg3d_point_image_features -- the lookup loop of tools/extract_image_feature.py:84-100.  `table` is a HOST pointer;
 * the kernel receives it by value.  Map m is camera m's feature map: `channels` values per pixel of float32
 * (elem_bytes 4) or float16 (2), element (c, y, x) at data[c * channel_stride + y * row_stride + x * col_stride] --
 * strides in ELEMENTS, so a (C, H, W) array as the image model returns it, an HWC array and a non-contiguous view are
 * all read in place.  data NULL = the camera is absent (:19-21, the image could not be read).
 * rows: the raw lidar file, [n, stride] of float32 (point_bytes 4) or float64 (8); columns cp_col .. cp_col + 5 hold
 * (camera name, x, y, camera name, x, y), cp_col = 6 in the parser's layout (:90-97).  A value v becomes an integer as
 * Python's int(v): truncation toward zero (7.9 -> 7; -0.5 -> 0, a valid coordinate).  Per row:
 *   take the first projection if name - 1 is in [0, n_maps) and that map is present (:90-93), otherwise the second
 *   under the same test (:94-97), otherwise the row misses.  With the first camera present the second is never
 *   consulted (if / elif).  Name 0, "no projection", gives -1 and misses.
 *   hit  (:99-100): out_dense[i, c] = float32(map element (c, y, x)) for c < channels, out_camera[i] = the camera index.
 *   miss:           out_dense[i, :] = 0, out_camera[i] = -1.
 * out_dense float32 [n, channels] and out_camera int32 [n] are written in full; the caller does not pre-zero them.
 * Outside pixels: a chosen camera whose (x, y) is outside [0, width) x [0, height), or a non-finite value or
 * |v| >= 2^31 in a column the decision reads, makes the row a miss and is counted in n_outside (int32 [1], device memory
 * for the device entry; the entry zeroes it first).  The reference raises IndexError for indices that are too large and
 * lets negative ones wrap around the image; refusing negative ones is a deliberate deviation.
 * SEG3D_EINVAL before any launch: channels outside 1..64, n_maps outside 1..8, elem_bytes not 2 / 4, point_bytes not
 * 4 / 8, cp_col < 0 or cp_col + 6 > stride, n < 0 or n > INT32_MAX, a present map with height, width or a stride < 1,
 * a NULL rows / out_dense / out_camera / n_outside with n > 0.  n == 0 returns 0 and launches nothing; a table whose
 * maps are all absent is legal (every row misses).  All offsets are 64-bit.  No allocation, no synchronisation.
 * seg3d_point_image_features_host: the same contract on HOST pointers, plain C++ without a HIP call; the same integers
 * and the same floats bit for bit (everything is a copy; float16 -> float32 is exact).
 */
#define SEG3D_IMAGE_MAX_CAMERAS 8
typedef struct {
  const void* data; /* NULL = camera absent */
  int32_t height, width;
  int64_t channel_stride, row_stride, col_stride; /* in elements, each >= 1 */
} seg3d_feature_map;
typedef struct {
  int32_t n_maps, channels, elem_bytes /* 4 float32, 2 float16 */, reserved;
  seg3d_feature_map maps[SEG3D_IMAGE_MAX_CAMERAS];
} seg3d_feature_map_table;
int seg3d_point_image_features(const seg3d_feature_map_table* table, const void* rows, int32_t point_bytes, int64_t n,
                               int32_t stride, int32_t cp_col, float* out_dense, int32_t* out_camera, int32_t* n_outside,
                               void* stream);
int seg3d_point_image_features_host(const seg3d_feature_map_table* table, const void* rows, int32_t point_bytes,
                                    int64_t n, int32_t stride, int32_t cp_col, float* out_dense, int32_t* out_camera,
                                    int32_t* n_outside);

/* Optimizer step (tools/train.py:136-149 optimizer.step(); builder.py:43-54: AdamW or SGD with momentum): every float32
 * parameter of a model updated by ONE launch.  `table` is an array of n_tensors records sorted by first_block (DEVICE
 * memory for seg3d_optim_step, HOST memory with host pointers for seg3d_optim_step_host); tensor i covers workgroups
 * [first_block_i, first_block_{i+1}) of seg3d_optim_block_elems() elements each (ceil(count / block_elems) of them; a
 * tensor with count == 0 owns none and is never touched), total_blocks is their sum.  A workgroup finds its tensor by
 * bisection and updates one chunk; tensors whose param, grad and state pointers are all 16-byte aligned move as
 * 16-byte vectors, the others (gradient views at an arbitrary 4-byte offset) and the tails element by element.
 * No atomics, no LDS, no allocation, no synchronisation.
 * `hyper` is a HOST array of n_hyper <= SEG3D_OPTIM_MAX_HYPER scalar sets; it is copied into the kernel arguments, so
 * the values may change every step without an upload.  record.hyper indexes it.  The arithmetic, in this order of
 * float32 operations (torch's single-tensor algorithms; no fused multiply-add anywhere, divide and sqrt correctly
 * rounded, so the device entry and the host entry give the same bits):
 *   SEG3D_OPTIM_SGD    v = {lr, wd, mu}: g' = g + wd * p (skipped when wd == 0); with state0 (momentum buffer):
 *                      m = g' when flags has SEG3D_OPTIM_FIRST_STEP, else m = mu * m + g'; p = p - lr * m.
 *                      state0 == NULL: p = p - lr * g'.  state1 is ignored.
 *   SEG3D_OPTIM_ADAMW  v = {1 - lr * wd, 1 - beta1, beta2, 1 - beta2, lr / bc1, sqrt(bc2), eps}, bc_i = 1 - beta_i^step:
 *                      p = p * v0; m = m + (g - m) * v1; v = v * v2 + v3 * g * g; p = p - v4 * m / (sqrt(v) / v5 + v6);
 *                      state0 = m (exp_avg), state1 = v (exp_avg_sq), both required.
 * SEG3D_EINVAL before any launch: table NULL with n_tensors > 0, hyper NULL with n_hyper > 0, a negative count,
 * n_hyper > SEG3D_OPTIM_MAX_HYPER, n_hyper == 0 with n_tensors > 0, total_blocks outside [0, INT32_MAX], an unknown
 * algo.  n_tensors == 0 or total_blocks == 0 returns 0 and does nothing.  The host entry also checks every record
 * (NULL param / grad with count > 0, missing AdamW state, hyper index out of range, first_block out of order); the
 * device entry cannot read its table, the kernel skips a record whose hyper index is out of range. */
#define SEG3D_OPTIM_SGD 0
#define SEG3D_OPTIM_ADAMW 1
#define SEG3D_OPTIM_MAX_HYPER 8
#define SEG3D_OPTIM_FIRST_STEP 1
typedef struct {
  float* param;
  const float* grad;
  float* state0;        /* momentum_buffer / exp_avg, or NULL */
  float* state1;        /* exp_avg_sq, or NULL */
  int64_t count;        /* elements */
  int64_t first_block;
  int32_t hyper;        /* index into the hyper sets of the call */
  int32_t flags;        /* SEG3D_OPTIM_FIRST_STEP */
  int64_t reserved;
} seg3d_optim_tensor;   /* 64 bytes */
typedef struct {
  float v[8];
} seg3d_optim_hyper;    /* 32 bytes */
int32_t seg3d_optim_block_elems(void);
int seg3d_optim_step(const seg3d_optim_tensor* table, int32_t n_tensors, int64_t total_blocks,
                     const seg3d_optim_hyper* hyper, int32_t n_hyper, int32_t algo, void* stream);
int seg3d_optim_step_host(const seg3d_optim_tensor* table, int32_t n_tensors, int64_t total_blocks,
                          const seg3d_optim_hyper* hyper, int32_t n_hyper, int32_t algo);

/* Gradient-norm clipping (torch.nn.utils.clip_grad_norm_, norm_type 2) between loss.backward() and optimizer.step(), over
 * the same record table and workgroup geometry as the step.  For these entries record.param is the GRADIENT array (read
 * by the norm, written by the scale); grad, state0, state1, hyper and flags are ignored and may be 0; count and
 * first_block mean what they mean for seg3d_optim_step.
 *   seg3d_grad_norm   two launches.  (1) one workgroup per chunk: every thread adds (double)g * (double)g (exact in
 *                     fp64) in a fixed order, the workgroup's sum goes to workspace[block] as one double; (2) one
 *                     workgroup adds the partials in a fixed order and writes result[0] = (float)sqrt(total) and
 *                     result[1] = c, c = max_norm / (result[0] + 1e-6f) in float32, replaced by 1.0f when c > 1.0f (a NaN
 *                     c stays NaN): torch's clip coefficient.  max_norm = +inf: the norm alone (c = 1 unless the norm is
 *                     not finite).  No atomics: the same bits on every run.  The sum of squares in fp64 is within
 *                     (n - 1) * 2^-53 of exact whatever the order, and squares that overflow or underflow float32 do not.
 *   seg3d_grad_scale  one launch on the same grid: a workgroup reads *coef (DEVICE memory, normally result + 1) and
 *                     returns when it is 1.0f, else g = g * coef over its chunk (a NaN coefficient is not 1).
 *   seg3d_grad_norm_workspace_bytes   8 bytes per workgroup; a smaller workspace_bytes is SEG3D_EWORKSPACE.
 *   seg3d_grad_norm_host / seg3d_grad_scale_host   the same definitions in plain C++ over HOST pointers (table, arrays,
 *                     result, coef): the twin the device is compared with and the path of CPU parameters.  They also check
 *                     every record: NULL array with count > 0, negative count, first_block out of order, wrong block sum.
 * SEG3D_EINVAL before any launch: table NULL with n_tensors > 0, NULL result / coef, n_tensors < 0, total_blocks outside
 * [0, INT32_MAX], a negative or NaN max_norm, workspace NULL with total_blocks > 0.  n_tensors == 0 or total_blocks == 0:
 * the norm entries write norm 0 and coefficient 1 and return 0, the scale entries do nothing. */
size_t seg3d_grad_norm_workspace_bytes(int64_t total_blocks);
int seg3d_grad_norm(const seg3d_optim_tensor* table, int32_t n_tensors, int64_t total_blocks, float max_norm,
                    void* workspace, size_t workspace_bytes, float* result, void* stream);
int seg3d_grad_scale(const seg3d_optim_tensor* table, int32_t n_tensors, int64_t total_blocks, const float* coef,
                     void* stream);
int seg3d_grad_norm_host(const seg3d_optim_tensor* table, int32_t n_tensors, int64_t total_blocks, float max_norm,
                         float* result);
int seg3d_grad_scale_host(const seg3d_optim_tensor* table, int32_t n_tensors, int64_t total_blocks, const float* coef);

#ifdef __cplusplus
}
#endif
#endif /* SEG3D_HIP_H */
