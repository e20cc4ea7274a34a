/* seevcn_hip.h — C ABI of libseevcn_hip.so (hand-written HIP kernels for gfx950 / MI355X).
 *
 * This is the drop-in boundary for the SEE-VCN hot path: every entry point below is what the
 * reference's Python would bind (ctypes / pybind) in place of the CUDA extension or third-party
 * call named in its comment (file:line relative to the reference tree).
 *
 * Conventions
 *   - all pointers are DEVICE pointers unless the name ends in `_host`;
 *   - every entry takes the HIP stream it must enqueue on (`void* stream` = hipStream_t; NULL = null stream)
 *     — the reference launches on the legacy default stream (e.g. pointnet2_stack/src/ball_query_gpu.cu:83);
 *   - entries never allocate, never synchronise and never exit(): they return 0 or an SV_ERR_* code and
 *     sv_last_error() gives the message (the reference prints and calls exit(-1), ball_query_gpu.cu:85-89);
 *   - counts that are only known on the device are written to caller-provided device int32 slots; callers
 *     pass capacities. Scratch/workspace sizes come from the matching *_bytes() query;
 *   - "persistent" workspaces must be zero-filled once by the caller (hipMemset) and are returned zeroed
 *     by every entry that uses them (entries clean exactly the cells they touched).
 *   - float = IEEE fp32, indices = int32, linear cell keys = int64.
 */
#ifndef SEEVCN_HIP_H
#define SEEVCN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SV_OK 0
#define SV_ERR_ARG 1
#define SV_ERR_HIP 2

#define SV_ABI_VERSION 1

int sv_abi_version(void);
const char* sv_last_error(void);
/* 1 when the library is the measurement build (`make measure`, libseevcn_hip_measure.so): only that build has the debug / trace kernel
 * instances, sv_debug_conv_trace / sv_debug_wgrad_trace and the environment switches that change results or skip launches (INTEGRATION.md,
 * "measurement build").  0: the production build, which answers to none of them. */
int sv_measure_build(void);

/* ------------------------------------------------------------------------------------------------
 * Coordinate index (persistent workspace shared by voxelisation and rulebook builds)
 * ---------------------------------------------------------------------------------------------- */
/* bytes of persistent (zero-initialised) workspace indexing `ncells` grid cells.  A workspace belongs to ONE cell count: its layout
 * (occupancy words | chunk counts | chunk bases) depends on ncells and a call returns only the words and counts to zero, so reusing
 * it with another ncells needs a memset in between. */
size_t sv_index_persistent_bytes(int64_t ncells);
/* bytes of per-call scratch used by the chunk scan for `ncells` cells */
size_t sv_index_scratch_bytes(int64_t ncells);

/* ------------------------------------------------------------------------------------------------
 * Dynamic voxelisation + mean VFE
 *   replaces DynamicMeanVFE.forward (detector3d/pcdet/models/backbones_3d/vfe/dynamic_mean_vfe.py:38-76):
 *   floor((xyz-min)/voxel) -> in-range mask -> key=b*XYZ+x*YZ+y*Z+z -> torch.unique(sorted) -> scatter_mean.
 *   points: (P, point_stride) fp32 rows [batch_idx, x, y, z, extra...]; the first `num_features`
 *   columns after batch_idx are averaged.  Outputs are ordered by ascending key (same as torch.unique):
 *   voxel_coords (cap,4) int32 [b,z,y,x], voxel_features (cap,num_features), point_to_voxel (P) int32
 *   (row of the voxel each point fell in, -1 if out of range; may be NULL), *num_voxels (device int32).
 *   index_ws: sv_index_persistent_bytes(batch*X*Y*Z); scratch: sv_voxelize_dynamic_scratch_bytes() (it includes a
 *   capacity x 4 x 8 B fixed-point accumulator).
 *   Means: with num_features <= 4, finite values with |v| < 2^15 (of a voxel's first 2^16 points) are summed as 64-bit
 *   fixed point (v x 2^32, exact for |v| >= 2^-9, off by <= 2^-33 below) -- order independent, so bit-reproducible
 *   run to run; NaN, +-inf, larger values and further points are summed in fp32 (NaN propagates).  The mean is
 *   (fixed sum + fp32 sum) / count in fp64, rounded once to fp32.  num_features > 4: fp32 sums in arrival order.
 * ---------------------------------------------------------------------------------------------- */
size_t sv_voxelize_dynamic_scratch_bytes(int64_t num_points, int64_t ncells, int64_t capacity);
int sv_voxelize_dynamic(const float* points, int64_t num_points, int point_stride, int num_features,
                        const float* pc_range_host /*6*/, const float* voxel_size_host /*3*/,
                        const int32_t* grid_size_host /*3: X,Y,Z*/, int batch_size,
                        void* index_ws, void* scratch,
                        int32_t* voxel_coords, float* voxel_features, int32_t* point_to_voxel,
                        int64_t capacity, int32_t* num_voxels, void* stream);

/* MeanVFE.forward (backbones_3d/vfe/mean_vfe.py:14-31): sum over the point axis / clamp_min(count,1).
 * voxels (V, max_points, C) fp32, num_points (V) int32 -> out (V, C). */
int sv_mean_vfe(const float* voxels, const int32_t* num_points, int64_t num_voxels, int max_points,
                int num_features, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * VCN surface completion (see/surface_completion/models/vcn/models/VCN_VC.py:178-214, VCN_CN.py:142-156)
 *   Activations are channel-last (M = B*n points, C) fp32; weights keep PyTorch's (C_out, C_in) layout.
 * ---------------------------------------------------------------------------------------------- */
#define SV_ACT_NONE 0
#define SV_ACT_RELU 1
#define SV_ACT_LRELU 2

int sv_fill_f32(float* dst, int64_t n, float value, void* stream);
/* *out = mul * sum(x^2) and, y != NULL, y = scale * x in ONE pass over x (n % 4 == 0, 16-byte aligned): a mean-square loss over a dense tensor that
 * leaves its own gradient behind while it reads the tensor (mul = 1 / n, scale = 2 / n) -- bench.py's stand-in for the loss behind HeightCompression
 * (the reference's BEV backbone + head, base_bev_backbone.py / anchor_head_single.py, are not in the headline step).  Deterministic (fixed grid,
 * fixed-order sums); scratch: sv_mean_square_scratch_bytes().  sv_scale_by_device_scalar: x *= *g, skipped on the device when *g == 1. */
size_t sv_mean_square_scratch_bytes(void);
int sv_mean_square(const float* x, int64_t n, float mul, float scale, float* y, float* out, void* scratch, void* stream);
int sv_scale_by_device_scalar(float* x, int64_t n, const float* g, void* stream);

/* C[M,N] = act(A[M,K] @ W[N,K]^T + bias[N] + group_bias[row / rows_per_group][N])  on the fp32 MFMA
 * (v_mfma_f32_32x32x2_f32: exact fp32).  Replaces the Conv1d(k=1)(+BN folded)(+ReLU/LeakyReLU) layers of
 * pose_encoder / FeatureEncoder (VCN_VC.py:81-106,116-123) and the Linear layers (:124-131).
 * C may be NULL (no store); group_max (M/rows_per_group, N), pre-filled with -inf, receives the max over each
 * group of rows (torch.max(feature, dim=2), VCN_VC.py:100,104 and AdaptiveMaxPool1d :122).  K must be a positive multiple of 16 (the K tile of the
 * kernel); lda, ldw >= K and multiples of 4, A and W 16-byte aligned; ldc >= N. */
int sv_gemm_bias_act(const float* A, int lda, const float* W, int ldw, const float* bias,
                     const float* group_bias, int rows_per_group, float* C, int ldc, float* group_max,
                     int M, int N, int K, int act, float slope, void* stream);
/* The same product (uniform groups, C stored, no column max) with K split over blockIdx.z when the output has few 128 x 128 tiles and K is long --
 * the shared FC over the pooled RoI grid of PV-RCNN's head (pcdet/models/roi_heads/pvrcnn_head.py:44-61: 27 648 -> 256 on 512 RoIs: 8 tiles, 1.9 ms
 * in one pass).  The split sums are added in split order by a second launch (bitwise reproducible), which also applies bias / group bias /
 * activation.  sv_gemm_splitk_splits(M, N, K) = number of splits (1: the one-pass kernel runs); scratch: sv_gemm_splitk_scratch_bytes. */
int sv_gemm_splitk_splits(int M, int N, int K);
size_t sv_gemm_splitk_scratch_bytes(int M, int N, int K);
int sv_gemm_bias_act_splitk(const float* A, int lda, const float* W, int ldw, const float* bias, const float* group_bias, int rows_per_group,
                            float* C, int ldc, int M, int N, int K, int act, float slope, void* scratch, void* stream);

/* out[m][c] = act(weight[c][0..2] . xyz[m] + bias[c])   (the Conv1d(3, C, 1) first layers; C % 4 == 0) */
int sv_pointwise_conv3(const float* xyz, const float* weight, const float* bias, float* out, int64_t M,
                       int C, int act, float slope, void* stream);
/* The same layer on gathered rows: out[m] = f(xyz[sel[m]]) for m < *m_dev (<= M_cap), sel int64 row indices (sv_unique_rows_compact). */
int sv_pointwise_conv3_gather(const float* xyz, const int64_t* sel, int64_t M_cap, const int32_t* m_dev, const float* weight, const float* bias,
                              float* out, int C, int act, float slope, void* stream);

/* ---- training side of the dense per-point / per-RoI layer stacks (see-vcn_amd/csrc/dense_train.hip).  The reference runs these through cuDNN / cuBLAS
 * under autograd: VCN_VC.forward in training mode (see/surface_completion/models/vcn/models/VCN_VC.py:97-106,116-131,178-214) and PV-RCNN's
 * point head / feature fusion / RoI head FC stacks (dense_heads/point_head_simple.py, pfe/voxel_set_abstraction.py:168-172, roi_heads/pvrcnn_head.py:171-176).
 * sv_gemm_tn: C (N, K) = A^T B with A (M, N), B (M, K) row-major as they lie -- the weight gradient dW = dY^T X; fp32 MFMA, M split over workgroups,
 * partial tiles summed in a fixed order (bitwise reproducible).  scratch: sv_gemm_tn_scratch_bytes(M, N, K). */
size_t sv_gemm_tn_scratch_bytes(int64_t M, int N, int K);
int sv_gemm_tn(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int64_t M, int N, int K, void* scratch, void* stream);
/* C[i][j] = sum_c A[i * stride_a_row + c * stride_a_c] * B[c * stride_b_c + j * stride_b_col] for small / odd-shaped products (element strides);
 * contraction split over workgroups, fixed-order sum.  scratch: sv_gemm_strided_scratch_bytes(rows, cols, contraction). */
size_t sv_gemm_strided_scratch_bytes(int rows, int cols, int64_t contraction);
int sv_gemm_strided(const float* A, int64_t stride_a_row, int64_t stride_a_c, const float* B, int64_t stride_b_c, int64_t stride_b_col, float* C, int64_t ldc,
                    int rows, int cols, int64_t contraction, void* scratch, void* stream);
/* out[n] = sum_m A[m][n] (bias gradient), fixed order.  scratch: sv_column_sums_scratch_bytes(M, N). */
size_t sv_column_sums_scratch_bytes(int64_t M, int N);
int sv_column_sums(const float* A, int64_t lda, int64_t M, int N, float* out, void* scratch, void* stream);
/* Rows g * rows_per_group .. form group g (an object's points): column max with the first arg-max row (torch.max(dim) / AdaptiveMaxPool1d), its
 * backward (dx written everywhere: the gradient at the arg-max row, zero elsewhere) and the column sum of a group's rows (gradient of a feature
 * broadcast to the group's rows). */
int sv_segment_max(const float* x, int64_t ldx, int groups, int rows_per_group, int channels, float* out, int32_t* arg, void* stream);
int sv_segment_max_backward(const float* dout, const int32_t* arg, int groups, int rows_per_group, int channels, float* dx, int64_t ldx, void* stream);
int sv_segment_sum(const float* x, int64_t ldx, int groups, int rows_per_group, int channels, float* out, void* stream);
/* dz = dy * act'(y) for act = SV_ACT_RELU / SV_ACT_LRELU taken from the layer's output y (0: copy) */
int sv_act_backward(const float* dy, const float* y, int64_t n, int act, float slope, float* dz, void* stream);

/* VCN_VC.py:185-190: frustum angle, rotation to the frustum view, mean-centering.
 * input (B,n,3) -> fview (B,n,3), centred (B,n,3), state (B,32) [angle, mean xyz, centre xyz, rot 3x3]. */
int sv_vcn_vc_prep(const float* input, int batch, int n, float* fview, float* centred, float* state, void* stream);
/* VCN_VC.py:195-200: rel_pose (B,9) -> centre, rot (ortho6d, :36-49) into state; pc_cn = (fview-centre) @ rot^T */
int sv_vcn_vc_pose(const float* fview, int batch, int n, const float* rel_pose, float* state, float* pc_cn, void* stream);
/* VCN_VC.py:205-212: coarse_cn (B,nc,3) -> coarse (B,nc,3) in the sensor view, reg_rot (B,3,3), reg_centre (B,3) */
int sv_vcn_vc_finish(const float* coarse_cn, int batch, int num_coarse, const float* state, float* coarse,
                     float* reg_rot, float* reg_centre, void* stream);
/* VCN_CN.py:146-154 with utils/transform.py:91-160: inverse=0: vc_to_cn + normalize_scale; 1: restore_scale + cn_to_vc */
int sv_vcn_cn_transform(const float* in, int batch, int n, const float* gt_boxes, int inverse, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Sparse 3-D convolution (replaces the un-vendored third-party `spconv`; call sites
 * detector3d/pcdet/models/backbones_3d/spconv_backbone.py:8-27,77-117,141-157, height_compression.py:21).
 * Coordinates are (N,4) int32 [b,z,y,x]; shapes/kernel/stride/padding/dilation are host int32[3] in z,y,x order.
 * Kernel offset index k = (kz*Ky + ky)*Kx + kx.  Rulebooks are output-major tables nbr[k][row] (or -1).
 * ---------------------------------------------------------------------------------------------- */
/* out_shape = floor((in + 2*pad - dil*(k-1) - 1)/stride) + 1 */
int sv_conv_out_shape(const int32_t* in_shape_host, const int32_t* ksize_host, const int32_t* stride_host,
                      const int32_t* padding_host, const int32_t* dilation_host, int32_t* out_shape_host);
/* scratch for either rulebook entry; `ncells` = batch * prod(shape of the level being indexed) */
size_t sv_rulebook_scratch_bytes(int64_t n_in, int64_t ncells);
/* SubMConv3d rulebook: nbr (K, n): row j with coord[j] = coord[i] + (k - K/2)*dilation (output set = input set,
 * caller's row order).  index_ws: sv_index_persistent_bytes(batch*Z*Y*X). dilation_host may be NULL (=1). */
int sv_rulebook_subm(const int32_t* coords, int64_t n, int batch, const int32_t* shape_host,
                     const int32_t* ksize_host, const int32_t* dilation_host, void* index_ws, void* scratch,
                     int32_t* nbr, void* stream);
/* Same table through a dense cell -> row map (int32 per cell in 4x4x8-cell tiles, sv_cellmap_persistent_bytes(batch, shape) bytes,
 * ALL ZERO on entry and on return): 3 launches instead of 8, no atomics.  For grids whose map fits comfortably in the 288 GB of HBM (16 KITTI scenes at
 * 5 cm: 5.9 GB); callers fall back to sv_rulebook_subm for larger grids. */
size_t sv_cellmap_persistent_bytes(int batch, const int32_t* spatial_shape);
/* table_rows (n, 32) int32 and masks (n) int32, both optional (K <= 27): the same table ROW-MAJOR ([0..26] source rows, rest -1: one 128-byte
 * line per row) and every row's neighbour mask (bit k = has neighbour k) -- what the convolution plan consumes (sv_conv_plan_build). */
int sv_rulebook_subm_cellmap(const int32_t* coords, int64_t n, int batch, const int32_t* spatial_shape, const int32_t* ksize,
                             const int32_t* dilation, void* cellmap, int32_t* nbr, int32_t* table_rows, int32_t* masks, void* stream);
/* SparseConv3d rulebook, phase 1: output coordinates in canonical (ascending ((b*Z+z)*Y+y)*X+x) order and the
 * input-major table nbr_in (K, n_in) = output row fed by (k, input) or -1; *num_out on the device.
 * in_block (optional, K <= 27): (32 + 1) * n_in int32 = [table_rows_in (n_in, 32) | masks_in (n_in)], the same table row-major plus every
 * input row's mask (bit k = feeds an output through offset k) -- what the data-gradient plan consumes.
 * index_ws: sv_index_persistent_bytes(batch * prod(out_shape)). */
int sv_rulebook_sparse(const int32_t* coords, int64_t n_in, int batch, const int32_t* in_shape_host,
                       const int32_t* ksize_host, const int32_t* stride_host, const int32_t* padding_host,
                       const int32_t* dilation_host, void* index_ws, void* scratch, int32_t* out_coords,
                       int32_t* nbr_in, int32_t* in_block, int64_t capacity, int32_t* num_out, void* stream);
/* A CHAIN of strided layers (spconv_backbone.py:141-157: conv2, conv3, conv4, conv_out; spconv reads every level's indice-pair count back
 * to the host) counted end to end on the device -- ONE device -> host read for all output-site counts, or none when the caller defers it:
 * level l marks its output cells from level l-1's site list (one lane per site; level 0 from `coords0`, whose length may live on the device:
 * n0_dev non-NULL overrides n0, which then only bounds the grid), counts its occupancy bitmap and writes its sites in canonical (ascending
 * key) order into sites[l] (capacity caps[l] rows of int4 [b,z,y,x]) and their number into num_out[l] (device).  Kernels up to 3 per axis.
 * geoms_host: n_levels x 15 int32 = {in_shape[3], ksize[3], stride[3], padding[3], dilation[3]}; index_ws[l]: sv_index_persistent_bytes(batch *
 * prod(out_shape_l)), all zero on entry and left MARKED (the SET jobs of sv_rulebook_batch return the touched words to zero);
 * scratch: sv_rulebook_chain_scratch_bytes(largest batch * prod(out_shape)). */
size_t sv_rulebook_chain_scratch_bytes(int64_t max_ncells);
int sv_rulebook_chain_count(const int32_t* coords0, int64_t n0, const int32_t* n0_dev, int batch, int n_levels, const int32_t* geoms_host,
                            void* const* index_ws, int32_t* const* sites, const int64_t* caps, int32_t* num_out, void* scratch, void* stream);
/* Every rulebook table of a network in three launches, through dense cell -> row maps (sv_cellmap_persistent_bytes per level, all zero between
 * calls).  jobs_host: n_jobs rows of 32 int64, row[0] = kind:
 *   1 SET    [1] sites (n, 4) of a level, [2] exact-size copy of them or 0, [3] the level's cell map or 0, [4] index workspace the sites were
 *            marked in (sv_rulebook_chain_count) to return to zero, or 0, [5] n, [6..8] level shape (Z, Y, X), [9] batch
 *   2 QUERY  one table: row r (coordinate c) and offset k = (kz, ky, kx) address cell (c * mul + add + k * step) / div of the TARGET level (exact
 *            division, inside its shape), whose map gives the source row.  [1] row sites, [2] target map, [3] nbr (K, n) k-major table, [4] (n, 32)
 *            row-major twin, [5] masks (n), [6] n, [7..9] row-level shape, [10..12] target shape, [13..15] ksize, [16..18] mul, [19..21] add,
 *            [22..24] step, [25..27] div, [28] batch.  Submanifold: mul 1, add -(ks/2)*dil, step dil, div 1; strided output-major: mul stride,
 *            add -pad, step dil, div 1 (target = input level); strided input-major: mul 1, add pad, step -dil, div stride (target = output level).
 * Runs every SET, then every QUERY, then zeroes the maps of the SET jobs.  Same tables as sv_rulebook_subm_cellmap / sv_rulebook_sparse +
 * sv_rulebook_invert_rows, bit for bit. */
int sv_rulebook_batch(const int64_t* jobs_host, int n_jobs, void* stream);
/* phase 2 (after the caller knows n_out): nbr_out (K, n_out) output-major table from nbr_in */
int sv_rulebook_invert(const int32_t* nbr_in, int64_t n_in, int K, int32_t* nbr_out, int64_t n_out, void* stream);
/* The same inversion (K <= 27) from the row-major input table (sv_rulebook_sparse's in_block) that also writes the row-major twin and the
 * neighbour masks of the output side:
 *   out_block ((32 + K + 1) * n_out int32, filled here) = [table_rows_out (n_out, 32) | nbr_out (K, n_out) | masks_out (n_out)] */
int sv_rulebook_invert_rows(const int32_t* table_rows_in, int64_t n_in, int K, int32_t* out_block, int64_t n_out, void* stream);
/* counts[k] = number of (in,out) pairs of offset k (spconv's indice_pair_num) */
int sv_rulebook_pair_counts(const int32_t* nbr, int64_t n_out, int K, int32_t* counts, void* stream);

/* Y[o][n] = epi( sum_k sum_c X[nbr[k][o]][c] * Wt[k][n][c] ),  epi: +bias, *scale+shift (folded BN), +residual, relu.
 *   forward:       X = features (N_in,C_in),  nbr = output-major table, Wt = weight as (K, C_out, C_in)
 *   backward-data: X = grad_out (N_out,C_out), nbr = input-major table, Wt = weight as (K, C_in, C_out)
 * X has n_src rows, nbr/Y have n_rows rows.  Plain entry: packed (K, Nc, Kd) weights and the k-major table; fp32 MFMA
 * (v_mfma_f32_16x16x4_f32, accumulators in registers) when Kd and Nc are multiples of 16, VALU otherwise (the 3-channel input layer).
 * This replaces spconv's per-offset gather / GEMM / scatter-add launches (spconv is un-vendored: spconv_backbone.py:8-27 are the call sites). */
int sv_sparse_conv_gather_gemm(const float* X, int64_t n_src, const int32_t* nbr, const float* Wt, float* Y,
                               int64_t n_rows, int K, int Kd, int Nc, const float* bias, const float* scale, const float* shift,
                               const float* residual, int relu, void* stream);

/* ---- the MFMA kernel on a PLAN of the table (what SubMConv3d / SparseConv3d of seevcn_amd.spconv run; csrc/sparse_conv.hip) ----
 * Inputs of a plan: the table row-major (n_rows, 32) and the rows' neighbour masks (n_rows) -- written by the rulebook builders
 * (sv_rulebook_subm_cellmap, sv_rulebook_invert_rows) or, for any k-major table with K <= 27, by sv_conv_table_rows.
 * sv_conv_plan_build, once per table: rows are split into 8 contiguous regions (one per XCD: workgroup b of the conv launch works on
 * region b % 8, so a scene's rows are gathered through one L2) and regrouped inside a region into 16-row tiles of equal neighbour-mask
 * class (counting sort): perm (16*ceil(n_rows/16)) int32 = row at each position (-1 = padding of the last tile), masks_p = its mask.
 * persistent: sv_conv_plan_persistent_bytes() bytes, all zero before the first call and left zero-consistent by every call.
 * sv_conv_plan_tiles, once per (table, tiles_per_wave): tile_of (sv_conv_plan_tiles_bytes(n_rows, tiles_per_wave)) maps [region][wave][slot] to a
 * tile of the region or -1.  A launch is one resident round of 4 waves per SIMD (8 regions x 128 workgroups); a region's tiles are
 * counting-sorted by their number of active offsets and dealt, round after round, to the 128 SIMDs of the region's XCD in ascending order of
 * their load so far (equal work per SIMD); a wave works through its slots tiles_per_wave tiles at a time.
 * tiles_per_wave = sv_conv_tiles_per_wave(n_rows, Kd, Nc) of the conv that will use it (2 or 4).
 * Results are bit-identical to sv_sparse_conv_gather_gemm (same summation order per output element). */
int sv_conv_table_rows(const int32_t* nbr, int64_t n_rows, int K, int32_t* table_rows, int32_t* masks, void* stream);
size_t sv_conv_plan_persistent_bytes(void);
size_t sv_conv_plan_perm_bytes(int64_t n_rows);
int sv_conv_plan_build(const int32_t* masks, int64_t n_rows, void* persistent, int32_t* perm, int32_t* masks_p, void* stream);
int sv_conv_tiles_per_wave(int64_t n_rows, int Kd, int Nc);
size_t sv_conv_plan_tiles_bytes(int64_t n_rows, int tiles_per_wave);
int sv_conv_plan_tiles(const int32_t* masks_p, int64_t n_rows, int tiles_per_wave, int32_t* tile_of, void* stream);
/* Both of the above for one tiles_per_wave value in ONE launch (one workgroup per region, all passes in LDS): perm, masks_p and tile_of as
 * sv_conv_plan_build + sv_conv_plan_tiles leave them, up to the order of the rows inside a class (results of the convolution do not depend
 * on it). */
int sv_conv_plan_build_dealt(const int32_t* masks, int64_t n_rows, int tiles_per_wave, int32_t* perm, int32_t* masks_p, int32_t* tile_of,
                             void* stream);
/* sv_conv_plan_build_dealt for several tables in ONE launch (one workgroup per region and table); jobs_host: n_jobs rows of 8 int64 =
 * {masks, n_rows, tiles_per_wave, perm, masks_p, tile_of, 0, 0} (device addresses). */
int sv_conv_plan_build_dealt_batch(const int64_t* jobs_host, int n_jobs, void* stream);
/* 1 iff the plan kernel is built for this layer shape (K <= 27 offsets, C_in in {16,32,64,128}, C_out in {16,32} or a multiple of 64 up to
 * 512) and X (n_src rows) is addressable through a 32-bit buffer descriptor; other shapes take sv_sparse_conv_gather_gemm. */
int sv_conv_mfma_kernel_applies(int K, int Kd, int Nc, int64_t n_src);
/* Weights of one layer in MFMA fragment order for both directions, from ANY (K, C_in, C_out) view given by its element strides (the
 * parameter of spconv-2.x layout (C_out, kz, ky, kx, C_in) is such a view: no transposing copy).  frag_fwd serves the forward
 * (Kd = C_in, Nc = C_out), frag_bwd the data gradient (Kd = C_out, Nc = C_in); K*C_in*C_out floats each, caller-owned (cache them per
 * weight version; either may be null). */
int sv_conv_weight_fragments(const float* W, int64_t stride_k, int64_t stride_cin, int64_t stride_cout, int K, int Cin, int Cout, float* frag_fwd,
                             float* frag_bwd, void* stream);
/* The same for n_layers weights in one launch.  descs_device: (n_layers, 10) int64 ON THE DEVICE, per layer {W pointer, stride_k, stride_cin,
 * stride_cout, K, C_in, C_out, frag_fwd pointer, frag_bwd pointer, first unit}; a layer has 2 * K * C_in * C_out / 4 units (float4, forward
 * then backward view), "first unit" is the running sum of the layers before it, total_units the sum over all layers. */
int sv_conv_weight_fragments_batch(const void* descs_device, int n_layers, int64_t total_units, void* stream);
/* Input transform of the NEXT sv_sparse_conv_gather_gemm_planned / sv_sparse_conv_wgrad* call of this host thread (consumed by it, whatever it
 * returns): that call reads X through y = [relu](x * scale[c] + shift[c]), coef (2, C_in) = scale | shift (16-byte aligned) -- X is then the RAW
 * output of the convolution below and coef the coefficients of its BatchNorm1d (sv_batchnorm_finalize_forward), i.e. the `norm_fn -> ReLU` tail of
 * post_act_block (spconv_backbone.py:9-27) is applied as the rows are gathered and the normalised tensor is never written.  Same expression as the
 * separate pass (fused multiply-add, then max): consumers see bit-identical values; absent neighbours contribute 0.  coef = NULL clears it.
 * Entry points that cannot apply it (the plain k-major conv, non-MFMA weight-gradient shapes) fail with SV_ERR_ARG. */
int sv_conv_next_input_norm(const float* coef, int relu);
/* table_k_reversed: offset k reads table entry K-1-k (a submanifold table serving its own data gradient, no flipped copy).
 * Epilogue (bias, scale + shift, residual, relu as for sv_sparse_conv_gather_gemm; per element: add bias, ONE fused multiply-add -- the instruction of
 * sv_batchnorm_apply, so a folded eval-mode BatchNorm gives the bits of the separate pass --, add residual, max with 0): when Y and every term given are
 * 16-byte aligned the launch stores whole rows (16 bytes per lane, the residual read the same way), otherwise 4 bytes per accumulator; the values are
 * the same.  residual must not alias Y (not checked: a residual that overlaps Y at a shifted address is read after other lanes wrote it).  Rows the table pads with (-1) are neither read nor written. */
int sv_sparse_conv_gather_gemm_planned(const float* X, int64_t n_src, const int32_t* table_rows, const int32_t* perm, const int32_t* masks_p,
                                       const int32_t* tile_of, int tiles_per_wave,
                                       const float* wfrag, float* Y, int64_t n_rows, int K, int Kd, int Nc, const float* bias,
                                       const float* scale, const float* shift, const float* residual, int relu, int table_k_reversed,
                                       float* bn_partial, void* stream);
/* Data gradient on a plan whose output is the gradient of a BatchNorm1d(+ReLU) OUTPUT (the layer below in VoxelBackBone8x, spconv_backbone.py:8-27):
 * the same kernel, and its epilogue also leaves the two per-channel sums of that BatchNorm's backward (sum of dy on the forward's ReLU branch,
 * and of dy * xhat) as sv_conv_planned_partials() per-workgroup partials in bn_partial -- sv_batchnorm_relu_backward_partial starts at the
 * combine.  bn_x = the BatchNorm's input (n_rows, Nc), bn_mean / bn_invstd its saved batch statistics, bn_gamma / bn_beta may be NULL. */
int sv_sparse_conv_dgrad_planned_bn(const float* dZ, int64_t n_src, const int32_t* table_rows, const int32_t* perm, const int32_t* masks_p,
                                    const int32_t* tile_of, int tiles_per_wave, const float* wfrag, float* dY, int64_t n_rows, int K, int Kd, int Nc,
                                    int table_k_reversed, const float* bn_x, const float* bn_mean, const float* bn_invstd, const float* bn_gamma,
                                    const float* bn_beta, int bn_relu, float* bn_partial, void* stream);
/* ---- half-precision inference (csrc/sparse_conv_half.hip): fp16 activations and weights, fp32 accumulation and epilogue.  Replaces the fp16 kernels
 * of spconv 2.x behind SubMConv3d / SparseConv3d in eval mode (detector3d/pcdet/models/backbones_3d/spconv_backbone.py:8-27,77-117).
 * 1 iff k_spconv_h16 is built for the layer: K <= 27 offsets, C_in and C_out in {16, 32, 64, 128}, and X (n_src rows of C_in fp16 values) is
 * addressable with 32-bit byte offsets. */
int sv_conv_h16_applies(int K, int Kd, int Nc, int64_t n_src);
/* fp16 fragment copy of one layer's weights for the FORWARD direction (the eval list has no other), from any (K, C_in, C_out) fp32 view given by its
 * element strides like sv_conv_weight_fragments; round to nearest even (the bits of torch.Tensor.half()).  frag16: K * C_in * C_out fp16 values,
 * 16-byte aligned, caller-owned.  Order: one unit = one lane's MFMA operand, E = 8 values (C_in >= 32) or 4 (C_in = 16):
 * frag16[(((k * KQ + q) * NT + t) * 64 + lane) * E + j] = W[k][q * 4 E + (lane >> 4) * E + j][t * 16 + (lane & 15)], KQ = C_in / (4 E), NT = C_out / 16. */
int sv_conv_weight_fragments_h16(const float* W, int64_t stride_k, int64_t stride_cin, int64_t stride_cout, int K, int Cin, int Cout, void* frag16,
                                 void* stream);
/* The same for n_layers weights in one launch.  descs_device: (n_layers, 10) int64 ON THE DEVICE, laid out like sv_conv_weight_fragments_batch's: per
 * layer {W pointer, stride_k, stride_cin, stride_cout, K, C_in, C_out, frag16 pointer, 0, first unit}; a layer has K * C_in * C_out / E units. */
int sv_conv_weight_fragments_h16_batch(const void* descs_device, int n_layers, int64_t total_units, void* stream);
/* Y (n_rows, Nc) = store(epilogue(sum_k X16[nbr[k]] @ W16[k])) on the plan of a table (table_rows, perm, masks_p as sv_conv_plan_build* leave them;
 * tile_of is not used: a wave takes 16 consecutive perm positions at a time, in perm order, inside the region of its XCD).  X16 (n_src, Kd) and
 * residual16 (n_rows, Nc) are fp16, bias / scale / shift (Nc) fp32, wfrag16 from sv_conv_weight_fragments_h16.  Products and sums in fp32 (offsets
 * ascending, channel blocks ascending: reproducible bit for bit); epilogue in fp32 in sv_sparse_conv_gather_gemm_planned's order (add bias, ONE fused
 * multiply-add, add residual, max with 0).  y_is_f32 = 0: Y is fp16, stored round-to-nearest-even; a finite result beyond 65504 is stored as +-inf
 * (not clamped).  y_is_f32 = 1: Y is fp32 (the last layer of a list).  Whole rows are stored when Y and every term given are 16-byte aligned, single
 * elements otherwise; the values are the same.  Rows the plan pads with (-1) are neither read nor written.  Shapes: sv_conv_h16_applies. */
int sv_sparse_conv_gather_gemm_planned_h16(const void* X16, int64_t n_src, const int32_t* table_rows, const int32_t* perm, const int32_t* masks_p,
                                           const void* wfrag16, void* Y, int y_is_f32, int64_t n_rows, int K, int Kd, int Nc, const float* bias,
                                           const float* scale, const float* shift, const void* residual16, int relu, void* stream);
/* y_f16[i] = half(x_f32[i]), round to nearest even (subnormals kept, +-inf beyond 65504): the fp16 copy of the fp32 input layer's output that the
 * second layer of a half-precision list gathers (the reference casts with features.half() in front of the backbone instead, which rounds raw
 * point coordinates). */
int sv_narrow_h16(const float* x_f32, int64_t n_elems, void* y_f16, void* stream);
/* bn_partial (null or sv_conv_planned_partials() x 2 x Nc floats; plain epilogue only: no bias / scale / residual / relu): per-workgroup column
 * sums and sums of squares of Y, the first pass of the training-mode BatchNorm behind the convolution (post_act_block, spconv_backbone.py:9-27)
 * made in the epilogue that holds the values in registers anyway; consumed by sv_batchnorm_relu_forward_partial. */
int sv_conv_planned_partials(void);
/* Measurement aid (tools/conv_trace.py): while buf is non-null every wave of sv_sparse_conv_gather_gemm_planned writes 8 uint64 to it
 * (s_memtime at start / after the prologue / after the main loop / at the end, HW_ID, XCC_ID, tile-offset steps, block << 8 | wave);
 * buf holds grid.x * grid.y * 4 slots of 64 bytes (size it as 8 * (n_tiles + 64) * columns / 64 slots).  Measurement build only
 * (sv_measure_build() == 1); the production library returns SV_ERR_ARG. */
int sv_debug_conv_trace(void* buf);
/* The same for the MFMA weight gradient (tools/wgrad_trace.py; the 64 -> 64 channel instance only): per wave s_memtime at start, ticks spent in the
 * pass prologues (table read + compaction), ticks in the MFMA loops, s_memtime at the end, XCC_ID << 32 | HW_ID, s_memtime after the last pass,
 * passes << 32 | pairs, offset << 32 | chunk; buf holds 4 x workgroups slots of 64 bytes.  Measurement build only, like sv_debug_conv_trace. */
int sv_debug_wgrad_trace(void* buf);
/* dW (K, C_in, C_out) = sum_o X[nbr[k][o]]^T dY[o]; deterministic two-stage reduction.  n_src = rows of X (every table entry is < n_src): when
 * n_src * C_in * 4 < 2^32 the operand rows are addressed with 32-bit byte offsets from uniform bases; n_src <= 0 = unknown (64-bit addresses). */
size_t sv_sparse_conv_wgrad_scratch_bytes(int64_t n_rows, int K, int Cin, int Cout);
int sv_sparse_conv_wgrad(const float* X, int64_t n_src, const int32_t* nbr, const float* dY, float* dW, int64_t n_rows, int K,
                         int Cin, int Cout, void* scratch, void* stream);
/* The same with element (k, c_in, c_out) written at dW[k * stride_k + c_in * stride_cin + c_out * stride_cout] -- the layout of the
 * caller's parameter (spconv's (C_out, kz, ky, kx, C_in)), so that no transposing copy of the gradient is needed.  The strides must
 * address a permutation of the K * C_in * C_out slab. */
int sv_sparse_conv_wgrad_strided(const float* X, int64_t n_src, const int32_t* nbr, const float* dY, float* dW, int64_t n_rows, int K, int Cin,
                                 int Cout, int64_t stride_k, int64_t stride_cin, int64_t stride_cout, void* scratch, void* stream);
/* The two stages apart, for a backward pass that runs many layers: stage 1 (partial slabs into `partial`, sv_sparse_conv_wgrad_partial_bytes; *job = 10 int64
 * on the host describing the pending sum) per layer, then sv_sparse_conv_wgrad_reduce_batch(jobs, n_jobs) sums the slabs of all layers in one launch -- bitwise the
 * values sv_sparse_conv_wgrad_strided writes. */
size_t sv_sparse_conv_wgrad_partial_bytes(int64_t n_rows, int K, int Cin, int Cout);
int sv_sparse_conv_wgrad_stage1(const float* X, int64_t n_src, const int32_t* nbr, const float* dY, float* dW, int64_t n_rows, int K, int Cin, int Cout,
                                int64_t stride_k, int64_t stride_cin, int64_t stride_cout, void* partial, int64_t* job, void* stream);
int sv_sparse_conv_wgrad_reduce_batch(const int64_t* jobs_host, int n_jobs, void* stream);
/* Weight gradient on EQUAL PIECES (the default of the trained path; replaces the role of spconv's indice_conv_backward filter gradient as the entries above do).
 * The chunked stage 1 above gives every (row chunk, offset) a workgroup: an offset's work follows its density, and the launch ends when the unluckiest CU
 * does (pairs per SIMD max / mean 1.4-1.6 on a LiDAR rulebook, tools/wgrad_trace.py).  Here a per-TABLE plan cuts the table's pairs, in (row eighth, offset, row) order, into
 * sv_wgrad_plan_pieces(Cin, Cout) pieces of equal pair count (up to one 64-row unit) -- as many as workgroups are resident -- and stage 1 runs one
 * workgroup per piece (one (Cin, Cout) slab per (row eighth, offset) a piece touches; the order of the cut is row eighth, offset, row, so that an XCD's
 * workgroups stay inside one eighth of the rows).  A plan is a function of (table, pieces) only: build it once per rulebook
 * table, use it for every layer on that table whose sv_wgrad_plan_pieces agrees.  Results are bitwise reproducible; they differ from the chunked
 * form's in the last bits (other partial sums).
 *   sv_wgrad_plan_bytes          bytes of a plan (device memory, caller-owned)
 *   sv_wgrad_plan_build          nbr (K, n_rows) -> plan; 2 launches
 *   sv_wgrad_planned_applies     1 iff the layer runs on this path (MFMA tile shape, 32-bit addressable operands); otherwise use sv_sparse_conv_wgrad*
 *   sv_sparse_conv_wgrad_planned_bytes   bytes of `partial`
 *   sv_sparse_conv_wgrad_planned         both stages; strides all 0 = contiguous (K, Cin, Cout) dW, else as sv_sparse_conv_wgrad_strided
 *   sv_sparse_conv_wgrad_planned_stage1  stage 1 only; *job for sv_sparse_conv_wgrad_reduce_batch */
size_t sv_wgrad_plan_bytes(int64_t n_rows, int K, int pieces);
int sv_wgrad_plan_pieces(int Cin, int Cout);
int sv_wgrad_plan_build(const int32_t* nbr, int64_t n_rows, int K, int pieces, void* plan, void* stream);
/* the plans of several tables in two launches; jobs_host: n_jobs rows of 8 int64 = {nbr, n_rows, K, pieces, plan, 0, 0, 0} (device addresses) */
int sv_wgrad_plan_build_batch(const int64_t* jobs_host, int n_jobs, void* stream);
int sv_wgrad_planned_applies(int64_t n_src, int64_t n_rows, int K, int Cin, int Cout);
size_t sv_sparse_conv_wgrad_planned_bytes(int K, int Cin, int Cout);
int sv_sparse_conv_wgrad_planned(const float* X, int64_t n_src, const int32_t* nbr, const float* dY, float* dW, int64_t n_rows, int K, int Cin, int Cout,
                                 int64_t stride_k, int64_t stride_cin, int64_t stride_cout, const void* plan, void* partial, void* stream);
int sv_sparse_conv_wgrad_planned_stage1(const float* X, int64_t n_src, const int32_t* nbr, const float* dY, float* dW, int64_t n_rows, int K, int Cin,
                                        int Cout, int64_t stride_k, int64_t stride_cin, int64_t stride_cout, const void* plan, void* partial, int64_t* job,
                                        void* stream);

/* SparseConvTensor.dense(): (N,C) + coords -> (B, C, D, H, W), every element written once */
size_t sv_sparse_to_dense_scratch_bytes(int batch, int D, int H, int W);
int sv_sparse_to_dense(const float* features, const int32_t* coords, int64_t n, int batch, int C, int D, int H, int W,
                       void* scratch, float* out, void* stream);
/* its backward: gather (B,C,D,H,W) at coords -> (N,C) */
int sv_dense_to_sparse(const float* dense, const int32_t* coords, int64_t n, int batch, int C, int D, int H, int W,
                       float* out, void* stream);
/* The same volume in channels-last memory for HeightCompression (height_compression.py:21-23: dense().view(N, C * D, H, W)) in front of a channels_last
 * 2-D backbone: out[b][y][x][c * D + d] -- on the torch side a (B, C D, H, W) tensor with channels_last strides -- and its backward from a gradient
 * in that order.  Scratch as sv_sparse_to_dense.  sv_sparse_to_dense_nhwc_applies: C % 4 == 0, D <= 8, H W % 16 == 0 (else use the pair above). */
int sv_sparse_to_dense_nhwc_applies(int C, int D, int H, int W);
int sv_sparse_to_dense_nhwc(const float* features, const int32_t* coords, int64_t n, int batch, int C, int D, int H, int W, void* scratch,
                            float* out, void* stream);
int sv_dense_to_sparse_nhwc(const float* dense, const int32_t* coords, int64_t n, int batch, int C, int D, int H, int W, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * PointNet++ stacked-batch primitives (detector3d/pcdet/ops/pointnet2/pointnet2_stack/src/ *.cu; pybind names in
 * src/pointnet2_api.cpp:12-31).  Scenes are described by device int32 arrays of first row and row count.
 * ---------------------------------------------------------------------------------------------- */
/* farthest_point_sampling_wrapper(b, n, m, points, temp, idx) (src/sampling.cpp:24-36; kernel sampling_gpu.cu:24-140):
 * xyz (b,n,3) -> idx (b,m) int32, first index 0, index-exact including the reference's tie rule.
 * temp (b*n floats) is only used when n > 24576 (larger scenes stream from HBM); may be NULL otherwise. */
int sv_farthest_point_sampling(const float* xyz, int b, int n, int m, float* temp, int32_t* idx, void* stream);
/* the same over ragged scenes in one launch (replaces the per-scene Python loop of
 * VoxelSetAbstraction.get_sampled_points, backbones_3d/pfe/voxel_set_abstraction.py:250-256): idx (batch,m) holds
 * GLOBAL row indices (scene start + local index). max_n = largest scene. */
int sv_stack_farthest_point_sampling(const float* xyz, const int32_t* xyz_batch_start, const int32_t* xyz_batch_cnt, int batch,
                                     int max_n, int m, float* temp, int32_t* idx, void* stream);
/* The same with SEVERAL workgroups per scene (16; batch * 16 <= 256 workgroups, 4096 <= max_n <= 65536, m < 65536 -- otherwise it falls back
 * to one workgroup per scene): every round the workgroups exchange their best candidate through self-tagged 16-byte granules in
 * multi_scratch (sv_fps_multi_scratch_bytes(batch) bytes, any content).  Index-exact with the single-workgroup kernel.  This path reads an
 * error word back and therefore returns with the stream synchronised; if a partner workgroup never arrives (bounded poll) it retries with
 * write-through granules and then fails with SV_ERR_HIP.  SEEVCN_FPS_MULTI=0: always one workgroup per scene; =1: write-through only. */
size_t sv_fps_multi_scratch_bytes(int batch);
int sv_stack_farthest_point_sampling_multi(const float* xyz, const int32_t* xyz_batch_start, const int32_t* xyz_batch_cnt, int batch,
                                           int max_n, int m, float* temp, void* multi_scratch, int32_t* idx, void* stream);
/* The same without the read-back (seevcn extension, for a sampling that runs on a side stream beside the backbone): ONE attempt -- write_through 0:
 * records kept in one XCD's L2 (fast, relies on the observed dispatch order), 1: write-through records (any placement) -- and nothing is
 * synchronised.  The int32 error word at multi_scratch + sv_fps_multi_error_offset(batch) is 0 when every partner workgroup arrived; the
 * caller reads it when it next synchronises with `stream` and, if non-zero, samples again with write_through = 1. */
size_t sv_fps_multi_error_offset(int batch);
int sv_stack_farthest_point_sampling_multi_async(const float* xyz, const int32_t* xyz_batch_start, const int32_t* xyz_batch_cnt, int batch, int max_n,
                                                 int m, float* temp, void* multi_scratch, int32_t* idx, int write_through, void* stream);
/* The same samples from ONE workgroup per scene that skips what a pick cannot change (seevcn extension; csrc/fps_bucket.hip): the scene's points are
 * put in Morton-cell order (64 consecutive points = one bucket with a bounding box and its largest running distance), a round re-computes only the
 * buckets whose box is nearer to the new pick than that maximum -- an exact test, IEEE rounding being monotone -- and reduces the arg-max over the
 * per-bucket maxima.  Index-exact with sv_farthest_point_sampling / sv_stack_farthest_point_sampling including the tie rule; nothing to poll, nothing
 * to read back.  Layouts: starts / counts given: stacked scenes, idx (batch, m) GLOBAL rows; both NULL: `batch` scenes of fixed_n (= max_n) points, idx
 * scene-local.  sv_fps_bucket_applies: 2048 <= max_n <= 24576 and m > 1 (SEEVCN_FPS_BUCKET=0: never; SEEVCN_FPS_BUCKET_MIN overrides the lower bound);
 * scratch: sv_fps_bucket_scratch_bytes(batch, max_n) bytes, any content. */
int sv_fps_bucket_applies(int batch, int max_n, int m);
size_t sv_fps_bucket_scratch_bytes(int batch, int max_n);
int sv_farthest_point_sampling_bucketed(const float* xyz, const int32_t* xyz_batch_start, const int32_t* xyz_batch_cnt, int batch, int fixed_n, int max_n,
                                        int m, void* scratch, int32_t* idx, void* stream);
/* Sectorized proposal-centric keypoint sampling of PV-RCNN++ and its RoI neighbour filter for a whole batch (csrc/spc_sampling.hip): three
 * launches, nothing read back.
 * sv_spc_select replaces sample_points_with_roi (backbones_3d/pfe/voxel_set_abstraction.py:45-75) and the sector expression of sector_fps (:88-90)
 * for all scenes at once: per point the nearest RoI centre by dist = sqrtf(dx*dx + dy*dy + dz*dz) (fp32, summed left to right, correctly rounded
 * sqrt; lowest RoI index among equal dist), selected iff dist < sqrtf((l/2)^2 + (w/2)^2 + (h/2)^2) + radius of THAT RoI.  rois (batch, num_rois,
 * roi_stride floats a row, [x, y, z, l, w, h, ...]); all-zero rows take part like any other, as in the reference.  sector (rows of xyz) int32:
 * -1 not selected, else floorf((atan2f(y, x) + fp32(pi)) / fp32(2 pi / num_sectors)) clamped to [0, num_sectors] (num_sectors itself: selected, in no
 * sector); the axis cases y == +-0 / x == 0 take their IEEE values whatever the device atan2f returns.  num_sectors == 0: 0 selected / -1 not (the
 * neighbour filter's mask).  max_n: the host's estimate of the largest scene, it sizes the grid only (every row of every scene is written whatever it is);
 * num_rois <= 2048, num_sectors <= 63. */
int sv_spc_select(const float* xyz, const int32_t* xyz_batch_start, const int32_t* xyz_batch_cnt, int batch, int max_n, const float* rois,
                  int num_rois, int roi_stride, float radius, int num_sectors, int32_t* sector, void* stream);
/* The per-sector masks, .sum().item() reads, quotas and host-built count tensors of sector_fps (voxel_set_abstraction.py:91-113), one workgroup per
 * scene, stable and without atomics.  order (rows of xyz) int32: the GLOBAL rows of every (scene, sector) segment in ascending row order, a scene's
 * segments inside the scene's own row range, sectors ascending, the selected rows of no sector behind them; rows of `order` outside the segments
 * are not written.  Tables of batch * num_sectors entries, scene-major: seg_start (first position in `order`), seg_cnt, seg_m = min(cnt, ceil(cnt /
 * n_sel * num_keypoints)) in float64 with n_sel = all selected rows of the scene, seg_out_start (scene b's picks start at b * (num_keypoints +
 * num_sectors), its segments follow each other); kp_cnt (batch) = the scene's sum of seg_m.  The reference's fallbacks: a scene without a selected row
 * samples its row 0 alone (segment of 1 row in that row's sector slot, quota 1 -- or slot 0 with quota num_keypoints when that row is in no sector,
 * :73, :105-108); a scene whose selected rows are all in no sector is ONE segment (slot 0) of all of them with quota num_keypoints.  xyz is read for
 * the row-0 fallback only.  num_sectors == 0 (tables of `batch` entries): seg_start / seg_cnt / kp_cnt describe the selected rows, seg_m and
 * seg_out_start are 0. */
int sv_spc_partition(const int32_t* sector, const float* xyz, const int32_t* xyz_batch_start, const int32_t* xyz_batch_cnt, int batch,
                     int num_keypoints, int num_sectors, int32_t* order, int32_t* seg_start, int32_t* seg_cnt, int32_t* seg_m,
                     int32_t* seg_out_start, int32_t* kp_cnt, void* stream);
/* stack_farthest_point_sampling_wrapper (src/sampling.cpp, kernel sampling_gpu.cu:188-319) with the segment table on the device: one workgroup per
 * segment samples seg_m[g] of the seg_cnt[g] points xyz[order[seg_start[g] + k]] (order NULL: xyz[seg_start[g] + k]) and writes their GLOBAL rows to
 * idx[seg_out_start[g] ...].  Index-exact with the reference kernel, whose reduction always runs over 1024 slots; seg_m > seg_cnt is legal (the rule
 * goes on picking once every running distance is 0).  max_n >= the largest segment (a larger one is left unwritten); temp (n_rows floats) is needed
 * when max_n > 24576, may be NULL otherwise.  A segment with seg_cnt <= 0 or seg_m <= 0, or one that does not fit n_rows / idx_len, touches no
 * memory. */
int sv_stack_farthest_point_sampling_ragged(const float* xyz, int64_t n_rows, const int32_t* order, const int32_t* seg_start, const int32_t* seg_cnt,
                                            const int32_t* seg_m, const int32_t* seg_out_start, int num_segments, int max_n, float* temp, int32_t* idx,
                                            int64_t idx_len, void* stream);
/* ball_query_wrapper(B, M, radius, nsample, new_xyz, new_xyz_batch_cnt, xyz, xyz_batch_cnt, idx) (src/ball_query.cpp:31-47,
 * kernel ball_query_gpu.cu:16-66): idx (M,nsample) scene-local indices of the first nsample points with d^2 < r^2 in index
 * order, padded with the first hit; idx[m][0] = -1 for an empty ball. */
int sv_ball_query_stack(int batch, int M, int max_queries_per_scene, float radius, int nsample, const float* new_xyz,
                        const int32_t* new_xyz_batch_start, const int32_t* new_xyz_batch_cnt, const float* xyz,
                        const int32_t* xyz_batch_start, const int32_t* xyz_batch_cnt, int32_t* idx, void* stream);
/* The same result, element for element, over a cell hash of the support points instead of the reference's scan of the whole scene per query
 * (seevcn extension): cells of edge radius * 1.0001 counting-sorted into hash buckets, a wave per query tests the candidates of the 27 cells
 * around it with the reference's own distance expression and writes the nsample smallest indices in ascending order.  n_points = rows of xyz;
 * scratch: sv_ball_query_hash_scratch_bytes(n_points) bytes (any content); nsample <= 64. */
size_t sv_ball_query_hash_scratch_bytes(int64_t n_points);
int sv_ball_query_stack_hashed(int batch, int M, int64_t n_points, float radius, int nsample, const float* new_xyz, const int32_t* new_xyz_batch_start,
                               const int32_t* new_xyz_batch_cnt, const float* xyz, const int32_t* xyz_batch_start, const int32_t* xyz_batch_cnt,
                               void* scratch, int32_t* idx, void* stream);
/* ---- fused set-abstraction reduction, eval mode (csrc/set_abstraction.hip): the tail of StackSAModuleMSG.forward
 * (ops/pointnet2/pointnet2_stack/pointnet2_modules.py:78-112) for one radius scale -- QueryAndGroup's gather (xyz relative to the query in
 * front of the features, an empty ball = zeros; pointnet2_utils.py:112-159) -> two Conv2d 1x1 + BatchNorm2d(eval) + ReLU -> max over nsample --
 * without the (M, C+3, nsample) tensor.  idx / row_start as for sv_group_points_stack (raw ball-query output).
 * sv_sa_prepare_weights folds an eval-mode BatchNorm into a conv weight (c_out, c_in): xyz_first = 1 for the first layer (c_in = 3 + C, C a
 * multiple of 16: output (c_out, 16*(C/16+1)) = [features | xyz | zeros]), 0 for the second (same shape); b_out (c_out).
 * sv_sa_mlp_max: C <= 128 features (multiple of 16, 0 = xyz only), nsample 16 or 32, C1 / C2 in {16, 32, 48, 64}; out (M, C2). */
int sv_sa_prepare_weights(const float* weight, const float* bn_weight, const float* bn_bias, const float* running_mean,
                          const float* running_var, float eps, int c_out, int c_in, int xyz_first, float* w_out, float* b_out, void* stream);
int sv_sa_mlp_max(const float* xyz, const float* features, const float* new_xyz, const int32_t* idx, const int32_t* row_start, int64_t M, int C,
                  int nsample, const float* w1, const float* b1, int C1, const float* w2, const float* b2, int C2, float* out, void* stream);
/* ---- set abstraction, TRAINING mode (csrc/set_abstraction_train.hip): one radius scale of StackSAModuleMSG.forward
 * (pointnet2_modules.py:78-112) with batch-statistics BatchNorm2d, and its backward, as chains of persistent MFMA launches over 16-row tiles;
 * no (M, C+3, nsample) tensor, no library GEMM.  Same operands as sv_sa_mlp_max, weights in the PARAMETER layouts: w1 (C1, 3 + C) with the xyz
 * columns first (QueryAndGroup's concatenation order, pointnet2_utils.py:147-152), w2 (C2, C1); gamma / beta / running_* / tracked = the two
 * nn.BatchNorm2d's weight, bias, running_mean, running_var, num_batches_tracked (updated like torch: biased variance to normalise, unbiased
 * into running_var).  R = M * nsample rows.
 * forward:  N = rows of xyz / features; proj (N, C1) is a work buffer (null when C == 0: the feature part of layer 1, made once per support
 *           point).  Writes z1 (R, C1), z2 (R, C2) [pre-BatchNorm activations, kept for the backward], save_mean* / save_invstd*, sel (M, C2) = the z2
 *           that makes each output, arg (M, C2) = its slot, out (M, C2); aux (M, C2) floats and aux_arg (M, C2) bytes are work buffers.
 * backward: grad_out (M, C2) -> grad_w1 (C1, 3 + C), grad_w2 (C2, C1), dgamma* / dbeta*, scatter (N, C1) = per support point the sum of dz1 over
 *           its (query, slot) pairs (zero-filled here; fp32 atomics like group_points_grad_kernel_stack, group_points_gpu.cu:38-41).  The
 *           feature gradient is linear in the gathered row: grad_features (N, C) = scatter . w1[:, 3:] (null when not wanted or C == 0).
 *           dy1 (R, C1) and aux (M, C2) are work buffers.
 * scratch: sv_sa_train_scratch_bytes(C, C1, C2) bytes, not shared between a forward and a backward in flight on different streams. */
size_t sv_sa_train_scratch_bytes(int C, int C1, int C2);
int sv_sa_train_forward(const float* xyz, const float* features, const float* new_xyz, const int32_t* idx, const int32_t* row_start, int64_t M,
                        int64_t N, int C, int nsample, const float* w1, const float* gamma1, const float* beta1, float* running_mean1, float* running_var1,
                        int64_t* tracked1, int C1, const float* w2, const float* gamma2, const float* beta2, float* running_mean2,
                        float* running_var2, int64_t* tracked2, int C2, float momentum, float eps, void* scratch, float* proj, float* z1,
                        float* z2,
                        float* save_mean1, float* save_invstd1, float* save_mean2, float* save_invstd2, float* sel, float* aux, uint8_t* arg,
                        uint8_t* aux_arg, float* out, void* stream);
int sv_sa_train_backward(const float* xyz, const float* features, const float* new_xyz, const int32_t* idx, const int32_t* row_start, int64_t M,
                         int64_t N, int C, int nsample, const float* w1, const float* gamma1, const float* beta1, int C1, const float* w2,
                         const float* gamma2, const float* beta2, int C2, const float* z1, const float* z2, const float* save_mean1,
                         const float* save_invstd1, const float* save_mean2, const float* save_invstd2, const float* sel, const uint8_t* arg,
                         const float* out, const float* grad_out, void* scratch, float* dy1, float* aux, float* scatter, float* grad_features,
                         float* grad_w1, float* grad_w2, float* dgamma1, float* dbeta1, float* dgamma2, float* dbeta2, void* stream);
/* sv_sa_train_backward with an order-fixed scatter (opt-in; replaces the atomicAdd scatter of group_points_grad_kernel_stack,
 * group_points_gpu.cu:38-41, inside the autograd chain behind pointnet2_modules.py:96-110).  Same arguments and the same launches, except:
 * the layer-1 launch scatters nothing, and scatter (N, C1) is then written once per element, without float atomics and without a zero-fill, as
 *   scatter[n][c] = +0.0f + dz1[q * nsample + slot][c]   summed in ascending key q * nsample + slot
 * over the slots of non-empty balls (idx[q][0] >= 0) with row_start[q] + idx[q][slot] == n; a point no key names is +0.0f.
 * dz1[row][c] = fmaf(k[c], dy1[row][c], fmaf(A[c], z1[row][c], B[c])) with the layer-1 launch's own coefficients: after the call the first
 * 4 * C1 floats of scratch hold {k, md, mx, mean} per channel, and A = -k * mx * save_invstd1, B = k * (mx * save_invstd1 * mean - md), every
 * product and sum rounded to fp32.  Weight, BatchNorm and feature gradients come from the unchanged launches, which sum in a fixed order.
 * scratch: sv_sa_train_backward_ordered_scratch_bytes bytes = the ordinary scratch followed by int32 key counts and segments per support point
 * and twice the M * nsample keys; needs M * nsample < 2^31 and N < 2^31 (else an error, never the atomic route). */
size_t sv_sa_train_backward_ordered_scratch_bytes(int64_t M, int64_t N, int C, int nsample, int C1, int C2);
int sv_sa_train_backward_ordered(const float* xyz, const float* features, const float* new_xyz, const int32_t* idx, const int32_t* row_start,
                                 int64_t M, int64_t N, int C, int nsample, const float* w1, const float* gamma1, const float* beta1, int C1,
                                 const float* w2, const float* gamma2, const float* beta2, int C2, const float* z1, const float* z2,
                                 const float* save_mean1, const float* save_invstd1, const float* save_mean2, const float* save_invstd2,
                                 const float* sel, const uint8_t* arg, const float* out, const float* grad_out, void* scratch, float* dy1,
                                 float* aux, float* scatter, float* grad_features, float* grad_w1, float* grad_w2, float* dgamma1, float* dbeta1,
                                 float* dgamma2, float* dbeta2, void* stream);
/* group_points_wrapper / group_points_grad_wrapper (src/group_points.cpp:31-69, kernels group_points_gpu.cu:15-102):
 * out (M,C,nsample)[m][c][s] = features[row_start[m] + idx[m][s]][c]; row_start[m] = first feature row of query m's scene.
 * The gradient zero-fills grad_features (N,C) and scatter-adds with fp32 atomics like the reference. */
int sv_group_points_stack(int M, int C, int nsample, const float* features, const int32_t* idx, const int32_t* row_start,
                          float* out, void* stream);
int sv_group_points_grad_stack(int M, int C, int N, int nsample, const float* grad_out, const int32_t* idx,
                               const int32_t* row_start, float* grad_features, void* stream);
/* group_points_grad_wrapper (src/group_points.cpp:52-69, kernel group_points_gpu.cu:15-45) with a fixed summation order (opt-in): no float
 * atomics, no zero-fill, every element of grad_features (N,C) written once as
 *   grad_features[n][c] = +0.0f + grad_out[m][c][s]   summed in ascending key m * nsample + s
 * over the pairs with row_start[m] + idx[m][s] == n, every sum rounded to fp32.  Slots that repeat the first neighbour are keys like any other;
 * a slot with a negative idx (the empty-ball mark) or a row outside [0, N) names nothing; a row no key names is +0.0f.
 * scratch: sv_group_points_grad_stack_ordered_scratch_bytes bytes (uninitialised): int32 key counts and segments per row and twice the
 * M * nsample keys; needs M * nsample < 2^31 (else an error, never the atomic route). */
size_t sv_group_points_grad_stack_ordered_scratch_bytes(int M, int N, int nsample);
int sv_group_points_grad_stack_ordered(int M, int C, int N, int nsample, const float* grad_out, const int32_t* idx, const int32_t* row_start,
                                       void* scratch, float* grad_features, void* stream);

/* ---- PV-RCNN++'s vector-pool local aggregation (csrc/vector_pool.hip).  Stacked batches as for sv_ball_query_stack: per-scene start and
 * count arrays for the queries (M rows in all) and the support points (N rows in all); max_queries_per_scene may be any upper bound (M).
 * Nothing is sized on the host, read back or retried (the reference's Python wrappers re-run their kernels in a `while True` loop with a
 * larger buffer, pointnet2_utils.py:331-347, 399-415).
 *
 * sv_vector_pool_choice: vector_pool_kernel_stack with pooling_type == 1, `voxel_random_choice` (src/vector_pool_gpu.cu:243-373, launcher
 * :376-430).  Per query, walk its scene in ascending row order; local = p - q in fp32; a row is in range unless any |local| > R (cube) or
 * lx^2 + ly^2 + lz^2 > R * R (neighbor_type == 1, ball); its cell is ix * ny * nz + iy * nz + iz with i = floorf((local + R) / gs),
 * gs = R * 2 / n in fp32, THEN clamped to [0, G - 1] (so a row at local == +R aliases, as in the reference); an in-range row whose cell is
 * still empty is taken; the walk ends after nsample taken rows (nsample > 0) or G.  G = nx * ny * nz <= 512.
 * Writes every element of: choice (M, G) global support row or -1; point_cnt (M, G) in {0, 1}; new_local_xyz (M, 3 G) the taken row's
 * local, zeros for an empty cell; new_features (M, G * c_each): channel j of a cell = features[row][c_in - c_each + j] (the reference's
 * `i % c_each` overwrite: the last channel group wins), zeros for an empty cell.  These are final: the reference's division by
 * clamp_min(cnt, 1e-6) divides by 1 or yields 0. */
int sv_vector_pool_choice(int batch, int M, int N, int max_queries_per_scene, const float* new_xyz, const int32_t* new_xyz_batch_start,
                          const int32_t* new_xyz_batch_cnt, const float* xyz, const float* features, const int32_t* xyz_batch_start,
                          const int32_t* xyz_batch_cnt, int c_in, int c_each, int nx, int ny, int nz, float max_neighbour_distance,
                          int nsample, int neighbor_type, int32_t* choice, int32_t* point_cnt, float* new_local_xyz, float* new_features,
                          void* stream);
/* vector_pool_grad_kernel_stack (src/vector_pool_gpu.cu:433-458) over choice instead of grouped_idxs: for every c < c_in
 *   grad_support[choice[m][g]][c] += grad_new[m][g * c_each + c % c_each] * (1 / max(cnt[m][g], 1))
 * (every input channel group receives the gradient).  The plain entry zero-fills grad_support (N, c_in) and adds with fp32 atomics; the
 * ordered entry (opt-in) writes every element once, +0.0f + the terms in ascending key m * G + g, every sum rounded to fp32, no float
 * atomics; scratch: sv_vector_pool_choice_grad_ordered_scratch_bytes bytes (uninitialised), needs M * G < 2^31. */
int sv_vector_pool_choice_grad(int M, int N, int G, int c_in, int c_each, const float* grad_new, const int32_t* choice,
                               const int32_t* point_cnt, float* grad_support, void* stream);
size_t sv_vector_pool_choice_grad_ordered_scratch_bytes(int M, int N, int G);
int sv_vector_pool_choice_grad_ordered(int M, int N, int G, int c_in, int c_each, const float* grad_new, const int32_t* choice,
                                       const int32_t* point_cnt, void* scratch, float* grad_support, void* stream);
/* `local_interpolation`: query_stacked_local_neighbor_idxs_kernel + query_three_nn_by_stacked_local_idxs_kernel (src/vector_pool_gpu.cu:122-205,
 * 19-86) in one launch, without stack_neighbor_idxs / start_len / cumsum.  A query's list = the first min(1000, nsample if nsample > 0) rows
 * of its scene, ascending, that pass the rejection test above with R = max_neighbour_distance (the caller passes distance * multiplier).  Per
 * grid centre (new_xyz_grid_centers (M, G, 3)): the three list entries smallest under (d, position in list), d = (cx-x)^2 + (cy-y)^2 + (cz-z)^2
 * in fp32.  idx (M, G, 3) global rows, dist2 (M, G, 3); one entry found: slots 2 and 3 repeat slot 1; two: slot 3 repeats slot 1; none:
 * idx = -1, dist2 = +inf. */
int sv_vector_pool_three_nn(int batch, int M, int N, int max_queries_per_scene, const float* new_xyz, const float* new_xyz_grid_centers,
                            const int32_t* new_xyz_batch_start, const int32_t* new_xyz_batch_cnt, const float* xyz,
                            const int32_t* xyz_batch_start, const int32_t* xyz_batch_cnt, int num_total_grids, float max_neighbour_distance,
                            int nsample, int neighbor_type, int32_t* idx, float* dist2, void* stream);
/* three_interpolate_kernel_stack / three_interpolate_grad_kernel_stack (src/interpolate_gpu.cu:107-126, 151-172): features (n_features, C),
 * idx / weight (rows, 3) -> out (rows, C) = w0 * f[i0] + w1 * f[i1] + w2 * f[i2], three rounded products summed left to right.  The plain
 * gradient zero-fills grad_features (n_features, C) and adds fp32(grad_out[r][c] * w[r][t]) with fp32 atomics; the ordered entry (opt-in) sums
 * the same terms from +0.0f in ascending key 3 r + t and writes every element once (scratch: ..._ordered_scratch_bytes, 3 * rows < 2^31).
 * An index outside [0, n_features) contributes nothing anywhere. */
int sv_three_interpolate_stack(int rows, int C, int n_features, const float* features, const int32_t* idx, const float* weight, float* out,
                               void* stream);
int sv_three_interpolate_grad_stack(int rows, int C, int n_features, const float* grad_out, const int32_t* idx, const float* weight,
                                    float* grad_features, void* stream);
size_t sv_three_interpolate_grad_stack_ordered_scratch_bytes(int rows, int n_features);
int sv_three_interpolate_grad_stack_ordered(int rows, int C, int n_features, const float* grad_out, const int32_t* idx, const float* weight,
                                            void* scratch, float* grad_features, void* stream);

/* ---- Voxel R-CNN's voxel RoI pooling (csrc/voxel_pool.hip).
 * generate_voxel2pinds / scatter_point_inds (detector3d/pcdet/utils/common_utils.py:235-252): volume (B, Z, Y, X) int32 = -1 everywhere and r at
 * [b, z, y, x] of row r of coords (N, 4), offsets in 64 bits (the volume may hold 2^31 cells or more); a row outside the volume writes nothing.
 * fill = 1 sets the whole volume to -1 first.  clear = 1 writes -1 where it would write r: with fill = 0 the same N-row scatter returns a
 * volume that was all -1 on entry to all -1 (a persistent volume costs two N-row scatters a call and no pass over its cells). */
int sv_voxel2pinds(const int32_t* coords, int64_t N, int B, int Z, int Y, int X, int fill, int clear, int32_t* volume, void* stream);
/* voxel_query_wrapper (pointnet2_stack/src/voxel_query.cpp, kernel voxel_query_gpu.cu:10-89), element for element: for query m with cell
 * new_coords[m] = [b, z, y, x] the window z - z_range .. z + z_range (outermost), y, x (innermost) of point_indices (B, R1, R2, R3) is walked,
 * cells outside the volume and cells holding -1 are passed over, a neighbour row j is kept unless
 *   (xyz[j].x - new_xyz[m].x)^2 + (.y)^2 + (.z)^2 > radius * radius     (each product and sum rounded to fp32, this operand order)
 * and the first nsample kept rows fill idx[m][0..]; the first kept row also fills every slot behind the last kept one; a query that keeps
 * nothing gets idx[m][0] = -1 and its other slots stay as the caller left them.  One wave per query, 64 cells of the clipped window per pass.
 * Beyond the reference: a query whose b is outside [0, B) keeps nothing, and a cell value >= n_points (the rows of xyz) is passed over.
 * Window extents up to 1024 each. */
int sv_voxel_query_stack(int M, int B, int R1, int R2, int R3, int64_t n_points, int nsample, float radius, int z_range, int y_range, int x_range,
                         const float* new_xyz, const float* xyz, const int32_t* new_coords, const int32_t* point_indices, int32_t* idx,
                         void* stream);
/* The eval-mode tail of one scale of NeighborVoxelSAModuleMSG.forward (pointnet2_stack/voxel_pool_modules.py:96-120, max_pool) without the
 * grouped (M, C1, nsample) and (M, 3, nsample) tensors:
 *   out[m][c] = max_s ReLU(f_in[idx[m][s]][c] + wp[c] . (xyz[idx[m][s]] - new_xyz[m]) + bp[c])
 * f_in (N, C1) = mlps_in applied to the support voxels, wp (C1, 3) / bp (C1) = mlps_pos with its eval-mode BatchNorm2d folded in, idx (M, nsample)
 * GLOBAL rows as sv_voxel_query_stack leaves them; a query with idx[m][0] < 0 gives ReLU(bp[c]) (the reference zeroes both grouped tensors of an
 * empty query).  C1 in {16, 32, 48, 64}, nsample <= 32; f_in, bp, out 16-byte aligned. */
int sv_voxel_pool_max(const float* f_in, const float* xyz, const float* new_xyz, const int32_t* idx, const float* wp, const float* bp, int64_t M,
                      int64_t N, int C1, int nsample, float* out, void* stream);

/* ---- Part-A2's RoI-aware point feature pooling (csrc/roiaware_pool.hip).  Every entry refuses null and host pointers, out sizes above 255
 * (the reference packs a cell into 3 x 8 bits and silently corrupts beyond), more than 4096 cells per box and max_pts_each_voxel < 2;
 * n_boxes == 0 and n_pts == 0 return cleanly.
 * generate_pts_mask_for_box3d + collect_inside_pts_for_box3d (detector3d/pcdet/ops/roiaware_pool3d/src/roiaware_pool3d_kernel.cu:39-108) without
 * the (boxes x points) mask and without one thread walking every point of the scene: pts_idx_of_voxels (n_boxes, out_x, out_y, out_z,
 * max_pts_each_voxel) int32, slot 0 of a cell = its count (at most max_pts_each_voxel - 1), slots 1..count = the rows of pts (n_pts, 3) inside
 * box rois[box] (7 floats) that fall into the cell, in ASCENDING row order, the later ones dropped.  The in-box test is the reference's (:16-36,
 * the one sv_points_in_boxes uses), the cell is int((local + d / 2) / (d / out)) per axis in fp32, clamped to the grid.  box_pt_range (n_boxes, 2)
 * int32 device, or NULL: box b looks at rows [lo, hi) only (clipped to [0, n_pts)) -- the rows of its scene, so that the boxes of every scene of
 * a batch are assigned in one launch; the stored rows are absolute.  Every count is written, so the tensor needs no zero-fill; slots behind a
 * count are left as they were and nothing reads them. */
int sv_roiaware_assign(const float* rois, int n_boxes, const float* pts, int n_pts, const int32_t* box_pt_range, int out_x, int out_y, int out_z,
                       int max_pts_each_voxel, int32_t* pts_idx_of_voxels, void* stream);
/* roiaware_maxpool3d / roiaware_avgpool3d (roiaware_pool3d_kernel.cu:111-190) over lists that sv_roiaware_assign left; cells = out_x * out_y *
 * out_z.  pool_method 0 = max: pooled (n_boxes, cells, C) = the largest feature of the listed rows, strict > in list order (the first row of
 * the largest value wins), argmax (n_boxes, cells, C) int32 = that row; an empty cell is 0 and -1.  pool_method 1 = avg: the fp32 sum in list
 * order over the count, an empty cell is 0; argmax may be NULL.  Every element of pooled (and argmax) is written. */
int sv_roiaware_pool(const float* pts_feature, int C, const int32_t* pts_idx_of_voxels, int n_boxes, int cells, int max_pts_each_voxel,
                     int pool_method, float* pooled, int32_t* argmax, void* stream);
/* roiaware_maxpool3d_backward / roiaware_avgpool3d_backward (roiaware_pool3d_kernel.cu:236-286): grad_in (n_pts, C) is zero-filled, then
 * max: grad_in[argmax] += grad_out; avg: grad_in[p] += grad_out / max(count, 1) for every listed row p -- with fp32 atomics like the reference. */
int sv_roiaware_pool_backward(const int32_t* pts_idx_of_voxels, const int32_t* argmax, const float* grad_out, int n_boxes, int cells, int C,
                              int max_pts_each_voxel, int pool_method, int n_pts, float* grad_in, void* stream);
/* The same gradient with a fixed summation order (opt-in): no float atomics, no zero-fill, every element of grad_in written once as
 * +0.0f + its contributions in ascending (box, cell) order, every sum rounded to fp32.  scratch: sv_roiaware_pool_backward_ordered_scratch_bytes
 * bytes (uninitialised) -- the inverse lists over the key space n_boxes * cells * C (max) or n_boxes * cells * max_pts_each_voxel (avg), which
 * must stay below 2^31 (else 0 bytes and an error, never the atomic route). */
size_t sv_roiaware_pool_backward_ordered_scratch_bytes(int n_boxes, int cells, int C, int max_pts_each_voxel, int pool_method, int n_pts);
int sv_roiaware_pool_backward_ordered(const int32_t* pts_idx_of_voxels, const int32_t* argmax, const float* grad_out, int n_boxes, int cells, int C,
                                      int max_pts_each_voxel, int pool_method, int n_pts, void* scratch, float* grad_in, void* stream);

/* ---- PointRCNN's RoI point pooling (csrc/roipoint_pool.hip; detector3d/pcdet/ops/roipoint_pool3d/src/roipoint_pool3d_kernel.cu:38-165) in ONE
 * launch, without the reference's (B, N, M) table and its one-thread-per-box walk.  xyz (B, N, 3), pts_feature (B, N, C), boxes3d (B, M, 7)
 * already enlarged by the caller; pooled (B, M, S, 3 + C), empty_flag (B, M) int32, S = n_sampled.  The list of box (b, m) is the rows of scene b
 * that pass the in-box test (the one sv_points_in_boxes uses), ascending, cut after S; cnt == 0: flag 1 and S rows of zeros; 0 < cnt < S: slot
 * k >= cnt repeats slot k % cnt; row s = [xyz[b, list[s]] | pts_feature[b, list[s]]].  EVERY element of pooled and empty_flag is written (the
 * reference relies on zero-filled outputs).  canonical = 1 (seevcn extension): the three xyz columns hold the point in the box's frame instead,
 * (lx, ly) of the in-box test and z - cz in fp32 -- rotate_points_along_z(p - centre, -heading) of pointrcnn_head.py:121-128, fused.
 * batch == 0, n_boxes == 0, n_pts == 0 (every box empty) and C == 0 (rows of xyz only) return cleanly; n_sampled outside 1..4096, a negative
 * size, a null or a host pointer is an error. */
int sv_roipoint_pool3d(const float* xyz, const float* pts_feature, const float* boxes3d, int batch, int n_pts, int n_boxes, int C, int n_sampled,
                       int canonical, float* pooled, int32_t* empty_flag, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Rotated-box geometry (detector3d/pcdet/ops/iou3d_nms/src/iou3d_nms_api.cpp:12-17,
 * detector3d/pcdet/ops/roiaware_pool3d/src/roiaware_pool3d.cpp:172-177). Boxes are (N,7) fp32 [x,y,z,dx,dy,dz,heading].
 * ---------------------------------------------------------------------------------------------- */
/* boxes_overlap_bev_gpu (iou=0) / boxes_iou_bev_gpu (iou=1): out (num_a, num_b) */
int sv_boxes_overlap_bev(const float* boxes_a, int num_a, const float* boxes_b, int num_b, float* out, int iou, void* stream);
/* boxes_iou3d_gpu (detector3d/pcdet/ops/iou3d_nms/iou3d_nms_utils.py:48-81: BEV overlap x height overlap / union volume, the elementwise chain
 * around boxes_overlap_bev_gpu) in ONE launch, for `batch` independent box sets at once: boxes_a (batch, num_a, stride_a), boxes_b (batch, num_b,
 * stride_b) rows whose first 7 floats are the box, out (batch, num_a, num_b). */
int sv_boxes_iou3d_batch(const float* boxes_a, int num_a, int stride_a, const float* boxes_b, int num_b, int stride_b, int batch, float* out,
                         void* stream);
/* nms_gpu (normal=0, rotated BEV IoU) / nms_normal_gpu (normal=1, axis-aligned) over boxes ALREADY sorted by score:
 * keep (n) int64 device indices of the kept boxes in order, *num_out device int32.  Unlike the reference
 * (iou3d_nms.cpp:111-131: D2H copy of the mask + host sweep) the greedy sweep runs on the device. n <= 65536. */
size_t sv_nms_scratch_bytes(int n);
int sv_nms(const float* boxes, int n, float thresh, int normal, void* scratch, int64_t* keep, int32_t* num_out, void* stream);
/* The same, stopping once max_keep boxes are kept: keep[0..*num_out) is the prefix sv_nms would return, *num_out = min(kept, max_keep)
 * (seevcn extension for callers that truncate to NMS_POST_MAXSIZE, model_nms_utils.py:21). */
int sv_nms_prefix(const float* boxes, int n, float thresh, int normal, int max_keep, void* scratch, int64_t* keep, int32_t* num_out, void* stream);
/* Class-wise NMS of a whole batch (multi_classes_nms, detector3d/pcdet/models/model_utils/model_nms_utils.py:28-66: one NMS per scene x head x
 * class) as ONE launch pair: `num_segments` independent box sets, segment s = rows [0, seg_count[s]) of boxes[s] (seg_stride rows of 7 floats,
 * already in descending score order); rows at or beyond seg_count[s] are padding, never read.  For every segment the result is
 * sv_nms_prefix(boxes[s], seg_count[s], thresh, normal, max_keep): keep[s] (max_keep slots) holds indices LOCAL to the segment in score order,
 * num_out[s] = min(survivors, max_keep).  seg_count and num_out are DEVICE arrays; no count is read on the host.  seg_stride <= 4096,
 * num_segments <= 65535.  scratch: num_segments * seg_stride * ceil(seg_stride / 64) * 8 bytes (the suppression mask words). */
size_t sv_nms_segments_scratch_bytes(int num_segments, int seg_stride);
int sv_nms_segments(const float* boxes, const int32_t* seg_count, int num_segments, int seg_stride, float thresh, int normal, int max_keep,
                    void* scratch, int64_t* keep, int32_t* num_out, void* stream);
/* points_in_boxes_gpu: boxes (B,T,7), pts (B,M,3) -> out (B,M) int32 index of the first box containing the point or -1 */
int sv_points_in_boxes(const float* boxes, const float* pts, int batch, int num_boxes, int num_points, int32_t* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Anchor head (detector3d/pcdet/models/dense_heads/anchor_head_template.py, target_assigner/axis_aligned_target_assigner.py)
 * ---------------------------------------------------------------------------------------------- */
/* generate_predicted_boxes (anchor_head_template.py:225-272) with ResidualCoder.decode_torch (box_coder_utils.py:48-77):
 * anchors (A,7) shared by the batch, box_encodings (B,A,7), dir_cls_preds (B,A,num_dir_bins) or NULL -> out (B,A,7). */
int sv_anchor_decode(const float* anchors, int64_t num_anchors, const float* box_encodings, const float* dir_cls_preds,
                     int batch, int num_dir_bins, float dir_offset, float dir_limit_offset, float* out, void* stream);
/* AxisAlignedTargetAssigner.assign_targets (axis_aligned_target_assigner.py:36-210), deterministic branch (POS_FRACTION < 0,
 * MATCH_HEIGHT False, NORM_BY_NUM_EXAMPLES False): anchors (A,7) in head order [(z,y,x), set, size, rot]; set s owns the
 * per-location slots [set_offset[s], set_offset[s+1]) and matches ground truth whose class id (column 7, 1-based) is
 * set_class[s]; gt_boxes (B,G,8) zero-padded.  Outputs labels (B,A) int32 {-1 ignore, 0 background, class id},
 * reg_targets (B,A,7) (ResidualCoder.encode_torch), reg_weights (B,A).  gt_max_scratch: B*G floats.  G <= 128.
 * set_offset/set_class/thresholds are DEVICE arrays. */
int sv_assign_targets_axis_aligned(const float* anchors, int64_t num_anchors, int anchors_per_location, int num_sets,
                                   const int32_t* set_offset, const int32_t* set_class, const float* matched_thr,
                                   const float* unmatched_thr, const float* gt_boxes, int batch, int max_gt, float* gt_max_scratch,
                                   int32_t* labels, float* reg_targets, float* reg_weights, void* stream);
/* The same two for coded boxes and head-major anchors (AnchorHeadMulti; ResidualCoder with code_size 7 + E and encode_angle_by_sincos):
 * anchors (A, 7+E), box_encodings (B, A, 7+sincos+E) -> out (B, A, 7+E).  sincos = 1: heading = atan2(t[7] + sin(ra), t[6] + cos(ra));
 * extras = t + anchor extras.  dir_cls_preds may be NULL (no direction classifier).  E = 0, sincos = 0 gives sv_anchor_decode's bits. */
int sv_anchor_decode_coded(const float* anchors, int64_t num_anchors, int num_extra, int sincos, const float* box_encodings,
                           const float* dir_cls_preds, int batch, int num_dir_bins, float dir_offset, float dir_limit_offset, float* out,
                           void* stream);
/* anchors (A, 7+E); gt_boxes (B, G, 8+E) [box7, extras, class] zero-padded; reg_targets (B, A, 7+sincos+E) (encode_torch: sincos = 1 codes the
 * heading as cos(rg) - cos(ra), sin(rg) - sin(ra); extras gt - anchor).  set_major = 0: anchors in sv_assign_targets_axis_aligned's order,
 * set_offset = prefix of slots per location.  set_major = 1: the multihead order (axis_aligned_target_assigner.py:69), every set's anchors one
 * contiguous run [size, rot, z, y, x], runs concatenated set by set, set_offset = prefix of ANCHORS per set (anchors_per_location unused).
 * G <= 256, A < 2^31.  E = 0, sincos = 0, set_major = 0 gives sv_assign_targets_axis_aligned's bits. */
int sv_assign_targets_axis_aligned_coded(const float* anchors, int64_t num_anchors, int num_extra, int sincos, int set_major,
                                         int anchors_per_location, int num_sets, const int32_t* set_offset, const int32_t* set_class,
                                         const float* matched_thr, const float* unmatched_thr, const float* gt_boxes, int batch, int max_gt,
                                         float* gt_max_scratch, int32_t* labels, float* reg_targets, float* reg_weights, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Hard voxelisation + pillar features (PointPillars path)
 * ---------------------------------------------------------------------------------------------- */
/* spconv VoxelGenerator(V2) / Point2VoxelCPU3d semantics as called by DataProcessor.transform_points_to_voxels
 * (detector3d/pcdet/datasets/processor/data_processor.py:15-60,115-143): first-come points per voxel (<= max_points),
 * voxels numbered in order of first appearance (<= max_voxels).  One workgroup per scene.
 * points rows of point_stride floats, x at column xyz_offset, num_features columns copied from there;
 * scenes given by device arrays scene_start/scene_cnt.  Outputs per scene: voxels (B,max_voxels,max_points,C) zero-padded,
 * coords (B,max_voxels,3) [z,y,x], num_points_per_voxel (B,max_voxels), num_voxels (B). */
size_t sv_voxelize_hard_scratch_bytes(int batch, int64_t total_points, int max_scene_points);
int sv_voxelize_hard(const float* points, int point_stride, int xyz_offset, int num_features, const int32_t* scene_start,
                     const int32_t* scene_cnt, int batch, int64_t total_points, int max_scene_points,
                     const float* pc_range_host, const float* voxel_size_host, const int32_t* grid_size_host, int max_points,
                     int max_voxels, void* scratch, float* voxels, int32_t* coords, int32_t* num_points_per_voxel,
                     int32_t* num_voxels, void* stream);
/* PillarVFE.forward feature decoration (backbones_3d/vfe/pillar_vfe.py:94-118): (V,mp,C) -> (V,mp,C+6[+1]).  voxel_size_host (3) and
 * pc_range_host (>= 3) are the configured values as doubles: the pillar-centre offsets voxel/2 + range start are formed in double, as the
 * reference's python does, and rounded to fp32 once. */
int sv_pillar_decorate(const float* voxels, const int32_t* num_points, const int32_t* coords, int64_t num_voxels, int max_points,
                       int num_features, const double* voxel_size_host, const double* pc_range_host, int use_absolute_xyz,
                       int with_distance, float* out, void* stream);

/* interpolate_from_bev_features (detector3d/pcdet/models/backbones_3d/pfe/voxel_set_abstraction.py:11-42,176-204):
 * keypoints (M,4) [b,x,y,z], bev (B,C,H,W) -> out (M,C); the gradient scatter-adds the taps into a channel-last staging map (scratch:
 * sv_bev_interpolate_grad_scratch_bytes bytes; a tap is then one contiguous run of C floats for the float atomics) and transposes it into
 * grad_bev (B,C,H,W), every element written. */
int sv_bev_interpolate(const float* keypoints, int64_t num_keypoints, const float* bev, int batch, int C, int H, int W, float x_min,
                       float y_min, float voxel_x, float voxel_y, float bev_stride, float* out, void* stream);
size_t sv_bev_interpolate_grad_scratch_bytes(int batch, int C, int H, int W);
int sv_bev_interpolate_grad(const float* keypoints, int64_t num_keypoints, const float* grad_out, int batch, int C, int H, int W,
                            float x_min, float y_min, float voxel_x, float voxel_y, float bev_stride, void* scratch, float* grad_bev, void* stream);
/* The same pair on a channel-last map: bev and grad_bev are (B,H,W,C), the storage of a channels_last (B,C,H,W) tensor; out and grad_out stay
 * (M,C).  Forward: per element the expression of sv_bev_interpolate, so the bits equal its result on the permuted map; rows with a batch index
 * outside [0, B) give zeros.  16-byte accesses along C when C % 4 == 0 and the pointers are 16-byte aligned, else one float a lane.
 * Gradient: no float atomics and a fixed order.  grad_bev[pixel, c] = +0.0f + grad_out[m, c] * w_t summed in ascending key 4 * m + t over the
 * taps that land on the pixel (t = 0..3: the taps y0x0, y1x0, y0x1, y1x1 of keypoint m; two taps of one keypoint clamped onto one pixel are two
 * terms), every product and every sum rounded to fp32; a pixel without taps is +0.0f.  Every element is written exactly once, the map is never
 * cleared or copied.  scratch (sv_bev_interpolate_grad_nhwc_scratch_bytes bytes, uninitialised), int32 words: allocator (4) | tap counts
 * (B*H*W) | key-list segments (B*H*W) | the 4 * M keys in arrival order | the 4 * M keys, every pixel's ascending; needs B*H*W < 2^31 and
 * M < 2^29.  M == 0 writes the zero map and reads no scratch. */
int sv_bev_interpolate_nhwc(const float* keypoints, int64_t num_keypoints, const float* bev, int batch, int C, int H, int W, float x_min,
                            float y_min, float voxel_x, float voxel_y, float bev_stride, float* out, void* stream);
size_t sv_bev_interpolate_grad_nhwc_scratch_bytes(int64_t num_keypoints, int batch, int H, int W);
int sv_bev_interpolate_grad_nhwc(const float* keypoints, int64_t num_keypoints, const float* grad_out, int batch, int C, int H, int W,
                                 float x_min, float y_min, float voxel_x, float voxel_y, float bev_stride, void* scratch, float* grad_bev,
                                 void* stream);

/* SigmoidFocalClassificationLoss.forward (detector3d/pcdet/utils/loss_utils.py:9-72: alpha-balanced sigmoid focal loss, un-reduced) and its
 * derivative w.r.t. the logits, one launch each instead of ~20 / ~30 elementwise ones.  input, target (n_rows, num_class), weights (n_rows) or
 * NULL.  grad_out NULL: out = loss (n_rows, num_class); grad_out given: out = grad_out * d loss / d input. */
int sv_sigmoid_focal_loss(const float* input, const float* target, const float* weights, int64_t n_rows, int num_class, float alpha, float gamma,
                          const float* grad_out, float* out, void* stream);
/* WeightedSmoothL1Loss.forward (loss_utils.py:75-136: code-wise weighted smooth-L1, nan targets ignored, un-reduced) and its derivative w.r.t.
 * input.  input, target (n_rows, num_codes), code_weights (num_codes) or NULL, weights (n_rows) or NULL; grad_out as above. */
int sv_weighted_smooth_l1_loss(const float* input, const float* target, const float* code_weights, const float* weights, int64_t n_rows,
                               int num_codes, float beta, const float* grad_out, float* out, void* stream);

/* CenterHead.assign_targets (detector3d/pcdet/models/dense_heads/center_head.py:103-213; gaussian_radius /
 * draw_gaussian_to_heatmap, models/model_utils/centernet_utils.py:9-69): all heads and scenes in one launch.
 * gt_boxes (B,G,box_dim) with the global 1-based class id in the last column (0 = padding); cls_to_local
 * (num_heads, num_class+1) device table = 1-based class index inside the head or 0.  Outputs: heatmaps (B,total_cls,H,W)
 * (head h owns channels [head_cls_offset[h], +head_num_class[h])), target_boxes (num_heads,B,num_max_objs,box_dim)
 * [dx, dy, z, log dims, cos, sin, extras], inds / masks (num_heads,B,num_max_objs) int64. */
int sv_center_assign_targets(const float* gt_boxes, int batch, int max_gt, int box_dim, int num_heads, int num_class,
                             const int32_t* cls_to_local, const int32_t* head_num_class, const int32_t* head_cls_offset, int total_cls,
                             int fm_w, int fm_h, float x_min, float y_min, float voxel_x, float voxel_y, float fm_stride,
                             int num_max_objs, float gaussian_overlap, int min_radius, float* heatmaps, float* target_boxes,
                             int64_t* inds, int64_t* masks, void* stream);

/* ---- pointnet2_batch_cuda wrappers (detector3d/pcdet/ops/pointnet2/pointnet2_batch/src/pointnet2_api.cpp:12-27; kernels in
 * ball_query_gpu.cu, group_points_gpu.cu, sampling_gpu.cu, interpolate_gpu.cu) and the stacked 3-NN interpolation
 * (pointnet2_stack/src/interpolate_gpu.cu:16-195).  Same argument order as the pybind wrappers, raw device pointers.
 * ball query: idx (B,m,nsample) must be zero-filled by the caller like the reference's Python does (queries without a hit
 * keep it).  Gradient entries zero-fill their output.  Batch farthest point sampling = sv_farthest_point_sampling. */
int sv_ball_query_batch(int batch, int n, int m, float radius, int nsample, const float* new_xyz, const float* xyz, int32_t* idx,
                        void* stream);
int sv_group_points_batch(int batch, int c, int n, int npoints, int nsample, const float* points, const int32_t* idx, float* out,
                          void* stream);
int sv_group_points_grad_batch(int batch, int c, int n, int npoints, int nsample, const float* grad_out, const int32_t* idx,
                               float* grad_points, void* stream);
int sv_gather_points_batch(int batch, int c, int n, int npoints, const float* points, const int32_t* idx, float* out, void* stream);
int sv_gather_points_grad_batch(int batch, int c, int n, int npoints, const float* grad_out, const int32_t* idx, float* grad_points,
                                void* stream);
int sv_three_nn_batch(int batch, int n, int m, const float* unknown, const float* known, float* dist2, int32_t* idx, void* stream);
int sv_three_interpolate_batch(int batch, int c, int m, int n, const float* points, const int32_t* idx, const float* weight, float* out,
                               void* stream);
int sv_three_interpolate_grad_batch(int batch, int c, int n, int m, const float* grad_out, const int32_t* idx, const float* weight,
                                    float* grad_points, void* stream);
/* The three batch gradients with a fixed summation order (opt-in): no float atomics, no zero-fill, every element of grad_points written once.
 * group / gather: grad_out (B, c, per), per = npoints * nsample (gather: nsample = 1), idx (B, per), grad_points (B, c, n):
 *   grad_points[b][ch][i] = +0.0f + grad_out[b][ch][j]                     summed in ascending j over the j in [0, per) with idx[b][j] == i
 * three-interpolate: grad_out (B, c, n), idx / weight (B, n, 3), grad_points (B, c, m):
 *   grad_points[b][ch][i] = +0.0f + fp32(grad_out[b][ch][p] * weight[b][p][t])   summed in ascending key 3 p + t over the keys with idx[b][p][t] == i
 * every product and every sum rounded to fp32, no FMA: the very terms the atomic kernels add.  Two slots of one p that name the same row are
 * two keys like any others.  A row no key names is +0.0f and no element is ever -0.0f.  An index outside [0, n) ([0, m) for interpolation)
 * names nothing in ANY batch element (the plain entries trust their indices).  batch, c or the row count <= 0: SV_OK, nothing written;
 * per == 0 (n == 0 for interpolation): +0.0f everywhere.
 * scratch (uninitialised): the inverse lists of keys = B * per (3 * B * n) over rows = B * n (B * m), 16 + 4 * (2 * rows + 2 * keys) bytes;
 * keys or rows >= 2^31 are an error, never the atomic route (the scratch function then returns 0). */
size_t sv_group_points_grad_batch_ordered_scratch_bytes(int batch, int n, int npoints, int nsample);
int sv_group_points_grad_batch_ordered(int batch, int c, int n, int npoints, int nsample, const float* grad_out, const int32_t* idx,
                                       void* scratch, float* grad_points, void* stream);
size_t sv_gather_points_grad_batch_ordered_scratch_bytes(int batch, int n, int npoints);
int sv_gather_points_grad_batch_ordered(int batch, int c, int n, int npoints, const float* grad_out, const int32_t* idx, void* scratch,
                                        float* grad_points, void* stream);
size_t sv_three_interpolate_grad_batch_ordered_scratch_bytes(int batch, int n, int m);
int sv_three_interpolate_grad_batch_ordered(int batch, int c, int n, int m, const float* grad_out, const int32_t* idx, const float* weight,
                                            void* scratch, float* grad_points, void* stream);

/* ---- launch-list executor (csrc/sequencer.hip): enqueue a list of this library's operations with ONE call.  An operation is SV_OP_WORDS int64:
 *   [0] code   [1..8] eight small integers i0..i7   [9..12] four sizes / strides n0..n3   [13..16] four doubles (bit patterns) f0..f3
 *   [17..31] fifteen pointers p0..p14 (device addresses; 0 = null)
 * executed in order on `stream`; the first failing operation's code is returned (sv_last_error names it).  Codes and their fields, in the
 * argument order of the entry point each one calls:
 *   SV_OP_CONV_PLANNED  sv_sparse_conv_gather_gemm_planned: p = X, table_rows, perm, masks_p, tile_of, wfrag, Y, bias, scale, shift, residual,
 *                       bn_partial; n = n_src, n_rows; i = tiles_per_wave, K, Kd, Nc, relu, table_k_reversed
 *   SV_OP_CONV_PLAIN    sv_sparse_conv_gather_gemm: p = X, nbr, Wt, Y, bias, scale, shift, residual; n = n_src, n_rows; i = K, Kd, Nc, relu
 *   SV_OP_BN_FWD        sv_batchnorm_relu_forward (i3 = 0) / _forward_partial (i3 = number of partials): p = x, gamma, beta, running_mean,
 *                       running_var, scratch, y, save_mean, save_invstd, num_batches_tracked; n = rows; i = channels, training, relu, n_partials;
 *                       f = momentum, eps
 *   SV_OP_BN_BWD        sv_batchnorm_relu_backward (i2 = 0) / _backward_partial (i2 = number of partials): p = x, dy, gamma, beta, save_mean,
 *                       save_invstd, scratch, dx, dgamma, dbeta; n = rows; i = channels, relu, n_partials
 *   SV_OP_WGRAD         sv_sparse_conv_wgrad_strided: p = X, nbr, dY, dW, scratch; n = n_rows, stride_k, stride_cin, stride_cout; i = K, Cin, Cout, n_src;
 *                       p5 = equal-pieces plan of the table (then sv_sparse_conv_wgrad_planned, p4 = sv_sparse_conv_wgrad_planned_bytes) or 0
 *   SV_OP_WGRAD_DEFERRED  the same fields as SV_OP_WGRAD, but only stage 1 runs in place (sv_sparse_conv_wgrad_stage1; p4 = this layer's OWN partial region of
 *                       sv_sparse_conv_wgrad_partial_bytes) and the slabs of every deferred layer are summed by ONE launch at the end of the list
 *                       (sv_sparse_conv_wgrad_reduce_batch): the gradients are complete when sv_run_ops returns, bitwise the values of SV_OP_WGRAD
 *   SV_OP_DGRAD_PLANNED_BN  sv_sparse_conv_dgrad_planned_bn: p = dZ, table_rows, perm, masks_p, tile_of, wfrag, dY, bn_x, bn_mean, bn_invstd, bn_gamma,
 *                       bn_beta, bn_partial; n = n_src, n_rows; i = tiles_per_wave, K, Kd, Nc, table_k_reversed, bn_relu
 *   SV_OP_BN_FINALIZE   sv_batchnorm_finalize_forward: p = gamma, beta, running_mean, running_var, scratch, coef, save_mean, save_invstd,
 *                       num_batches_tracked, x (0: partials in scratch); n = rows; i = channels, n_partials; f = momentum, eps
 *   SV_OP_BN_APPLY      sv_batchnorm_apply: p = x, coef, y; n = rows; i = channels, relu
 *   SV_OP_BN_STATS_LOCAL       sv_batchnorm_stats_local: p = x (0: partials in scratch), scratch, sums; n = rows; i = channels, n_partials
 *   SV_OP_BN_FINALIZE_GLOBAL   sv_batchnorm_finalize_global: p = gathered, gamma, beta, running_mean, running_var, coef, save_mean, save_invstd,
 *                       num_batches_tracked, total_rows; i = channels, world; f = momentum, eps
 *   SV_OP_BN_BWD_SUMS_LOCAL    sv_batchnorm_backward_sums_local: p = x, dy, gamma, beta, save_mean, save_invstd, scratch, dgamma, dbeta, sums; n = rows;
 *                       i = channels, relu, n_partials (0: the reduce pass over x, dy runs first)
 *   SV_OP_BN_BWD_APPLY_GLOBAL  sv_batchnorm_backward_apply_global: p = x, dy, gamma, beta, save_mean, save_invstd, scratch, gathered, total_rows, dx;
 *                       n = rows; i = channels, relu, world
 *                       (SyncBatchNorm: a list is CUT behind a *_LOCAL operation, the caller all-gathers `sums` between the ranks, and the next list
 *                       starts with the matching *_GLOBAL operation)
 *   SV_OP_BN_EVAL_COEF_BATCH   sv_batchnorm_eval_coef_batch: p0 = HOST address of the job table (read before sv_run_ops returns); i = n_jobs
 *   SV_OP_CONV_PLANNED_H16     sv_sparse_conv_gather_gemm_planned_h16: p = X16, table_rows, perm, masks_p, wfrag16, Y, bias, scale, shift, residual16;
 *                       n = n_src, n_rows; i = K, Kd, Nc, relu, y_is_f32
 *   SV_OP_NARROW_H16    sv_narrow_h16: p = x_f32, y_f16; n = n_elems
 * Input transform: SV_OP_CONV_PLANNED with p12 = coef (2, Kd) and i6 = relu, SV_OP_WGRAD[_DEFERRED] with p6 = coef (2, Cin) and i4 = relu read their
 * X through sv_conv_next_input_norm(coef, relu): X is then the RAW output of the convolution below, its BatchNorm (+ReLU) is applied as the rows are
 * gathered, and the normalised activation tensor is never written.
 * Used by seevcn_amd/spconv/chain.py: the forward and the backward of a conv -> BatchNorm -> ReLU chain (VoxelBackBone8x, spconv_backbone.py:128-180)
 * as two calls inside one autograd node; and the eval-mode forward of both 3-D backbones as one call (SV_OP_BN_EVAL_COEF_BATCH + one conv per layer,
 * BatchNorm, conv bias, identity and ReLU in the convs' epilogues), in fp32 or -- SV_OP_NARROW_H16 behind the fp32 input layer, SV_OP_CONV_PLANNED_H16
 * for every layer behind it -- with fp16 activations. */
#define SV_OP_WORDS 32
#define SV_OP_CONV_PLANNED 1
#define SV_OP_CONV_PLAIN 2
#define SV_OP_BN_FWD 3
#define SV_OP_BN_BWD 5
#define SV_OP_WGRAD 6
#define SV_OP_DGRAD_PLANNED_BN 7
#define SV_OP_WGRAD_DEFERRED 8
#define SV_OP_BN_FINALIZE 9
#define SV_OP_BN_APPLY 10
#define SV_OP_BN_STATS_LOCAL 11
#define SV_OP_BN_FINALIZE_GLOBAL 12
#define SV_OP_BN_BWD_SUMS_LOCAL 13
#define SV_OP_BN_BWD_APPLY_GLOBAL 14
#define SV_OP_BN_EVAL_COEF_BATCH 15
#define SV_OP_CONV_PLANNED_H16 16
#define SV_OP_NARROW_H16 17
int sv_run_ops(const int64_t* ops, int n_ops, void* stream);
/* measurement form: events around every operation on `stream`, the call waits for the stream and writes each operation's elapsed milliseconds to
 * ms[0 .. n_ops) (bench.py's roofline block times the conv launches of the step's own launch lists with it) */
int sv_run_ops_timed(const int64_t* ops, int n_ops, void* stream, float* ms);
/* The same list with its weight gradients (SV_OP_WGRAD, SV_OP_WGRAD_DEFERRED, the deferred reduction) on `side_stream`: each goes behind an event recorded on
 * `stream` after the operations in front of it; the other operations do not wait for it; `stream` waits for `side_stream` once, at the end, so that when
 * the call returns everything is ordered on `stream` as after sv_run_ops.  A weight gradient only feeds the optimiser: the backward chain need not stop
 * for it, and its matrix-core work fills the bandwidth-bound BatchNorm launches and the tails of the data-gradient launches.  Same kernels, same
 * results. */
int sv_run_ops_two_streams(const int64_t* ops, int n_ops, void* stream, void* side_stream);

/* ---- BatchNorm1d (+ReLU) on (N,C) voxel features: the norm_fn -> ReLU tail of post_act_block
 * (detector3d/pcdet/models/backbones_3d/spconv_backbone.py:9-27,73; torch.nn.BatchNorm1d semantics: biased batch variance for
 * normalisation, unbiased for running_var, running = (1-momentum)*running + momentum*batch).  C multiple of 4, C/4 divides 256.
 * scratch: sv_batchnorm_scratch_bytes(C) bytes (uninitialised).  gamma/beta may be null (affine=False); running_* may be null when training.
 * Backward recomputes the ReLU mask from x, so only x, save_mean and save_invstd need to be kept.  num_batches_tracked (device
 * int64, may be null): nn.BatchNorm1d's counter, += 1 by the training forward. */
size_t sv_batchnorm_scratch_bytes(int channels);
int sv_batchnorm_relu_forward(const float* x, int64_t n, int channels, const float* gamma, const float* beta, float* running_mean,
                              float* running_var, float momentum, float eps, int training, int relu, void* scratch, float* y,
                              float* save_mean, float* save_invstd, int64_t* num_batches_tracked, void* stream);
/* the training forward with its statistics pass already done by the producer of x: scratch holds n_partials x 2 x channels partial sums behind its
 * 4 * channels coefficient floats (sv_sparse_conv_gather_gemm_planned's bn_partial = (float*)scratch + 4 * channels) */
int sv_batchnorm_relu_forward_partial(const float* x, int64_t n, int channels, const float* gamma, const float* beta, float* running_mean,
                                      float* running_var, float momentum, float eps, int relu, void* scratch, int n_partials, float* y,
                                      float* save_mean, float* save_invstd, int64_t* num_batches_tracked, void* stream);
/* the statistics of the training forward WITHOUT its elementwise pass: partials in scratch as above -> save_mean, save_invstd, running statistics and
 * coef (2, channels) = scale | shift of y = x * scale + shift in the caller's buffer (16-byte aligned); y itself is made by the consumers as they read
 * x (sv_conv_next_input_norm) or by sv_batchnorm_apply where a tensor is needed */
int sv_batchnorm_finalize_forward(const float* x /* NULL: partials in scratch; else the statistics pass over x runs first */, int64_t n, int channels, const float* gamma, const float* beta, float* running_mean, float* running_var,
                                  float momentum, float eps, void* scratch, int n_partials, float* coef, float* save_mean, float* save_invstd,
                                  int64_t* num_batches_tracked, void* stream);
/* Eval-mode coefficients of n_jobs BatchNorm layers in one launch: scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale -- what
 * F.batch_norm(..., training=False) inside post_act_block / SparseBasicBlock (spconv_backbone.py:8-66) derives from the running statistics on every call,
 * and bit for bit what sv_batchnorm_relu_forward(training = 0) computes for its own elementwise pass.  jobs_host: n_jobs rows of 8 int64 = {gamma | 0,
 * beta | 0, running_mean, running_var, coef_out (2 * C floats: scale | shift, 16-byte aligned), C, eps (bits of a double), 0} (device addresses; the table
 * itself is host memory, read before the call returns).  The consumers are the epilogues of the convolutions (scale = coef_out, shift = coef_out + C). */
int sv_batchnorm_eval_coef_batch(const int64_t* jobs_host, int n_jobs, void* stream);
/* y = [relu](x * scale + shift), coef (2, channels) = scale | shift: the elementwise pass on its own */
int sv_batchnorm_apply(const float* x, int64_t n, int channels, const float* coef, int relu, float* y, void* stream);
int sv_batchnorm_relu_backward(const float* x, const float* dy, int64_t n, int channels, const float* gamma, const float* beta,
                               const float* save_mean, const float* save_invstd, int relu, void* scratch, float* dx, float* dgamma,
                               float* dbeta, void* stream);
/* sv_batchnorm_relu_backward with the first pass of its two sums already in `scratch` (n_partials workgroup partials behind the 4 * C coefficient
 * floats, written by sv_sparse_conv_dgrad_planned_bn's epilogue): combine + elementwise pass only. */
int sv_batchnorm_relu_backward_partial(const float* x, const float* dy, int64_t n, int channels, const float* gamma, const float* beta,
                                       const float* save_mean, const float* save_invstd, int relu, void* scratch, int n_partials, float* dx,
                                       float* dgamma, float* dbeta, void* stream);
/* ---- SyncBatchNorm (torch.nn.SyncBatchNorm in training mode over more than one rank): the two combines above cut in two around the exchange of the
 * per-channel sums between the ranks.  Every rank makes its own sums in fp64 (*_local), the caller all-gathers them (rank-major), and every rank adds
 * the gathered buffers in rank order in fp64 (*_global): the same bits on every rank, whatever the transport.  Row counts may differ per rank.
 * With world = 1 the pairs reproduce sv_batchnorm_finalize_forward and sv_batchnorm_relu_backward_partial bit for bit.
 * sums (2 * channels + 1 doubles) = sum x | sum x^2 | n, from n_partials workgroup partials in scratch (x NULL) or after the statistics pass over x */
int sv_batchnorm_stats_local(const float* x, int64_t n, int channels, void* scratch, int n_partials, double* sums, void* stream);
/* gathered (world, 2 * channels + 1) -> save_mean, save_invstd, running statistics (unbiased variance with the TOTAL row count), coef (2, channels) =
 * scale | shift, num_batches_tracked += 1, *total_rows (device double, may be null) = the row count of all ranks, kept for the backward */
int sv_batchnorm_finalize_global(const double* gathered, int world, int channels, const float* gamma, const float* beta, float* running_mean,
                                 float* running_var, float momentum, float eps, float* coef, float* save_mean, float* save_invstd,
                                 int64_t* num_batches_tracked, double* total_rows, void* stream);
/* dgamma, dbeta (LOCAL sums) and sums (2 * channels doubles) = sum dy | sum dy * xhat (dy behind the ReLU mask), from n_partials workgroup partials in
 * scratch (the epilogue of sv_sparse_conv_dgrad_planned_bn) or, n_partials = 0, after the reduce pass over x, dy */
int sv_batchnorm_backward_sums_local(const float* x, const float* dy, int64_t n, int channels, const float* gamma, const float* beta,
                                     const float* save_mean, const float* save_invstd, int relu, void* scratch, int n_partials, float* dgamma,
                                     float* dbeta, double* sums, void* stream);
/* gathered (world, 2 * channels) and *total_rows -> dx (n, channels) = gamma * invstd * (dy - sum dy / N - xhat * sum(dy * xhat) / N), N the total count */
int sv_batchnorm_backward_apply_global(const float* x, const float* dy, int64_t n, int channels, const float* gamma, const float* beta,
                                       const float* save_mean, const float* save_invstd, int relu, const double* gathered, int world,
                                       const double* total_rows, void* scratch, float* dx, void* stream);

/* Ragged-group variant of sv_gemm_bias_act: row_group[M] (non-decreasing int32) names the group of every row; used after
 * sv_unique_rows, when each object keeps only its distinct points (ResamplePoints, vcn/datasets/data_transforms.py:254-262,
 * tiles Ni points to 1024 copies: every Conv1d(k=1) row and the max-pools over them only depend on the distinct rows). */
int sv_gemm_bias_act_ragged(const float* A, int lda, const float* W, int ldw, const float* bias, const float* group_bias,
                            const int32_t* row_group, float* C, int ldc, float* group_max, int M, int N, int K, int act, float slope,
                            void* stream);
/* The ragged form with the number of rows ON THE DEVICE: M_cap rows of A / C / row_group are addressable and size the launch, the first *m_dev
 * (<= M_cap) are computed -- sv_unique_rows_compact's total feeds it directly, so that VCN's forward needs no device -> host read. */
int sv_gemm_bias_act_ragged_dev(const float* A, int lda, const float* W, int ldw, const float* bias, const float* group_bias,
                                const int32_t* row_group, float* C, int ldc, float* group_max, int M_cap, const int32_t* m_dev, int N, int K,
                                int act, float slope, void* stream);
/* x (B,n,3), n <= 1024 -> uniq_idx (B,n): the first counts[b] entries of row b index one copy of each distinct point of object b
 * (exact float equality, -0.0 == 0.0), lexicographic order. */
int sv_unique_rows(const float* x, int batch, int n, int32_t* uniq_idx, int32_t* counts, void* stream);
/* Packs sv_unique_rows' per-object lists: sel (>= sum(counts)) int64 flat row b*n + uniq_idx[b][r], row_group int32 = b, object
 * after object; *total (device int32) = sum(counts).  Replaces ~25 torch indexing kernels in the VCN eval forward. */
int sv_unique_rows_compact(const int32_t* uniq_idx, const int32_t* counts, int batch, int n, int64_t* sel, int32_t* row_group,
                           int32_t* total, void* stream);

/* ---- Chamfer distance of the VCN training loss: the reference's `chamfer` extension,
 * see/surface_completion/models/vcn/extensions/chamfer_dist/chamfer_cuda.cpp:36-39 (forward -> [dist1, dist2, idx1, idx2],
 * backward -> [grad_xyz1, grad_xyz2]) over chamfer.cu:15-201.  xyz1 (B,n,3), xyz2 (B,m,3); squared distances; idx = first
 * nearest neighbour; backward zero-fills its outputs. */
int sv_chamfer_forward(const float* xyz1, const float* xyz2, int batch, int n, int m, float* dist1, float* dist2, int32_t* idx1,
                       int32_t* idx2, void* stream);
int sv_chamfer_backward(const float* xyz1, const float* xyz2, const int32_t* idx1, const int32_t* idx2, const float* grad_dist1,
                        const float* grad_dist2, int batch, int n, int m, float* grad_xyz1, float* grad_xyz2, void* stream);
/* chamfer backward (chamfer_cuda.cpp:38, chamfer_dist_grad_kernel chamfer.cu:134-166) with a fixed summation order (opt-in): the terms of
 * sv_chamfer_backward, no float atomics, no zero-fill, every element written once.  For point (b, i) of cloud 1 and coordinate d:
 *   grad_xyz1[b][i][d] = +0.0f + (2 * grad_dist1[b][i]) * (xyz1[b][i][d] - xyz2[b][idx1[b][i]][d])
 *                              + -((2 * grad_dist2[b][k]) * (xyz2[b][k][d] - xyz1[b][i][d]))   for every k with idx2[b][k] == i, ascending k,
 * every product and sum rounded to fp32; cloud 2 likewise (own term from direction 2, then the idx1 hits in ascending j).  The hits are found
 * by a scan of the other cloud's idx: sv_chamfer_backward_ordered_scratch_bytes is 0 and scratch may be null.  batch <= 65535. */
size_t sv_chamfer_backward_ordered_scratch_bytes(int batch, int n, int m);
int sv_chamfer_backward_ordered(const float* xyz1, const float* xyz2, const int32_t* idx1, const int32_t* idx2, const float* grad_dist1,
                                const float* grad_dist2, int batch, int n, int m, void* scratch, float* grad_xyz1, float* grad_xyz2,
                                void* stream);

/* ---- VCN post-processing (CPU code in the reference) ------------------------------------------
 * partial_with_KDTree / get_partial_mesh_batch (see/surface_completion/models/vcn/utils/sampling.py:8-41,69-81): per object,
 * np.unique(partial) -> k nearest coarse points each (float64 distances) -> list(set(indices)) in CPython's set iteration
 * order -> np.tile(...)[:surface_pts].  partial (B,n,3), complete (B,m,3), n,m <= 1024 -> surface (B,surface_pts,3),
 * n_selected (B) = size of the index set. */
size_t sv_vcn_surface_select_scratch_bytes(int batch);
int sv_vcn_surface_select(const float* partial, const float* complete, int batch, int n_partial, int n_complete, int k,
                          int surface_pts, void* scratch, float* surface, int32_t* n_selected, void* stream);
/* get_largest_cluster(_batch) (sampling.py:83-110): open3d cluster_dbscan(eps, min_points) + np.argmax(np.bincount(labels>=0))
 * + tile to total_pts.  min_points <= 2 (VCN.inference passes 2, models/VCN.py:90-93).  n_cluster[b] = 0 when every point is
 * noise (the reference raises there); out rows of that object are left untouched. */
int sv_vcn_largest_cluster(const float* points, int batch, int n, double eps, int min_points, int total_pts, float* out,
                           int32_t* n_cluster, void* stream);
/* the same with a hint (device int32 per object): the cloud of object b repeats its first period[b] rows cyclically -- what sv_vcn_surface_select returns
 * (np.tile(selected)[:surface_pts], sampling.py:37-39, n_selected as the period).  The pair tests then run over the first period[b] rows only (copies hang
 * under their originals: distance 0); the hint is verified on the device, a cloud that does not repeat takes the all-pairs path.  Same output. */
int sv_vcn_largest_cluster_periodic(const float* points, int batch, int n, const int32_t* period, double eps, int min_points, int total_pts, float* out,
                                    int32_t* n_cluster, void* stream);
/* Exact duplicates among n rows [b,x,y,z] (float32, 16-byte aligned): every copy of a row but the first gets b = -1 in place.  The unsorted form of np.unique(np.vstack(instances), axis=0) (SEE_VCN.py:115) for consumers that need the set only; no host
 * sync.  scratch: sv_dedup_rows_scratch_bytes(n) bytes, any content. */
size_t sv_dedup_rows_scratch_bytes(int64_t n);
int sv_dedup_rows(float* rows, int64_t n, void* scratch, void* stream);

/* replace_with_completed_pts (see/surface_completion/SEE_VCN.py:247-265): near[i] = 1 iff some ref point lies closer than
 * thresh to query i (float64 distance, strict <).  ref is expected row-sorted (np.unique) for the tile culling to pay.
 * row_dim 3: rows [x,y,z]; row_dim 4: rows [b,x,y,z] (a batch of scenes, only rows with equal b are compared). */
int sv_points_near_set(const float* query, int64_t n_query, const float* ref, int64_t n_ref, int row_dim, double thresh,
                       uint8_t* near, void* stream);
/* The same result through per-tile boxes made once (scratch: sv_points_near_set_scratch_bytes(n_ref) bytes): waves open a reference tile
 * only if one of their queries is within thresh of its box; reference rows with scene id < 0 (row_dim 4, sv_dedup_rows) are ignored. */
size_t sv_points_near_set_scratch_bytes(int64_t n_ref);
int sv_points_near_set_boxed(const float* query, int64_t n_query, const float* ref, int64_t n_ref, int row_dim, double thresh, void* scratch,
                             uint8_t* near, void* stream);

/* ---- point isolation: the CPU step in front of VCN --------------------------------------------------
 * isolate_gt_pts (see/surface_completion/SEE_VCN.py:61-82): open3d `pcd.crop(OrientedBoundingBox)` for every box of a scene.
 * boxes (G,15) float64 host-or-device rows [centre(3), R row-major(9), extent(3)] (device pointer); a point is inside iff
 * |(p - c) . R[:,a]| <= extent[a]/2 for a = 0,1,2 (float64, like open3d's GetPointIndicesWithinBoundingBox).
 * out_index (G,cap): ascending point indices of box g (first cap of them); out_count (G): their number (may exceed cap). */
int sv_crop_points_in_boxes(const float* points, int64_t n_points, int row_stride, const double* boxes, int n_boxes, int64_t cap,
                            int32_t* out_index, int32_t* out_count, void* stream);
/* KittiObjects.map_pointcloud_to_image (datasets/kitti/kitti_objects.py:153-176) with Calibration.project_velo_to_imageuv /
 * project_velo_to_rect (datasets/kitti/kitti_utils.py:69-114), float64.  v2c (3x4), r0 (3x3), p (3x4): HOST pointers, row-major.
 * fov[i] = 0 <= u < img_w and 0 <= v < img_h and x > min_dist; uv (n,2) = floor(u,v) (-1 outside the FOV); rect (n,3) optional. */
int sv_project_lidar_to_image_kitti(const float* points, int64_t n_points, int row_stride, const double* v2c, const double* r0,
                                    const double* p, int img_w, int img_h, double min_dist, int32_t* uv, uint8_t* fov, float* rect,
                                    void* stream);
/* CustomDatasetObjects.map_pointcloud_to_image (datasets/custom_dataset/custom_dataset_objects.py:141-192): extrinsic (3x4), intrinsic
 * (3x3), distcoeff (5) HOST pointers row-major; camera_model 0 = "pinhole" (k1,k2,p1,p2,k3), 1 = "equidistant" (4 coefficients).
 * uvd_int (n,3) = round-half-even [u, v, depth] (-1 outside), uvd (n,3) float64 optional, fov[i] = z_cam > 0 and |x/z| < atan(W/H) and
 * 0 < u < W-1 and 0 < v < H-1. */
int sv_project_lidar_to_image_camera(const float* points, int64_t n_points, int row_stride, const double* extrinsic, const double* intrinsic,
                                     const double* distcoeff, int camera_model, int img_w, int img_h, int32_t* uvd_int, double* uvd,
                                     uint8_t* fov, void* stream);
/* NuScenesObjects.map_pointcloud_to_image (datasets/nuscenes/nuscenes_objects.py:237-295; the nuscenes-devkit chain it restates, devkit not
 * vendored): lidar -> ego(sweep) -> global -> ego(image) -> camera with float32 storage after each of the 8 rotate / translate steps, then
 * view_points(K, normalize) in float64.  rotations (4,3,3) HOST row-major: [R_lidar2ego, R_ego2global, R_ego_cam2global^T, R_cam2ego^T];
 * translations (4,3) HOST: [t_lidar, t_ego, -t_ego_cam, -t_cam]; intrinsic (3,3) HOST.  fov[i] = depth > min_dist and 0 < u < W and 0 < v < H;
 * pts_img (n,2) = floor(u,v) (-1 outside the FOV); pc_cam (n,3) float32 camera-frame points. */
int sv_project_lidar_to_image_nuscenes(const float* points, int64_t n_points, int row_stride, const double* rotations, const double* translations,
                                       const double* intrinsic, int img_w, int img_h, double min_dist, float* pc_cam, int32_t* pts_img,
                                       uint8_t* fov, void* stream);
/* get_pts_in_mask (datasets/shared_utils.py:36-106): per instance the FOV points with mask[v,u] set.  Give either masks
 * (I,img_h,img_w) uint8 or rects (I,4) int32 [x0,y0,x1,y1] (use_bbox, :56-60).  Lists as in sv_crop_points_in_boxes. */
/* COCO polygons -> binary instance masks on the device: `dataset.annToMask(instance)` of get_pts_in_mask (shared_utils.py:66), i.e. pycocotools'
 * rleFrPoly + rleMerge(union) + rleDecode (cocoapi common/maskApi.c) with the same boundary arithmetic; the run-length code is replaced by a parity
 * scan (a pixel is inside iff an odd number of run boundaries lies at or before its column-major index).  xy: flat (x, y) doubles of all polygons;
 * poly_off (n_polygons + 1) first vertex of each; poly_inst (n_polygons) the instance each belongs to; masks (n_instances, img_h, img_w) uint8, written
 * whole; scratch: sv_polygon_masks_scratch_bytes.  max_vertices = the longest polygon (<= 4096); img_w <= 8192. */
size_t sv_polygon_masks_scratch_bytes(int n_polygons, int img_h, int img_w);
int sv_polygons_to_masks(const double* xy, const int32_t* poly_off, const int32_t* poly_inst, int n_polygons, int max_vertices, int n_instances, int img_h,
                         int img_w, void* scratch, uint8_t* masks, void* stream);
/* The same with every polygon's boundary moved inwards first (the reference's shrink_instance_masks, shared_utils.py:295-330: Polygon.buffer(-d) with
 * d = SHRINK_MASK_PERCENTAGE % of the half diagonal of the polygon's bounding box, then annToMask): a pixel of the polygon's mask is kept when its
 * centre lies at least shrink[p] from every edge of polygon p.  This is the region GEOS's negative buffer describes, sampled at the pixel centres --
 * NOT its vertex list (arcs cut into 16 chords per quadrant, vertices truncated to int, rasterised again): masks agree except in a band of about one
 * pixel along the shrunken boundary (shapely is not available here: unpinned).  shrink NULL = no shrinking; kept (n_polygons int32, nullable): pixels
 * each polygon wrote, 0 = its shrunken part is empty (the caller then falls back like shared_utils.py:325-326). */
int sv_polygons_to_masks_shrunk(const double* xy, const int32_t* poly_off, const int32_t* poly_inst, const double* shrink, int n_polygons, int max_vertices,
                                int n_instances, int img_h, int img_w, void* scratch, uint8_t* masks, int32_t* kept, void* stream);
int sv_points_in_masks(const int32_t* uv, const uint8_t* fov, int64_t n_points, const uint8_t* masks, const int32_t* rects,
                       int n_instances, int img_w, int img_h, int64_t cap, int32_t* out_index, int32_t* out_count, void* stream);
/* isolate_det_pts (SEE_VCN.py:144-181) and db_scan(..., return_largest_cluster=True) (shared_utils.py:395-409), one workgroup
 * per instance: eps = clip(eps_scaling * (|mean(xyz)| * tan_vres), min_eps, max_eps) unless fixed_eps >= 0; open3d
 * cluster_dbscan(eps, min_points) incl. border points; first largest cluster.  Instance g = counts[g] points: rows
 * point_index[starts[g]+r] of `points` (or rows starts[g]+r when point_index is null).  out_local[starts[g]+r] = position within
 * the instance of the r-th member (ascending), out_count[g] = members (0: instance has <= min_cluster points or is all noise;
 * -1: counts[g] > max_points), out_eps[g] = eps used.  Instances above 4096 points need
 * sv_isolate_cluster_scratch_bytes(n_instances, max_points) bytes of scratch. */
int64_t sv_isolate_cluster_scratch_bytes(int n_instances, int64_t max_points);
int sv_isolate_largest_cluster(const float* points, int row_stride, const int32_t* point_index, const int64_t* starts,
                               const int32_t* counts, int n_instances, int64_t max_points, double tan_vres, double eps_scaling,
                               double min_eps, double max_eps, double fixed_eps, int min_points, int min_cluster, void* scratch,
                               int32_t* out_local, int32_t* out_count, double* out_eps, void* stream);

/* ---- roiaware_pool3d_cuda.points_in_boxes_cpu (detector3d/pcdet/ops/roiaware_pool3d/src/roiaware_pool3d.cpp:121-165; a host loop in the
 * reference): out (N,M) int32 0/1, box test with MARGIN 1e-2 (points_in_boxes_gpu uses 1e-5 and returns one box per point).
 * The PV-RCNN++ entries of pointnet2_stack_cuda (vector_pool, local 3-NN) are the sv_vector_pool_* entries above, voxel_query is
 * sv_voxel_query_stack. */
int sv_points_in_boxes_matrix(const float* boxes, const float* pts, int num_boxes, int num_points, int32_t* out, void* stream);

/* ---- Focal sparse convolution (detector3d/pcdet/models/backbones_3d/focal_sparse_conv/): the data-dependent dilation of the active set that the
 * reference writes as per-scene Python loops.  s (n, 27) fp32 = sigmoid(imps) as torch computed it: column 26 the voxel importance mv, column
 * o < 26 the importance of kernel_offsets[o] (focal_sparse_conv.py:43-44).  coords (n, 4) int32 [b, z, y, x]; rows of a scene need not be contiguous.
 * Cells are keyed by the true linear key ((b*Z + z)*Y + y)*X + x, not by the reference's z*max(y)*max(x) + y*max(x) + x (focal_sparse_utils.py:48,
 * :71), which merges distinct voxels once one has y = 0 or x = 0; the two agree wherever that key is injective.  A scene without voxels contributes
 * nothing (the reference raises).
 *
 * Foreground flags fore (n) uint8 -- split_voxels, focal_sparse_utils.py:112-118.  topk != 0: per scene the int(n_b * threshold) rows of largest mv
 * (product in float64), equal values taken lower row first (the reference's unstable sort leaves that open), by an 8-bit radix select with the scene
 * sizes counted on the device; topk == 0: mv > (float)threshold.  scratch: sv_focal_select_scratch_bytes(batch) (top-k only); batch <= 1024. */
size_t sv_focal_select_scratch_bytes(int batch);
int sv_focal_select(const float* s, const int32_t* coords, int64_t n, int batch, int topk, double threshold, void* scratch, uint8_t* fore,
                    void* stream);
/* Output set -- split_voxels, focal_sparse_utils.py:120-142, check_repeat :56-86 and combine_out, focal_sparse_conv.py:171-197: the input cells and,
 * for every foreground row j and offset o with s[j, o] >= (float)threshold, the cell coords[j] + offset[o] when 0 < c < dim on all three axes
 * (:130-131: `> 0`, so a candidate never has a coordinate 0), each once in ascending key order.  out_coords (capacity, 4): rows at or past capacity
 * are not written; *num_out (device) = size of the set, which the caller compares with capacity; row_of_in (n) = output row of every input row (-1:
 * coordinate outside the grid, or past capacity).  index_ws: sv_index_persistent_bytes(batch * Z * Y * X), all zero on entry, its words and chunk
 * counts zero again on return; scratch: sv_focal_expand_scratch_bytes(batch * Z * Y * X). */
size_t sv_focal_expand_scratch_bytes(int64_t ncells);
int sv_focal_expand(const int32_t* coords, const float* s, const uint8_t* fore, int64_t n, int batch, const int32_t* shape_host, double threshold,
                    void* index_ws, void* scratch, int32_t* out_coords, int32_t* row_of_in, int64_t capacity, int32_t* num_out, void* stream);
/* Output features -- the mask multiply (focal_sparse_utils.py:109-110), check_repeat's mean of mask_kernel (:82-85), focal_sparse_conv.py:213-214 and the
 * index_add_ of combine_out: out (num_out, channels), zero-filled here, then out[row_of_in[i]] = f[i] * (mv[i] if mask_multi) * w[i] with
 * w[i] = (1 + sum s[j, o]) / (1 + c_i) over the c_i kept candidates landing on a foreground i -- a gather through nbr (27, n), the k = 3 submanifold
 * table of the INPUT set (sv_rulebook_subm*), offsets in ascending o, fp32 -- and 1 for background rows or under skip_mask_kernel.  w (n) and
 * cnt (n) = c_i are kept for the backward. */
int sv_focal_place(const float* f, const float* s, const int32_t* coords, const uint8_t* fore, const int32_t* nbr, const int32_t* row_of_in,
                   int64_t n, int channels, int mask_multi, int skip_mask_kernel, double threshold, int64_t num_out, float* w, int32_t* cnt,
                   float* out, void* stream);
/* Its gradients (autograd through the same lines; the selection is constant): grad_f (n, channels) = g[row_of_in[i]] * (mv[i]) * w[i];
 * grad_s (n, 27): column o < 26 = t_i for the foreground row i the kept candidate (j, o) lands on, t_i = (g[row_of_in[i]] . f[i]) * (mv[i]) / (1 + c_i),
 * column 26 = w[j] * (g[row_of_in[j]] . f[j]) under mask_multi, 0 elsewhere.  A gather through the same table: no atomics, bit-identical run to run.
 * dots (n) fp32: scratch. */
int sv_focal_backward(const float* g, const float* f, const float* s, const int32_t* coords, const uint8_t* fore, const int32_t* nbr,
                      const int32_t* row_of_in, const float* w, const int32_t* cnt, int64_t n, int channels, int mask_multi, int skip_mask_kernel,
                      double threshold, float* dots, float* grad_f, float* grad_s, void* stream);

/* ---- Focal sparse convolution, image branch: FocalSparseConv.construct_multimodal_features (focal_sparse_conv.py:50-113), which the reference runs
 * per scene with the projection on the host (`.cpu().numpy()` at :92, Calibration.lidar_to_img, detector3d/pcdet/utils/calibration_kitti.py:65-93) and
 * a (B, C, H, W) map from F.interpolate (:69-70).  coords (n, 4) int32 [b, z, y, x], 16-byte aligned; rows of a scene need not be contiguous.
 *
 * Pixels -- :62-64, :82-96: pix (n) int32 = v * W + u of the voxel's projection into its scene's (H, W) image, -1 when it falls outside (or b is
 * not in [0, batch)).  voxel_size_host / origin_host: the layer's z-first voxel_size and point_cloud_range[:3], 3 floats each on the host.
 * calib (batch, 24) fp32 on the device: M = np.dot(V2C.T, R0.T) (4 x 3, row-major; formed on the host in float32 as lidar_to_rect forms it), then P2
 * (3 x 4, row-major).  aug (batch, 4) fp32 on the device: noise_scale, noise_rot, flip_x, flip_y (non-zero = flipped); 1, 0, 0, 0 stand in for keys
 * the batch does not carry.  Per row in fp32, statement for statement:
 *     (z, y, x) = (idx * voxel_stride) * voxel_size + origin            the integer product first
 *     (x, y, z) /= noise_scale                                           :84
 *     (x, y, z) = [x y z] @ [[c s 0] [-s c 0] [0 0 1]], c = cosf(-noise_rot), s = sinf(-noise_rot)      :86, rotate_points_along_z
 *     y = -y under flip_x, x = -x under flip_y                           :88, :90 (the reference's z-first columns 1 and 2)
 *     rect = [x y z 1] @ M;  p = [rect 1] @ P2^T;  u = p0 / rect_z,  v = p1 / rect_z      the divisor is the rect depth, as rect_to_img's
 *     u, v truncated toward zero (.long()); kept iff 0 <= u < W and 0 <= v < H            :94-96
 * Every sum runs in ascending term order with one fp32 rounding per operation and no FMA contraction (numpy's BLAS and torch's matmul leave their
 * order open).  As in the reference there is no depth test: a voxel behind the camera that projects into the image keeps its pixel, and u in (-1, 0)
 * truncates to 0 and counts as inside.  A non-finite u or v gives -1 (the reference leaves that cast undefined). */
int sv_focal_image_pixels(const int32_t* coords, int64_t n, int batch, int voxel_stride, const float* voxel_size_host, const float* origin_host,
                          const float* calib, const float* aug, int H, int W, int32_t* pix, void* stream);
/* Fused rows -- :69-70, :102-108.  features (batch, h, w, C): the storage of a channels_last (batch, C, h, w) tensor; f (n, Cv) the voxel features.
 * mode 0 (concat): out (n, C + Cv) = [img | f]; mode 1 (sum): out (n, Cv) = f + img, C == Cv.  img of row i: zero when pix[i] < 0 (or is not a
 * pixel of the image); features[b, v, u, :] when (h, w) == (H, W); otherwise what F.interpolate(features, (H, W), mode='bilinear',
 * align_corners=False) holds at (v, u), read through its four taps.  Per axis src = max(in / out * (dst + 0.5) - 0.5, 0) is the rational
 * (in * (2 dst + 1) - out) / (2 out): i0 its integer part, i1 = i0 + (i0 < in - 1), l1 the remainder over 2 out rounded to fp32 once, l0 = 1 - l1.
 * Taps t = 0..3 = (y0,x0), (y0,x1), (y1,x0), (y1,x1), w_t = ly * lx, img = ((f_0 w_0 + f_1 w_1) + f_2 w_2) + f_3 w_3 in fp32.  Nothing of size
 * batch * C * H * W is allocated.  16-byte accesses along C when C % 4 == 0, Cv % 4 == 0 and features, f and out are 16-byte aligned, else one
 * float a lane.  Needs H * W < 2^31 and batch * h * w < 2^31. */
int sv_focal_image_sample(const float* features, int batch, int h, int w, int C, int H, int W, const float* f, int Cv, const int32_t* coords,
                          const int32_t* pix, int64_t n, int mode, float* out, void* stream);
/* Its gradient with respect to features (the one with respect to f is a slice or the identity and stays with the caller): no float atomics, a
 * fixed order, every element of grad_features (batch, h, w, C) written exactly once and the map never cleared beforehand.  grad_out (n, ldg): its
 * first C columns are the gradient of img (ldg = C + Cv after a concat, C after a sum).  Key 4 * i + t names the low-resolution pixel of tap t of
 * row i; with (h, w) == (H, W) key i names row i's pixel; rows without a pixel have no keys.  One wave per pixel walks its keys in ascending order
 * (sv_inv_lists_build): grad_features[pixel, c] = +0.0f + sum of grad_out[i, c] * w_t, every product and every sum rounded to fp32.  n == 0
 * writes the zero map.  scratch: sv_focal_image_sample_grad_scratch_bytes bytes, uninitialised (0: the sizes exceed the guards).  Needs
 * batch * h * w < 2^31, H * W < 2^31 and 4 * n < 2^31. */
size_t sv_focal_image_sample_grad_scratch_bytes(int64_t n, int batch, int h, int w, int H, int W);
int sv_focal_image_sample_grad(const float* grad_out, int ldg, const int32_t* coords, const int32_t* pix, int64_t n, int batch, int h, int w, int C,
                               int H, int W, void* scratch, float* grad_features, void* stream);

/* ------------------------------------------------------------------------------------------------
 * KITTI AP evaluation (detector3d/pcdet/datasets/kitti/kitti_object_eval_python/eval.py, rotate_iou.py).  All arrays are device memory.  Frame f
 * owns detections [dt_off[f], dt_off[f+1]) and ground truths [gt_off[f], gt_off[f+1]); its (n_dt_f, n_gt_f) overlap block starts at
 * overlaps[ov_off[f]].  A combination c is (class, difficulty, min-overlap row): min_overlaps[c] >= 0, and combo_cd[c] names the row of the
 * ignored_dt (rows, total_dt) / ignored_gt (rows, total_gt) int8 tables (values -1, 0, 1 of clean_data, eval.py:30-83) it uses.  The entries
 * refuse empty work (zero frames, combinations, detections, ground truths or pairs): the caller skips the launch.
 * ---------------------------------------------------------------------------------------------- */
/* the most detections one frame may hold in sv_kitti_match_scores / sv_kitti_match_stats (the caller refuses more before any launch) */
int sv_kitti_eval_max_detections(void);
/* Ragged overlaps, one launch: segment s owns rows [row_off[s], row_off[s+1]) and columns [col_off[s], col_off[s+1]) and only its (rows, cols)
 * block is computed, at out[out_off[s]]; total_pairs = out_off[num_segments].  metric 0: image_box_overlap (eval.py:86-113) on boxes of 4 floats,
 * criterion -1, 0, 1; metric 1: devRotateIoUEval(col, row) (rotate_iou.py:17-260, fp32, formula for formula) on (x, z, l, w, ry), criterion -1, 0,
 * 1, 2; metric 2: d3_box_overlap (eval.py:121-154) on (x, y, z, l, h, w, ry).  The intersection polygon holds 8 points; a candidate past that is
 * dropped (the reference writes past its array).  One segment gives the dense (N, K) matrix of rotate_iou_gpu_eval. */
int sv_kitti_overlaps(const float* row_boxes, const float* col_boxes, const int64_t* row_off, const int64_t* col_off, const int64_t* out_off,
                      int num_segments, int64_t total_pairs, int metric, int criterion, float* out, void* stream);
/* Pass 1 of compute_statistics_jit (compute_fp=False, eval.py:192-242), one wave per (frame, combination): per ground truth the unassigned, non -1
 * detection with overlap > min_overlap and the highest score, lowest index on ties.  tp_scores (num_combos, total_gt): the caller fills it with
 * -inf; the true-positive scores of frame f land at [c, gt_off[f] + 0, 1, ...]; tp_count (num_combos), zero on entry, gets their number. */
int sv_kitti_match_scores(const float* overlaps, const int64_t* dt_off, const int64_t* gt_off, const int64_t* ov_off, int num_frames,
                          const double* dt_scores, const int8_t* ignored_dt, const int8_t* ignored_gt, const int32_t* combo_cd,
                          const double* min_overlaps, int num_combos, int64_t total_dt, int64_t total_gt, double* tp_scores, int32_t* tp_count,
                          void* stream);
/* get_thresholds (eval.py:9-27), one lane per combination, fp64, on rows of scores sorted in DESCENDING order of which the first counts[c] are
 * real; num_valid_gt[c] is the combination's total_num_valid_gt.  thresholds (num_combos, 41), num_thresholds (num_combos). */
int sv_kitti_thresholds(const double* sorted_scores, int64_t row_stride, const int32_t* counts, const int32_t* num_valid_gt, int num_combos,
                        double* thresholds, int32_t* num_thresholds, void* stream);
/* Pass 2 (compute_fp=True, eval.py:178-275 as fused_compute_statistics calls it), one wave per (frame, combination, threshold), then the table:
 * table (num_combos, 41, 4) fp64 = tp, fp, fn, similarity summed over the frames, rows at or past num_thresholds[c] zero.  counts (num_combos, 41, 3)
 * int32 zero on entry.  metric 0 subtracts the DontCare "stuff" (dt_bbox (total_dt, 4), dc_boxes with per-frame dc_off; may be NULL otherwise).
 * compute_aos: gt_alpha / dt_alpha fp64 and sim_part (num_frames, num_combos, 41) fp64 scratch; the similarity of a frame is summed in
 * ground-truth order and the frames in ascending order by one thread -- no float atomics, equal bits run to run. */
int sv_kitti_match_stats(const float* overlaps, const int64_t* dt_off, const int64_t* gt_off, const int64_t* ov_off, int num_frames,
                         const double* dt_scores, const int8_t* ignored_dt, const int8_t* ignored_gt, const int32_t* combo_cd,
                         const double* min_overlaps, int num_combos, int64_t total_dt, int64_t total_gt, const double* thresholds,
                         const int32_t* num_thresholds, int metric, int compute_aos, const float* dt_bbox, const float* dc_boxes,
                         const int64_t* dc_off, const double* gt_alpha, const double* dt_alpha, int32_t* counts, double* sim_part, double* table,
                         void* stream);

/* CaDDN's frustum sampling grid, FrustumGridGenerator.forward (detector3d/pcdet/models/backbones_3d/vfe/image_vfe_modules/f2v/
 * frustum_grid_generator.py:79-145 with transform_utils.py:14-91): out (B, X, Y, Z, 3) = normalised (image column, image row, depth bin) of every
 * voxel centre.  Per voxel in fp32: (x + .5, y + .5, z + .5, 1); T = lidar_to_cam @ grid_to_lidar formed once per scene; from-homogeneous with
 * scale = |z| > 1e-8 ? 1 / (z + 1e-8) : 1; cam_to_img; depth = z' - P[2][3]; bin_depths (mode 0 UD, 1 LID, 2 SID); coords / ((W_img, H_img,
 * num_bins) - 1) * 2 - 1; non-finite components become -2.  lidar_to_cam (B, 4, 4), cam_to_img (B, 3, 4), image_shape (B, 2) int32 [H, W] on the
 * device: its maximum over the batch is taken there, nothing is read on the host.  pc_range_host: 6 floats on the host. */
int sv_frustum_grid(const float* lidar_to_cam, const float* cam_to_img, const int32_t* image_shape, int batch, int X, int Y, int Z,
                    const float* pc_range_host, int mode, double depth_min, double depth_max, int num_bins, float* out, void* stream);
/* FrustumToVoxel.forward fused with DepthFFN.create_frustum_features (f2v/frustum_to_voxel.py:29-54, f2v/sampler.py:26-37,
 * ffn/depth_ffn.py: frustum_features = depth_probs[:, :-1] * image_features, then the 5-D grid_sample(bilinear, zeros, align_corners=True)).
 * image_features (B, H, W, C) and depth_probs (B, H, W, D + 1) are the storages of channels_last (B, C, H, W) / (B, D + 1, H, W) tensors; the last
 * depth bin is never read; D is the discretisation's num_bins.  out has the storage order (B, Y, X, C, Z) -- the reference's (B, C, Z, Y, X) tensor
 * is a permuted view of it -- and every element is written.  Per voxel, with the coordinates of sv_frustum_grid unnormalised as
 * ((g + 1) / 2) * (size - 1), pixel taps t = 0..3 = (y0,x0), (y0,x1), (y1,x0), (y1,x1) with w_t = wy * wx, and depth taps d0, d0 + 1:
 *     a_t = w_t * (wd0 * p[d0, pix_t] + wd1 * p[d1, pix_t]),    out[c] = ((((0 + a_0 f[pix_0, c]) + a_1 f[pix_1, c]) + a_2 ...) + a_3 ...)
 * where a tap outside the map or the depth range is left out.  Nothing of size C*D*H*W or X*Y*Z*3 is allocated.  16-byte reads along C when
 * C % 4 == 0 and image_features is 16-byte aligned, else one float a lane.  Needs B*H*W < 2^31, 4*B*X*Y*Z < 2^31, Z <= 512.
 *
 * Gradient (none w.r.t. the calibration): no float atomics, a fixed order, every element of grad_features (B, H, W, C) and grad_probs
 * (B, H, W, D + 1) written exactly once, neither cleared beforehand.  grad_out is in out's storage order.  Key 4 * v + t, with
 * v = ((b * Y + y) * X + x) * Z + z, names the pixel of tap t of voxel v; keys of taps outside the map, and of voxels with both depth taps
 * outside, do not exist.  One wave per pixel walks the pixel's keys in ascending order (sv_inv_lists_build):
 *     grad_features[pix, c] = +0.0f + sum of a_t * g[v, c]                                           in ascending key
 *     grad_probs[pix, d]    = +0.0f + sum of (w_t * wd) * dot(v)   over the keys whose d0 or d1 is d,   in ascending key (d0 before d1 within a key)
 *     dot(v) = sum over c of g[v, c] * f[pix, c]: lane l adds its channels l, l + 64 in ascending order, then the wave's xor butterfly 32 -> 1;
 *     for C > 128 the walk repeats per block of 128 channels and each block's dot is added on its own, blocks ascending.
 * grad_probs[pix, D] = +0.0f.  Every product and sum is rounded to fp32.  scratch: sv_frustum_to_voxel_grad_scratch_bytes bytes (0: the sizes
 * exceed the guards above), uninitialised: the per-scene matrices, then the inverse lists.  Needs D <= 4095. */
int sv_frustum_to_voxel(const float* image_features, const float* depth_probs, const float* lidar_to_cam, const float* cam_to_img,
                        const int32_t* image_shape, int batch, int C, int D, int H, int W, int X, int Y, int Z, const float* pc_range_host,
                        int mode, double depth_min, double depth_max, float* out, void* stream);
size_t sv_frustum_to_voxel_grad_scratch_bytes(int batch, int H, int W, int X, int Y, int Z);
int sv_frustum_to_voxel_grad(const float* image_features, const float* depth_probs, const float* lidar_to_cam, const float* cam_to_img,
                             const int32_t* image_shape, const float* grad_out, int batch, int C, int D, int H, int W, int X, int Y, int Z,
                             const float* pc_range_host, int mode, double depth_min, double depth_max, void* scratch, float* grad_features,
                             float* grad_probs, void* stream);

/* Training augmentation on the device (csrc/augment.hip).  One layout for every entry: points are rows of C >= 3 floats in one buffer, scene b owns
 * rows pt_start[b] .. pt_start[b] + pt_cnt[b]; boxes are rows of W >= 7 floats [x, y, z, dx, dy, dz, heading, ...] at box_start[b] .. + box_cnt[b], at
 * most 256 per scene.  box_cls, one int32 per box row: >= 0 index into class_names, -1 another class (gt_boxes_mask == 0), -2 filtered out.  keep, one
 * int32 per point row, 0 = dropped.  Starts and counts are device int32; max_scene_points is a host upper bound of pt_cnt that sizes the grid.
 * No float atomics: equal bits run to run.
 *
 * counts[i] = points of its scene (keep != 0; keep may be NULL) inside box row i by the CPU matrix test, margin 1e-2 in x / y and none in z:
 * points_in_boxes_cpu(...).sum(axis=1) of detector3d/pcdet/datasets/dataset.py:131-133 (the MIN_POINTS_OF_GT filter). */
int sv_points_in_boxes_count(const float* points, int C, const int32_t* pt_start, const int32_t* pt_cnt, const int32_t* keep, int batch,
                             int max_scene_points, const float* boxes, int W, const int32_t* box_start, const int32_t* box_cnt, int total_boxes,
                             int32_t* counts, void* stream);
/* scale_pre_object, the boxes (detector3d/pcdet/datasets/augmentor/augmentor_utils.py:26-50, 61, 66, 69): one workgroup per scene visits its boxes in
 * order; a box with box_cls < 0 is skipped (-1 still blocks the others); noises (box rows, num_try <= 64) fp64; try_idx = the first try whose BEV IoU
 * (s_overlap / fmaxf(sa + sb - s_overlap, 1e-8)) with every other box, at its current size, is exactly 0; one box alone takes try 0.  plan[i] = the
 * chosen scale, 0 = none.  boxes are updated in place (dx, dy, dz scaled, z lifted by (new_dz - dz) / 2) and later boxes see that. */
int sv_object_scale_plan(float* boxes, int W, const int32_t* box_start, const int32_t* box_cnt, const int32_t* box_cls, int batch,
                         const double* noises, int num_try, double* plan, void* stream);
/* scale_pre_object, the points (augmentor_utils.py:52-78): one thread per point walks the scene's scaled boxes in order.  boxes_before: the boxes as
 * sv_object_scale_plan found them.  A point inside box k (margin 1e-2) goes into the box frame, is scaled, goes back and is lifted; columns past z
 * stay.  Only a scale > 1 drops points: those with in_before XOR in_after against the new box get keep = 0 and meet no later box. */
int sv_object_scale_points(float* points, int C, const int32_t* pt_start, const int32_t* pt_cnt, int32_t* keep, int batch, int max_scene_points,
                           const float* boxes_before, int W, const int32_t* box_start, const int32_t* box_cnt, const int32_t* box_cls,
                           const double* plan, void* stream);
/* DataBaseSampler.__call__ (detector3d/pcdet/datasets/augmentor/database_sampler.py:438-468), one workgroup per scene.  The database: db_boxes
 * (K, W) fp32 and db_cls (K) int32.  The scene's candidates: rows cand_start[b] .. cand_start[b + 1] of cand_idx (database rows) and cand_group (the
 * SAMPLE_GROUPS entry that drew them, ascending).  Groups in order; a candidate is valid when its BEV IoU with every existing box (box_cls >= -1,
 * and the earlier groups' accepted boxes) and with every other candidate of its group is exactly 0 (max(iou1) + max(iou2) == 0: not greedy).
 * Accepted boxes are appended behind the scene's box_cnt[b] rows in candidate order (spare rows the caller left: the scene owns box_cap[b] <= 256 rows
 * in all, and a valid candidate beyond them is not accepted), with box_cls = db_cls; box_cnt[b] grows; accept[i] = 0 / 1 per candidate. */
int sv_gt_sample_select(float* boxes, int W, const int32_t* box_start, int32_t* box_cnt, const int32_t* box_cap, int32_t* box_cls, int batch,
                        const float* db_boxes, const int32_t* db_cls, const int32_t* cand_idx, const int32_t* cand_group, const int32_t* cand_start, int total_candidates,
                        int32_t* accept, void* stream);
/* add_sampled_boxes_to_scene (database_sampler.py:381-415).  db_points (T, C) fp32 with db_offsets (K + 1) int64.  Candidate i owns rows cand_dest[i]
 * .. of the point buffer, as many as its object has points (cand_ptoff (candidates + 1): their prefix sum, total_rows in all), at the head of its
 * scene (head_rows[b] rows, keep == 0 on entry) in candidate order, so that the final stable compaction gives [object points in acceptance order,
 * surviving scene points].  Accepted: rows = db_points + box3d_lidar[:3] in fp32, keep = 1.  The scene's own points inside any accepted box enlarged
 * by (extra_x, extra_y, extra_z) (REMOVE_EXTRA_WIDTH; the CPU matrix test, margin 1e-2) get keep = 0.  Nothing accepted: the scene is unchanged. */
int sv_gt_sample_paste(float* points, int C, const int32_t* pt_start, const int32_t* pt_cnt, const int32_t* head_rows, int32_t* keep, int batch,
                       int max_scene_points, const float* db_points, const int64_t* db_offsets, const float* db_boxes, int W, const int32_t* cand_idx,
                       const int32_t* cand_start, const int32_t* cand_ptoff, const int32_t* cand_dest, const int32_t* accept, int total_candidates,
                       int total_rows, float extra_x, float extra_y, float extra_z, void* stream);
/* random_flip_along_x / _y, global_rotation, global_scaling, random_translation_along_x / _y / _z (augmentor_utils.py:82-160, 203-254) in the order
 * given: ops holds num_ops <= 16 codes of 4 bits, first op lowest (1 flip x, 2 flip y, 3 rotation, 4 scaling, 5 / 6 / 7 translation x / y / z); params
 * (batch, num_ops) fp64, one value per scene and op (flips: 0 / 1).  Boxes: centres, sizes, heading and for W > 7 the velocity columns 7 / 8; rows
 * with box_cls == -2 stay; limit_heading applies limit_period(heading, 0.5, 2 pi) afterwards (data_augmentor.py:258-260). */
int sv_world_transform_points(float* points, int C, const int32_t* pt_start, const int32_t* pt_cnt, int batch, int max_scene_points, int64_t ops,
                              int num_ops, const double* params, void* stream);
int sv_world_transform_boxes(float* boxes, int W, const int32_t* box_start, const int32_t* box_cnt, const int32_t* box_cls, int batch, int64_t ops,
                             int num_ops, const double* params, int limit_heading, void* stream);
/* The tail of prepare_data / DataProcessor in one stable compaction.  Points survive with keep != 0 and, pt_range_host (x0, y0, x1, y1 fp64 on the
 * host, may be NULL) given, inside it with both bounds inclusive (common_utils.py:60-63): out_points rows [b, x, y, z, ...] of C + 1 floats, ordered by
 * scene and inside a scene as they came; out_start (batch + 1) their starts; out_counts (2 * batch) = points per scene, then boxes per scene.  Boxes
 * survive with box_cls >= 0 (data_augmentor.py:265-267, dataset.py:152-156) and, min_num_corners > 0, that many corners inside box_range_host (6 fp64:
 * box_utils.py:93-109): gt_out (batch, gt_stride, W + 1), in order, box_cls + 1 in the last column, zero padded.  keep is overwritten with the final
 * flags; box_keep (one int32 per box row, may be NULL) receives the boxes' flags.  scratch: sv_augment_compact_scratch_bytes bytes, uninitialised. */
size_t sv_augment_compact_scratch_bytes(int batch, int max_scene_points);
int sv_augment_compact(const float* points, int C, const int32_t* pt_start, const int32_t* pt_cnt, int32_t* keep, int batch, int max_scene_points,
                       const double* pt_range_host, const float* boxes, int W, const int32_t* box_start, const int32_t* box_cnt,
                       const int32_t* box_cls, const double* box_range_host, int min_num_corners, void* scratch, float* out_points,
                       int32_t* out_start, int32_t* out_counts, float* gt_out, int gt_stride, int32_t* box_keep, void* stream);

/* The local augmentors (csrc/augment_local.hip) on the same layout.  steps: num_steps <= 16 codes of 4 bits, first step lowest:
 *   1 / 2 / 3 random_local_translation_along_x / _y / _z (augmentor_utils.py:257-320)   4 local_rotation (:425-470)   5 local_scaling (:391-422)
 *   6 / 7 / 8 / 9 local_frustum_dropout_top / _bottom / _left / _right (:473-550)
 * sv_local_transform_plan: one thread per box row walks the steps.  draws (total_boxes, num_steps) fp64, one value per box row and step (offset,
 * angle, scale, intensity); rows with box_cls == -2 are skipped and their draws not read, rows with -1 move like the others (the reference loops
 * over all of gt_boxes).  Per (step, row) it writes 12 floats at plan + (step * total_boxes + row) * 12: the box as that step's get_points_in_box
 * (:553-570) sees it -- centre, float32(dx / 2.0 + 0.1), float32(dy / 2.0 + 0.1), dz / 2, float32 of the float64 cos(-rz) / sin(-rz) -- the step's
 * parameter (float32 offset; cosf / sinf of the float32 angle; float32 scale; the float64 threshold (z + dz / 2) - intensity * dz and its kin,
 * rounded) and a skip flag.  The boxes are advanced in place: centre coordinate += offset and heading += angle as float64 sums rounded, sizes *=
 * float32(scale).  Local rotation of boxes wider than 8 columns is refused (np.hstack at :465-468 raises in the reference).
 * sv_local_transform_points: one thread per point walks, per step, the scene's boxes in order (their plan rows staged through LDS) and applies the
 * step wherever the test (margin 0.1 in x / y, none in z, all three comparisons <=) holds at the point's current position; a dropout clears keep
 * and ends the point's walk.  Points with keep == 0 on entry are left alone. */
int sv_local_transform_plan(float* boxes, int W, const int32_t* box_start, const int32_t* box_cnt, const int32_t* box_cls, int batch, int total_boxes,
                            int64_t steps, int num_steps, const double* draws, float* plan, void* stream);
int sv_local_transform_points(float* points, int C, const int32_t* pt_start, const int32_t* pt_cnt, int32_t* keep, int batch, int max_scene_points,
                              const int32_t* box_start, const int32_t* box_cnt, int total_boxes, int64_t steps, int num_steps, const float* plan,
                              void* stream);
/* global_frustum_dropout_top / _bottom / _left / _right (augmentor_utils.py:323-388): dirs holds num_dirs <= 16 codes of 4 bits (1 top, 2 bottom on z;
 * 3 left, 4 right on y), applied in order, each over the survivors of the last; intensity (batch, num_dirs) fp64.  Per direction the minimum and
 * maximum of the coordinate over the scene's live points (integer atomics on an order-preserving code: equal bits run to run), the threshold
 * max - intensity * (max - min) or min + intensity * (max - min) in float64, rounded; points and boxes (box_cls >= -1, by their centre) that fail
 * the strict < / > get keep = 0 / box_cls = -2.  The reference shortens gt_boxes but not gt_names; here the class goes with the box.  A scene
 * without live points is left alone.  scratch: sv_world_frustum_dropout_scratch_bytes bytes, uninitialised. */
size_t sv_world_frustum_dropout_scratch_bytes(int batch, int num_dirs);
int sv_world_frustum_dropout(const float* points, int C, const int32_t* pt_start, const int32_t* pt_cnt, int32_t* keep, int batch,
                             int max_scene_points, const float* boxes, int W, const int32_t* box_start, const int32_t* box_cnt, int32_t* box_cls,
                             int total_boxes, int64_t dirs, int num_dirs, const double* intensity, void* scratch, void* stream);

/* The pyramid augmentor, random_local_pyramid_aug (csrc/augment_pyramid.hip; data_augmentor.py:221-242) on the same layout.  A box row has six
 * pyramids, the centre as apex over one face's corners, faces in pyramid_orders' order (augmentor_utils.py:574-581).  One membership test serves
 * every entry: float32 corners as boxes_to_corners_3d makes them (box_utils.py:28-53; cos / sin are the float64 functions rounded once), the five
 * face planes in float64, closed -- what in_hull's Delaunay.find_simplex(p) >= 0 decides (box_utils.py:12-25, augmentor_utils.py:606-611).
 * sv_get_pyramids (augmentor_utils.py:573-595): out (total_boxes, 6, 15) fp32, apex then the four base corners. */
int sv_get_pyramids(const float* boxes, int W, int total_boxes, float* out, void* stream);
/* local_pyramid_dropout's point half (augmentor_utils.py:620-624): face holds one int32 per box row, 0..5 or anything else for none; every live
 * point inside a marked pyramid of a box of its scene (box_cls != -2) gets keep = 0.  One thread per point, the scene's marked boxes through LDS. */
int sv_pyramid_dropout(const float* points, int C, const int32_t* pt_start, const int32_t* pt_cnt, int32_t* keep, int batch, int max_scene_points,
                       const float* boxes, int W, const int32_t* box_start, const int32_t* box_cnt, const int32_t* box_cls, const int32_t* face,
                       void* stream);
/* points_in_pyramids_mask(...).sum(0) (augmentor_utils.py:643-644, :690-691): mask holds 6 bits per box row, the faces asked for; counts
 * (total_boxes, 6) int32 receives the live member points per pyramid (integer atomics, in LDS first; cleared here).  member (may be NULL; zeroed by
 * the caller): one byte per (point row, box of its scene) at member[row * member_stride + box], the faces among those asked for that hold the point. */
int sv_pyramid_count(const float* points, int C, const int32_t* pt_start, const int32_t* pt_cnt, const int32_t* keep, int batch, int max_scene_points,
                     const float* boxes, int W, const int32_t* box_start, const int32_t* box_cnt, const int32_t* box_cls, int total_boxes,
                     const int32_t* mask, int32_t* counts, uint8_t* member, int member_stride, void* stream);
/* local_pyramid_sparsify's point half (augmentor_utils.py:647-659), one workgroup per pyramid that holds more than SPARSIFY_MAX_NUM points.  pyr
 * (num_pyramids, 5) int32: scene, box row, face, the member count the host read, the first output row (a row of the scene with keep == 0); ranks
 * (num_pyramids, K) int32: np.random.choice(count, K, replace=False), a member's rank being the number of live members before it in row order.
 * Liveness is read from keep_in, a copy of keep made before the call, so that pyramids which share a point each see it; every member's keep is
 * cleared, and the member of rank ranks[j][q] is copied, bits untouched, to row out + q with keep = 1.  flag (one int32, kept by the caller):
 * |= 1 when a pyramid holds another number of members than the host planned with, |= 2 / 4 for output rows outside the scene / a plan row that
 * names nothing; the caller reads it with its next host read and raises.  K <= 1024. */
int sv_pyramid_sparsify(float* points, int C, const int32_t* pt_start, const int32_t* pt_cnt, const int32_t* keep_in, int32_t* keep, int batch,
                        const float* boxes, int W, int total_boxes, const int32_t* pyr, int num_pyramids, const int32_t* ranks, int K, int32_t* flag,
                        void* stream);
/* local_pyramid_swap's point half (augmentor_utils.py:664-682, :716-758), one workgroup per pair.  pairs (num_pairs, 8) int32: scene; box row, face
 * and member count of the to-swap pyramid; the same three of its partner; the first output row.  On the entry flags keep_in: the members of both
 * pyramids in row order, the minimum and maximum of the last column of each (integer atomics on an order-preserving code); rows out .. receive the
 * partner's points mapped into the to-swap pyramid, then rows out + |partner| .. the to-swap pyramid's points mapped into the partner, keep = 1; the
 * members' keep is cleared.  get_points_ratio / recover_points_by_ratio and the last column's rescaling by np.clip(max - min, 1e-6, 1) are float32
 * with one rounding per operation.  C must be 4 (the reference raises otherwise); flag as above, and nothing is written on a count mismatch. */
int sv_pyramid_swap(float* points, int C, const int32_t* pt_start, const int32_t* pt_cnt, const int32_t* keep_in, int32_t* keep, int batch,
                    const float* boxes, int W, int total_boxes, const int32_t* pairs, int num_pairs, int32_t* flag, void* stream);

/* Mesh ray casting for the VCN's "VC" training data (csrc/raycast.hip); replaces open3d.t.geometry.RaycastingScene (Embree, CPU) in
 * see/surface_completion/models/vcn/vc_shapenet/dataset_functions.py:265-342 and raycast_surface_from_meshes.py:16-52.  The arithmetic is stated in
 * tests/raycast_reference.py: Moeller-Trumbore without culling in fp32, one rounding per operation; a triangle is hit when det != 0 && u >= 0 &&
 * v >= 0 && u + v <= 1 && t >= 0; the result is the smallest t, ties to the lowest (geometry, primitive); a miss is t = +inf and ids -1.  The
 * hierarchy skips only triangles that test would reject (padded boxes: DESIGN.md section 3 "VC ray casting"), so results equal brute force.
 *
 * The hierarchy (scene.add_triangles, :266-306): tris (T, 3, 3) fp32 in scene order (geometry-major), T <= 2^24.  sv_bvh_keys writes
 * keys[i] = Morton code of triangle i's centroid << 32 | i and status[0] |= 1 when a vertex is not finite (status: 2 int32, cleared here; the caller
 * refuses such a scene); the caller sorts the keys ascending; sv_bvh_build makes nodes (max(T - 1, 1), 16) and leaves (T, 12) 4-byte words: a radix
 * tree over the sorted keys, every node in parallel, boxes united bottom-up behind one integer counter per node.  A root-to-leaf path holds at most
 * 54 internal nodes (30 Morton + 24 index bits).  scratch: sv_bvh_scratch_bytes(T) bytes for both (0: T out of range), uninitialised. */
size_t sv_bvh_scratch_bytes(int64_t T);
int sv_bvh_keys(const float* tris, int64_t T, int64_t* keys, int32_t* status, void* scratch, void* stream);
int sv_bvh_build(const float* tris, const int32_t* geom_ids, const int32_t* prim_ids, int64_t T, const int64_t* sorted_keys, float* nodes,
                 float* leaves, void* scratch, void* stream);
/* scene.cast_rays(rays) (dataset_functions.py:320, raycast_surface_from_meshes.py:27): rays (N, 6) fp32 [origin, direction], directions as given
 * (not normalised).  t_hit (N) fp32, geometry_ids / primitive_ids (N) int32, primitive_uvs (N, 2) fp32: open3d's keys without the normals.  One
 * wave per 64 consecutive rays; the traversal stack is 64 entries a lane in LDS and the walk visits every node once at most.  status[1] |= 1 were
 * the stack ever full (it cannot be: 54 < 64).  T == 0: every ray misses. */
int sv_cast_rays(const float* nodes, const float* leaves, int64_t T, const float* rays, int64_t N, float* t_hit, int32_t* geometry_ids,
                 int32_t* primitive_ids, float* primitive_uvs, int32_t* status, void* stream);
/* create_rays_pinhole + cast_rays for C cameras in one launch (cast_rays_at_point, :310-323; generate_views, :16-32) without a ray tensor.  cams
 * (C, 12) fp64 on the device: M = R^-1 K^-1 row-major (made on the host) and the eye.  Ray (c, y, x), row-major with y outer: direction
 * M (x + 0.5, y + 0.5, 1) as three fp64 products summed left to right and rounded once to fp32, origin = the eye rounded.  One wave per 8 x 8 pixel
 * tile.  Outputs as sv_cast_rays, C * H * W rays.  C <= 65535, C * W * H < 2^31. */
int sv_cast_pinhole(const float* nodes, const float* leaves, int64_t T, const double* cams, int C, int W, int H, float* t_hit, int32_t* geometry_ids,
                    int32_t* primitive_ids, float* primitive_uvs, int32_t* status, void* stream);
/* RaycastingScene.create_rays_pinhole (:311-318): the rays of sv_cast_pinhole as a tensor, out (C, H, W, 6) fp32. */
int sv_rays_pinhole(const double* cams, int C, int W, int H, float* out, void* stream);
/* rays[hit][:, :3] + rays[hit][:, 3:] * t_hit[hit] (:321-322) and the crop of raycast_object (:331-334) as one stable compaction per segment.
 * Segment c owns rays c * W * H .. ; give either the ray tensor (C * W * H, 6) or cams (the other NULL).  hit = t_hit is finite; the point is
 * o + d * t per component in fp32, two roundings.  points (rows of 3 fp32): segment 0's hit points in ray order, then segment 1's, ...; flags one
 * int32 per point row: 1 inside the segment's box, boxes (C, 7) [x, y, z, l, w, h, yaw] by the test of csrc/box_test.h with no margin (boxes NULL:
 * all 0); obj_points: the rows with flag 1, compacted the same way.  counts (2, C) int32: hit points per segment, then in-box points per segment.
 * points / flags / obj_points hold C * W * H rows.  No float atomics, equal bits run to run.  scratch: sv_ray_hit_points_scratch_bytes bytes. */
size_t sv_ray_hit_points_scratch_bytes(int C, int W, int H);
int sv_ray_hit_points(const float* rays, const double* cams, int C, int W, int H, const float* t_hit, const float* boxes, void* scratch,
                      float* points, int32_t* flags, float* obj_points, int32_t* counts, void* stream);

/* ---- the VC training transforms (see/surface_completion/models/vcn/datasets/data_transforms.py), csrc/lidar_sim.hip.  Objects are stacked: points
 * (sum N, 3) fp32, start / cnt (batch) int32 on the device.  No float atomics, equal bits run to run. */
#define SV_VC_MAX_RINGS 1024
#define SV_VC_PLAN_WORDS 40
/* The ring index of LidarSimulation (data_transforms.py:161-164, fixed_bins = 0: bins = 'sqrt') and DownsampleRings (:128-133, fixed_bins = 50):
 * elevation = arctan2(norm(xy), z) of the float64 rows (utils/misc.py:280-287), np.histogram's equal bins over [min, max] and np.digitize against
 * the left edges of the non-empty bins, i.e. the 1-based rank of the point's own bin among the non-empty bins.  One workgroup per object.  ring
 * (sum N) int32; num_rings (batch); ring_cnt (batch, SV_VC_MAX_RINGS) points per ring, 0 beyond num_rings; elevation (sum N) fp64 or NULL.  An
 * object with cnt < min_in_pts is not looked at (:124, :158): num_rings = 0 and ring = 0.  cnt <= 2^20, so that 'sqrt' gives at most 1024 bins. */
int sv_vc_rings(const float* points, const int32_t* start, const int32_t* cnt, int batch, int fixed_bins, int min_in_pts, int32_t* ring,
                int32_t* num_rings, int32_t* ring_cnt, double* elevation, void* stream);
/* sph2cart(sph_pts[mask][first::step]) (:73, :134-138, :171-194) as an order-preserving copy of rows.  plan (batch, SV_VC_PLAN_WORDS) int32 made on
 * the host: 0 pass-through (the object's rows as they are), 1 use the ring bitmask, 2 use keep (sum N bytes, RandomPointDropout's mask), 3 first,
 * 4 step, 5 out_start (row of `out`), 6 out_len, 7 unused, 8..39 the bitmask of chosen rings (bit r - 1 = ring r).  ring / keep may be NULL when no
 * plan uses them.  Rows beyond out_len are not written. */
int sv_vc_select(const float* points, const int32_t* start, const int32_t* cnt, int batch, const int32_t* ring, const uint8_t* keep,
                 const int32_t* plan, float* out, void* stream);
/* ResamplePoints (:254-262): out (batch, n_points, 3), out[b, j] = points[start_b + index[b, j] % cnt_b]; index (batch, n_points) int32 = the first
 * n_points of the permutation of the tiled cloud, drawn on the host. */
int sv_vc_resample(const float* points, const int32_t* start, const int32_t* cnt, int batch, const int32_t* index, int n_points, float* out,
                   void* stream);
/* mode 0 Jitter (:214-217): p + noise, noise (total, 3) fp64.  mode 1 AddGNSpherical (:240-243): p * ((r + noise) / r), noise (total) fp64, r == 0
 * gives (0, 0, noise).  In place, float64 arithmetic rounded once to fp32. */
int sv_vc_pointwise(float* points, int64_t total, const double* noise, int mode, void* stream);
/* RandomObjectScaling (:302-316): params (batch, 8) fp64 = enable, box centre (3), heading, scale (3).  Into the box frame (float64 difference,
 * fp32 rotation of utils/transform.py:33-58), float64 product with the scale, fp32 rotation back, float64 sum with the centre.  In place. */
int sv_vc_object_scale(float* points, const int32_t* start, const int32_t* cnt, int batch, int max_points, const double* params, void* stream);

/* ---- VCN validation metrics (csrc/vc_metrics.hip): see/surface_completion/models/vcn/utils/metrics.py (Metrics.get, the six enabled items over the
 * whole batch and the four num_pts levels), utils/losses.py:90-103 (get_oob_error), utils/bbox_utils.py:29-78, utils/transform.py:163-187.  The
 * arithmetic is stated in tests/vc_metrics_reference.py.
 * sv_vc_metrics_objects: coarse (B,n,3), complete (B,m,3), gt_boxes (B,7), reg_rot (B,3,3) or null, reg_centre (B,3) or null -> table
 * (B, SV_VCM_COLS) of 4-byte words, fp32 unless said otherwise, one row an object:
 *    0 .. 3   sum d1, sum sqrt d1 (coarse -> complete), sum d2, sum sqrt d2 (complete -> coarse); d = the minimum over the other cloud of the fp32
 *             (dx*dx + dy*dy) + dz*dz
 *    4 .. 7   the same four over the rows with (x + y) + z != 0 in fp32, the minimum over such rows of the other cloud (0 when it has none)
 *    8, 9     int32: rows of coarse, of complete with (x + y) + z != 0
 *   10 .. 15  get_bbox_from_keypoints: centre of the bounds, extents in the ground-truth heading frame (the heading is gt_boxes[:, 6])
 *   16        3-D IoU of that box with the ground-truth box (sv_boxes_iou3d_batch's arithmetic, this pair only)
 *   17, 18    int32: distinct rows of coarse outside the ground-truth cuboid (float64 test, faces inclusive); distinct scalars among its 3 n coordinates
 *   19        fp32(17) / fp32(18)
 *   20        |atan2f(r01 / |r0|, r00 / |r0|) - heading|, r0 = row 0 of reg_rot; -1 when reg_rot is null
 *   21        ((|dx| + |dy|) + |dz|) / 3 of reg_centre - centre; -1 when reg_centre is null
 *   22, 23    int32: n, m
 * One workgroup of 1024 an object; the summation order is stated in the source's header.  1 <= n <= 4096 (the cloud and its sort live in LDS), m >= 1;
 * complete == null with m == 0 skips the Chamfer columns (they are written as 0): get_oob_error's call.
 * sv_vc_metrics_levels: table, num_pts (B) int32 -> out (30) fp32 in Metrics.names() order: CDL1, CDL2, OUT_OF_BOX, IOU_3D, Rotation_Error,
 * Translation_Error, each for the whole batch, then L1 (num_pts 201 .. 1000000), L2 (81 .. 200), L3 (31 .. 80), L4 (5 .. 30); sums over the objects in
 * ascending index.  An empty group gives -1; the Chamfer values of a one-object group come from columns 4 .. 9 (-1 when a count is 0) and are -1 when
 * m == 1; Rotation_Error is the lower median; columns 20 / 21 at -1 give -1.  1 <= B <= 4096.
 * sv_vc_metrics_columns() == SV_VCM_COLS; sv_vc_metrics_tile(): rows of the complete cloud staged in LDS at a time. */
#define SV_VCM_COLS 24
int sv_vc_metrics_columns(void);
int sv_vc_metrics_tile(void);
int sv_vc_metrics_objects(const float* coarse, const float* complete, const float* gt_boxes, const float* reg_rot, const float* reg_centre,
                          int batch, int n, int m, float* table, void* stream);
int sv_vc_metrics_levels(const float* table, const int32_t* num_pts, int batch, float* out, void* stream);

/* ---- optimizer step (csrc/optim.hip): the parameter update of every detector config and of the VCN.  Replaces, per train step,
 * detector3d/tools/train_utils/train_utils.py:53-54 (clip_grad_norm_, optimizer.step()), the per-parameter p.data.mul_(1 - wd*lr) loops of
 * detector3d/tools/train_utils/optimization/fastai_optim.py:135-152 and torch.optim.Adam / AdamW as built by
 * detector3d/tools/train_utils/optimization/__init__.py:11-36 and see/surface_completion/models/vcn/tools/builder.py:49-58.
 * The kernels run over a chunk table on the device: `chunks` is nchunks records of sv_optim_chunk_bytes() == 48 bytes,
 *    { float* p, g, m, v;  int32 n, tensor, group, pad }
 * one per slice of at most sv_optim_chunk_elems() == SV_OPTIM_CHUNK consecutive elements of one fp32 tensor that has a gradient (parameter,
 * gradient, exp_avg, exp_avg_sq at the slice, its element count, the tensor's index into t / tensor_scal, its parameter group).  A tensor
 * without a gradient has no record and is not touched: no decay, no state change, no advance of t (torch skips .grad is None).
 * sv_optim_grad_sqnorm (clip_grad_norm_'s norms): partials[c] = sum of g*g over chunk c in float64, one workgroup of 256 a chunk, no atomics.
 * Thread t adds the exact float64 squares of elements 4i .. 4i+3, i = t, t + 256, ..., ascending, to one accumulator (the n % 4 last elements
 * go to the thread whose group they would complete); xor butterfly over the wave (32 .. 1); the four wave totals in ascending order.  The
 * order does not depend on the gradient's alignment.
 * sv_optim_adam_step: two launches.  (1) one workgroup: the partials in ascending chunk order in float64, in 256 blocks (thread j adds partials
 * [j B, (j + 1) B), B = ceil(nchunks / 256), ascending; thread 0 adds the 256 block sums, ascending) give total,
 * total_norm = fp32(sqrt(total)), clip = min(1, max_norm / (total_norm + 1e-6f)) in fp32 (a NaN stays NaN, as torch.clamp keeps it);
 * partials == null or max_norm <= 0: no clipping, total_norm = 0, clip = 1.  For each of the npresent (tensor, group) int32 pairs of `present`:
 * t[tensor] += 1, bc1 = 1 - beta1^t, bc2 = 1 - beta2^t in float64 with the group's CURRENT betas (torch's semantics under a schedule that
 * moves beta1), tensor_scal[2 tensor] = {step = fp32(lr / bc1), rbc2 = fp32(sqrt(bc2))}.  (2) one workgroup a chunk, per element in fp32,
 * every operation rounded once:
 *      g = grad * clip
 *      g = g + wd * p                        mode SV_OPTIM_L2 (OPTIMIZER: adam)
 *      p = p * decay                         mode SV_OPTIM_DECOUPLED (true_wd / AdamW), decay = fp32(1 - lr * wd) from float64
 *      m = b1 * m + omb1 * g                 b1 = fp32(beta1), omb1 = fp32(1 - beta1), likewise b2, omb2
 *      v = b2 * v + (omb2 * g) * g
 *      p = p - (step * m) / (sqrt(v) / rbc2 + eps)
 * consume != 0 stores zeros over the gradient it has read.  dwordx4 loads and stores where all four pointers of a chunk are 16-byte aligned
 * (then only a tensor's last chunk has a scalar tail of n % 4); a chunk with any pointer off a 16-byte boundary takes coalesced dwords
 * throughout.  Nothing outside [0, n) of a slice is read or written.
 * groups: ngroups x 6 float64 ON THE HOST, {lr, beta1, beta2, eps, wd, mode}, passed on to the kernels by value; 1 <= ngroups <=
 * SV_OPTIM_MAX_GROUPS.  norm_out (2) fp32 on the device: total_norm, clip.  t (tensors) int32, tensor_scal (2 x tensors) fp32.  No host read. */
#define SV_OPTIM_CHUNK 4096
#define SV_OPTIM_MAX_GROUPS 16
#define SV_OPTIM_NO_DECAY 0
#define SV_OPTIM_L2 1
#define SV_OPTIM_DECOUPLED 2
int sv_optim_chunk_elems(void);
int sv_optim_chunk_bytes(void);
int sv_optim_max_groups(void);
int sv_optim_grad_sqnorm(const void* chunks, int nchunks, double* partials, void* stream);
int sv_optim_adam_step(const void* chunks, int nchunks, const int32_t* present, int npresent, const double* groups, int ngroups,
                       const double* partials, float max_norm, int consume, int32_t* t, float* tensor_scal, float* norm_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SEEVCN_HIP_H */
