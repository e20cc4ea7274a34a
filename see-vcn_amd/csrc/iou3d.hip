// Rotated-box geometry: BEV overlap / IoU for all pairs, rotated and axis-aligned NMS, points-in-boxes.
//
// Reference: detector3d/pcdet/ops/iou3d_nms/src/iou3d_nms_kernel.cu (box_overlap :95-223, iou_bev :225-231,
// nms_kernel :267-302, nms_normal_kernel :317-355) + host sweep iou3d_nms.cpp:90-135;
// detector3d/pcdet/ops/roiaware_pool3d/src/roiaware_pool3d_kernel.cu:16-36,313-337 (points_in_boxes).
//
// What is different here (same results):
//   * a conservative bounding-circle test skips the polygon construction for pairs that cannot touch (after the score
//     sort of NMS that is almost every pair);
//   * NMS masks are produced one 64-bit word per wave-wide ballot and only for the upper triangle; the greedy sweep
//     runs ON THE GPU (one wave, 64 boxes per step: the diagonal word decides suppression inside the block, kept rows
//     are OR-ed into the remaining words with coalesced loads) — the reference copies the N x N/64 mask to the host
//     and sweeps there (iou3d_nms.cpp:111-131);
//   * per-box sin/cos are computed once per tile/box, not once per pair.
#include <math.h>

#include "box_test.h"
#include "common.h"
#include "rbox.h"                     // RBox, overlap_area, iou_bev

__device__ __forceinline__ float iou_axis_aligned(const float* a, const float* b) {
  const float left = fmaxf(a[0] - a[3] / 2, b[0] - b[3] / 2), right = fminf(a[0] + a[3] / 2, b[0] + b[3] / 2);
  const float top = fmaxf(a[1] - a[4] / 2, b[1] - b[4] / 2), bottom = fminf(a[1] + a[4] / 2, b[1] + b[4] / 2);
  const float w = fmaxf(right - left, 0.f), h = fmaxf(bottom - top, 0.f), inter = w * h;
  return inter / fmaxf(a[3] * a[4] + b[3] * b[4] - inter, 1e-8f);
}

// ------------------------------------------------------------------ all-pairs overlap / IoU: one thread per pair
__global__ __launch_bounds__(256) void k_boxes_pairs(int na, const float* __restrict__ A, int nb, const float* __restrict__ B,
                                                     float* __restrict__ out, int iou) {
  __shared__ RBox sb[64];
  // tile: 4 rows of A x 64 columns of B per workgroup
  const int col0 = blockIdx.x * 64, row0 = blockIdx.y * 4;
  if (threadIdx.x < 64 && col0 + threadIdx.x < nb) sb[threadIdx.x] = make_rbox(B + (int64_t)(col0 + threadIdx.x) * 7);
  __syncthreads();
  const int r = row0 + (threadIdx.x >> 6), c = col0 + (threadIdx.x & 63);
  if (r >= na || c >= nb) return;
  const RBox a = make_rbox(A + (int64_t)r * 7);
  const RBox& b = sb[threadIdx.x & 63];
  out[(int64_t)r * nb + c] = iou ? iou_bev(a, b) : overlap_area(a, b);
}

extern "C" int sv_boxes_overlap_bev(const float* boxes_a, int num_a, const float* boxes_b, int num_b, float* out, int iou, void* stream) {
  SV_CHECK_ARG(num_a >= 0 && num_b >= 0, "boxes_overlap_bev: bad arguments");
  if (num_a == 0 || num_b == 0) return SV_OK;
  SV_CHECK_ARG(boxes_a && boxes_b && out, "boxes_overlap_bev: null pointer");
  dim3 grid(sv_div_up(num_b, 64), sv_div_up(num_a, 4));
  hipLaunchKernelGGL(k_boxes_pairs, grid, dim3(256), 0, sv_stream(stream), num_a, boxes_a, num_b, boxes_b, out, iou);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// 3-D IoU of every (a, b) pair of `batch` independent box sets: BEV overlap x height overlap / union volume, the arithmetic of the reference's
// boxes_iou3d_gpu (iou3d_nms_utils.py:48-81) operation by operation -- there ~22 elementwise launches around the overlap kernel, per scene.
// Boxes are rows of `stride` floats whose first 7 are [x,y,z,dx,dy,dz,heading] (ground-truth blocks carry a class column behind them).
__global__ __launch_bounds__(256) void k_boxes_iou3d(int na, const float* __restrict__ A, int stride_a, int nb, const float* __restrict__ B, int stride_b,
                                                     float* __restrict__ out) {
  __shared__ RBox sb[64];
  __shared__ float sbz[64][3];                                 // height max, height min, volume of the b boxes of the tile
  const int scene = blockIdx.z;
  A += (int64_t)scene * na * stride_a, B += (int64_t)scene * nb * stride_b, out += (int64_t)scene * na * nb;
  const int col0 = blockIdx.x * 64, row0 = blockIdx.y * 4;
  if (threadIdx.x < 64 && col0 + threadIdx.x < nb) {
    const float* b = B + (int64_t)(col0 + threadIdx.x) * stride_b;
    sb[threadIdx.x] = make_rbox(b);
    sbz[threadIdx.x][0] = b[2] + b[5] / 2.f, sbz[threadIdx.x][1] = b[2] - b[5] / 2.f, sbz[threadIdx.x][2] = b[3] * b[4] * b[5];
  }
  __syncthreads();
  const int r = row0 + (threadIdx.x >> 6), c = col0 + (threadIdx.x & 63);
  if (r >= na || c >= nb) return;
  const float* a = A + (int64_t)r * stride_a;
  const float a_hmax = a[2] + a[5] / 2.f, a_hmin = a[2] - a[5] / 2.f, vol_a = a[3] * a[4] * a[5];
  const float* bz = sbz[threadIdx.x & 63];
  const float overlap_bev = overlap_area(make_rbox(a), sb[threadIdx.x & 63]);
  const float overlap_h = fmaxf(fminf(a_hmax, bz[0]) - fmaxf(a_hmin, bz[1]), 0.f);
  const float overlap_3d = overlap_bev * overlap_h;
  out[(int64_t)r * nb + c] = overlap_3d / fmaxf(vol_a + bz[2] - overlap_3d, 1e-6f);
}

extern "C" int sv_boxes_iou3d_batch(const float* boxes_a, int num_a, int stride_a, const float* boxes_b, int num_b, int stride_b, int batch, float* out,
                                    void* stream) {
  SV_CHECK_ARG(num_a >= 0 && num_b >= 0 && batch >= 0 && stride_a >= 7 && stride_b >= 7, "boxes_iou3d_batch: bad arguments");
  if (num_a == 0 || num_b == 0 || batch == 0) return SV_OK;
  SV_CHECK_ARG(boxes_a && boxes_b && out && batch <= 65535, "boxes_iou3d_batch: null pointer or more than 65535 box sets");
  dim3 grid(sv_div_up(num_b, 64), sv_div_up(num_a, 4), batch);
  hipLaunchKernelGGL(k_boxes_iou3d, grid, dim3(256), 0, sv_stream(stream), num_a, boxes_a, stride_a, num_b, boxes_b, stride_b, out);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ------------------------------------------------------------------ NMS: suppression masks (upper triangle)
// one wave per 64x64 tile (row block rb, column block cb >= rb) of the n boxes at `boxes`; lane = column box; each row contributes one ballot word
__device__ __forceinline__ void nms_mask_tile(int n, int rb, int cb, const float* __restrict__ boxes, unsigned long long* __restrict__ mask,
                                              int col_blocks, float thresh, int normal) {
  const int lane = threadIdx.x;
  const int col = cb * 64 + lane;
  const bool col_ok = col < n;
  float cbox[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) cbox[k] = col_ok ? boxes[(int64_t)col * 7 + k] : 0.f;
  const RBox c = make_rbox(cbox);
  const int rows = min(64, n - rb * 64);
  for (int r = 0; r < rows; ++r) {
    const int row = rb * 64 + r;
    float rbox[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) rbox[k] = boxes[(int64_t)row * 7 + k];   // wave-uniform address: one broadcast load
    bool sup = false;
    if (col_ok && col > row) sup = (normal ? iou_axis_aligned(rbox, cbox) : iou_bev(make_rbox(rbox), c)) > thresh;
    const unsigned long long w = __ballot(sup);
    if (lane == 0) mask[(int64_t)row * col_blocks + cb] = w;
  }
}

// (row blocks rb0 + blockIdx.y of a chunked sweep; `done` non-null and set = an earlier chunk already kept max_keep boxes: nothing to do)
__global__ __launch_bounds__(64) void k_nms_mask(int n, float thresh, const float* __restrict__ boxes, unsigned long long* __restrict__ mask,
                                                 int col_blocks, int normal, int rb0, const int32_t* __restrict__ done) {
  if (done && *done) return;
  const int rb = rb0 + blockIdx.y, cb = blockIdx.x;
  if (cb < rb) return;                                       // the sweep never reads words left of the diagonal
  nms_mask_tile(n, rb, cb, boxes, mask, col_blocks, thresh, normal);
}

// greedy sweep on the device: one workgroup, removal bitmap in LDS (n <= 65536).  Per block of 64 boxes wave 0 resolves the block against
// itself (diagonal word of each row, 64 serial steps on registers), then all four waves fold the kept rows into the words of the later
// blocks (lanes over words: every row read is one coalesced run).  The sweep stops once max_keep boxes are kept: callers that only take the
// first NMS_POST_MAXSIZE survivors (model_nms_utils.py:21, roi_head_template.py:68-72) get the same prefix without the rest of the sweep
// (9000 proposals at threshold 0.8, 512 wanted: 4.3 ms -> 0.3 ms).
constexpr int NMS_MAX_WORDS = 1024;
constexpr int NMS_SWEEP_THREADS = 256;

// One wave resolves block nb (`rows` boxes) against itself.  cur: the block's word of the removal bitmap; diag: this lane's row of the
// block's diagonal mask word (0 beyond `rows`).  64 serial steps on registers give the kept rows as a bit set, the same in every lane; lane r
// writes kept row r into keep[] at its rank behind the kept_total boxes kept so far, as long as that is below max_keep.
__device__ __forceinline__ unsigned long long nms_resolve_block(unsigned long long cur, unsigned long long diag, int nb, int rows, int kept_total,
                                                                int max_keep, int64_t* __restrict__ keep) {
  const int lane = threadIdx.x & 63;
  unsigned long long keptbits = 0ull;
  for (int r = 0; r < rows; ++r) {
    const unsigned long long d = __shfl(diag, r, 64);
    if (!((cur >> r) & 1ull)) {
      keptbits |= 1ull << r;
      cur |= d;
    }
  }
  const int slot = kept_total + __popcll(keptbits & ((1ull << lane) - 1ull));
  if (((keptbits >> lane) & 1ull) && slot < max_keep) keep[slot] = (int64_t)nb * 64 + lane;
  return keptbits;
}
// nb0 .. nb1: the blocks this launch resolves.  A whole sweep is one launch (nb0 = 0, nb1 = col_blocks, state = null); a CHUNKED sweep is
// a sequence of launches that carry the removal bitmap and the kept count in `state` ([0] kept so far, [1] done flag, then the bitmap
// words) -- the mask rows of a chunk are computed right before its launch and not at all once max_keep is reached (k_nms_mask checks the
// flag): 9000 proposals at threshold 0.8 keep their 512th box inside the first 1024, the other 88 % of the 40 M rotated IoUs are never made.
struct NmsState {
  int32_t kept, done;
  unsigned long long remv[NMS_MAX_WORDS];
};
__global__ __launch_bounds__(NMS_SWEEP_THREADS) void k_nms_sweep(int n, const unsigned long long* __restrict__ mask, int col_blocks, int max_keep,
                                                                 int64_t* __restrict__ keep, int32_t* __restrict__ num_out, int nb0, int nb1,
                                                                 NmsState* __restrict__ state) {
  __shared__ unsigned long long remv[NMS_MAX_WORDS];
  __shared__ unsigned long long s_kept;
  const int tid = threadIdx.x, lane = tid & 63;
  if (state && state->done) return;                            // (the count was written by the launch that set the flag)
  for (int j = tid; j < col_blocks; j += NMS_SWEEP_THREADS) remv[j] = (state && nb0 > 0) ? state->remv[j] : 0ull;
  __syncthreads();
  int kept_total = (state && nb0 > 0) ? state->kept : 0;
  for (int nb = nb0; nb < nb1 && kept_total < max_keep; ++nb) {
    if (tid < 64) {
      const int rows = min(64, n - nb * 64);
      const unsigned long long diag = lane < rows ? mask[(int64_t)(nb * 64 + lane) * col_blocks + nb] : 0ull;
      const unsigned long long keptbits = nms_resolve_block(remv[nb], diag, nb, rows, kept_total, max_keep, keep);
      if (lane == 0) s_kept = keptbits;
    }
    __syncthreads();
    const unsigned long long keptbits = s_kept;
    kept_total += __popcll(keptbits);
    if (kept_total < max_keep) {
      for (int j = nb + 1 + tid; j < col_blocks; j += NMS_SWEEP_THREADS) {
        unsigned long long acc = remv[j];
        unsigned long long kb = keptbits;
        const unsigned long long* col = mask + (int64_t)nb * 64 * col_blocks + j;
        while (kb) {
          const int r = __ffsll((long long)kb) - 1;
          kb &= kb - 1;
          acc |= col[(int64_t)r * col_blocks];
        }
        remv[j] = acc;
      }
    }
    __syncthreads();
  }
  const bool finished = kept_total >= max_keep || nb1 >= col_blocks;
  if (state) {
    if (!finished)
      for (int j = tid; j < col_blocks; j += NMS_SWEEP_THREADS) state->remv[j] = remv[j];
    if (tid == 0) state->kept = kept_total, state->done = finished ? 1 : 0;
  }
  if (tid == 0 && finished) *num_out = min(kept_total, max_keep);
}

extern "C" size_t sv_nms_scratch_bytes(int n) {
  const size_t cb = (size_t)(n + 63) / 64;
  return ((size_t)n * cb + 8) * sizeof(unsigned long long) + sizeof(NmsState);
}

extern "C" int sv_nms_prefix(const float* boxes, int n, float thresh, int normal, int max_keep, void* scratch, int64_t* keep, int32_t* num_out,
                             void* stream);
extern "C" int sv_nms(const float* boxes, int n, float thresh, int normal, void* scratch, int64_t* keep, int32_t* num_out, void* stream) {
  return sv_nms_prefix(boxes, n, thresh, normal, n, scratch, keep, num_out, stream);
}

extern "C" int sv_nms_prefix(const float* boxes, int n, float thresh, int normal, int max_keep, void* scratch, int64_t* keep, int32_t* num_out,
                             void* stream) {
  SV_CHECK_ARG(n >= 0 && num_out && max_keep >= 0, "nms: bad arguments");
  hipStream_t st = sv_stream(stream);
  if (n == 0) {
    SV_HIP(hipMemsetAsync(num_out, 0, 4, st));
    return SV_OK;
  }
  SV_CHECK_ARG(boxes && scratch && keep, "nms: null pointer");
  const int cb = (n + 63) / 64;
  SV_CHECK_ARG(cb <= NMS_MAX_WORDS, "nms: at most %d boxes", NMS_MAX_WORDS * 64);
  unsigned long long* mask = reinterpret_cast<unsigned long long*>(scratch);
  if (max_keep >= n || cb <= 32) {                             // the whole sweep is wanted, or it is small: two launches
    hipLaunchKernelGGL(k_nms_mask, dim3(cb, cb), dim3(64), 0, st, n, thresh, boxes, mask, cb, normal, 0, (const int32_t*)nullptr);
    hipLaunchKernelGGL(k_nms_sweep, dim3(1), dim3(NMS_SWEEP_THREADS), 0, st, n, mask, cb, max_keep, keep, num_out, 0, cb, (NmsState*)nullptr);
    SV_LAUNCH_CHECK();
    return SV_OK;
  }
  // a prefix is wanted: row chunks of growing size (16, 32, 64, ... blocks), masks of a chunk only if the chunks before did not reach max_keep
  NmsState* state = reinterpret_cast<NmsState*>(mask + (size_t)n * cb + 8);
  SV_HIP(hipMemsetAsync(state, 0, 8, st));
  for (int nb0 = 0, step = 16; nb0 < cb; nb0 += step, step *= 2) {
    const int nb1 = nb0 + step < cb ? nb0 + step : cb;
    hipLaunchKernelGGL(k_nms_mask, dim3(cb, nb1 - nb0), dim3(64), 0, st, n, thresh, boxes, mask, cb, normal, nb0, &state->done);
    hipLaunchKernelGGL(k_nms_sweep, dim3(1), dim3(NMS_SWEEP_THREADS), 0, st, n, mask, cb, max_keep, keep, num_out, nb0, nb1, state);
  }
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ------------------------------------------------------------------ segmented NMS: S independent box sets in one launch pair
// Class-wise NMS (model_nms_utils.py:28-66) is one greedy NMS per scene x head x class over at most NMS_PRE_MAXSIZE boxes: dozens of small box
// sets per batch.  Here they are the segments of one (S, seg_stride, 7) block: the mask grid is (column block, row block, segment), the sweep
// one single-wave workgroup per segment, all segments at once.  A segment's valid row count is read from device memory by both kernels; rows
// at or beyond it are padding that neither kernel touches.
constexpr int NMS_SEG_MAX_WORDS = 64;                          // seg_stride <= 4096: a row of the mask is at most one word per lane

__device__ __forceinline__ int seg_rows(const int32_t* __restrict__ seg_count, int s, int seg_stride) {
  return min(max(seg_count[s], 0), seg_stride);
}

// one wave per 64x64 tile of one segment, as k_nms_mask: lane = column box, one ballot word per row
__global__ __launch_bounds__(64) void k_nms_seg_mask(const int32_t* __restrict__ seg_count, int seg_stride, float thresh, const float* __restrict__ boxes,
                                                     unsigned long long* __restrict__ mask, int col_blocks, int normal) {
  const int s = blockIdx.z, rb = blockIdx.y, cb = blockIdx.x;
  const int n = seg_rows(seg_count, s, seg_stride);
  if (cb < rb || cb * 64 >= n) return;                         // left of the diagonal, or beyond the segment's rows (cb >= rb here, so this covers rb * 64 >= n)
  boxes += (int64_t)s * seg_stride * 7;
  mask += (int64_t)s * seg_stride * col_blocks;
  nms_mask_tile(n, rb, cb, boxes, mask, col_blocks, thresh, normal);
}

// greedy sweep of one segment by one wave: the removal bitmap (<= 64 words) in LDS, lane j owns word j.  Per block of 64 boxes the diagonal
// word of each row decides suppression inside the block (64 serial steps on registers), then the kept rows are OR-ed into the words of the
// later blocks: 8 rows at a time, loaded unconditionally (row index clamped into the segment, unkept rows masked to 0) so that the 8 loads
// are in flight together.  Stops at max_keep, reads the upper triangle only and only words below ceil(n / 64).
__global__ __launch_bounds__(64) void k_nms_seg_sweep(const int32_t* __restrict__ seg_count, int seg_stride, const unsigned long long* __restrict__ mask,
                                                      int col_blocks, int max_keep, int64_t* __restrict__ keep, int32_t* __restrict__ num_out) {
  __shared__ unsigned long long remv[NMS_SEG_MAX_WORDS];
  const int s = blockIdx.x, lane = threadIdx.x;
  const int n = seg_rows(seg_count, s, seg_stride);
  const int nblk = (n + 63) / 64;                               // <= col_blocks <= 64
  mask += (int64_t)s * seg_stride * col_blocks;
  keep += (int64_t)s * max_keep;
  remv[lane] = 0ull;
  __syncthreads();
  int kept_total = 0;
  for (int nb = 0; nb < nblk && kept_total < max_keep; ++nb) {
    const int rows = min(64, n - nb * 64);
    const unsigned long long diag = lane < rows ? mask[(int64_t)(nb * 64 + lane) * col_blocks + nb] : 0ull;
    const unsigned long long keptbits = nms_resolve_block(remv[nb], diag, nb, rows, kept_total, max_keep, keep);
    kept_total += __popcll(keptbits);
    const int j = nb + 1 + lane;                                // this lane's word of the later blocks
    if (kept_total < max_keep && j < nblk) {
      unsigned long long acc = remv[j];
      const unsigned long long* col = mask + (int64_t)nb * 64 * col_blocks + j;
      for (int r0 = 0; r0 < rows; r0 += 8) {
        const unsigned kb8 = (unsigned)(keptbits >> r0) & 0xffu;
        if (!kb8) continue;
        unsigned long long v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = col[(int64_t)min(r0 + u, rows - 1) * col_blocks];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc |= ((kb8 >> u) & 1u) ? v[u] : 0ull;
      }
      remv[j] = acc;
    }
    __syncthreads();                                            // lane j's word is read as remv[nb] by the whole wave in a later round
  }
  if (lane == 0) num_out[s] = min(kept_total, max_keep);
}

extern "C" size_t sv_nms_segments_scratch_bytes(int num_segments, int seg_stride) {
  if (num_segments <= 0 || seg_stride <= 0) return 0;
  return (size_t)num_segments * (size_t)seg_stride * (size_t)((seg_stride + 63) / 64) * sizeof(unsigned long long);
}

extern "C" int sv_nms_segments(const float* boxes, const int32_t* seg_count, int num_segments, int seg_stride, float thresh, int normal, int max_keep,
                               void* scratch, int64_t* keep, int32_t* num_out, void* stream) {
  SV_CHECK_ARG(num_segments >= 0 && seg_stride >= 0 && max_keep >= 0, "nms_segments: bad arguments");
  if (num_segments == 0) return SV_OK;
  SV_CHECK_ARG(num_out && seg_count, "nms_segments: null pointer");
  SV_CHECK_ARG(num_segments <= 65535, "nms_segments: more than 65535 segments");
  hipStream_t st = sv_stream(stream);
  if (seg_stride == 0) {
    SV_HIP(hipMemsetAsync(num_out, 0, (size_t)num_segments * 4, st));
    return SV_OK;
  }
  const int cb = (seg_stride + 63) / 64;
  SV_CHECK_ARG(cb <= NMS_SEG_MAX_WORDS, "nms_segments: at most %d boxes per segment", NMS_SEG_MAX_WORDS * 64);
  SV_CHECK_ARG(boxes && scratch && (keep || max_keep == 0), "nms_segments: null pointer");
  unsigned long long* mask = reinterpret_cast<unsigned long long*>(scratch);
  hipLaunchKernelGGL(k_nms_seg_mask, dim3(cb, cb, num_segments), dim3(64), 0, st, seg_count, seg_stride, thresh, boxes, mask, cb, normal);
  hipLaunchKernelGGL(k_nms_seg_sweep, dim3(num_segments), dim3(64), 0, st, seg_count, seg_stride, mask, cb, max_keep, keep, num_out);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ------------------------------------------------------------------ points in boxes
// boxes (B,T,7), pts (B,M,3) -> idx (B,M): first box containing the point, else -1
__global__ __launch_bounds__(256) void k_points_in_boxes(int T, int M, const float* __restrict__ boxes, const float* __restrict__ pts,
                                                         int32_t* __restrict__ out) {
  extern __shared__ float sbox[];                            // [T][9]: cx cy cz dx dy dz cos(-rz) sin(-rz)
  const int b = blockIdx.y;
  for (int k = threadIdx.x; k < T; k += blockDim.x) {
    const float* bx = boxes + ((int64_t)b * T + k) * 7;
    float* s = sbox + k * 8;
    s[0] = bx[0]; s[1] = bx[1]; s[2] = bx[2]; s[3] = bx[3]; s[4] = bx[4]; s[5] = bx[5];
    s[6] = cosf(-bx[6]); s[7] = sinf(-bx[6]);
  }
  __syncthreads();
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= M) return;
  const float* p = pts + ((int64_t)b * M + m) * 3;
  const float x = p[0], y = p[1], z = p[2];
  int32_t found = -1;
  for (int k = 0; k < T; ++k) {
    const float* s = sbox + k * 8;
    float lx, ly;
    if (sv_pt_in_box3d(x, y, z, s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], 1e-5f, lx, ly)) { found = k; break; }
  }
  out[(int64_t)b * M + m] = found;
}

extern "C" int sv_points_in_boxes(const float* boxes, const float* pts, int batch, int num_boxes, int num_points, int32_t* out, void* stream) {
  SV_CHECK_ARG(batch >= 0 && num_boxes >= 0 && num_points >= 0, "points_in_boxes: bad arguments");
  if (batch == 0 || num_points == 0) return SV_OK;
  SV_CHECK_ARG(pts && out && (num_boxes == 0 || boxes), "points_in_boxes: null pointer");
  SV_CHECK_ARG((size_t)num_boxes * 32 <= 64 * 1024, "points_in_boxes: more than 2048 boxes per scene");
  dim3 grid(sv_div_up(num_points, 256), batch);
  hipLaunchKernelGGL(k_points_in_boxes, grid, dim3(256), (size_t)num_boxes * 32, sv_stream(stream), num_boxes, num_points, boxes, pts, out);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// points_in_boxes_cpu (roiaware_pool3d.cpp:121-165): (N boxes x M points) 0/1 matrix, MARGIN 1e-2 (the GPU variant uses 1e-5)
__global__ __launch_bounds__(256) void k_points_in_boxes_matrix(int N, int M, const float* __restrict__ boxes, const float* __restrict__ pts,
                                                                int32_t* __restrict__ out) {
  const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
  if (j >= M) return;
  const float* b = boxes + (size_t)i * 7;
  const float x = pts[(size_t)j * 3], y = pts[(size_t)j * 3 + 1], z = pts[(size_t)j * 3 + 2];
  float lx, ly;                                              // no table of boxes here: cosf / sinf only for the points that pass z
  const bool in = sv_pt_in_box_z(z, b[2], b[5]) && sv_pt_in_box_xy(x, y, b[0], b[1], b[3], b[4], cosf(-b[6]), sinf(-b[6]), 1e-2f, lx, ly);
  out[(size_t)i * M + j] = in ? 1 : 0;
}

extern "C" int sv_points_in_boxes_matrix(const float* boxes, const float* pts, int num_boxes, int num_points, int32_t* out, void* stream) {
  SV_CHECK_ARG(num_boxes >= 0 && num_points >= 0, "sv_points_in_boxes_matrix: negative size");
  if (num_boxes == 0 || num_points == 0) return SV_OK;
  SV_CHECK_ARG(boxes && pts && out, "sv_points_in_boxes_matrix: null pointer");
  hipLaunchKernelGGL(k_points_in_boxes_matrix, dim3(sv_div_up(num_points, 256), num_boxes), dim3(256), 0, sv_stream(stream), num_boxes,
                     num_points, boxes, pts, out);
  SV_LAUNCH_CHECK();
  return SV_OK;
}
