// The pyramid augmentor (SE-SSD's shape-aware augmentation) on the device: face dropout, sparsify and swap on the batch layout of augment.h.
//
// Reference (numpy + scipy on dataloader workers): detector3d/pcdet/datasets/augmentor/data_augmentor.py:221-242 and augmentor_utils.py:573-762
// (get_pyramids, points_in_pyramids_mask, local_pyramid_dropout, local_pyramid_sparsify, local_pyramid_swap), utils/box_utils.py:28-53 and :12-25
// (boxes_to_corners_3d, in_hull: scipy Delaunay.find_simplex >= 0).
//
// Every box has six pyramids: the box centre as apex over one face's four corners.  Membership is ONE function (pyr_member) for every kernel
// here, so that the counts the host sizes its draws and rows by and the lists the emitting kernels walk cannot disagree: float32 corners as
// boxes_to_corners_3d makes them, the five face planes in float64, closed.  Ordered ranks (the position of a member among the live members of
// its pyramid, in row order) are block scans with a running carry; the minimum and maximum of the last column are integer atomics on an
// order-preserving code.  No float atomics, no recursion, no scratch.
#include <math.h>

#include "augment.h"
#include "common.h"
#include "wave.h"

constexpr int PYR_ROW = 28;                                    // 8 corners, the centre, the squared reach of the quick reject
constexpr int PYR_MAX_K = 1024;                                // SPARSIFY_MAX_NUM the sparsify kernel holds in LDS

// pyramid_orders (augmentor_utils.py:574-581): the four base corners of face f as 3-bit corner numbers, the first in the lowest bits
__device__ __forceinline__ unsigned pyr_face_code(int f) {
  constexpr unsigned long long lo = (0ull | 1ull << 3 | 5ull << 6 | 4ull << 9) | (4ull | 5ull << 3 | 6ull << 6 | 7ull << 9) << 12 |
                                    (7ull | 6ull << 3 | 2ull << 6 | 3ull << 9) << 24;
  constexpr unsigned long long hi = (3ull | 2ull << 3 | 1ull << 6 | 0ull << 9) | (1ull | 2ull << 3 | 6ull << 6 | 5ull << 9) << 12 |
                                    (0ull | 4ull << 3 | 7ull << 6 | 3ull << 9) << 24;
  return (unsigned)((f < 3 ? lo >> (12 * f) : hi >> (12 * (f - 3))) & 0xfffull);
}

// The staged row of a box: boxes_to_corners_3d in float32, one rounding per operation (template * size, rotate_points_along_z(heading) as the
// matmul row x c + y (-s), + centre).  cos / sin are the float64 functions rounded once: the correctly rounded float32 value on every machine.
__device__ __forceinline__ void pyr_stage(float* s, const float* __restrict__ bx) {
  const float c = (float)cos((double)bx[6]), sn = (float)sin((double)bx[6]);
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const float tx = (m & 3) == 0 || (m & 3) == 1 ? 0.5f : -0.5f, ty = (m & 3) == 0 || (m & 3) == 3 ? 0.5f : -0.5f, tz = m < 4 ? -0.5f : 0.5f;
    const float lx = bx[3] * tx, ly = bx[4] * ty, lz = bx[5] * tz;
    const float x = lx * c + ly * (-sn), y = lx * sn + ly * c;
    s[3 * m] = x + bx[0], s[3 * m + 1] = y + bx[1], s[3 * m + 2] = lz + bx[2];
  }
  s[24] = bx[0], s[25] = bx[1], s[26] = bx[2];
  // no member is farther from the centre than half the diagonal; 1 % and 1e-3 m^2 on top cover the float32 rounding of corners and distance
  s[27] = 0.25f * (bx[3] * bx[3] + bx[4] * bx[4] + bx[5] * bx[5]) * 1.01f + 1e-3f;
}

__device__ __forceinline__ bool pyr_near(float x, float y, float z, const float* s) {
  const float dx = x - s[24], dy = y - s[25], dz = z - s[26];
  return dx * dx + dy * dy + dz * dz <= s[27];
}

// The closed half-space of the plane through p0 p1 p2 that holds `opp`, in float64: n = (p1 - p0) x (p2 - p0), side = n . (v - p0).
__device__ __forceinline__ bool pyr_side(double p0x, double p0y, double p0z, double p1x, double p1y, double p1z, double p2x, double p2y, double p2z,
                                         double ox, double oy, double oz, double x, double y, double z) {
  const double ax = p1x - p0x, ay = p1y - p0y, az = p1z - p0z, bx = p2x - p0x, by = p2y - p0y, bz = p2z - p0z;
  const double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
  const double so = (nx * (ox - p0x) + ny * (oy - p0y)) + nz * (oz - p0z);
  const double sp = (nx * (x - p0x) + ny * (y - p0y)) + nz * (z - p0z);
  return so >= 0.0 ? sp >= 0.0 : sp <= 0.0;
}

// in_hull(point, the 5 vertices of face f's pyramid) (augmentor_utils.py:606-611, box_utils.py:12-25): the four side planes apex q_i q_(i+1)
// against q_(i+2), the base plane q_0 q_1 q_2 against the apex.  s: the staged row.
__device__ __forceinline__ bool pyr_member(float x, float y, float z, const float* s, int f) {
  const unsigned code = pyr_face_code(f);
  double q[4][3];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = (code >> (3 * i)) & 7;
    q[i][0] = s[3 * m], q[i][1] = s[3 * m + 1], q[i][2] = s[3 * m + 2];
  }
  const double ax = s[24], ay = s[25], az = s[26], px = x, py = y, pz = z;
  bool in = pyr_side(q[0][0], q[0][1], q[0][2], q[1][0], q[1][1], q[1][2], q[2][0], q[2][1], q[2][2], ax, ay, az, px, py, pz);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int j = (i + 1) & 3, k = (i + 2) & 3;
    in = in && pyr_side(ax, ay, az, q[i][0], q[i][1], q[i][2], q[j][0], q[j][1], q[j][2], q[k][0], q[k][1], q[k][2], px, py, pz);
  }
  return in;
}

// ------------------------------------------------------------------ get_pyramids (augmentor_utils.py:573-595)
__global__ __launch_bounds__(AUG_THREADS) void k_pyr_pyramids(const float* __restrict__ boxes, int W, int total_boxes, float* __restrict__ out) {
  const int row = blockIdx.x * AUG_THREADS + threadIdx.x;
  if (row >= total_boxes) return;
  float s[PYR_ROW];
  pyr_stage(s, boxes + (int64_t)row * W);
  float* o = out + (int64_t)row * 90;
#pragma unroll
  for (int f = 0; f < 6; ++f) {
    const unsigned code = pyr_face_code(f);
    o[15 * f] = s[24], o[15 * f + 1] = s[25], o[15 * f + 2] = s[26];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int m = 0; m < 8; ++m)                              // (a select per corner keeps s in registers)
        if (m == (int)((code >> (3 * i)) & 7)) o[15 * f + 3 + 3 * i] = s[3 * m], o[15 * f + 4 + 3 * i] = s[3 * m + 1], o[15 * f + 5 + 3 * i] = s[3 * m + 2];
    }
  }
}

extern "C" int sv_get_pyramids(const float* boxes, int W, int total_boxes, float* out, void* stream) {
  SV_CHECK_ARG(W >= 7 && total_boxes >= 0, "get_pyramids: bad arguments");
  if (total_boxes == 0) return SV_OK;
  SV_CHECK_ARG(boxes && out, "get_pyramids: null pointer");
  hipLaunchKernelGGL(k_pyr_pyramids, dim3(sv_div_up(total_boxes, AUG_THREADS)), dim3(AUG_THREADS), 0, sv_stream(stream), boxes, W, total_boxes, out);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ------------------------------------------------------------------ local_pyramid_dropout (augmentor_utils.py:614-627)
// The scene's marked boxes (face 0..5, box_cls != -2) are staged through LDS in box order; a thread per point clears its flag at the first hit.
__global__ __launch_bounds__(AUG_THREADS) void k_pyr_dropout(const float* __restrict__ points, int C, const int32_t* __restrict__ pt_start,
                                                             const int32_t* __restrict__ pt_cnt, int32_t* __restrict__ keep,
                                                             const float* __restrict__ boxes, int W, const int32_t* __restrict__ box_start,
                                                             const int32_t* __restrict__ box_cnt, const int32_t* __restrict__ box_cls,
                                                             const int32_t* __restrict__ face) {
  __shared__ float sb[AUG_MAX_BOXES][PYR_ROW];
  __shared__ int32_t sf[AUG_MAX_BOXES];
  __shared__ int32_t wave_sums[AUG_THREADS / SV_WAVE];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int b0 = box_start[b], nb = aug_box_count(box_cnt, b);
  if (nb == 0) return;
  const int32_t fc = tid < nb ? face[b0 + tid] : -1;
  const bool marked = tid < nb && box_cls[b0 + tid] != -2 && fc >= 0 && fc < 6;
  int32_t n;
  const int32_t slot = sv_block_excl_scan<AUG_THREADS>((int32_t)marked, &n, wave_sums);
  if (marked) {
    pyr_stage(sb[slot], boxes + (int64_t)(b0 + tid) * W);
    sf[slot] = fc;
  }
  __syncthreads();
  const int i = blockIdx.x * AUG_THREADS + tid;
  if (n == 0 || i >= pt_cnt[b]) return;
  const int64_t p = (int64_t)pt_start[b] + i;
  if (!keep[p]) return;
  const float x = points[p * C], y = points[p * C + 1], z = points[p * C + 2];
  for (int k = 0; k < n; ++k) {
    if (pyr_near(x, y, z, sb[k]) && pyr_member(x, y, z, sb[k], sf[k])) {
      keep[p] = 0;
      return;
    }
  }
}

extern "C" int sv_pyramid_dropout(const float* points, int C, const int32_t* pt_start, const int32_t* pt_cnt, int32_t* keep, int batch,
                                  int max_scene_points, const float* boxes, int W, const int32_t* box_start, const int32_t* box_cnt,
                                  const int32_t* box_cls, const int32_t* face, void* stream) {
  SV_CHECK_ARG(batch >= 0 && max_scene_points >= 0 && C >= 3 && W >= 7, "pyramid_dropout: bad arguments");
  if (batch == 0 || max_scene_points == 0) return SV_OK;
  SV_CHECK_ARG(points && pt_start && pt_cnt && keep && boxes && box_start && box_cnt && box_cls && face && batch <= 65535,
               "pyramid_dropout: null pointer or batch > 65535");
  hipLaunchKernelGGL(k_pyr_dropout, dim3(sv_div_up(max_scene_points, AUG_THREADS), batch), dim3(AUG_THREADS), 0, sv_stream(stream), points, C,
                     pt_start, pt_cnt, keep, boxes, W, box_start, box_cnt, box_cls, face);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ------------------------------------------------------------------ points per pyramid (points_in_pyramids_mask(...).sum(0), :643-644, :690-691)
// mask: 6 bits per box row, the faces asked for.  counts (total_boxes, 6) int32: live member points, summed in LDS first.  member (may be NULL):
// one byte per (point row, box of its scene), the faces among those asked for whose pyramid holds the point; zeroed by the caller.
__global__ __launch_bounds__(AUG_THREADS) void k_pyr_count(const float* __restrict__ points, int C, const int32_t* __restrict__ pt_start,
                                                           const int32_t* __restrict__ pt_cnt, const int32_t* __restrict__ keep,
                                                           const float* __restrict__ boxes, int W, const int32_t* __restrict__ box_start,
                                                           const int32_t* __restrict__ box_cnt, const int32_t* __restrict__ box_cls,
                                                           const int32_t* __restrict__ mask, int32_t* __restrict__ counts,
                                                           uint8_t* __restrict__ member, int member_stride) {
  __shared__ float sb[AUG_MAX_BOXES][PYR_ROW];
  __shared__ int32_t sm[AUG_MAX_BOXES], sk[AUG_MAX_BOXES];
  __shared__ int32_t sc[AUG_MAX_BOXES * 6];
  __shared__ int32_t wave_sums[AUG_THREADS / SV_WAVE];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int b0 = box_start[b], nb = aug_box_count(box_cnt, b);
  if (nb == 0) return;
  const int32_t mk = tid < nb && box_cls[b0 + tid] != -2 ? (mask[b0 + tid] & 63) : 0;
  int32_t n;
  const int32_t slot = sv_block_excl_scan<AUG_THREADS>((int32_t)(mk != 0), &n, wave_sums);
  if (mk) {
    pyr_stage(sb[slot], boxes + (int64_t)(b0 + tid) * W);
    sm[slot] = mk, sk[slot] = tid;
  }
  for (int t = tid; t < AUG_MAX_BOXES * 6; t += AUG_THREADS) sc[t] = 0;
  __syncthreads();
  if (n == 0) return;
  const int i = blockIdx.x * AUG_THREADS + tid;
  if (i < pt_cnt[b]) {
    const int64_t p = (int64_t)pt_start[b] + i;
    if (keep[p]) {
      const float x = points[p * C], y = points[p * C + 1], z = points[p * C + 2];
      for (int k = 0; k < n; ++k) {
        if (!pyr_near(x, y, z, sb[k])) continue;
        const int m = sm[k];
        int bits = 0;
        for (int f = 0; f < 6; ++f)
          if (((m >> f) & 1) && pyr_member(x, y, z, sb[k], f)) {
            atomicAdd(&sc[k * 6 + f], 1);
            bits |= 1 << f;
          }
        if (member && bits && sk[k] < member_stride) member[p * member_stride + sk[k]] = (uint8_t)bits;
      }
    }
  }
  __syncthreads();
  for (int t = tid; t < n * 6; t += AUG_THREADS)
    if (sc[t]) atomicAdd(&counts[(int64_t)(b0 + sk[t / 6]) * 6 + t % 6], sc[t]);
}

extern "C" int sv_pyramid_count(const float* points, int C, const int32_t* pt_start, const int32_t* pt_cnt, const int32_t* keep, int batch,
                                int max_scene_points, const float* boxes, int W, const int32_t* box_start, const int32_t* box_cnt,
                                const int32_t* box_cls, int total_boxes, const int32_t* mask, int32_t* counts, uint8_t* member, int member_stride,
                                void* stream) {
  SV_CHECK_ARG(batch >= 0 && max_scene_points >= 0 && total_boxes >= 0 && C >= 3 && W >= 7 && member_stride >= 0, "pyramid_count: bad arguments");
  if (total_boxes == 0) return SV_OK;
  SV_CHECK_ARG(counts, "pyramid_count: null pointer");
  SV_HIP(hipMemsetAsync(counts, 0, (size_t)total_boxes * 6 * 4, sv_stream(stream)));
  if (batch == 0 || max_scene_points == 0) return SV_OK;
  SV_CHECK_ARG(points && pt_start && pt_cnt && keep && boxes && box_start && box_cnt && box_cls && mask && batch <= 65535,
               "pyramid_count: null pointer or batch > 65535");
  hipLaunchKernelGGL(k_pyr_count, dim3(sv_div_up(max_scene_points, AUG_THREADS), batch), dim3(AUG_THREADS), 0, sv_stream(stream), points, C, pt_start,
                     pt_cnt, keep, boxes, W, box_start, box_cnt, box_cls, mask, counts, member, member_stride);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ------------------------------------------------------------------ what the two emitting kernels share
// flag bits: 1 a pyramid's member count differs from the count the host planned with, 2 an output row outside the scene's rows, 4 a plan row that
// names no scene / box / face.  Raised, never clamped: the host turns a non-zero flag into an error at its next read.
constexpr int PYR_FLAG_COUNT = 1, PYR_FLAG_ROW = 2, PYR_FLAG_PLAN = 4;

__device__ __forceinline__ void pyr_copy_row(float* __restrict__ points, int C, int64_t dst, int64_t src) {
  const uint32_t* s = reinterpret_cast<const uint32_t*>(points) + src * C;
  uint32_t* d = reinterpret_cast<uint32_t*>(points) + dst * C;
  for (int c = 0; c < C; ++c) d[c] = s[c];
}

// ------------------------------------------------------------------ local_pyramid_sparsify, the valid pyramids (augmentor_utils.py:647-659)
// One workgroup per pyramid.  pyr (n, 5) int32: scene, box row, face, the member count the host read, the first output row.  ranks (n, K): the
// chosen members in choice order (np.random.choice(count, K, replace=False)), as ranks among the pyramid's live members in row order.  The sweep
// over the scene's rows reads liveness from keep_in (the flags on entry: pyramids that share a point each see it), clears every member's flag in
// keep and copies the member of rank ranks[j][q] to row out + q, whose flag it sets.
__global__ __launch_bounds__(AUG_THREADS) void k_pyr_sparsify(float* __restrict__ points, int C, const int32_t* __restrict__ pt_start,
                                                              const int32_t* __restrict__ pt_cnt, const int32_t* __restrict__ keep_in,
                                                              int32_t* __restrict__ keep, int batch, const float* __restrict__ boxes, int W,
                                                              int total_boxes, const int32_t* __restrict__ pyr, const int32_t* __restrict__ ranks,
                                                              int K, int32_t* __restrict__ flag) {
  __shared__ float s[PYR_ROW];
  __shared__ int32_t sr[PYR_MAX_K];
  __shared__ int32_t wave_sums[AUG_THREADS / SV_WAVE];
  const int j = blockIdx.x, tid = threadIdx.x;
  const int32_t* pj = pyr + (int64_t)j * 5;
  const int b = pj[0], row = pj[1], f = pj[2], expected = pj[3], out = pj[4];
  if (b < 0 || b >= batch || row < 0 || row >= total_boxes || f < 0 || f >= 6) {   // (uniform over the workgroup)
    if (tid == 0) atomicOr(flag, PYR_FLAG_PLAN);
    return;
  }
  const int64_t p0 = pt_start[b];
  const int cnt = pt_cnt[b];
  if (out < p0 || (int64_t)out + K > p0 + cnt) {
    if (tid == 0) atomicOr(flag, PYR_FLAG_ROW);
    return;
  }
  if (tid == 0) pyr_stage(s, boxes + (int64_t)row * W);
  for (int q = tid; q < K; q += AUG_THREADS) sr[q] = ranks[(int64_t)j * K + q];
  __syncthreads();
  int32_t carry = 0;
  for (int base = 0; base < cnt; base += AUG_THREADS) {
    const int i = base + tid;
    const int64_t p = p0 + i;
    bool m = false;
    if (i < cnt && keep_in[p]) {
      const float x = points[p * C], y = points[p * C + 1], z = points[p * C + 2];
      m = pyr_near(x, y, z, s) && pyr_member(x, y, z, s, f);
    }
    int32_t total;
    const int32_t rank = carry + sv_block_excl_scan<AUG_THREADS>((int32_t)m, &total, wave_sums);
    if (m) {
      keep[p] = 0;
      for (int q = 0; q < K; ++q)
        if (sr[q] == rank) {                                   // (the ranks of a choice are distinct)
          pyr_copy_row(points, C, (int64_t)out + q, p);
          keep[out + q] = 1;
          break;
        }
    }
    carry += total;
    __syncthreads();                                           // wave_sums is free again
  }
  if (tid == 0 && carry != expected) atomicOr(flag, PYR_FLAG_COUNT);
}

extern "C" int sv_pyramid_sparsify(float* points, int C, const int32_t* pt_start, const int32_t* pt_cnt, const int32_t* keep_in, int32_t* keep,
                                   int batch, const float* boxes, int W, int total_boxes, const int32_t* pyr, int num_pyramids,
                                   const int32_t* ranks, int K, int32_t* flag, void* stream) {
  SV_CHECK_ARG(batch >= 0 && C >= 3 && W >= 7 && total_boxes >= 0 && num_pyramids >= 0 && K >= 0 && K <= PYR_MAX_K,
               "pyramid_sparsify: bad arguments (0 <= SPARSIFY_MAX_NUM <= %d)", PYR_MAX_K);
  if (num_pyramids == 0) return SV_OK;
  SV_CHECK_ARG(points && pt_start && pt_cnt && keep_in && keep && keep_in != keep && boxes && pyr && (ranks || K == 0) && flag,
               "pyramid_sparsify: null pointer, or keep_in is keep");
  hipLaunchKernelGGL(k_pyr_sparsify, dim3(num_pyramids), dim3(AUG_THREADS), 0, sv_stream(stream), points, C, pt_start, pt_cnt, keep_in, keep, batch,
                     boxes, W, total_boxes, pyr, ranks, K, flag);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ------------------------------------------------------------------ local_pyramid_swap, the pairs (augmentor_utils.py:664-682, :720-758)
// get_points_ratio / recover_points_by_ratio in float32, one rounding per operation (the library is built with contraction off; sums of three run
// left to right, as numpy's do).  fr: q0 (3), v0, v1, v2, the surface centre, |v0|^2 |v1|^2 |v2|^2.
__device__ __forceinline__ void pyr_frame(float* fr, const float* s, int f) {
  const unsigned code = pyr_face_code(f);
  const int m0 = code & 7, m1 = (code >> 3) & 7, m2 = (code >> 6) & 7, m3 = (code >> 9) & 7;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float q0 = s[3 * m0 + c], q1 = s[3 * m1 + c], q2 = s[3 * m2 + c], q3 = s[3 * m3 + c];
    const float sc = (((q0 + q1) + q2) + q3) / 4.0f;
    fr[c] = q0, fr[3 + c] = q1 - q0, fr[6 + c] = q3 - q0, fr[9 + c] = s[24 + c] - sc, fr[12 + c] = sc;
  }
#pragma unroll
  for (int v = 0; v < 3; ++v) fr[15 + v] = (fr[3 + 3 * v] * fr[3 + 3 * v] + fr[4 + 3 * v] * fr[4 + 3 * v]) + fr[5 + 3 * v] * fr[5 + 3 * v];
}

__device__ __forceinline__ void pyr_ratio(const float* fr, float x, float y, float z, float& al, float& be, float& ga) {
  const float ax = x - fr[0], ay = y - fr[1], az = z - fr[2], cx = x - fr[12], cy = y - fr[13], cz = z - fr[14];
  al = ((ax * fr[3] + ay * fr[4]) + az * fr[5]) / fr[15];
  be = ((ax * fr[6] + ay * fr[7]) + az * fr[8]) / fr[16];
  ga = ((cx * fr[9] + cy * fr[10]) + cz * fr[11]) / fr[17];
}

__device__ __forceinline__ float pyr_recover(const float* fr, int c, float al, float be, float ga) {
  return ((al * fr[3 + c] + be * fr[6 + c]) + fr[c]) + ga * fr[9 + c];
}

__device__ __forceinline__ float pyr_clip_span(float d) { return fminf(fmaxf(d, 1e-6f), 1.0f); }   // np.clip(max - min, 1e-6, 1) in float32

// One workgroup per pair.  pairs (n, 8) int32: scene, the to-swap pyramid's box row, face and member count, the partner's three, the first output
// row.  Two sweeps over the scene's rows on the entry flags (keep_in): the first counts both pyramids' members and reduces the minimum and maximum
// of the last column (integer atomics on sv_ordered_f32); the second ranks the members in row order and writes the partner's points mapped into the
// to-swap pyramid to rows out .. out + |partner|, then the to-swap pyramid's points mapped into the partner, sets those rows' flags and clears the
// members'.  C == 4: the reference re-assembles x y z and the last column.
__global__ __launch_bounds__(AUG_THREADS) void k_pyr_swap(float* __restrict__ points, const int32_t* __restrict__ pt_start,
                                                          const int32_t* __restrict__ pt_cnt, const int32_t* __restrict__ keep_in,
                                                          int32_t* __restrict__ keep, int batch, const float* __restrict__ boxes, int W,
                                                          int total_boxes, const int32_t* __restrict__ pairs, int32_t* __restrict__ flag) {
  constexpr int C = 4;
  __shared__ float sa[PYR_ROW], sb[PYR_ROW], fa[18], fb[18];
  __shared__ uint32_t lo[2], hi[2];
  __shared__ int32_t tot[2];
  __shared__ int32_t wave_a[AUG_THREADS / SV_WAVE], wave_b[AUG_THREADS / SV_WAVE];
  const int tid = threadIdx.x;
  const int32_t* pr = pairs + (int64_t)blockIdx.x * 8;
  const int b = pr[0], row_a = pr[1], f_a = pr[2], cnt_a = pr[3], row_b = pr[4], f_b = pr[5], cnt_b = pr[6], out = pr[7];
  if (b < 0 || b >= batch || row_a < 0 || row_a >= total_boxes || row_b < 0 || row_b >= total_boxes || f_a < 0 || f_a >= 6 || f_b < 0 || f_b >= 6 ||
      cnt_a < 0 || cnt_b < 0) {
    if (tid == 0) atomicOr(flag, PYR_FLAG_PLAN);
    return;
  }
  const int64_t p0 = pt_start[b];
  const int cnt = pt_cnt[b];
  if (out < p0 || (int64_t)out + cnt_a + cnt_b > p0 + cnt) {
    if (tid == 0) atomicOr(flag, PYR_FLAG_ROW);
    return;
  }
  if (tid == 0) {
    pyr_stage(sa, boxes + (int64_t)row_a * W);
    pyr_frame(fa, sa, f_a);
    lo[0] = lo[1] = 0xffffffffu, hi[0] = hi[1] = 0u, tot[0] = tot[1] = 0;
  }
  if (tid == SV_WAVE) {
    pyr_stage(sb, boxes + (int64_t)row_b * W);
    pyr_frame(fb, sb, f_b);
  }
  __syncthreads();
  for (int base = 0; base < cnt; base += AUG_THREADS) {       // sweep 1: counts, minimum and maximum of the last column
    const int i = base + tid;
    const int64_t p = p0 + i;
    bool ma = false, mb = false;
    uint32_t e = 0;
    if (i < cnt && keep_in[p]) {
      const float x = points[p * C], y = points[p * C + 1], z = points[p * C + 2];
      ma = pyr_near(x, y, z, sa) && pyr_member(x, y, z, sa, f_a);
      mb = pyr_near(x, y, z, sb) && pyr_member(x, y, z, sb, f_b);
      e = sv_ordered_f32(points[p * C + 3]);
    }
    int na, nb;
    sv_wave_ballot_rank(ma, &na);
    sv_wave_ballot_rank(mb, &nb);
    const uint32_t la = sv_wave_reduce_min(ma ? e : 0xffffffffu), ha = sv_wave_reduce_max(ma ? e : 0u);
    const uint32_t lb = sv_wave_reduce_min(mb ? e : 0xffffffffu), hb = sv_wave_reduce_max(mb ? e : 0u);
    if ((tid & (SV_WAVE - 1)) == 0) {
      if (na) atomicAdd(&tot[0], na), atomicMin(&lo[0], la), atomicMax(&hi[0], ha);
      if (nb) atomicAdd(&tot[1], nb), atomicMin(&lo[1], lb), atomicMax(&hi[1], hb);
    }
  }
  __syncthreads();
  if (tot[0] != cnt_a || tot[1] != cnt_b || cnt_a == 0 || cnt_b == 0) {   // nothing is written on a mismatch
    if (tid == 0) atomicOr(flag, PYR_FLAG_COUNT);
    return;
  }
  const float min_a = sv_unordered_f32(lo[0]), max_a = sv_unordered_f32(hi[0]), min_b = sv_unordered_f32(lo[1]), max_b = sv_unordered_f32(hi[1]);
  const float span_a = max_a - min_a, span_b = max_b - min_b;
  int32_t carry_a = 0, carry_b = 0;
  for (int base = 0; base < cnt; base += AUG_THREADS) {       // sweep 2: ordered ranks, the two blocks
    const int i = base + tid;
    const int64_t p = p0 + i;
    bool ma = false, mb = false;
    float x = 0.f, y = 0.f, z = 0.f, w = 0.f;
    if (i < cnt && keep_in[p]) {
      x = points[p * C], y = points[p * C + 1], z = points[p * C + 2], w = points[p * C + 3];
      ma = pyr_near(x, y, z, sa) && pyr_member(x, y, z, sa, f_a);
      mb = pyr_near(x, y, z, sb) && pyr_member(x, y, z, sb, f_b);
    }
    int32_t ta, tb;
    const int32_t ra = carry_a + sv_block_excl_scan<AUG_THREADS>((int32_t)ma, &ta, wave_a);
    const int32_t rb = carry_b + sv_block_excl_scan<AUG_THREADS>((int32_t)mb, &tb, wave_b);
    if (mb && rb < cnt_b) {                                    // new_to_swap_points: the partner's ratios recovered in the to-swap pyramid (:741, :744)
      float al, be, ga;
      pyr_ratio(fb, x, y, z, al, be, ga);
      float* o = points + ((int64_t)out + rb) * C;
      o[0] = pyr_recover(fa, 0, al, be, ga), o[1] = pyr_recover(fa, 1, al, be, ga), o[2] = pyr_recover(fa, 2, al, be, ga);
      o[3] = (w - min_b) / pyr_clip_span(span_b) * span_a + min_a;
      keep[(int64_t)out + rb] = 1;
    }
    if (ma && ra < cnt_a) {                                    // new_swapped_points: the to-swap ratios recovered in the partner (:742, :747)
      float al, be, ga;
      pyr_ratio(fa, x, y, z, al, be, ga);
      float* o = points + ((int64_t)out + cnt_b + ra) * C;
      o[0] = pyr_recover(fb, 0, al, be, ga), o[1] = pyr_recover(fb, 1, al, be, ga), o[2] = pyr_recover(fb, 2, al, be, ga);
      o[3] = (w - min_a) / pyr_clip_span(span_a) * span_b + min_b;
      keep[(int64_t)out + cnt_b + ra] = 1;
    }
    if (ma || mb) keep[p] = 0;
    carry_a += ta, carry_b += tb;
    __syncthreads();                                           // wave_a / wave_b are free again
  }
}

extern "C" int sv_pyramid_swap(float* points, int C, const int32_t* pt_start, const int32_t* pt_cnt, const int32_t* keep_in, int32_t* keep, int batch,
                               const float* boxes, int W, int total_boxes, const int32_t* pairs, int num_pairs, int32_t* flag, void* stream) {
  SV_CHECK_ARG(batch >= 0 && W >= 7 && total_boxes >= 0 && num_pairs >= 0, "pyramid_swap: bad arguments");
  SV_CHECK_ARG(C == 4, "pyramid_swap: %d point columns; the swap re-assembles x y z and the last column, the reference raises for any C but 4", C);
  if (num_pairs == 0) return SV_OK;
  SV_CHECK_ARG(points && pt_start && pt_cnt && keep_in && keep && keep_in != keep && boxes && pairs && flag,
               "pyramid_swap: null pointer, or keep_in is keep");
  hipLaunchKernelGGL(k_pyr_swap, dim3(num_pairs), dim3(AUG_THREADS), 0, sv_stream(stream), points, pt_start, pt_cnt, keep_in, keep, batch, boxes, W,
                     total_boxes, pairs, flag);
  SV_LAUNCH_CHECK();
  return SV_OK;
}
