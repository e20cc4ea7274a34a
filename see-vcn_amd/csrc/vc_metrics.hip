// VCN validation metrics (see/surface_completion/models/vcn/utils/metrics.py: Metrics.get; losses.get_oob_error; bbox_utils.get_oob_points,
// get_bbox_from_keypoints; transform.rotm_to_heading): every per-object quantity once, then the 30 values of the whole batch and the four num_pts
// levels from the table.  The reference recomputes each metric per group on a masked copy of the batch with one .item() each; the work per object
// is the same for every group.
//
// k_vc_metrics_objects: ONE workgroup of VCM_THREADS = 1024 (16 waves) per object, no float atomics, no per-point output, no scratch.
//   LDS: the object's coarse cloud as float4 {x, y, z, flag} (16 n bytes, resident for the whole kernel) and one region used in turn as the tile of
//   the complete cloud (VCM_TILE = 1024 rows of 16 bytes) and as the sort buffer (4 bytes x the power of two >= 3 n), plus 768 bytes of wave partials:
//   33.5 KB at n = 1024, 128.8 KB at the largest n = VCM_MAX_N = 4096 (inside 160 KB).  m is unlimited.
//   Per-point distance: k_chamfer_nn's fp32 (dx*dx + dy*dy) + dz*dz, minimum over the other cloud.
//   SUMMATION ORDER of every per-object sum (d, sqrt d, both directions, with and without the zero-sum rows): thread t adds its rows t, t + 1024,
//   t + 2048, ... in ascending row order starting from +0.0f; the 64 lanes of a wave are combined by wave.h's xor butterfly (d = 32 ... 1); thread 0's
//   copy of the 16 wave partials is added in ascending wave order.  All fp32, one rounding per addition; sqrtf is correctly rounded.
//   A zero-sum row is one with (x + y) + z == 0 in fp32.  The stripped sums run over the surviving rows and take the minimum over the surviving rows
//   of the other cloud; without a zero-sum row in either cloud they are the unstripped sums bit for bit.  When the other cloud has no surviving row
//   the stripped sums of that direction are stored as 0 (the counts say that the value is void).
//   Box: centre = (max + min) / 2, extents = max - min of (p - centre) rotated by the ground-truth heading (cosf / sinf, fp32, one rounding per
//   operation), heading = ground truth; 3-D IoU with the ground-truth box by k_boxes_iou3d's expressions on rbox.h's overlap_area, diagonal pair only.
//   Out of box, float64 on the float32 inputs: d = p - centre, c = cos(h), s = sin(h), lx = d.x * c + d.y * s, ly = -d.x * s + d.y * c; inside iff
//   |lx| <= l / 2 && |ly| <= w / 2 && |d.z| <= h / 2 (opd_to_boxpts' cuboid, inclusive).  num_oob: distinct rows outside; num_pc: distinct scalars among
//   the 3 n coordinates (-0.0 == 0.0 in both); both by a bitonic sort in LDS and a count of the first elements of the runs.
// k_vc_metrics_levels: one workgroup; threads 0 .. 4 each sum one group (whole batch, L1 .. L4) over the objects in ascending index, fp32; the lower
//   median of the heading errors by rank counting (ties broken by object index).
#include <math.h>

#include "common.h"
#include "rbox.h"
#include "wave.h"

#define VCM_THREADS 1024
#define VCM_WAVES (VCM_THREADS / SV_WAVE)
#define VCM_TILE 1024
#define VCM_MAX_N 4096
#define VCM_MAX_B 4096
#define VCM_PAD 0xffffffffu

// table columns (SV_VCM_* in the header)
enum {
  C_D1 = 0, C_S1, C_D2, C_S2, C_ZD1, C_ZS1, C_ZD2, C_ZS2, C_NZ1, C_NZ2, C_BOX, C_IOU = C_BOX + 6, C_NOOB, C_NPC, C_OOB, C_ROT, C_TRANS, C_N, C_M,
  C_COLS
};
static_assert(C_COLS == SV_VCM_COLS, "table layout differs from the header");

// v combined over the workgroup: the wave butterfly, then the wave partials in ascending wave order; every thread gets the result.  part: VCM_WAVES
// 8-byte words of LDS, free again after the call's second barrier only for a caller that syncs before writing them -- the first barrier here does that.
template <class T, class Op>
__device__ __forceinline__ T vcm_block_reduce(T v, Op op, unsigned long long* part) {
  T* p = reinterpret_cast<T*>(part);
  v = sv_wave_reduce(v, op);
  __syncthreads();
  if ((threadIdx.x & (SV_WAVE - 1)) == 0) p[threadIdx.x / SV_WAVE] = v;
  __syncthreads();
  T r = p[0];
#pragma unroll 1
  for (int w = 1; w < VCM_WAVES; ++w) r = op(r, p[w]);
  return r;
}
template <class T>
__device__ __forceinline__ T vcm_block_sum(T v, unsigned long long* part) { return vcm_block_reduce(v, [](T a, T b) { return a + b; }, part); }

// component-wise minimum and maximum of three floats over the workgroup, two barriers in all
__device__ __forceinline__ void vcm_block_bounds(float (&mn)[3], float (&mx)[3], unsigned long long* part) {
  float* p = reinterpret_cast<float*>(part);
#pragma unroll
  for (int k = 0; k < 3; ++k) mn[k] = sv_wave_reduce_min(mn[k]), mx[k] = sv_wave_reduce_max(mx[k]);
  __syncthreads();
  if ((threadIdx.x & (SV_WAVE - 1)) == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) p[(threadIdx.x / SV_WAVE) * 6 + k] = mn[k], p[(threadIdx.x / SV_WAVE) * 6 + 3 + k] = mx[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 3; ++k) mn[k] = p[k], mx[k] = p[3 + k];
#pragma unroll 1                                                  // (unrolled, the 96 partials are loaded at once and spill)
  for (int w = 1; w < VCM_WAVES; ++w) {
#pragma unroll
    for (int k = 0; k < 3; ++k) mn[k] = fminf(mn[k], p[w * 6 + k]), mx[k] = fmaxf(mx[k], p[w * 6 + 3 + k]);
  }
}

// The R own points against rows[0 .. cnt) in LDS (every lane reads the same row: a broadcast): best = minimum over all rows, best_nz = minimum over
// the rows whose flag is set.  has_zero (workgroup-uniform): some row's flag is clear; without one the flag is not looked at.
template <int R>
__device__ __forceinline__ void vcm_scan(const float4* __restrict__ rows, int cnt, bool has_zero, const float (&x)[R], const float (&y)[R],
                                         const float (&z)[R], float (&best)[R], float (&best_nz)[R]) {
  float tb[R], tz[R];
#pragma unroll
  for (int r = 0; r < R; ++r) tb[r] = INFINITY, tz[r] = INFINITY;
  if (!has_zero) {
    for (int k = 0; k < cnt; ++k) {
      const float4 q = rows[k];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float dx = q.x - x[r], dy = q.y - y[r], dz = q.z - z[r];
        tb[r] = fminf(tb[r], (dx * dx + dy * dy) + dz * dz);
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) tz[r] = tb[r];
  } else {
    for (int k = 0; k < cnt; ++k) {
      const float4 q = rows[k];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float dx = q.x - x[r], dy = q.y - y[r], dz = q.z - z[r];
        const float d = (dx * dx + dy * dy) + dz * dz;
        tb[r] = fminf(tb[r], d);
        if (q.w != 0.f) tz[r] = fminf(tz[r], d);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) best[r] = fminf(best[r], tb[r]), best_nz[r] = fminf(best_nz[r], tz[r]);
}

// Ascending bitonic sort of a[0 .. P) (P a power of two) by the whole workgroup; ends with a barrier.
template <class Less>
__device__ __forceinline__ void vcm_bitonic(uint32_t* a, int P, Less less) {
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int t = threadIdx.x; t < P / 2; t += VCM_THREADS) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const uint32_t u = a[i], v = a[l];
        if ((i & k) == 0 ? less(v, u) : less(u, v)) a[i] = v, a[l] = u;
      }
    }
  __syncthreads();
}

__device__ __forceinline__ int vcm_pow2_at_least(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

__global__ __launch_bounds__(VCM_THREADS) void k_vc_metrics_objects(const float* __restrict__ coarse, int n, const float* __restrict__ complete, int m,
                                                                    const float* __restrict__ gt_boxes, const float* __restrict__ reg_rot,
                                                                    const float* __restrict__ reg_centre, float* __restrict__ table) {
  extern __shared__ float4 s_dyn[];
  __shared__ unsigned long long s_part[VCM_WAVES * 6];
  __shared__ P2 s_poly[24];                                       // overlap_area's polygon, in LDS: private arrays indexed at run time are scratch
  __shared__ float s_ang[24];
  float4* s_c = s_dyn;                                            // [n] the coarse cloud, resident
  float4* s_tile = s_dyn + n;                                     // [VCM_TILE] a tile of the complete cloud, later ...
  uint32_t* s_keys = reinterpret_cast<uint32_t*>(s_dyn + n);      // ... the sort buffer
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* pc = coarse + (size_t)b * n * 3;
  const float* box = gt_boxes + (size_t)b * 7;
  float* row = table + (size_t)b * C_COLS;
  int32_t* irow = reinterpret_cast<int32_t*>(row);

  // ---- stage the coarse cloud (-0.0 -> +0.0: the same distances and sums, and equal rows get equal bits), its bounds and surviving rows
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  int own_nz = 0;
  for (int i = tid; i < n; i += VCM_THREADS) {
    const float x = pc[i * 3] + 0.f, y = pc[i * 3 + 1] + 0.f, z = pc[i * 3 + 2] + 0.f;
    const bool nz = (x + y) + z != 0.f;
    s_c[i] = make_float4(x, y, z, nz ? 1.f : 0.f);
    own_nz += nz;
    mn[0] = fminf(mn[0], x), mn[1] = fminf(mn[1], y), mn[2] = fminf(mn[2], z);
    mx[0] = fmaxf(mx[0], x), mx[1] = fmaxf(mx[1], y), mx[2] = fmaxf(mx[2], z);
  }
  const int n1_nz = vcm_block_sum(own_nz, s_part);                // (its barriers publish s_c)
  vcm_block_bounds(mn, mx, s_part);

  // ---- Chamfer, coarse -> complete: a thread per coarse row, the complete cloud through the tile
  float a_d1 = 0.f, a_s1 = 0.f, a_zd1 = 0.f, a_zs1 = 0.f, a_d2 = 0.f, a_s2 = 0.f, a_zd2 = 0.f, a_zs2 = 0.f;
  int n2_nz = 0;
  if (m > 0) {
    const float* pm = complete + (size_t)b * m * 3;
    for (int i0 = 0; i0 < n; i0 += VCM_THREADS) {
      const int i = i0 + tid;
      const bool live = i < n;
      const float4 own = s_c[live ? i : 0];
      const float x[1] = {own.x}, y[1] = {own.y}, z[1] = {own.z};
      float best[1] = {INFINITY}, best_nz[1] = {INFINITY};
      for (int k2 = 0; k2 < m; k2 += VCM_TILE) {
        const int cnt = min(m - k2, VCM_TILE);
        __syncthreads();                                          // the tile is free
        bool zero_here = false;
        for (int t = tid; t < cnt; t += VCM_THREADS) {
          const float* q = pm + (size_t)(k2 + t) * 3;
          const float qx = q[0], qy = q[1], qz = q[2];
          const bool nz = (qx + qy) + qz != 0.f;
          s_tile[t] = make_float4(qx, qy, qz, nz ? 1.f : 0.f);
          zero_here |= !nz;
        }
        const bool has_zero = __syncthreads_or(zero_here) != 0;
        vcm_scan<1>(s_tile, cnt, has_zero, x, y, z, best, best_nz);
      }
      if (live) {
        a_d1 = a_d1 + best[0], a_s1 = a_s1 + sqrtf(best[0]);
        if (own.w != 0.f) a_zd1 = a_zd1 + best_nz[0], a_zs1 = a_zs1 + sqrtf(best_nz[0]);
      }
    }
    // ---- complete -> coarse: four complete rows a thread against the resident coarse cloud
    const bool coarse_has_zero = n1_nz < n;
    for (int j0 = 0; j0 < m; j0 += VCM_THREADS * 4) {
      float x[4], y[4], z[4], best[4], best_nz[4];
      bool live[4], nz[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = j0 + r * VCM_THREADS + tid;
        live[r] = j < m;
        const float* q = pm + (size_t)(live[r] ? j : 0) * 3;
        x[r] = q[0], y[r] = q[1], z[r] = q[2];
        nz[r] = (x[r] + y[r]) + z[r] != 0.f;
        best[r] = INFINITY, best_nz[r] = INFINITY;
      }
      vcm_scan<4>(s_c, n, coarse_has_zero, x, y, z, best, best_nz);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (!live[r]) continue;
        a_d2 = a_d2 + best[r], a_s2 = a_s2 + sqrtf(best[r]);
        if (nz[r]) a_zd2 = a_zd2 + best_nz[r], a_zs2 = a_zs2 + sqrtf(best_nz[r]), ++n2_nz;
      }
    }
    n2_nz = vcm_block_sum(n2_nz, s_part);
    if (n2_nz == 0) a_zd1 = 0.f, a_zs1 = 0.f;                     // nothing to take a minimum over: void, not +inf
    if (n1_nz == 0) a_zd2 = 0.f, a_zs2 = 0.f;
  }
  {                                                               // every phase's results leave at once: nothing is held across the next phase
    const float sums[8] = {a_d1, a_s1, a_d2, a_s2, a_zd1, a_zs1, a_zd2, a_zs2};   // in column order
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float v = vcm_block_sum(sums[k], s_part);
      if (tid == 0) row[C_D1 + k] = v;
    }
    if (tid == 0) irow[C_NZ1] = n1_nz, irow[C_NZ2] = n2_nz, irow[C_N] = n, irow[C_M] = m;
  }

  // ---- box from the key points: extents of (p - centre) in the ground-truth heading frame
  const float heading = box[6];
  const float cx = (mx[0] + mn[0]) / 2.f, cy = (mx[1] + mn[1]) / 2.f, cz = (mx[2] + mn[2]) / 2.f;
  {
    const float c = cosf(heading), s = sinf(heading);
    mn[0] = mn[1] = mn[2] = INFINITY, mx[0] = mx[1] = mx[2] = -INFINITY;
    for (int i = tid; i < n; i += VCM_THREADS) {
      const float4 p = s_c[i];
      const float dx = p.x - cx, dy = p.y - cy, dz = p.z - cz;
      const float nx = dx * c + dy * s, ny = dx * (-s) + dy * c;
      mn[0] = fminf(mn[0], nx), mn[1] = fminf(mn[1], ny), mn[2] = fminf(mn[2], dz);
      mx[0] = fmaxf(mx[0], nx), mx[1] = fmaxf(mx[1], ny), mx[2] = fmaxf(mx[2], dz);
    }
    vcm_block_bounds(mn, mx, s_part);
  }
  if (tid == 0) {
    const float pred[7] = {cx, cy, cz, mx[0] - mn[0], mx[1] - mn[1], mx[2] - mn[2], heading};
#pragma unroll
    for (int k = 0; k < 6; ++k) row[C_BOX + k] = pred[k];
    // k_boxes_iou3d's expressions, a = the predicted box, b = the ground truth
    const float a_hmax = pred[2] + pred[5] / 2.f, a_hmin = pred[2] - pred[5] / 2.f, vol_a = pred[3] * pred[4] * pred[5];
    const float b_hmax = box[2] + box[5] / 2.f, b_hmin = box[2] - box[5] / 2.f, vol_b = box[3] * box[4] * box[5];
    const float overlap_bev = overlap_area_in(make_rbox(pred), make_rbox(box), s_poly, s_ang);
    const float overlap_h = fmaxf(fminf(a_hmax, b_hmax) - fmaxf(a_hmin, b_hmin), 0.f);
    const float overlap_3d = overlap_bev * overlap_h;
    row[C_IOU] = overlap_3d / fmaxf(vol_a + vol_b - overlap_3d, 1e-6f);
    float rot_err = -1.f, trans_err = -1.f;                       // the sentinel of a missing input: an error is never negative
    if (reg_rot) {
      const float* r = reg_rot + (size_t)b * 9;                   // rotm_to_heading: atan2 of row 0's normalised y and x
      const float nrm = sqrtf((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
      rot_err = fabsf(atan2f(r[1] / nrm, r[0] / nrm) - heading);
    }
    if (reg_centre) {
      const float* t = reg_centre + (size_t)b * 3;
      trans_err = ((fabsf(t[0] - box[0]) + fabsf(t[1] - box[1])) + fabsf(t[2] - box[2])) / 3.f;
    }
    row[C_ROT] = rot_err, row[C_TRANS] = trans_err;
  }

  // ---- out of box: the float64 membership test of every row into its flag (the Chamfer passes are done with it)
  __syncthreads();
  {
    const double bx = box[0], by = box[1], bz = box[2], hl = (double)box[3] / 2, hw = (double)box[4] / 2, hh = (double)box[5] / 2;
    const double c = cos((double)heading), s = sin((double)heading);
    for (int i = tid; i < n; i += VCM_THREADS) {
      const float4 p = s_c[i];
      const double dx = (double)p.x - bx, dy = (double)p.y - by, dz = (double)p.z - bz;
      const double lx = dx * c + dy * s, ly = -dx * s + dy * c;
      const bool in = fabs(lx) <= hl && fabs(ly) <= hw && fabs(dz) <= hh;
      s_c[i].w = in ? 0.f : 1.f;
    }
  }
  // distinct scalars among the 3 n coordinates
  const int p1 = vcm_pow2_at_least(3 * n);
  __syncthreads();                                                // the flags are written, the tile is free
  for (int t = tid; t < p1; t += VCM_THREADS) s_keys[t] = t < 3 * n ? sv_ordered_f32(pc[t] + 0.f) : VCM_PAD;
  vcm_bitonic(s_keys, p1, [](uint32_t u, uint32_t v) { return u < v; });
  int cnt = 0;
  for (int t = tid; t < 3 * n; t += VCM_THREADS) cnt += t == 0 || s_keys[t] != s_keys[t - 1];
  const int num_pc = vcm_block_sum(cnt, s_part);
  // distinct rows outside the box: row numbers sorted by (x, y, z)
  const int p2 = vcm_pow2_at_least(n);
  __syncthreads();
  for (int t = tid; t < p2; t += VCM_THREADS) s_keys[t] = t < n ? (uint32_t)t : VCM_PAD;
  vcm_bitonic(s_keys, p2, [s_c](uint32_t u, uint32_t v) {
    if (u == VCM_PAD || v == VCM_PAD) return u != VCM_PAD;        // the padding sorts behind every row
    const float4 p = s_c[u], q = s_c[v];
    if (p.x != q.x) return p.x < q.x;
    if (p.y != q.y) return p.y < q.y;
    return p.z < q.z;
  });
  cnt = 0;
  for (int t = tid; t < n; t += VCM_THREADS) {
    const float4 p = s_c[min(s_keys[t], (uint32_t)(n - 1))];       // (the first n sorted entries are rows; the clamp keeps any read inside s_c)
    bool first = t == 0;
    if (!first) {
      const float4 q = s_c[min(s_keys[t - 1], (uint32_t)(n - 1))];
      first = p.x != q.x || p.y != q.y || p.z != q.z;
    }
    cnt += first && p.w != 0.f;
  }
  const int num_oob = vcm_block_sum(cnt, s_part);

  if (tid == 0) {
    irow[C_NOOB] = num_oob, irow[C_NPC] = num_pc;
    row[C_OOB] = (float)num_oob / (float)num_pc;
  }
}

// The 30 values in Metrics.names() order: item k (CDL1, CDL2, OUT_OF_BOX, IOU_3D, Rotation_Error, Translation_Error) at out[5 k + g], g = 0 the whole
// batch, 1 .. 4 = L1 (201 ..), L2 (81 .. 200), L3 (31 .. 80), L4 (5 .. 30).  fp32 throughout; the denominators count * n and count * m are converted
// to fp32 with one rounding.
__global__ __launch_bounds__(VCM_THREADS) void k_vc_metrics_levels(const float* __restrict__ table, const int32_t* __restrict__ num_pts, int batch,
                                                                   float* __restrict__ out) {
  __shared__ float s_err[VCM_MAX_B];
  __shared__ uint8_t s_grp[VCM_MAX_B];
  __shared__ int s_cnt[5];
  const int tid = threadIdx.x;
  const int32_t* itable = reinterpret_cast<const int32_t*>(table);
  for (int i = tid; i < batch; i += VCM_THREADS) {
    const int np = num_pts[i];
    s_err[i] = table[(size_t)i * C_COLS + C_ROT];
    s_grp[i] = (uint8_t)(1 | ((np >= 201 && np <= 1000000) << 1) | ((np >= 81 && np <= 200) << 2) | ((np >= 31 && np <= 80) << 3) |
                         ((np >= 5 && np <= 30) << 4));
  }
  __syncthreads();
  const int n = itable[C_N], m = itable[C_M];
  const bool has_rot = table[C_ROT] >= 0.f, has_centre = table[C_TRANS] >= 0.f;
  if (tid < 5) {
    const int g = tid;
    float d1 = 0.f, s1 = 0.f, d2 = 0.f, s2 = 0.f, oob = 0.f, iou = 0.f, tr = 0.f;
    int count = 0, last = 0;
    for (int i = 0; i < batch; ++i) {
      if (!((s_grp[i] >> g) & 1)) continue;
      const float* row = table + (size_t)i * C_COLS;
      d1 = d1 + row[C_D1], s1 = s1 + row[C_S1], d2 = d2 + row[C_D2], s2 = s2 + row[C_S2];
      oob = oob + row[C_OOB], iou = iou + row[C_IOU], tr = tr + row[C_TRANS];
      ++count, last = i;
    }
    s_cnt[g] = count;
    float cdl1 = -1.f, cdl2 = -1.f;
    if (count > 0 && m != 1) {
      if (count == 1) {                                           // ignore_zeros acts at one object: the stripped sums over the surviving rows
        const float* row = table + (size_t)last * C_COLS;
        const int k1 = itable[(size_t)last * C_COLS + C_NZ1], k2 = itable[(size_t)last * C_COLS + C_NZ2];
        if (k1 > 0 && k2 > 0) {
          cdl1 = (row[C_ZS1] / (float)k1 + row[C_ZS2] / (float)k2) / 2.f * 1000.f;
          cdl2 = (row[C_ZD1] / (float)k1 + row[C_ZD2] / (float)k2) * 1000.f;
        }
      } else {
        const float r1 = (float)((int64_t)count * n), r2 = (float)((int64_t)count * m);
        cdl1 = (s1 / r1 + s2 / r2) / 2.f * 1000.f;
        cdl2 = (d1 / r1 + d2 / r2) * 1000.f;
      }
    }
    out[g] = cdl1, out[5 + g] = cdl2;
    out[10 + g] = count > 0 ? oob / (float)count : -1.f;
    out[15 + g] = count > 0 ? iou / (float)count : -1.f;
    if (count == 0 || !has_rot) out[20 + g] = -1.f;
    out[25 + g] = count > 0 && has_centre ? tr / (float)count : -1.f;
  }
  __syncthreads();
  if (!has_rot) return;
  for (int g = 0; g < 5; ++g) {                                   // torch.median: the element of rank (count - 1) / 2
    const int target = (s_cnt[g] - 1) / 2;
    for (int i = tid; i < batch; i += VCM_THREADS) {
      if (!((s_grp[i] >> g) & 1)) continue;
      const float e = s_err[i];
      int rank = 0;
      for (int j = 0; j < batch; ++j) rank += ((s_grp[j] >> g) & 1) && (s_err[j] < e || (s_err[j] == e && j < i));
      if (rank == target) out[20 + g] = e;
    }
  }
}

extern "C" int sv_vc_metrics_columns(void) { return C_COLS; }
extern "C" int sv_vc_metrics_tile(void) { return VCM_TILE; }

static size_t vcm_lds_bytes(int n) {
  size_t p = 1;
  while (p < (size_t)3 * n) p <<= 1;
  const size_t region = p * 4 > (size_t)VCM_TILE * 16 ? p * 4 : (size_t)VCM_TILE * 16;
  return (size_t)n * 16 + region;
}

extern "C" int sv_vc_metrics_objects(const float* coarse, const float* complete, const float* gt_boxes, const float* reg_rot, const float* reg_centre,
                                     int batch, int n, int m, float* table, void* stream) {
  SV_CHECK_ARG(batch >= 0 && n >= 1 && m >= 0, "sv_vc_metrics_objects: bad sizes (batch %d, n %d, m %d)", batch, n, m);
  SV_CHECK_ARG(n <= VCM_MAX_N, "sv_vc_metrics_objects: at most %d predicted rows an object (got %d): the cloud and its sort live in LDS", VCM_MAX_N, n);
  if (batch == 0) return SV_OK;
  SV_CHECK_ARG(coarse && gt_boxes && table && (complete || m == 0) && (m > 0 || !complete), "sv_vc_metrics_objects: null pointer");
  const size_t lds = vcm_lds_bytes(n);
  if (lds > 48 * 1024) {                                          // above 48 KB a kernel's dynamic LDS limit has to be raised, per device
    constexpr int MAX_DEV = 64;
    static bool raised[MAX_DEV] = {};
    int dev = 0;
    SV_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= MAX_DEV || !raised[dev]) {
      SV_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_vc_metrics_objects), hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024));
      if (dev >= 0 && dev < MAX_DEV) raised[dev] = true;
    }
  }
  hipLaunchKernelGGL(k_vc_metrics_objects, dim3(batch), dim3(VCM_THREADS), lds, sv_stream(stream), coarse, n, complete, m, gt_boxes, reg_rot,
                     reg_centre, table);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_vc_metrics_levels(const float* table, const int32_t* num_pts, int batch, float* out, void* stream) {
  SV_CHECK_ARG(batch >= 1 && batch <= VCM_MAX_B, "sv_vc_metrics_levels: 1 .. %d objects a call (got %d)", VCM_MAX_B, batch);
  SV_CHECK_ARG(table && num_pts && out, "sv_vc_metrics_levels: null pointer");
  hipLaunchKernelGGL(k_vc_metrics_levels, dim3(1), dim3(VCM_THREADS), 0, sv_stream(stream), table, num_pts, batch, out);
  SV_LAUNCH_CHECK();
  return SV_OK;
}
