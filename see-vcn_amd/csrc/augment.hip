// Training augmentation on the device: per-box point counts, ST3D-style per-object scaling, world flip / rotation / scaling / translation and
// the final range mask + stable compaction into the batch the detectors consume.
//
// Reference (numpy on dataloader workers): detector3d/pcdet/datasets/dataset.py:126-137 (MIN_POINTS_OF_GT), datasets/augmentor/
// augmentor_utils.py:10-80 (scale_pre_object), :82-160 and :203-254 (world transforms), datasets/augmentor/data_augmentor.py:258-272,
// datasets/processor/data_processor.py (mask_points_and_boxes_outside_range), utils/box_utils.py:28-53,93-109.
//
// The batch layout every entry shares is stated in augment.h.
#include <math.h>

#include "augment.h"
#include "box_test.h"
#include "common.h"
#include "rbox.h"
#include "wave.h"

constexpr int AUG_MAX_TRY = 64;
constexpr float AUG_MARGIN = 1e-2f;                            // the CPU matrix test's x/y margin (roiaware_pool3d.cpp:121-165)

// ------------------------------------------------------------------ points per box (dataset.py:131-133)
__global__ __launch_bounds__(AUG_THREADS) void k_aug_count(const float* __restrict__ points, int C, const int32_t* __restrict__ pt_start,
                                                           const int32_t* __restrict__ pt_cnt, const int32_t* __restrict__ keep,
                                                           const float* __restrict__ boxes, int W, const int32_t* __restrict__ box_start,
                                                           const int32_t* __restrict__ box_cnt, int32_t* __restrict__ counts) {
  __shared__ float sb[AUG_MAX_BOXES][8];                       // aug_box_row
  __shared__ int32_t sc[AUG_MAX_BOXES];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int b0 = box_start[b], nb = aug_box_count(box_cnt, b);
  if (nb == 0) return;
  for (int k = tid; k < nb; k += AUG_THREADS) {
    aug_box_row(sb[k], boxes + (int64_t)(b0 + k) * W);
    sc[k] = 0;
  }
  __syncthreads();
  const int i = blockIdx.x * AUG_THREADS + tid;
  if (i < pt_cnt[b]) {
    const int64_t p = (int64_t)pt_start[b] + i;
    if (!keep || keep[p]) {
      const float x = points[p * C], y = points[p * C + 1], z = points[p * C + 2];
      for (int k = 0; k < nb; ++k) {
        const float* s = sb[k];
        float lx, ly;
        if (sv_pt_in_box3d(x, y, z, s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], AUG_MARGIN, lx, ly)) atomicAdd(&sc[k], 1);
      }
    }
  }
  __syncthreads();
  for (int k = tid; k < nb; k += AUG_THREADS)
    if (sc[k]) atomicAdd(&counts[b0 + k], sc[k]);
}

extern "C" int sv_points_in_boxes_count(const float* points, int C, const int32_t* pt_start, const int32_t* pt_cnt, const int32_t* keep, int batch,
                                        int max_scene_points, const float* boxes, int W, const int32_t* box_start, const int32_t* box_cnt,
                                        int total_boxes, int32_t* counts, void* stream) {
  SV_CHECK_ARG(batch >= 0 && max_scene_points >= 0 && total_boxes >= 0 && C >= 3 && W >= 7, "points_in_boxes_count: bad arguments");
  if (total_boxes == 0) return SV_OK;
  SV_CHECK_ARG(counts, "points_in_boxes_count: null pointer");
  SV_HIP(hipMemsetAsync(counts, 0, (size_t)total_boxes * 4, sv_stream(stream)));
  if (batch == 0 || max_scene_points == 0) return SV_OK;
  SV_CHECK_ARG(points && pt_start && pt_cnt && boxes && box_start && box_cnt && batch <= 65535, "points_in_boxes_count: null pointer or batch > 65535");
  hipLaunchKernelGGL(k_aug_count, dim3(sv_div_up(max_scene_points, AUG_THREADS), batch), dim3(AUG_THREADS), 0, sv_stream(stream), points, C, pt_start,
                     pt_cnt, keep, boxes, W, box_start, box_cnt, counts);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ------------------------------------------------------------------ per-object scaling: the plan (augmentor_utils.py:26-50, 61, 66, 69)
// The reference runs under NumPy's value-based casting: scl_box[:, 3:6] * scale_noises[k] (two arrays) is a float64 product rounded into the
// float32 try box, while lwh * scale_noises[k][try_idx] and obj_points * scale_noises[k][try_idx] (float32 array, float64 scalar) are float32
// products with the scale rounded to float32.  Both are kept: the tries are tested with the former, the chosen size is the latter.
__device__ __forceinline__ float aug_new_z(float z, float dz, float ndz) { return z + (ndz - dz) / 2; }

__global__ __launch_bounds__(AUG_THREADS) void k_aug_scale_plan(float* __restrict__ boxes, int W, const int32_t* __restrict__ box_start,
                                                                const int32_t* __restrict__ box_cnt, const int32_t* __restrict__ box_cls,
                                                                const double* __restrict__ noises, int num_try, double* __restrict__ plan) {
  __shared__ float sx[AUG_MAX_BOXES], sy[AUG_MAX_BOXES], sz[AUG_MAX_BOXES], sdx[AUG_MAX_BOXES], sdy[AUG_MAX_BOXES], sdz[AUG_MAX_BOXES];
  __shared__ float sang[AUG_MAX_BOXES], sc[AUG_MAX_BOXES], ss[AUG_MAX_BOXES], snc[AUG_MAX_BOXES], sns[AUG_MAX_BOXES];
  __shared__ int32_t scls[AUG_MAX_BOXES];
  __shared__ unsigned long long blocked;
  __shared__ int32_t n_present;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int b0 = box_start[b], nb = aug_box_count(box_cnt, b);
  if (nb == 0) return;
  if (tid == 0) n_present = 0;
  __syncthreads();
  for (int k = tid; k < nb; k += AUG_THREADS) {
    const float* bx = boxes + (int64_t)(b0 + k) * W;
    sx[k] = bx[0], sy[k] = bx[1], sz[k] = bx[2], sdx[k] = bx[3], sdy[k] = bx[4], sdz[k] = bx[5], sang[k] = bx[6];
    sc[k] = cosf(bx[6]), ss[k] = sinf(bx[6]), snc[k] = cosf(-bx[6]), sns[k] = sinf(-bx[6]);
    scls[k] = box_cls[b0 + k];
    if (scls[k] >= -1) atomicAdd(&n_present, 1);
  }
  __syncthreads();
  const int present = n_present;
  for (int k = 0; k < nb; ++k) {
    if (scls[k] < 0) {                                         // filtered out, or gt_boxes_mask == 0 (:28-29); uniform over the workgroup
      if (tid == 0) plan[b0 + k] = 0.0;
      continue;
    }
    const double* nz = noises + (int64_t)(b0 + k) * num_try;
    int try_idx = 0;
    if (present > 1) {
      if (tid == 0) blocked = 0ull;
      __syncthreads();
      for (int p = tid; p < num_try * nb; p += AUG_THREADS) {  // the num_try x (N - 1) pairs of box k over the lanes
        const int t = p / nb, j = p - t * nb;
        if (j == k || scls[j] < -1) continue;
        RBox a, o;
        a.x = sx[k], a.y = sy[k], a.ang = sang[k], a.c = sc[k], a.s = ss[k], a.nc = snc[k], a.ns = sns[k];
        a.dx = (float)((double)sdx[k] * nz[t]), a.dy = (float)((double)sdy[k] * nz[t]);
        o.x = sx[j], o.y = sy[j], o.dx = sdx[j], o.dy = sdy[j], o.ang = sang[j], o.c = sc[j], o.s = ss[j], o.nc = snc[j], o.ns = sns[j];
        if (!(iou_bev(a, o) == 0.f)) atomicOr(&blocked, 1ull << t);
      }
      __syncthreads();
      const unsigned long long all = num_try >= 64 ? ~0ull : (1ull << num_try) - 1ull;
      const unsigned long long free_tries = ~blocked & all;    // the first try whose maximum IoU is exactly 0 (:41-48)
      try_idx = free_tries ? __ffsll((long long)free_tries) - 1 : -1;
    }
    if (tid == 0) {
      if (try_idx < 0) {
        plan[b0 + k] = 0.0;                                    // every try collides: box and points stay (:44-45)
      } else {
        const double s = nz[try_idx];
        const float sf = (float)s;
        plan[b0 + k] = s;
        const float ndz = sdz[k] * sf;
        sz[k] = aug_new_z(sz[k], sdz[k], ndz);                 // obj_center is a view of the box (:66)
        sdx[k] = sdx[k] * sf, sdy[k] = sdy[k] * sf, sdz[k] = ndz;
      }
    }
    __syncthreads();                                           // later boxes see the new size and height
  }
  for (int k = tid; k < nb; k += AUG_THREADS) {
    float* bx = boxes + (int64_t)(b0 + k) * W;
    bx[2] = sz[k], bx[3] = sdx[k], bx[4] = sdy[k], bx[5] = sdz[k];
  }
}

extern "C" int sv_object_scale_plan(float* boxes, int W, const int32_t* box_start, const int32_t* box_cnt, const int32_t* box_cls, int batch,
                                    const double* noises, int num_try, double* plan, void* stream) {
  SV_CHECK_ARG(batch >= 0 && W >= 7 && num_try >= 1 && num_try <= AUG_MAX_TRY, "object_scale_plan: bad arguments (1 <= num_try <= %d)", AUG_MAX_TRY);
  if (batch == 0) return SV_OK;
  SV_CHECK_ARG(boxes && box_start && box_cnt && box_cls && noises && plan, "object_scale_plan: null pointer");
  hipLaunchKernelGGL(k_aug_scale_plan, dim3(batch), dim3(AUG_THREADS), 0, sv_stream(stream), boxes, W, box_start, box_cnt, box_cls, noises, num_try,
                     plan);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ------------------------------------------------------------------ per-object scaling: the points (augmentor_utils.py:52-78)
// One thread per point walks the scene's boxes in order.  boxes_before are the boxes as sv_object_scale_plan found them: box k is changed by its
// own step only, so its size and height before that step are the original ones, and after it the original ones scaled.
__global__ __launch_bounds__(AUG_THREADS) void k_aug_scale_points(float* __restrict__ points, int C, const int32_t* __restrict__ pt_start,
                                                                  const int32_t* __restrict__ pt_cnt, int32_t* __restrict__ keep,
                                                                  const float* __restrict__ boxes_before, int W,
                                                                  const int32_t* __restrict__ box_start, const int32_t* __restrict__ box_cnt,
                                                                  const int32_t* __restrict__ box_cls, const double* __restrict__ plan) {
  __shared__ float sb[AUG_MAX_BOXES][12];                      // aug_box_row, then cos(r) sin(r) scale grows
  __shared__ int32_t wave_sums[AUG_THREADS / SV_WAVE];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int b0 = box_start[b], nb = aug_box_count(box_cnt, b);
  if (nb == 0) return;
  const bool scaled = tid < nb && box_cls[b0 + tid] >= 0 && plan[b0 + tid] != 0.0;   // thread k looks at box k (nb <= AUG_THREADS)
  int32_t n;
  const int32_t slot = sv_block_excl_scan<AUG_THREADS>((int32_t)scaled, &n, wave_sums);
  if (scaled) {                                                // the scaled boxes, in box order
    const float* bx = boxes_before + (int64_t)(b0 + tid) * W;
    float* s = sb[slot];
    aug_box_row(s, bx);
    s[8] = cosf(bx[6]), s[9] = sinf(bx[6]);
    s[10] = (float)plan[b0 + tid], s[11] = plan[b0 + tid] > 1.0 ? 1.f : 0.f;
  }
  __syncthreads();
  const int i = blockIdx.x * AUG_THREADS + tid;
  if (n == 0 || i >= pt_cnt[b]) return;
  const int64_t p = (int64_t)pt_start[b] + i;
  if (!keep[p]) return;
  float x = points[p * C], y = points[p * C + 1], z = points[p * C + 2];
  bool moved = false, alive = true;
  for (int k = 0; k < n && alive; ++k) {
    const float* s = sb[k];
    const float cx = s[0], cy = s[1], cz = s[2], sf = s[10];
    const float ndx = s[3] * sf, ndy = s[4] * sf, ndz = s[5] * sf, ncz = aug_new_z(cz, s[5], ndz);
    float lx, ly;
    const bool in_before = sv_pt_in_box3d(x, y, z, cx, cy, cz, s[3], s[4], s[5], s[6], s[7], AUG_MARGIN, lx, ly);
    if (in_before) {
      const float px = x - cx, py = y - cy, pz = z - cz;       // into the box frame: rotate_points_along_z(-ry) (common_utils.py:35-57)
      const float x1 = px * s[6] + py * (-s[7]), y1 = px * s[7] + py * s[6];
      const float x2 = x1 * sf, y2 = y1 * sf, z2 = pz * sf;
      const float x3 = x2 * s[8] + y2 * (-s[9]), y3 = x2 * s[9] + y2 * s[8];   // and back: rotate_points_along_z(ry)
      x = x3 + cx, y = y3 + cy, z = z2 + ncz;
      moved = true;
    }
    if (s[11] != 0.f) {                                        // an enlarged box drops in_before XOR in_after (:72-78)
      const bool in_after = sv_pt_in_box3d(x, y, z, cx, cy, ncz, ndx, ndy, ndz, s[6], s[7], AUG_MARGIN, lx, ly);
      if (in_before != in_after) alive = false;
    }
  }
  if (moved) points[p * C] = x, points[p * C + 1] = y, points[p * C + 2] = z;
  if (!alive) keep[p] = 0;
}

extern "C" int sv_object_scale_points(float* points, int C, const int32_t* pt_start, const int32_t* pt_cnt, int32_t* keep, int batch,
                                      int max_scene_points, const float* boxes_before, int W, const int32_t* box_start, const int32_t* box_cnt,
                                      const int32_t* box_cls, const double* plan, void* stream) {
  SV_CHECK_ARG(batch >= 0 && max_scene_points >= 0 && C >= 3 && W >= 7, "object_scale_points: bad arguments");
  if (batch == 0 || max_scene_points == 0) return SV_OK;
  SV_CHECK_ARG(points && pt_start && pt_cnt && keep && boxes_before && box_start && box_cnt && box_cls && plan && batch <= 65535,
               "object_scale_points: null pointer or batch > 65535");
  hipLaunchKernelGGL(k_aug_scale_points, dim3(sv_div_up(max_scene_points, AUG_THREADS), batch), dim3(AUG_THREADS), 0, sv_stream(stream), points, C,
                     pt_start, pt_cnt, keep, boxes_before, W, box_start, box_cnt, box_cls, plan);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ------------------------------------------------------------------ world transforms (augmentor_utils.py:82-160, 203-254)
// ops: up to 16 codes of 4 bits, first op in the lowest bits; params (batch, num_ops) fp64, one value per scene and op.
//   1 flip along x (param != 0: y, heading, vy negated)      2 flip along y (x, vx negated, heading = -(heading + pi))
//   3 rotation by param (fp32 cos / sin of the fp32 angle)    4 scaling by param (fp32 products)
//   5 / 6 / 7 translation along x / y / z (the offset is a float64 array there: the sum is made in fp64 and rounded)
__device__ __forceinline__ void aug_rotate(float& x, float& y, float c, float s) {
  const float nx = x * c + y * (-s), ny = x * s + y * c;
  x = nx, y = ny;
}

__global__ __launch_bounds__(AUG_THREADS) void k_aug_world_points(float* __restrict__ points, int C, const int32_t* __restrict__ pt_start,
                                                                  const int32_t* __restrict__ pt_cnt, int64_t ops, int num_ops,
                                                                  const double* __restrict__ params) {
  const int b = blockIdx.y, i = blockIdx.x * AUG_THREADS + threadIdx.x;
  if (i >= pt_cnt[b]) return;
  float* q = points + ((int64_t)pt_start[b] + i) * C;
  float x = q[0], y = q[1], z = q[2];
  for (int t = 0; t < num_ops; ++t) {
    const double v = params[(int64_t)b * num_ops + t];
    switch (aug_code(ops, t)) {
      case 1: if (v != 0.0) y = -y; break;
      case 2: if (v != 0.0) x = -x; break;
      case 3: aug_rotate(x, y, cosf((float)v), sinf((float)v)); break;
      case 4: x *= (float)v, y *= (float)v, z *= (float)v; break;
      case 5: x = (float)((double)x + v); break;
      case 6: y = (float)((double)y + v); break;
      case 7: z = (float)((double)z + v); break;
      default: break;
    }
  }
  q[0] = x, q[1] = y, q[2] = z;
}

extern "C" int sv_world_transform_points(float* points, int C, const int32_t* pt_start, const int32_t* pt_cnt, int batch, int max_scene_points,
                                         int64_t ops, int num_ops, const double* params, void* stream) {
  SV_CHECK_ARG(batch >= 0 && max_scene_points >= 0 && C >= 3 && num_ops >= 0 && num_ops <= 16, "world_transform_points: bad arguments");
  if (batch == 0 || max_scene_points == 0 || num_ops == 0) return SV_OK;
  SV_CHECK_ARG(points && pt_start && pt_cnt && params && batch <= 65535, "world_transform_points: null pointer or batch > 65535");
  hipLaunchKernelGGL(k_aug_world_points, dim3(sv_div_up(max_scene_points, AUG_THREADS), batch), dim3(AUG_THREADS), 0, sv_stream(stream), points, C,
                     pt_start, pt_cnt, ops, num_ops, params);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// boxes: the same ops on centres, sizes, heading and (W > 7) the velocity columns 7 / 8; then, with limit_heading, limit_period(heading, 0.5, 2 pi)
// (data_augmentor.py:258-260, common_utils.py:22-25).  Rows with box_cls == -2 are left alone.
__global__ __launch_bounds__(AUG_THREADS) void k_aug_world_boxes(float* __restrict__ boxes, int W, const int32_t* __restrict__ box_start,
                                                                 const int32_t* __restrict__ box_cnt, const int32_t* __restrict__ box_cls,
                                                                 int64_t ops, int num_ops, const double* __restrict__ params, int limit_heading) {
  const int b = blockIdx.x, k = threadIdx.x;
  if (k >= aug_box_count(box_cnt, b)) return;
  const int64_t row = (int64_t)box_start[b] + k;
  if (box_cls[row] < -1) return;
  float* q = boxes + row * W;
  float x = q[0], y = q[1], z = q[2], dx = q[3], dy = q[4], dz = q[5], h = q[6];
  const bool vel = W > 7;
  float vx = vel ? q[7] : 0.f, vy = W > 8 ? q[8] : 0.f;
  for (int t = 0; t < num_ops; ++t) {
    const double v = params[(int64_t)b * num_ops + t];
    switch (aug_code(ops, t)) {
      case 1: if (v != 0.0) y = -y, h = -h, vy = -vy; break;
      case 2: if (v != 0.0) x = -x, h = -(h + (float)M_PI), vx = -vx; break;
      case 3: {
        const float c = cosf((float)v), s = sinf((float)v);
        aug_rotate(x, y, c, s);
        h += (float)v;
        aug_rotate(vx, vy, c, s);
        break;
      }
      case 4: x *= (float)v, y *= (float)v, z *= (float)v, dx *= (float)v, dy *= (float)v, dz *= (float)v; break;
      case 5: x = (float)((double)x + v); break;
      case 6: y = (float)((double)y + v); break;
      case 7: z = (float)((double)z + v); break;
      default: break;
    }
  }
  if (limit_heading) {
    const float period = (float)(2 * M_PI);
    h = h - floorf(h / period + 0.5f) * period;
  }
  q[0] = x, q[1] = y, q[2] = z, q[3] = dx, q[4] = dy, q[5] = dz, q[6] = h;
  if (vel) q[7] = vx;
  if (W > 8) q[8] = vy;
}

extern "C" int sv_world_transform_boxes(float* boxes, int W, const int32_t* box_start, const int32_t* box_cnt, const int32_t* box_cls, int batch,
                                        int64_t ops, int num_ops, const double* params, int limit_heading, void* stream) {
  SV_CHECK_ARG(batch >= 0 && W >= 7 && num_ops >= 0 && num_ops <= 16, "world_transform_boxes: bad arguments");
  if (batch == 0 || (num_ops == 0 && !limit_heading)) return SV_OK;
  SV_CHECK_ARG(boxes && box_start && box_cnt && box_cls && (params || num_ops == 0), "world_transform_boxes: null pointer");
  hipLaunchKernelGGL(k_aug_world_boxes, dim3(batch), dim3(AUG_THREADS), 0, sv_stream(stream), boxes, W, box_start, box_cnt, box_cls, ops, num_ops,
                     params, limit_heading);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ------------------------------------------------------------------ the tail: range masks and one stable compaction
// Points: keep != 0 and, with pt_range (x0, y0, x1, y1 as fp64, both bounds inclusive: common_utils.py:60-63, the fp32 coordinate is widened),
// inside the range.  A chunk is the AUG_THREADS points of one workgroup; pass 1 writes each chunk's survivor count, pass 2 scans the counts
// (scene-major, so the output is ordered by scene and inside a scene by input order) and scatters rows [b, x, y, z, ...].
__global__ __launch_bounds__(AUG_THREADS) void k_aug_compact_flags(const float* __restrict__ points, int C, const int32_t* __restrict__ pt_start,
                                                                   const int32_t* __restrict__ pt_cnt, int32_t* __restrict__ keep, int use_range,
                                                                   double x0, double y0, double x1, double y1, int32_t* __restrict__ chunk_cnt) {
  __shared__ int32_t wave_sums[AUG_THREADS / SV_WAVE];
  const int b = blockIdx.y, i = blockIdx.x * AUG_THREADS + threadIdx.x;
  int flag = 0;
  if (i < pt_cnt[b]) {
    const int64_t p = (int64_t)pt_start[b] + i;
    flag = keep[p] != 0;
    if (flag && use_range) {
      const double x = points[p * C], y = points[p * C + 1];
      flag = x >= x0 && x <= x1 && y >= y0 && y <= y1;
    }
    keep[p] = flag;
  }
  int32_t total;
  sv_block_excl_scan<AUG_THREADS>((int32_t)flag, &total, wave_sums);
  if (threadIdx.x == 0) chunk_cnt[(int64_t)b * gridDim.x + blockIdx.x] = total;
}

__global__ __launch_bounds__(AUG_THREADS) void k_aug_compact_scatter(const float* __restrict__ points, int C, const int32_t* __restrict__ pt_start,
                                                                     const int32_t* __restrict__ pt_cnt, const int32_t* __restrict__ keep,
                                                                     const int32_t* __restrict__ chunk_cnt, float* __restrict__ out_points,
                                                                     int32_t* __restrict__ out_start, int32_t* __restrict__ out_cnt) {
  __shared__ int32_t wave_sums[AUG_THREADS / SV_WAVE];
  __shared__ int32_t part[2][AUG_THREADS / SV_WAVE];
  const int b = blockIdx.y, tid = threadIdx.x, chunks = gridDim.x, batch = gridDim.y;
  const int mine = b * chunks + blockIdx.x;                     // chunks before this one, and (first chunk of a scene) the scene's own
  int32_t before = 0, scene = 0;
  for (int j = tid; j < mine; j += AUG_THREADS) before += chunk_cnt[j];
  if (blockIdx.x == 0)
    for (int j = tid; j < chunks; j += AUG_THREADS) scene += chunk_cnt[mine + j];
  before = sv_wave_reduce_sum(before), scene = sv_wave_reduce_sum(scene);
  if ((tid & (SV_WAVE - 1)) == 0) part[0][tid / SV_WAVE] = before, part[1][tid / SV_WAVE] = scene;
  __syncthreads();
  before = scene = 0;
#pragma unroll
  for (int w = 0; w < AUG_THREADS / SV_WAVE; ++w) before += part[0][w], scene += part[1][w];
  if (blockIdx.x == 0 && tid == 0) {
    out_start[b] = before, out_cnt[b] = scene;
    if (b == batch - 1) out_start[batch] = before + scene;
  }
  const int i = blockIdx.x * AUG_THREADS + tid;
  const bool live = i < pt_cnt[b];
  const int64_t p = (int64_t)pt_start[b] + i;
  const int32_t flag = live ? keep[p] : 0;
  int32_t total;
  const int32_t rank = sv_block_excl_scan<AUG_THREADS>(flag, &total, wave_sums);
  if (flag) {
    float* o = out_points + (int64_t)(before + rank) * (C + 1);
    o[0] = (float)b;
    for (int c = 0; c < C; ++c) o[1 + c] = points[p * C + c];
  }
}

// Boxes: rows with box_cls >= 0 (data_augmentor.py:265-267 and dataset.py:152-156 select the same boxes) and, with min_num_corners > 0, at least
// that many of their 8 corners inside box_range (box_utils.py:28-53, 93-109: fp32 corners, rotate_points_along_z(heading)), in order, with
// box_cls + 1 appended as the last column: gt_out (batch, gt_stride, W + 1), zero beyond a scene's count.
__global__ __launch_bounds__(AUG_THREADS) void k_aug_compact_boxes(const float* __restrict__ boxes, int W, const int32_t* __restrict__ box_start,
                                                                   const int32_t* __restrict__ box_cnt, const int32_t* __restrict__ box_cls,
                                                                   int min_num_corners, double x0, double y0, double z0, double x1, double y1,
                                                                   double z1, float* __restrict__ gt_out, int gt_stride,
                                                                   int32_t* __restrict__ out_box_cnt, int32_t* __restrict__ box_keep) {
  __shared__ int32_t wave_sums[AUG_THREADS / SV_WAVE];
  const int b = blockIdx.x, k = threadIdx.x;
  const int64_t row = (int64_t)box_start[b] + k;
  int32_t flag = 0;
  if (k < aug_box_count(box_cnt, b) && box_cls[row] >= 0) {
    flag = 1;
    if (min_num_corners > 0) {
      const float* q = boxes + row * W;
      const float c = cosf(q[6]), s = sinf(q[6]);
      int inside = 0;
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        const float tx = (m & 3) == 0 || (m & 3) == 1 ? 0.5f : -0.5f, ty = (m & 3) == 0 || (m & 3) == 3 ? 0.5f : -0.5f, tz = m < 4 ? -0.5f : 0.5f;
        float lx = q[3] * tx, ly = q[4] * ty;
        aug_rotate(lx, ly, c, s);
        const double wx = lx + q[0], wy = ly + q[1], wz = q[5] * tz + q[2];
        inside += wx >= x0 && wx <= x1 && wy >= y0 && wy <= y1 && wz >= z0 && wz <= z1;
      }
      flag = inside >= min_num_corners;
    }
  }
  if (box_keep && k < aug_box_count(box_cnt, b)) box_keep[row] = flag;
  int32_t total;
  const int32_t rank = sv_block_excl_scan<AUG_THREADS>(flag, &total, wave_sums);
  if (flag && rank < gt_stride) {
    float* o = gt_out + ((int64_t)b * gt_stride + rank) * (W + 1);
    for (int c = 0; c < W; ++c) o[c] = boxes[row * W + c];
    o[W] = (float)(box_cls[row] + 1);
  }
  if (k == 0) out_box_cnt[b] = total;
}

extern "C" size_t sv_augment_compact_scratch_bytes(int batch, int max_scene_points) {
  if (batch <= 0 || max_scene_points <= 0) return 0;
  return (size_t)batch * (size_t)sv_div_up(max_scene_points, AUG_THREADS) * sizeof(int32_t);
}

extern "C" int sv_augment_compact(const float* points, int C, const int32_t* pt_start, const int32_t* pt_cnt, int32_t* keep, int batch,
                                  int max_scene_points, const double* pt_range_host, const float* boxes, int W, const int32_t* box_start,
                                  const int32_t* box_cnt, const int32_t* box_cls, const double* box_range_host, int min_num_corners, void* scratch,
                                  float* out_points, int32_t* out_start, int32_t* out_counts, float* gt_out, int gt_stride, int32_t* box_keep,
                                  void* stream) {
  SV_CHECK_ARG(batch >= 1 && batch <= 65535 && max_scene_points >= 0 && C >= 3 && W >= 7 && gt_stride >= 0 && gt_stride <= AUG_MAX_BOXES &&
                   min_num_corners >= 0 && min_num_corners <= 8,
               "augment_compact: bad arguments");
  SV_CHECK_ARG(pt_start && pt_cnt && box_start && box_cnt && box_cls && out_start && out_counts && (min_num_corners == 0 || box_range_host),
               "augment_compact: null pointer");
  hipStream_t st = sv_stream(stream);
  if (max_scene_points == 0) {
    SV_HIP(hipMemsetAsync(out_start, 0, (size_t)(batch + 1) * 4, st));
    SV_HIP(hipMemsetAsync(out_counts, 0, (size_t)batch * 4, st));
  } else {
    SV_CHECK_ARG(points && keep && scratch && out_points, "augment_compact: null pointer");
    const int chunks = sv_div_up(max_scene_points, AUG_THREADS);
    int32_t* chunk_cnt = reinterpret_cast<int32_t*>(scratch);
    const double* r = pt_range_host;
    hipLaunchKernelGGL(k_aug_compact_flags, dim3(chunks, batch), dim3(AUG_THREADS), 0, st, points, C, pt_start, pt_cnt, keep, r ? 1 : 0, r ? r[0] : 0.0,
                       r ? r[1] : 0.0, r ? r[2] : 0.0, r ? r[3] : 0.0, chunk_cnt);
    hipLaunchKernelGGL(k_aug_compact_scatter, dim3(chunks, batch), dim3(AUG_THREADS), 0, st, points, C, pt_start, pt_cnt, keep, chunk_cnt, out_points,
                       out_start, out_counts);
  }
  if (gt_stride > 0) {
    SV_CHECK_ARG(boxes && gt_out, "augment_compact: null pointer");
    SV_HIP(hipMemsetAsync(gt_out, 0, (size_t)batch * gt_stride * (W + 1) * sizeof(float), st));
  }
  const double* r = box_range_host;
  hipLaunchKernelGGL(k_aug_compact_boxes, dim3(batch), dim3(AUG_THREADS), 0, st, boxes, W, box_start, box_cnt, box_cls, min_num_corners,
                     r ? r[0] : 0.0, r ? r[1] : 0.0, r ? r[2] : 0.0, r ? r[3] : 0.0, r ? r[4] : 0.0, r ? r[5] : 0.0, gt_out, gt_stride,
                     out_counts + batch, box_keep);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ------------------------------------------------------------------ GT sampling: which candidates go in (database_sampler.py:438-468)
// One workgroup per scene.  The scene's candidates are rows cand_start[b] .. cand_start[b + 1] of cand_idx (rows of the database) and cand_group (the
// SAMPLE_GROUPS entry that drew them, ascending).  Groups are visited in order; a candidate is valid when its BEV IoU with every existing box
// (the scene's boxes with box_cls >= -1 and the earlier groups' accepted boxes) and with every other candidate of its group is exactly 0 --
// max(iou1) + max(iou2) == 0, not greedy: two colliding candidates both go.  Accepted boxes are appended to the scene's box rows in candidate
// order (the rows behind box_cnt[b] are the caller's spare capacity: box_cap[b] rows in all, a valid candidate beyond them is not accepted),
// box_cls = the database's class, box_cnt[b] grows; accept[i] = 0 / 1.
__global__ __launch_bounds__(AUG_THREADS) void k_aug_gt_select(float* __restrict__ boxes, int W, const int32_t* __restrict__ box_start,
                                                               int32_t* __restrict__ box_cnt, const int32_t* __restrict__ box_cap,
                                                               int32_t* __restrict__ box_cls,
                                                               const float* __restrict__ db_boxes, const int32_t* __restrict__ db_cls,
                                                               const int32_t* __restrict__ cand_idx, const int32_t* __restrict__ cand_group,
                                                               const int32_t* __restrict__ cand_start, int32_t* __restrict__ accept) {
  __shared__ RBox s_e[AUG_MAX_BOXES], s_c[AUG_MAX_BOXES];
  __shared__ int32_t s_valid[AUG_MAX_BOXES], s_blk[AUG_MAX_BOXES];
  __shared__ int32_t wave_sums[AUG_THREADS / SV_WAVE];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int b0 = box_start[b], c1 = cand_start[b + 1], cap = aug_box_count(box_cap, b);
  int n = min(aug_box_count(box_cnt, b), cap);
  if (tid < n) {
    s_e[tid] = make_rbox(boxes + (int64_t)(b0 + tid) * W);
    s_valid[tid] = box_cls[b0 + tid] >= -1;
  }
  __syncthreads();
  int g0 = cand_start[b];
  while (g0 < c1) {                                            // (every thread walks the same group boundaries)
    const int gid = cand_group[g0];
    int g1 = g0 + 1;
    while (g1 < c1 && cand_group[g1] == gid) ++g1;
    const int G = min(g1 - g0, AUG_MAX_BOXES);
    if (tid < G) {
      s_c[tid] = make_rbox(db_boxes + (int64_t)cand_idx[g0 + tid] * W);
      s_blk[tid] = 0;
    }
    __syncthreads();
    for (int p = tid; p < G * (n + G); p += AUG_THREADS) {
      const int i = p / (n + G), j = p - i * (n + G);
      bool hit;
      if (j < n) hit = s_valid[j] && !(iou_bev(s_c[i], s_e[j]) == 0.f);                 // iou1: against the existing boxes
      else hit = j - n != i && !(iou_bev(s_c[i], s_c[j - n]) == 0.f);                   // iou2: among the group, zero diagonal
      if (hit) s_blk[i] = 1;
    }
    __syncthreads();
    const int32_t ok = tid < G && !s_blk[tid];
    int32_t total;
    const int32_t rank = sv_block_excl_scan<AUG_THREADS>(ok, &total, wave_sums);
    if (tid < G) accept[g0 + tid] = ok && n + rank < cap;
    if (ok && n + rank < cap) {
      const int src = cand_idx[g0 + tid];
      s_e[n + rank] = s_c[tid], s_valid[n + rank] = 1;
      for (int c = 0; c < W; ++c) boxes[(int64_t)(b0 + n + rank) * W + c] = db_boxes[(int64_t)src * W + c];
      box_cls[b0 + n + rank] = db_cls[src];
    }
    __syncthreads();
    n = min(n + total, cap);
    g0 = g1;
  }
  if (tid == 0) box_cnt[b] = n;
}

extern "C" int sv_gt_sample_select(float* boxes, int W, const int32_t* box_start, int32_t* box_cnt, const int32_t* box_cap, int32_t* box_cls, int batch,
                                   const float* db_boxes,
                                   const int32_t* db_cls, const int32_t* cand_idx, const int32_t* cand_group, const int32_t* cand_start,
                                   int total_candidates, int32_t* accept, void* stream) {
  SV_CHECK_ARG(batch >= 0 && W >= 7 && total_candidates >= 0, "gt_sample_select: bad arguments");
  if (batch == 0 || total_candidates == 0) return SV_OK;
  SV_CHECK_ARG(boxes && box_start && box_cnt && box_cap && box_cls && db_boxes && db_cls && cand_idx && cand_group && cand_start && accept,
               "gt_sample_select: null pointer");
  hipLaunchKernelGGL(k_aug_gt_select, dim3(batch), dim3(AUG_THREADS), 0, sv_stream(stream), boxes, W, box_start, box_cnt, box_cap, box_cls, db_boxes,
                     db_cls, cand_idx, cand_group, cand_start, accept);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ------------------------------------------------------------------ GT sampling: the points (database_sampler.py:381-415)
// Every candidate owns a run of rows at the head of its scene (cand_dest[i], as many rows as the object has points; keep == 0 until now), in
// candidate order, so that the final stable compaction yields [object points in acceptance order, surviving scene points].  An accepted
// candidate's rows become db_points + box3d_lidar[:3] (fp32) with keep = 1.  The scene's own points (rows from pt_start[b] + head_rows[b]) inside
// any accepted box enlarged by extra_width (enlarge_box3d + the CPU matrix test, margin 1e-2) get keep = 0.
__global__ __launch_bounds__(AUG_THREADS) void k_aug_gt_paste(float* __restrict__ points, int C, int32_t* __restrict__ keep,
                                                              const float* __restrict__ db_points, const int64_t* __restrict__ db_offsets,
                                                              const float* __restrict__ db_boxes, int W, const int32_t* __restrict__ cand_idx,
                                                              const int32_t* __restrict__ cand_ptoff, const int32_t* __restrict__ cand_dest,
                                                              const int32_t* __restrict__ accept, int total_candidates, int total_rows) {
  const int t = blockIdx.x * AUG_THREADS + threadIdx.x;
  if (t >= total_rows) return;
  int lo = 0, hi = total_candidates;                           // the candidate whose run holds row t: cand_ptoff[lo] <= t < cand_ptoff[lo + 1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (cand_ptoff[mid] <= t) lo = mid; else hi = mid;
  }
  if (!accept[lo]) return;
  const int src_obj = cand_idx[lo], j = t - cand_ptoff[lo];
  const float* src = db_points + (db_offsets[src_obj] + j) * C;
  const float* box = db_boxes + (int64_t)src_obj * W;
  const int64_t row = (int64_t)cand_dest[lo] + j;
  float* dst = points + row * C;
  dst[0] = src[0] + box[0], dst[1] = src[1] + box[1], dst[2] = src[2] + box[2];
  for (int c = 3; c < C; ++c) dst[c] = src[c];
  keep[row] = 1;
}

__global__ __launch_bounds__(AUG_THREADS) void k_aug_gt_remove(const float* __restrict__ points, int C, const int32_t* __restrict__ pt_start,
                                                               const int32_t* __restrict__ pt_cnt, const int32_t* __restrict__ head_rows,
                                                               int32_t* __restrict__ keep, const float* __restrict__ db_boxes, int W,
                                                               const int32_t* __restrict__ cand_idx, const int32_t* __restrict__ cand_start,
                                                               const int32_t* __restrict__ accept, float ex, float ey, float ez) {
  __shared__ float sb[AUG_MAX_BOXES][8];                       // aug_box_row of the enlarged box
  __shared__ int32_t wave_sums[AUG_THREADS / SV_WAVE];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int c0 = cand_start[b], nc = min(cand_start[b + 1] - c0, AUG_MAX_BOXES);
  const bool mine = tid < nc && accept[c0 + tid];
  int32_t n;
  const int32_t slot = sv_block_excl_scan<AUG_THREADS>((int32_t)mine, &n, wave_sums);
  if (mine) {
    aug_box_row<true>(sb[slot], db_boxes + (int64_t)cand_idx[c0 + tid] * W, ex, ey, ez);
  }
  __syncthreads();
  const int i = head_rows[b] + blockIdx.x * AUG_THREADS + tid;
  if (n == 0 || i >= pt_cnt[b]) return;
  const int64_t p = (int64_t)pt_start[b] + i;
  if (!keep[p]) return;
  const float x = points[p * C], y = points[p * C + 1], z = points[p * C + 2];
  for (int k = 0; k < n; ++k) {
    const float* s = sb[k];
    float lx, ly;
    if (sv_pt_in_box3d(x, y, z, s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], AUG_MARGIN, lx, ly)) {
      keep[p] = 0;
      return;
    }
  }
}

extern "C" int sv_gt_sample_paste(float* points, int C, const int32_t* pt_start, const int32_t* pt_cnt, const int32_t* head_rows, int32_t* keep, int batch,
                                  int max_scene_points, const float* db_points, const int64_t* db_offsets, const float* db_boxes, int W,
                                  const int32_t* cand_idx, const int32_t* cand_start, const int32_t* cand_ptoff, const int32_t* cand_dest,
                                  const int32_t* accept, int total_candidates, int total_rows, float extra_x, float extra_y, float extra_z,
                                  void* stream) {
  SV_CHECK_ARG(batch >= 0 && max_scene_points >= 0 && C >= 3 && W >= 7 && total_candidates >= 0 && total_rows >= 0, "gt_sample_paste: bad arguments");
  if (batch == 0 || total_candidates == 0) return SV_OK;
  SV_CHECK_ARG(points && pt_start && pt_cnt && head_rows && keep && db_boxes && db_offsets && cand_idx && cand_start && cand_ptoff && cand_dest && accept &&
                   (db_points || total_rows == 0) && batch <= 65535,
               "gt_sample_paste: null pointer or batch > 65535");
  hipStream_t st = sv_stream(stream);
  if (total_rows > 0)
    hipLaunchKernelGGL(k_aug_gt_paste, dim3(sv_div_up(total_rows, AUG_THREADS)), dim3(AUG_THREADS), 0, st, points, C, keep, db_points, db_offsets,
                       db_boxes, W, cand_idx, cand_ptoff, cand_dest, accept, total_candidates, total_rows);
  if (max_scene_points > 0)
    hipLaunchKernelGGL(k_aug_gt_remove, dim3(sv_div_up(max_scene_points, AUG_THREADS), batch), dim3(AUG_THREADS), 0, st, points, C, pt_start, pt_cnt,
                       head_rows, keep, db_boxes, W, cand_idx, cand_start, accept, extra_x, extra_y, extra_z);
  SV_LAUNCH_CHECK();
  return SV_OK;
}
