// Local and frustum augmentors on the device: per-box translation / rotation / scaling, per-box frustum dropout and the world frustum dropout.
//
// Reference (numpy on dataloader workers, a Python loop over the boxes with a whole-scene in-box pass per box, axis and direction):
// detector3d/pcdet/datasets/augmentor/augmentor_utils.py:257-320 (random_local_translation_along_x / _y / _z), :323-388
// (global_frustum_dropout_*), :391-422 (local_scaling), :425-470 (local_rotation), :473-550 (local_frustum_dropout_*), :553-570 (get_points_in_box).
//
// The batch layout is the one augment.h states: stacked point rows of C floats with keep flags, stacked box rows of W >= 7 floats with box_cls
// (-2: the row does not exist), starts and counts on the device, at most 256 boxes per scene.
//
// Why two kernels.  A box's own state never depends on the points (translation adds to one centre coordinate, scaling multiplies the sizes,
// rotation adds to the heading), so one thread per box can walk all the steps and write down, per (step, box), the box as that step's test sees
// it and the step's parameter: the plan.  The points cannot be split that way: every function changes `points` in place while it loops over the
// boxes, so a point moved by box k is tested by box k + 1 at its new position (get_points_in_box carries a 0.1 m margin: boxes less than 0.2 m
// apart share a strip of points).  Per point the walk is strictly sequential, across points it is independent: one thread per point.
//
// Arithmetic types follow the reference under NumPy's value-based casting: a float32 array against a Python float is a float32 operation with
// the scalar rounded first (the points); a float32 scalar against a Python float is float64 (box[k] += offset, dx / 2.0 + MARGIN, the
// thresholds), rounded to float32 where it meets a float32 array.  No float atomics: equal bits run to run.
#include <math.h>

#include "augment.h"
#include "common.h"
#include "wave.h"

namespace {
constexpr int AUGL_ROW = 12;                                   // floats per plan row
constexpr double AUGL_MARGIN = 1e-1;                           // get_points_in_box's MARGIN (:559): x / y only

// step codes, 4 bits each, first step in the lowest bits
enum { L_TX = 1, L_TY = 2, L_TZ = 3, L_ROT = 4, L_SCALE = 5, L_DROP_TOP = 6, L_DROP_BOTTOM = 7, L_DROP_LEFT = 8, L_DROP_RIGHT = 9 };
// directions of the world frustum dropout
enum { D_TOP = 1, D_BOTTOM = 2, D_LEFT = 3, D_RIGHT = 4 };
}  // namespace

// ------------------------------------------------------------------ the plan: one thread per box row
// Plan row (step t, box row r) at plan + ((int64_t)t * total_boxes + r) * 12:
//   0-2 centre   3 / 4 float32(dx / 2.0 + 0.1), float32(dy / 2.0 + 0.1)   5 dz / 2   6 / 7 float32(cos(-rz)), float32(sin(-rz)) of the float64 math.cos / sin
//   8-10 the parameter: translation float32(offset); rotation cosf / sinf of float32(angle); scaling float32(scale); dropout float32(threshold)
//   11 skip != 0 (box_cls == -2)
__global__ __launch_bounds__(AUG_THREADS) void k_augl_plan(float* __restrict__ boxes, int W, const int32_t* __restrict__ box_start,
                                                           const int32_t* __restrict__ box_cnt, const int32_t* __restrict__ box_cls,
                                                           int total_boxes, int64_t steps, int num_steps, const double* __restrict__ draws,
                                                           float* __restrict__ plan) {
  const int b = blockIdx.x, k = threadIdx.x;
  if (k >= aug_box_count(box_cnt, b)) return;
  const int64_t row = (int64_t)box_start[b] + k;
  if (row >= total_boxes) return;
  const bool skip = box_cls[row] < -1;
  float* q = boxes + row * W;
  float c[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, 0.f}, h = 0.f;
  if (!skip) c[0] = q[0], c[1] = q[1], c[2] = q[2], d[0] = q[3], d[1] = q[4], d[2] = q[5], h = q[6];
  for (int t = 0; t < num_steps; ++t) {
    float* o = plan + ((int64_t)t * total_boxes + row) * AUGL_ROW;
    if (skip) {                                                // its draws are not read
#pragma unroll
      for (int j = 0; j < AUGL_ROW; ++j) o[j] = j == AUGL_ROW - 1 ? 1.f : 0.f;
      continue;
    }
    const double v = draws[row * num_steps + t];
    o[0] = c[0], o[1] = c[1], o[2] = c[2];
    o[3] = (float)((double)d[0] / 2.0 + AUGL_MARGIN), o[4] = (float)((double)d[1] / 2.0 + AUGL_MARGIN), o[5] = d[2] / 2.f;
    o[6] = (float)cos(-(double)h), o[7] = (float)sin(-(double)h);
    float p0 = 0.f, p1 = 0.f;
    switch (aug_code(steps, t)) {
      case L_TX: p0 = (float)v, c[0] = (float)((double)c[0] + v); break;                        // :270-272
      case L_TY: p0 = (float)v, c[1] = (float)((double)c[1] + v); break;
      case L_TZ: p0 = (float)v, c[2] = (float)((double)c[2] + v); break;
      case L_ROT:                                              // the centre goes to zero, is rotated and comes back (:447-461): itself
        p0 = cosf((float)v), p1 = sinf((float)v);
        c[0] = (c[0] - c[0]) + c[0], c[1] = (c[1] - c[1]) + c[1], c[2] = (c[2] - c[2]) + c[2];
        h = (float)((double)h + v);                            // :463
        break;
      case L_SCALE: p0 = (float)v, d[0] *= (float)v, d[1] *= (float)v, d[2] *= (float)v; break;   // :421
      case L_DROP_TOP: p0 = (float)(((double)c[2] + (double)d[2] / 2.0) - v * (double)d[2]); break;    // :486
      case L_DROP_BOTTOM: p0 = (float)(((double)c[2] - (double)d[2] / 2.0) + v * (double)d[2]); break; // :506
      case L_DROP_LEFT: p0 = (float)(((double)c[1] + (double)d[1] / 2.0) - v * (double)d[1]); break;   // :526, world y
      case L_DROP_RIGHT: p0 = (float)(((double)c[1] - (double)d[1] / 2.0) + v * (double)d[1]); break;  // :546
      default: break;
    }
    o[8] = p0, o[9] = p1, o[10] = 0.f, o[11] = 0.f;
  }
  if (!skip) q[0] = c[0], q[1] = c[1], q[2] = c[2], q[3] = d[0], q[4] = d[1], q[5] = d[2], q[6] = h;
}

extern "C" int sv_local_transform_plan(float* boxes, int W, const int32_t* box_start, const int32_t* box_cnt, const int32_t* box_cls, int batch,
                                       int total_boxes, int64_t steps, int num_steps, const double* draws, float* plan, void* stream) {
  SV_CHECK_ARG(batch >= 0 && total_boxes >= 0 && W >= 7 && num_steps >= 0 && num_steps <= 16, "local_transform_plan: bad arguments (at most 16 steps)");
  for (int t = 0; t < num_steps; ++t) {
    const int code = aug_code(steps, t);
    SV_CHECK_ARG(code >= L_TX && code <= L_DROP_RIGHT, "local_transform_plan: unknown step code %d", code);
    SV_CHECK_ARG(!(code == L_ROT && W > 8), "local_transform_plan: local rotation of boxes wider than 8 columns");
  }
  if (batch == 0 || total_boxes == 0 || num_steps == 0) return SV_OK;
  SV_CHECK_ARG(boxes && box_start && box_cnt && box_cls && draws && plan, "local_transform_plan: null pointer");
  hipLaunchKernelGGL(k_augl_plan, dim3(batch), dim3(AUG_THREADS), 0, sv_stream(stream), boxes, W, box_start, box_cnt, box_cls, total_boxes, steps,
                     num_steps, draws, plan);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ------------------------------------------------------------------ the walk: one thread per point
// Per step the scene's plan rows (at most 256 x 12 floats = 12 KB) are staged through LDS; the whole plan of 16 steps would not fit and need not.
// A dead point (keep == 0) is skipped, which equals the reference's removal: nothing a dead point does reaches a live one.  No coarse reject in
// front of the test: the z comparison already comes first and is one subtraction.
__global__ __launch_bounds__(AUG_THREADS) void k_augl_points(float* __restrict__ points, int C, const int32_t* __restrict__ pt_start,
                                                             const int32_t* __restrict__ pt_cnt, int32_t* __restrict__ keep,
                                                             const int32_t* __restrict__ box_start, const int32_t* __restrict__ box_cnt,
                                                             int total_boxes, int64_t steps, int num_steps, const float* __restrict__ plan) {
  __shared__ float sb[AUG_MAX_BOXES * AUGL_ROW];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int b0 = box_start[b];
  const int nb = min(aug_box_count(box_cnt, b), max(total_boxes - b0, 0));
  if (nb == 0) return;                                         // (uniform over the workgroup)
  const int i = blockIdx.x * AUG_THREADS + tid;
  const int64_t p = (int64_t)pt_start[b] + i;
  bool alive = i < pt_cnt[b];
  if (alive) alive = keep[p] != 0;
  const bool was_alive = alive;
  float x = 0.f, y = 0.f, z = 0.f;
  if (alive) x = points[p * C], y = points[p * C + 1], z = points[p * C + 2];
  bool moved = false;
  for (int t = 0; t < num_steps; ++t) {
    const float* src = plan + ((int64_t)t * total_boxes + b0) * AUGL_ROW;
    __syncthreads();                                           // the last step's readers are done
    for (int j = tid; j < nb * AUGL_ROW; j += AUG_THREADS) sb[j] = src[j];
    __syncthreads();
    const int op = aug_code(steps, t);
    for (int k = 0; k < nb && alive; ++k) {
      const float* s = sb + k * AUGL_ROW;
      if (s[11] != 0.f) continue;
      const float sx = x - s[0], sy = y - s[1], sz = z - s[2];   // get_points_in_box (:553-566): every comparison is <=
      if (!(fabsf(sz) <= s[5])) continue;
      const float lx = sx * s[6] + sy * (-s[7]), ly = sx * s[7] + sy * s[6];
      if (!(fabsf(lx) <= s[3] && fabsf(ly) <= s[4])) continue;
      switch (op) {
        case L_TX: x = x + s[8], moved = true; break;
        case L_TY: y = y + s[8], moved = true; break;
        case L_TZ: z = z + s[8], moved = true; break;
        case L_ROT: {                                          // :444-458: to the centre, rotate_points_along_z's matmul row, back
          const float nx = sx * s[8] + sy * (-s[9]), ny = sx * s[9] + sy * s[8];
          x = nx + s[0], y = ny + s[1], z = sz + s[2], moved = true;
          break;
        }
        case L_SCALE: x = sx * s[8] + s[0], y = sy * s[8] + s[1], z = sz * s[8] + s[2], moved = true; break;   // :409-419
        case L_DROP_TOP: if (z >= s[8]) alive = false; break;
        case L_DROP_BOTTOM: if (z <= s[8]) alive = false; break;
        case L_DROP_LEFT: if (y >= s[8]) alive = false; break;
        case L_DROP_RIGHT: if (y <= s[8]) alive = false; break;
        default: break;
      }
    }
  }
  if (!was_alive) return;
  if (!alive) keep[p] = 0;
  else if (moved) points[p * C] = x, points[p * C + 1] = y, points[p * C + 2] = z;
}

extern "C" int sv_local_transform_points(float* points, int C, const int32_t* pt_start, const int32_t* pt_cnt, int32_t* keep, int batch,
                                         int max_scene_points, const int32_t* box_start, const int32_t* box_cnt, int total_boxes, int64_t steps,
                                         int num_steps, const float* plan, void* stream) {
  SV_CHECK_ARG(batch >= 0 && max_scene_points >= 0 && total_boxes >= 0 && C >= 3 && num_steps >= 0 && num_steps <= 16,
               "local_transform_points: bad arguments (at most 16 steps)");
  if (batch == 0 || max_scene_points == 0 || total_boxes == 0 || num_steps == 0) return SV_OK;
  SV_CHECK_ARG(points && pt_start && pt_cnt && keep && box_start && box_cnt && plan && batch <= 65535,
               "local_transform_points: null pointer or batch > 65535");
  hipLaunchKernelGGL(k_augl_points, dim3(sv_div_up(max_scene_points, AUG_THREADS), batch), dim3(AUG_THREADS), 0, sv_stream(stream), points, C,
                     pt_start, pt_cnt, keep, box_start, box_cnt, total_boxes, steps, num_steps, plan);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ------------------------------------------------------------------ world frustum dropout (augmentor_utils.py:323-388)
// Per direction a launch pair.  The first reduces the coordinate's minimum and maximum over the scene's live points: a wave reduction, then one
// integer atomicMin per wave on the order-preserving encoding (the maximum as the minimum of the inverted code), so the result does not depend
// on the order.  The second forms the threshold as the reference does -- the float32 range times the Python float, in float64, rounded where it
// meets the float32 columns -- and clears keep for the points and sets box_cls = -2 for the boxes whose coordinate fails the strict comparison.
// A scene without live points keeps both words at 0xffffffff and passes through (np.max of an empty array raises in the reference).
__global__ __launch_bounds__(AUG_THREADS) void k_augl_minmax(const float* __restrict__ points, int C, const int32_t* __restrict__ pt_start,
                                                             const int32_t* __restrict__ pt_cnt, const int32_t* __restrict__ keep, int col,
                                                             uint32_t* __restrict__ minmax) {
  const int b = blockIdx.y, i = blockIdx.x * AUG_THREADS + threadIdx.x;
  uint32_t lo = 0xffffffffu, hi = 0xffffffffu;
  if (i < pt_cnt[b]) {
    const int64_t p = (int64_t)pt_start[b] + i;
    if (keep[p]) {
      const uint32_t e = sv_ordered_f32(points[p * C + col]);
      lo = e, hi = ~e;
    }
  }
  lo = sv_wave_reduce_min(lo), hi = sv_wave_reduce_min(hi);
  if ((threadIdx.x & (SV_WAVE - 1)) == 0) {
    if (lo != 0xffffffffu) atomicMin(&minmax[2 * b], lo);
    if (hi != 0xffffffffu) atomicMin(&minmax[2 * b + 1], hi);
  }
}

__global__ __launch_bounds__(AUG_THREADS) void k_augl_world_drop(const float* __restrict__ points, int C, const int32_t* __restrict__ pt_start,
                                                                 const int32_t* __restrict__ pt_cnt, int32_t* __restrict__ keep,
                                                                 const float* __restrict__ boxes, int W, const int32_t* __restrict__ box_start,
                                                                 const int32_t* __restrict__ box_cnt, int32_t* __restrict__ box_cls,
                                                                 int total_boxes, int dir, const double* __restrict__ intensity, int num_dirs,
                                                                 int which, const uint32_t* __restrict__ minmax) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const uint32_t elo = minmax[2 * b], ehi = minmax[2 * b + 1];
  if (elo == 0xffffffffu && ehi == 0xffffffffu) return;        // no live point
  const float mn = sv_unordered_f32(elo), mx = sv_unordered_f32(~ehi);
  const double v = intensity[(int64_t)b * num_dirs + which];
  const double span = (double)(mx - mn);                       // float32 scalar - float32 scalar
  const bool upper = dir == D_TOP || dir == D_LEFT;
  const float thr = (float)(upper ? (double)mx - v * span : (double)mn + v * span);
  const int col = (dir == D_TOP || dir == D_BOTTOM) ? 2 : 1;
  const int i = blockIdx.x * AUG_THREADS + tid;
  if (i < pt_cnt[b]) {
    const int64_t p = (int64_t)pt_start[b] + i;
    const float c = points[p * C + col];
    if (keep[p] && !(upper ? c < thr : c > thr)) keep[p] = 0;
  }
  if (blockIdx.x == 0 && tid < aug_box_count(box_cnt, b)) {   // the scene's boxes: at most one workgroup's worth
    const int64_t row = (int64_t)box_start[b] + tid;
    if (row < total_boxes && box_cls[row] >= -1) {
      const float c = boxes[row * W + col];
      if (!(upper ? c < thr : c > thr)) box_cls[row] = -2;     // the box goes with its class (the reference leaves gt_names behind)
    }
  }
}

extern "C" size_t sv_world_frustum_dropout_scratch_bytes(int batch, int num_dirs) {
  if (batch <= 0 || num_dirs <= 0) return 0;
  return (size_t)batch * (size_t)num_dirs * 2 * sizeof(uint32_t);
}

extern "C" int sv_world_frustum_dropout(const float* points, int C, const int32_t* pt_start, const int32_t* pt_cnt, int32_t* keep, int batch,
                                        int max_scene_points, const float* boxes, int W, const int32_t* box_start, const int32_t* box_cnt,
                                        int32_t* box_cls, int total_boxes, int64_t dirs, int num_dirs, const double* intensity, void* scratch,
                                        void* stream) {
  SV_CHECK_ARG(batch >= 0 && max_scene_points >= 0 && total_boxes >= 0 && C >= 3 && W >= 7 && num_dirs >= 0 && num_dirs <= 16,
               "world_frustum_dropout: bad arguments (at most 16 directions)");
  for (int t = 0; t < num_dirs; ++t) {
    const int dir = aug_code(dirs, t);
    SV_CHECK_ARG(dir >= D_TOP && dir <= D_RIGHT, "world_frustum_dropout: unknown direction code %d", dir);
  }
  if (batch == 0 || max_scene_points == 0 || num_dirs == 0) return SV_OK;
  SV_CHECK_ARG(points && pt_start && pt_cnt && keep && boxes && box_start && box_cnt && box_cls && intensity && scratch && batch <= 65535,
               "world_frustum_dropout: null pointer or batch > 65535");
  hipStream_t st = sv_stream(stream);
  uint32_t* minmax = reinterpret_cast<uint32_t*>(scratch);
  SV_HIP(hipMemsetAsync(minmax, 0xff, sv_world_frustum_dropout_scratch_bytes(batch, num_dirs), st));
  const dim3 grid(sv_div_up(max_scene_points, AUG_THREADS), batch);
  for (int t = 0; t < num_dirs; ++t) {
    const int dir = aug_code(dirs, t);
    uint32_t* mm = minmax + (size_t)t * batch * 2;
    hipLaunchKernelGGL(k_augl_minmax, grid, dim3(AUG_THREADS), 0, st, points, C, pt_start, pt_cnt, keep, (dir == D_TOP || dir == D_BOTTOM) ? 2 : 1, mm);
    hipLaunchKernelGGL(k_augl_world_drop, grid, dim3(AUG_THREADS), 0, st, points, C, pt_start, pt_cnt, keep, boxes, W, box_start, box_cnt, box_cls,
                       total_boxes, dir, intensity, num_dirs, t, mm);
  }
  SV_LAUNCH_CHECK();
  return SV_OK;
}
