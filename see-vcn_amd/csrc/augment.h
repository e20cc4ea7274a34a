// What augment.hip and augment_local.hip share: the batch layout, its limits, the op codes' packing and the box row of the in-box test.
//
// Layout shared by every entry: the batch's points are rows of C floats in one buffer, scene b owns rows pt_start[b] .. pt_start[b] + pt_cnt[b];
// its boxes are rows of W >= 7 floats [x, y, z, dx, dy, dz, heading, ...] at box_start[b] .. + box_cnt[b] (at most 256 per scene).  box_cls holds
// one int32 per box row: >= 0 the index into class_names, -1 a box of another class (gt_boxes_mask == 0: never changed, still an obstacle),
// -2 a box already filtered out (it does not exist for anyone).  keep holds one int32 per point row, 0 = dropped.  Starts and counts live on the
// device; max_scene_points is a host upper bound of pt_cnt that only sizes the grid.  No float atomics anywhere: equal bits run to run.
#pragma once
#include <math.h>

#include "common.h"

constexpr int AUG_MAX_BOXES = 256;
constexpr int AUG_THREADS = 256;                               // one thread per box of a scene, or per point of a chunk

__device__ __forceinline__ int aug_box_count(const int32_t* __restrict__ box_cnt, int b) { return min(max(box_cnt[b], 0), AUG_MAX_BOXES); }

// ops, steps and directions travel as up to 16 codes of 4 bits, the first in the lowest bits (host side: data_pipeline.py OP_CODES / pack_codes)
__host__ __device__ __forceinline__ int aug_code(int64_t codes, int t) { return (int)((codes >> (4 * t)) & 15); }

// The 8-float row of a box as sv_pt_in_box3d takes it: cx cy cz dx dy dz cos(-rz) sin(-rz); ENLARGED: the sizes grown by (ex, ey, ez).
template <bool ENLARGED = false>
__device__ __forceinline__ void aug_box_row(float* s, const float* __restrict__ bx, float ex = 0.f, float ey = 0.f, float ez = 0.f) {
  s[0] = bx[0], s[1] = bx[1], s[2] = bx[2];
  s[3] = ENLARGED ? bx[3] + ex : bx[3], s[4] = ENLARGED ? bx[4] + ey : bx[4], s[5] = ENLARGED ? bx[5] + ez : bx[5];
  s[6] = cosf(-bx[6]), s[7] = sinf(-bx[6]);
}
