// The reference's in-box test (detector3d/pcdet/ops/roiaware_pool3d/src/roiaware_pool3d_kernel.cu:16-36), stated once: k_points_in_boxes and
// k_points_in_boxes_matrix (iou3d.hip), the RoI-aware assignment (roiaware_pool.hip) and the RoI point pooling (roipoint_pool.hip) all call it.
// z is compared in double, the x/y margin is added in double, the rotation is cosf/sinf(-rz) computed by the caller (once per box); there is
// no margin on z.  The margin is the caller's: 1e-5f in the reference's GPU tests, 1e-2f in its CPU matrix (roiaware_pool3d.cpp:121-165).
#pragma once
#include "common.h"

#ifdef __HIPCC__
// the two halves of the test; a caller that has no cosa / sina at hand yet asks for z first and computes them only for the points that pass
__device__ __forceinline__ bool sv_pt_in_box_z(float z, float cz, float dz) {
  return !(fabsf(z - cz) > dz / 2.0);                        // double-precision compare like the reference (:32)
}
__device__ __forceinline__ bool sv_pt_in_box_xy(float x, float y, float cx, float cy, float dx, float dy, float cosa, float sina, float margin,
                                                float& lx, float& ly) {
  const float sx = x - cx, sy = y - cy;
  lx = sx * cosa + sy * (-sina);
  ly = sx * sina + sy * cosa;
  return fabs(lx) < dx / 2.0 + (double)margin && fabs(ly) < dy / 2.0 + (double)margin;
}

// (x, y, z) against the box centre (cx, cy, cz), extents (dx, dy, dz) and cosa = cosf(-rz), sina = sinf(-rz).  lx / ly: the point in the box's
// frame, set whenever the z test passes.
__device__ __forceinline__ bool sv_pt_in_box3d(float x, float y, float z, float cx, float cy, float cz, float dx, float dy, float dz, float cosa,
                                               float sina, float margin, float& lx, float& ly) {
  return sv_pt_in_box_z(z, cz, dz) && sv_pt_in_box_xy(x, y, cx, cy, dx, dy, cosa, sina, margin, lx, ly);
}
#endif
