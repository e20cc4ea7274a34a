// The reference's in-box test (detector3d/pcdet/ops/roiaware_pool3d/src/roiaware_pool3d_kernel.cu:16-36), stated once: k_points_in_boxes
// (iou3d.hip) and the RoI-aware assignment (roiaware_pool.hip) both call it.  z is compared in double, the x/y margin is added in double, the
// rotation is cosf/sinf(-rz) computed by the caller (once per box); there is no margin on z.
#pragma once
#include "common.h"

#ifdef __HIPCC__
// (x, y, z) against the box centre (cx, cy, cz), extents (dx, dy, dz) and cosa = cosf(-rz), sina = sinf(-rz).  lx / ly: the point in the box's
// frame, set whenever the z test passes.
__device__ __forceinline__ bool sv_pt_in_box3d(float x, float y, float z, float cx, float cy, float cz, float dx, float dy, float dz, float cosa,
                                               float sina, float& lx, float& ly) {
  if (fabsf(z - cz) > dz / 2.0) return false;                // double-precision compare like the reference (:32)
  const float sx = x - cx, sy = y - cy;
  lx = sx * cosa + sy * (-sina);
  ly = sx * sina + sy * cosa;
  return fabs(lx) < dx / 2.0 + (double)1e-5f && fabs(ly) < dy / 2.0 + (double)1e-5f;
}
#endif
