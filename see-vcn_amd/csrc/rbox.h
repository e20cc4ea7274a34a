// Rotated BEV box overlap / IoU as device functions, the reference's statements (detector3d/pcdet/ops/iou3d_nms/src/iou3d_nms_kernel.cu:
// box_overlap :95-223, iou_bev :225-231).  Stated once: the all-pairs / NMS kernels (iou3d.hip) and the augmentation kernels (augment.hip) call it.
// A conservative bounding-circle test skips the polygon construction for pairs that cannot touch: the construction would return exactly 0.
#pragma once
#include <math.h>

#include "common.h"

#ifdef __HIPCC__
struct P2 { float x, y; };

__device__ __forceinline__ float crs(P2 p1, P2 p2, P2 p0) { return (p1.x - p0.x) * (p2.y - p0.y) - (p2.x - p0.x) * (p1.y - p0.y); }

struct RBox {       // a box with its trigonometry evaluated once
  float x, y, dx, dy, ang, c, s;      // c = cos(ang), s = sin(ang)
  float nc, ns;                       // cos(-ang), sin(-ang) (separate evaluations, as the reference does)
};

__device__ __forceinline__ RBox make_rbox(const float* b) {
  RBox r;
  r.x = b[0]; r.y = b[1]; r.dx = b[3]; r.dy = b[4]; r.ang = b[6];
  r.c = cosf(r.ang); r.s = sinf(r.ang);
  r.nc = cosf(-r.ang); r.ns = sinf(-r.ang);
  return r;
}

__device__ __forceinline__ void corners(const RBox& b, P2 (&c)[5]) {
  const float hx = b.dx / 2, hy = b.dy / 2;
  const float px[4] = {b.x - hx, b.x + hx, b.x + hx, b.x - hx};
  const float py[4] = {b.y - hy, b.y - hy, b.y + hy, b.y + hy};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    c[k].x = (px[k] - b.x) * b.c + (py[k] - b.y) * (-b.s) + b.x;
    c[k].y = (px[k] - b.x) * b.s + (py[k] - b.y) * b.c + b.y;
  }
  c[4] = c[0];
}

__device__ __forceinline__ bool inside(const RBox& b, P2 p) {   // with the reference's 1e-2 margin
  const float rx = (p.x - b.x) * b.nc + (p.y - b.y) * (-b.ns);
  const float ry = (p.x - b.x) * b.ns + (p.y - b.y) * b.nc;
  return fabsf(rx) < b.dx / 2 + 1e-2f && fabsf(ry) < b.dy / 2 + 1e-2f;
}

__device__ __forceinline__ bool seg_x(P2 p1, P2 p0, P2 q1, P2 q0, P2& ans) {
  const bool boxes_meet = fminf(p0.x, p1.x) <= fmaxf(q0.x, q1.x) && fminf(q0.x, q1.x) <= fmaxf(p0.x, p1.x) &&
                          fminf(p0.y, p1.y) <= fmaxf(q0.y, q1.y) && fminf(q0.y, q1.y) <= fmaxf(p0.y, p1.y);
  if (!boxes_meet) return false;
  const float s1 = crs(q0, p1, p0), s2 = crs(p1, q1, p0), s3 = crs(p0, q1, q0), s4 = crs(q1, p1, q0);
  if (!(s1 * s2 > 0 && s3 * s4 > 0)) return false;
  const float s5 = crs(q1, p1, p0);
  if (fabsf(s5 - s1) > 1e-8f) {
    ans.x = (s5 * q0.x - s1 * q1.x) / (s5 - s1);
    ans.y = (s5 * q0.y - s1 * q1.y) / (s5 - s1);
  } else {
    const float a0 = p0.y - p1.y, b0 = p1.x - p0.x, c0 = p0.x * p1.y - p1.x * p0.y;
    const float a1 = q0.y - q1.y, b1 = q1.x - q0.x, c1 = q0.x * q1.y - q1.x * q0.y;
    const float D = a0 * b1 - a1 * b0;
    ans.x = (b0 * c1 - b1 * c0) / D;
    ans.y = (a1 * c0 - a0 * c1) / D;
  }
  return true;
}

// pts, ang: room for 24 polygon points and their angles, the caller's (private arrays, or LDS where a kernel must stay without scratch)
__device__ inline float overlap_area_in(const RBox& a, const RBox& b, P2* pts, float* ang) {
  // pairs whose bounding circles (+ the 1e-2 corner margin, + slack) are apart have no crossing and no corner inside:
  // the construction below would return exactly 0
  {
    const float ra = 0.5f * sqrtf(a.dx * a.dx + a.dy * a.dy), rb = 0.5f * sqrtf(b.dx * b.dx + b.dy * b.dy);
    const float ddx = a.x - b.x, ddy = a.y - b.y, reach = ra + rb + 0.05f;
    if (ddx * ddx + ddy * ddy > reach * reach) return 0.f;
  }
  P2 A[5], B[5];
  corners(a, A);
  corners(b, B);
  int cnt = 0;
  float sx = 0.f, sy = 0.f;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      P2 x;
      if (seg_x(A[i + 1], A[i], B[j + 1], B[j], x)) { sx += x.x; sy += x.y; pts[cnt++] = x; }
    }
  for (int k = 0; k < 4; ++k) {
    if (inside(a, B[k])) { sx += B[k].x; sy += B[k].y; pts[cnt++] = B[k]; }
    if (inside(b, A[k])) { sx += A[k].x; sy += A[k].y; pts[cnt++] = A[k]; }
  }
  if (cnt < 3) return 0.f;                 // fewer than 3 points span no area (the reference's sums are empty or zero)
  sx /= cnt; sy /= cnt;
  for (int i = 0; i < cnt; ++i) ang[i] = atan2f(pts[i].y - sy, pts[i].x - sx);
  for (int j = 0; j < cnt - 1; ++j)        // same bubble order as the reference (stable for equal angles)
    for (int i = 0; i < cnt - j - 1; ++i)
      if (ang[i] > ang[i + 1]) {
        const P2 t = pts[i]; pts[i] = pts[i + 1]; pts[i + 1] = t;
        const float u = ang[i]; ang[i] = ang[i + 1]; ang[i + 1] = u;
      }
  float area = 0.f;
  for (int k = 0; k < cnt - 1; ++k)
    area += (pts[k].x - pts[0].x) * (pts[k + 1].y - pts[0].y) - (pts[k].y - pts[0].y) * (pts[k + 1].x - pts[0].x);
  return fabsf(area) / 2.0f;
}

__device__ inline float overlap_area(const RBox& a, const RBox& b) {
  P2 pts[24];
  float ang[24];
  return overlap_area_in(a, b, pts, ang);
}

__device__ __forceinline__ float iou_bev(const RBox& a, const RBox& b) {
  const float sa = a.dx * a.dy, sb = b.dx * b.dy, so = overlap_area(a, b);
  return so / fmaxf(sa + sb - so, 1e-8f);
}
#endif
