// The image branch of focal sparse convolution: FocalSparseConv.construct_multimodal_features
// (detector3d/pcdet/models/backbones_3d/focal_sparse_conv/focal_sparse_conv.py:50-113).  The reference loops over the scenes, sends every scene's
// voxel centres to the host, projects them with numpy (Calibration.lidar_to_img, detector3d/pcdet/utils/calibration_kitti.py:65-93), uploads the
// pixels and indexes a (B, C, H, W) map that F.interpolate made from the quarter-resolution features.  Here: one launch projects every row of every
// scene (sv_focal_image_pixels), one reads the features at the pixel -- through the four taps the bilinear up-sampling would have blended, so the
// up-sampled map is never built -- and writes the fused rows (sv_focal_image_sample), and the gradient into the feature map walks per-pixel key
// lists in ascending order (sv_focal_image_sample_grad): no float atomics, equal bits run to run.
#include "common.h"
#include "inverse_lists.h"

namespace {

constexpr int FI_CALIB_FLOATS = 24;     // per scene: M = V2C^T R0^T (4 x 3, row-major), then P2 (3 x 4, row-major)
constexpr int FI_AUG_FLOATS = 4;        // per scene: noise_scale, noise_rot, flip_x, flip_y

struct FiGrid {
  float vs[3], org[3];                  // z-first, as the layer keeps them
  int stride, B, H, W;
};

// Image size (H, W) and feature size (h, w); eq: the two agree and a row reads its own pixel.
struct FiMap {
  int B, H, W, h, w, C, eq;
};

// One axis of F.interpolate(mode='bilinear', align_corners=False) at integer destination d: src = max(in / out * (d + 0.5) - 0.5, 0) is the rational
// (in * (2 d + 1) - out) / (2 out), so i0 is an integer quotient and the weight of i1 the remainder over 2 out, rounded to fp32 once.
__device__ __forceinline__ void fi_axis(int d, int in, int out, int& i0, int& i1, float& l0, float& l1) {
  const int64_t num = (int64_t)in * (2 * (int64_t)d + 1) - out;
  const int64_t den = 2 * (int64_t)out;
  if (num <= 0) {
    i0 = 0;
    l1 = 0.f;
  } else {
    i0 = (int)(num / den);
    l1 = (float)(num - (int64_t)i0 * den) / (float)den;
  }
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l0 = 1.f - l1;
}

// The low-resolution pixels (within a scene) and weights of the taps t = 0..3 = (y0,x0), (y0,x1), (y1,x0), (y1,x1) of image pixel p = v * W + u.
__device__ __forceinline__ void fi_taps(const FiMap& m, int p, int32_t px[4], float wt[4]) {
  const int v = p / m.W, u = p - v * m.W;
  int y0, y1, x0, x1;
  float ly0, ly1, lx0, lx1;
  fi_axis(v, m.h, m.H, y0, y1, ly0, ly1);
  fi_axis(u, m.w, m.W, x0, x1, lx0, lx1);
  px[0] = y0 * m.w + x0; wt[0] = ly0 * lx0;
  px[1] = y0 * m.w + x1; wt[1] = ly0 * lx1;
  px[2] = y1 * m.w + x0; wt[2] = ly1 * lx0;
  px[3] = y1 * m.w + x1; wt[3] = ly1 * lx1;
}

// whether row i has a pixel the maps hold: the caller's pix may be anything, so the scene index and the pixel are tested here
__device__ __forceinline__ bool fi_row(const FiMap& m, const int32_t* __restrict__ coords, const int32_t* __restrict__ pix, int64_t i, int& b, int& p) {
  p = pix[i];
  b = coords[i * 4];
  return p >= 0 && p < m.H * m.W && b >= 0 && b < m.B;
}

__global__ __launch_bounds__(256) void k_focal_image_pixels(const int32_t* __restrict__ coords, int64_t n, FiGrid g, const float* __restrict__ calib,
                                                            const float* __restrict__ aug, int32_t* __restrict__ pix) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int4 c = *reinterpret_cast<const int4*>(coords + i * 4);
    if (c.x < 0 || c.x >= g.B) {
      pix[i] = -1;
      continue;
    }
    const float* A = aug + (int64_t)c.x * FI_AUG_FLOATS;
    const float* M = calib + (int64_t)c.x * FI_CALIB_FLOATS;
    const float* P = M + 12;
    // :63-64: spatial_indices * voxel_size + point_cloud_range[:3], the product of the integers first
    float z = (float)(c.y * g.stride) * g.vs[0] + g.org[0];
    float y = (float)(c.z * g.stride) * g.vs[1] + g.org[1];
    float x = (float)(c.w * g.stride) * g.vs[2] + g.org[2];
    const float scale = A[0];
    x = x / scale; y = y / scale; z = z / scale;                       // :84
    const float ang = -A[1];                                           // :86, rotate_points_along_z: [x y z] @ [[c s 0] [-s c 0] [0 0 1]]
    const float ca = cosf(ang), sa = sinf(ang);
    const float xr = (x * ca + y * (-sa)) + z * 0.f;
    const float yr = (x * sa + y * ca) + z * 0.f;
    const float zr = (x * 0.f + y * 0.f) + z * 1.f;
    x = xr; y = yr; z = zr;
    if (A[2] != 0.f) y = -y;                                           // :88, flip_x negates y
    if (A[3] != 0.f) x = -x;                                           // :90, flip_y negates x
    float r[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) r[j] = ((x * M[j] + y * M[3 + j]) + z * M[6 + j]) + 1.f * M[9 + j];          // lidar_to_rect
    const float p0 = ((r[0] * P[0] + r[1] * P[1]) + r[2] * P[2]) + 1.f * P[3];                             // rect_to_img
    const float p1 = ((r[0] * P[4] + r[1] * P[5]) + r[2] * P[6]) + 1.f * P[7];
    const float u = p0 / r[2], v = p1 / r[2];
    // .long() truncates toward zero: trunc(u) >= 0 iff u > -1, trunc(u) < W iff u < W; a NaN fails the comparisons, an infinity one of them
    const bool in = u > -1.f && u < (float)g.W && v > -1.f && v < (float)g.H;
    pix[i] = in ? (int)v * g.W + (int)u : -1;
  }
}

// mode 0: out (n, C + Cv) = [img | f]; mode 1: out (n, Cv) = f + img.  One work item per VEC floats of an output row.
template <int VEC>
__global__ __launch_bounds__(256) void k_focal_image_sample(const float* __restrict__ feat, FiMap m, const float* __restrict__ f, int Cv,
                                                            const int32_t* __restrict__ coords, const int32_t* __restrict__ pix, int64_t n, int mode,
                                                            float* __restrict__ out) {
  const int ld = mode ? Cv : m.C + Cv;
  const int per = ld / VEC;
  const int64_t total = n * per;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = e / per;
    const int col = (int)(e - i * per) * VEC;
    float* o = out + i * ld + col;
    const bool image_col = mode || col < m.C;
    float acc[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
    if (image_col) {
      int b, p;
      if (fi_row(m, coords, pix, i, b, p)) {
        const float* base = feat + (int64_t)b * m.h * m.w * m.C + col;
        if (m.eq) {
          const float* s = base + (int64_t)p * m.C;
          if constexpr (VEC == 4) {
            const float4 x = *reinterpret_cast<const float4*>(s);
            acc[0] = x.x; acc[1] = x.y; acc[2] = x.z; acc[3] = x.w;
          } else {
            acc[0] = *s;
          }
        } else {
          int32_t px[4];
          float wt[4];
          fi_taps(m, p, px, wt);
          float t[4][VEC];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float* s = base + (int64_t)px[q] * m.C;
            if constexpr (VEC == 4) {
              const float4 x = *reinterpret_cast<const float4*>(s);
              t[q][0] = x.x; t[q][1] = x.y; t[q][2] = x.z; t[q][3] = x.w;
            } else {
              t[q][0] = *s;
            }
          }
#pragma unroll
          for (int k = 0; k < VEC; ++k) acc[k] = ((t[0][k] * wt[0] + t[1][k] * wt[1]) + t[2][k] * wt[2]) + t[3][k] * wt[3];
        }
      }
    }
    if (!image_col || mode) {
      const float* s = f + i * Cv + (mode ? col : col - m.C);
      if constexpr (VEC == 4) {
        const float4 x = *reinterpret_cast<const float4*>(s);
        if (mode) { acc[0] = x.x + acc[0]; acc[1] = x.y + acc[1]; acc[2] = x.z + acc[2]; acc[3] = x.w + acc[3]; }
        else { acc[0] = x.x; acc[1] = x.y; acc[2] = x.z; acc[3] = x.w; }
      } else {
        acc[0] = mode ? *s + acc[0] : *s;
      }
    }
    if constexpr (VEC == 4) *reinterpret_cast<float4*>(o) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    else *o = acc[0];
  }
}

// Key 4 * i + t names the low-resolution pixel of tap t of row i; with equal sizes key i names row i's pixel.  A row without a pixel has no keys.
struct FiTapRow {
  const int32_t* coords;
  const int32_t* pix;
  FiMap m;
  __device__ __forceinline__ int64_t operator()(int64_t key) const {
    const int64_t i = m.eq ? key : key >> 2;
    int b, p;
    if (!fi_row(m, coords, pix, i, b, p)) return -1;
    int32_t local = p;
    if (!m.eq) {
      int32_t px[4];
      float wt[4];
      fi_taps(m, p, px, wt);
      const int t = (int)(key & 3);
      local = t == 0 ? px[0] : t == 1 ? px[1] : t == 2 ? px[2] : px[3];
    }
    return (int64_t)b * m.h * m.w + local;
  }
};

// One wave per low-resolution pixel, the terms in the order of the pixel's list; g (n, ldg), of which the first C columns are read.
template <int VEC>
__global__ __launch_bounds__(256) void k_focal_image_grad_gather(const float* __restrict__ g, int ldg, const int32_t* __restrict__ pix, FiMap m,
                                                                 int64_t npix, SvInvLists L, float* __restrict__ gfeat) {
  const int lane = threadIdx.x & 63;
  const int cv = m.C / VEC;
  const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t q = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); q < npix; q += nwaves) {
    int32_t cnt;
    const int32_t* keys = sv_inv_list(L, q, cnt);
    for (int cb = 0; cb < cv; cb += 64) {                             // one trip for C <= 64 * VEC
      const int c = cb + lane;
      float acc[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
      for (int32_t j = 0; j < cnt; ++j) {
        const int32_t key = __builtin_amdgcn_readfirstlane(keys[j]);
        const int64_t i = m.eq ? key : key >> 2;
        float w = 1.f;
        if (!m.eq) {
          int32_t px[4];
          float wt[4];
          fi_taps(m, pix[i], px, wt);
          const int t = key & 3;
          w = t == 0 ? wt[0] : t == 1 ? wt[1] : t == 2 ? wt[2] : wt[3];
        }
        if (c < cv) {
          const float* s = g + i * ldg + (int64_t)c * VEC;
          if constexpr (VEC == 4) {
            const float4 x = *reinterpret_cast<const float4*>(s);
            acc[0] = acc[0] + x.x * w; acc[1] = acc[1] + x.y * w; acc[2] = acc[2] + x.z * w; acc[3] = acc[3] + x.w * w;
          } else {
            acc[0] = acc[0] + *s * w;
          }
        }
      }
      if (c < cv) {
        float* o = gfeat + q * m.C + (int64_t)c * VEC;
        if constexpr (VEC == 4) *reinterpret_cast<float4*>(o) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        else *o = acc[0];
      }
    }
  }
}

inline bool fi_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline bool fi_map_ok(int batch, int H, int W, int h, int w, int C) {
  return batch > 0 && H > 0 && W > 0 && h > 0 && w > 0 && C > 0 && (int64_t)H * W < ((int64_t)1 << 31) && (int64_t)batch * h * w < ((int64_t)1 << 31);
}

inline FiMap fi_map(int batch, int H, int W, int h, int w, int C) { return FiMap{batch, H, W, h, w, C, (h == H && w == W) ? 1 : 0}; }

}  // namespace

extern "C" int sv_focal_image_pixels(const int32_t* coords, int64_t n, int batch, int voxel_stride, const float* voxel_size_host,
                                     const float* origin_host, const float* calib, const float* aug, int H, int W, int32_t* pix, void* stream) {
  SV_CHECK_ARG(n >= 0 && batch > 0 && voxel_stride > 0 && H > 0 && W > 0 && (int64_t)H * W < ((int64_t)1 << 31) && voxel_size_host && origin_host,
               "focal_image_pixels: bad arguments");
  if (n == 0) return SV_OK;
  SV_CHECK_ARG(coords && calib && aug && pix, "focal_image_pixels: null pointer");
  SV_CHECK_ARG(fi_aligned16(coords), "focal_image_pixels: coords is read a row (16 bytes) at a time and must be 16-byte aligned");
  FiGrid g;
  for (int k = 0; k < 3; ++k) {
    g.vs[k] = voxel_size_host[k];
    g.org[k] = origin_host[k];
  }
  g.stride = voxel_stride; g.B = batch; g.H = H; g.W = W;
  hipLaunchKernelGGL(k_focal_image_pixels, dim3(sv_grid_1d(n, 256)), dim3(256), 0, sv_stream(stream), coords, n, g, calib, aug, pix);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_focal_image_sample(const float* features, int batch, int h, int w, int C, int H, int W, const float* f, int Cv,
                                     const int32_t* coords, const int32_t* pix, int64_t n, int mode, float* out, void* stream) {
  SV_CHECK_ARG(n >= 0 && Cv > 0 && (mode == 0 || mode == 1) && fi_map_ok(batch, H, W, h, w, C), "focal_image_sample: bad arguments");
  SV_CHECK_ARG(mode == 0 || C == Cv, "focal_image_sample: the sum needs as many image channels (%d) as voxel channels (%d)", C, Cv);
  if (n == 0) return SV_OK;
  SV_CHECK_ARG(features && f && coords && pix && out, "focal_image_sample: null pointer");
  const FiMap m = fi_map(batch, H, W, h, w, C);
  const int ld = mode ? Cv : C + Cv;
  if (C % 4 == 0 && Cv % 4 == 0 && fi_aligned16(features) && fi_aligned16(f) && fi_aligned16(out))
    hipLaunchKernelGGL(k_focal_image_sample<4>, dim3(sv_grid_1d(n * (ld / 4), 256, 256 * 16)), dim3(256), 0, sv_stream(stream), features, m, f, Cv,
                       coords, pix, n, mode, out);
  else
    hipLaunchKernelGGL(k_focal_image_sample<1>, dim3(sv_grid_1d(n * ld, 256, 256 * 16)), dim3(256), 0, sv_stream(stream), features, m, f, Cv, coords,
                       pix, n, mode, out);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// an SvInvLists of 4 n keys (n with equal sizes) over B * h * w rows; 0: the sizes exceed the guards
extern "C" size_t sv_focal_image_sample_grad_scratch_bytes(int64_t n, int batch, int h, int w, int H, int W) {
  if (n < 0 || !fi_map_ok(batch, H, W, h, w, 1) || n >= ((int64_t)1 << 29)) return 0;
  return sv_inv_lists_bytes((h == H && w == W) ? n : 4 * n, (int64_t)batch * h * w);
}

extern "C" int sv_focal_image_sample_grad(const float* grad_out, int ldg, const int32_t* coords, const int32_t* pix, int64_t n, int batch, int h,
                                          int w, int C, int H, int W, void* scratch, float* grad_features, void* stream) {
  SV_CHECK_ARG(n >= 0 && fi_map_ok(batch, H, W, h, w, C) && ldg >= C && grad_features, "focal_image_sample_grad: bad arguments");
  SV_CHECK_ARG(n < ((int64_t)1 << 29), "focal_image_sample_grad: the tap keys 4 * n exceed int32");
  const int64_t npix = (int64_t)batch * h * w;
  hipStream_t st = sv_stream(stream);
  if (n == 0) {
    SV_HIP(hipMemsetAsync(grad_features, 0, (size_t)npix * C * 4, st));
    return SV_OK;
  }
  SV_CHECK_ARG(grad_out && coords && pix && scratch, "focal_image_sample_grad: null pointer");
  const FiMap m = fi_map(batch, H, W, h, w, C);
  const int64_t nkeys = m.eq ? n : 4 * n;
  const SvInvLists L = sv_inv_lists_view(scratch, nkeys, npix);
  if (int rc = sv_inv_lists_build(nkeys, npix, FiTapRow{coords, pix, m}, L, st)) return rc;            // the gradient map itself is never cleared
  const dim3 grid(sv_grid_1d(npix * 64, 256, 256 * 16));
  if (C % 4 == 0 && ldg % 4 == 0 && fi_aligned16(grad_out) && fi_aligned16(grad_features))
    hipLaunchKernelGGL(k_focal_image_grad_gather<4>, grid, dim3(256), 0, st, grad_out, ldg, pix, m, npix, L, grad_features);
  else
    hipLaunchKernelGGL(k_focal_image_grad_gather<1>, grid, dim3(256), 0, st, grad_out, ldg, pix, m, npix, L, grad_features);
  SV_LAUNCH_CHECK();
  return SV_OK;
}
