// CaDDN's frustum -> voxel sampling (FrustumToVoxel.forward, detector3d/pcdet/models/backbones_3d/vfe/image_vfe_modules/f2v/frustum_to_voxel.py:29-54
// with FrustumGridGenerator, f2v/frustum_grid_generator.py:79-145, transform_utils.py:14-91 and DepthFFN.create_frustum_features,
// ffn/depth_ffn.py).  The reference materialises softmax(depth_logits)[:, :-1] * image_features as (B, C, D, H, W), a (B, X, Y, Z, 3) grid, and
// calls the 5-D grid_sample.  Trilinear sampling of a product that is separable in (depth, pixel) factors: for voxel v with pixel taps t = 0..3
// and depth taps d0, d1
//     a_t    = w_t * (wd0 * p[d0, pix_t] + wd1 * p[d1, pix_t])
//     out[c] = sum over t of a_t * f[pix_t, c]
// so neither the volume nor the grid is built.  Taps: t = 0..3 are (y0,x0), (y0,x1), (y1,x0), (y1,x1), w_t = wy * wx; taps outside the map or the
// depth range contribute zero (padding_mode="zeros"); coordinates are unnormalised as grid_sample(align_corners=True) does.
#include "common.h"
#include "inverse_lists.h"
#include "wave.h"

namespace {

enum { FR_UD = 0, FR_LID = 1, FR_SID = 2 };

struct FrustumGeom {
  int B, C, D, H, W;              // D depth bins (the probabilities have D + 1 channels), feature map H x W
  int X, Y, Z;
  float pc_min[3], vsize[3];      // voxel size = (pc_max - pc_min) / grid_size in fp32, as the reference's tensors
  int mode;
  float depth_min, bin_size;      // UD / LID: the bin size; SID: bin_size = log(1 + depth_max) - log(1 + depth_min), depth_min = log(1 + depth_min)
};

// per scene: T = lidar_to_cam @ grid_to_lidar (4 x 4), P = cam_to_img (3 x 4), the image size - 1 of the batch's largest image
struct FrustumScene {
  float T[16], P[12], wm1, hm1;
};
constexpr int FR_SCENE_FLOATS = 32;                                  // a record's stride in a scene table

__device__ __forceinline__ void frustum_scene(const FrustumGeom& g, const float* __restrict__ l2c, const float* __restrict__ c2i,
                                              const int32_t* __restrict__ ishape, int b, float* __restrict__ s) {
  const float* Cm = l2c + (int64_t)b * 16;
  for (int i = 0; i < 4; ++i) {
    for (int j = 0; j < 3; ++j) s[i * 4 + j] = Cm[i * 4 + j] * g.vsize[j];          // grid_to_lidar is diag(voxel size) with the translation pc_min
    s[i * 4 + 3] = ((Cm[i * 4 + 0] * g.pc_min[0] + Cm[i * 4 + 1] * g.pc_min[1]) + Cm[i * 4 + 2] * g.pc_min[2]) + Cm[i * 4 + 3];
  }
  for (int i = 0; i < 12; ++i) s[16 + i] = c2i[(int64_t)b * 12 + i];
  int hmax = ishape[0], wmax = ishape[1];
  for (int k = 1; k < g.B; ++k) {
    hmax = max(hmax, ishape[2 * k]);
    wmax = max(wmax, ishape[2 * k + 1]);
  }
  s[28] = (float)(wmax - 1);
  s[29] = (float)(hmax - 1);
  s[30] = 0.f;
  s[31] = 0.f;
}

__device__ __forceinline__ float frustum_unhomogenise(float z) { return fabsf(z) > 1e-8f ? 1.f / (z + 1e-8f) : 1.f; }

__device__ __forceinline__ float frustum_bin(const FrustumGeom& g, float d) {
  if (g.mode == FR_UD) return (d - g.depth_min) / g.bin_size;
  if (g.mode == FR_LID) return -0.5f + 0.5f * sqrtf(1.f + 8.f * (d - g.depth_min) / g.bin_size);
  return (float)g.D * (logf(1.f + d) - g.depth_min) / g.bin_size;
}

// the normalised grid coordinate (x -> image column, y -> image row, z -> depth bin) of voxel (x, y, z); non-finite components become -2
__device__ __forceinline__ void frustum_coord(const FrustumGeom& g, const float* __restrict__ s, int x, int y, int z, float gc[3]) {
  const float px = (float)x + 0.5f, py = (float)y + 0.5f, pz = (float)z + 0.5f;
  float h[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) h[i] = ((s[i * 4] * px + s[i * 4 + 1] * py) + s[i * 4 + 2] * pz) + s[i * 4 + 3];
  const float sc = frustum_unhomogenise(h[3]);
  const float cx = sc * h[0], cy = sc * h[1], cz = sc * h[2];
  const float* P = s + 16;
  float q[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) q[i] = ((P[i * 4] * cx + P[i * 4 + 1] * cy) + P[i * 4 + 2] * cz) + P[i * 4 + 3];
  const float si = frustum_unhomogenise(q[2]);
  const float u = si * q[0], v = si * q[1];
  const float bin = frustum_bin(g, q[2] - P[11]);
  gc[0] = u / s[28] * 2.f + -1.f;
  gc[1] = v / s[29] * 2.f + -1.f;
  gc[2] = bin / (float)(g.D - 1) * 2.f + -1.f;
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (!isfinite(gc[k])) gc[k] = -2.f;
}

struct FrustumTaps {
  int pix[4];        // y * W + x of tap t, -1: outside the map
  float w[4];        // wy * wx
  int d0, d1;        // depth taps, -1: outside [0, D)
  float wd0, wd1;
};

// one axis: the lower tap, both weights, which taps are inside
__device__ __forceinline__ void frustum_axis(float gcoord, int size, int& i0, bool& in0, bool& in1, float& w0, float& w1) {
  const float c = ((gcoord + 1.f) / 2.f) * (float)(size - 1);
  const float f0 = floorf(c);
  w1 = c - f0;
  w0 = (f0 + 1.f) - c;
  in0 = f0 >= 0.f && f0 <= (float)(size - 1);
  in1 = f0 >= -1.f && f0 <= (float)(size - 2);
  i0 = (in0 || in1) ? (int)f0 : 0;
}

__device__ __forceinline__ void frustum_taps(const FrustumGeom& g, const float* __restrict__ s, int x, int y, int z, FrustumTaps& t) {
  float gc[3];
  frustum_coord(g, s, x, y, z, gc);
  int x0, y0, z0; bool ix0, ix1, iy0, iy1, iz0, iz1; float wx0, wx1, wy0, wy1;
  frustum_axis(gc[0], g.W, x0, ix0, ix1, wx0, wx1);
  frustum_axis(gc[1], g.H, y0, iy0, iy1, wy0, wy1);
  frustum_axis(gc[2], g.D, z0, iz0, iz1, t.wd0, t.wd1);
  t.pix[0] = (iy0 && ix0) ? y0 * g.W + x0 : -1;
  t.pix[1] = (iy0 && ix1) ? y0 * g.W + x0 + 1 : -1;
  t.pix[2] = (iy1 && ix0) ? (y0 + 1) * g.W + x0 : -1;
  t.pix[3] = (iy1 && ix1) ? (y0 + 1) * g.W + x0 + 1 : -1;
  t.w[0] = wy0 * wx0; t.w[1] = wy0 * wx1; t.w[2] = wy1 * wx0; t.w[3] = wy1 * wx1;
  t.d0 = iz0 ? z0 : -1;
  t.d1 = iz1 ? z0 + 1 : -1;
}

__global__ __launch_bounds__(64) void k_frustum_scenes(FrustumGeom g, const float* __restrict__ l2c, const float* __restrict__ c2i,
                                                       const int32_t* __restrict__ ishape, float* __restrict__ scenes) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < g.B) frustum_scene(g, l2c, c2i, ishape, b, scenes + (int64_t)b * FR_SCENE_FLOATS);
}

// (B, X, Y, Z, 3); blockIdx.y is the scene
__global__ __launch_bounds__(256) void k_frustum_grid(FrustumGeom g, const float* __restrict__ l2c, const float* __restrict__ c2i,
                                                      const int32_t* __restrict__ ishape, float* __restrict__ out) {
  __shared__ float s[FR_SCENE_FLOATS];
  const int b = blockIdx.y;
  if (threadIdx.x == 0) frustum_scene(g, l2c, c2i, ishape, b, s);
  __syncthreads();
  const int64_t nvox = (int64_t)g.X * g.Y * g.Z;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nvox; e += (int64_t)gridDim.x * blockDim.x) {
    const int z = (int)(e % g.Z);
    const int y = (int)((e / g.Z) % g.Y);
    const int x = (int)(e / ((int64_t)g.Z * g.Y));
    float gc[3];
    frustum_coord(g, s, x, y, z, gc);
    float* o = out + ((int64_t)b * nvox + e) * 3;
    o[0] = gc[0]; o[1] = gc[1]; o[2] = gc[2];
  }
}

// Forward.  One workgroup per column (b, y, x): the Z voxels' taps and a_t go to LDS, then the lanes run along (z, c) with c fastest -- a tap is
// one contiguous row of C floats -- and stage out[c][z] in LDS, so that the column's C * Z values (cchunk * Z when C * Z does not fit) leave as one
// contiguous run of the (B, Y, X, C, Z) storage.  LDS: scene | a (4 Z) | pix (4 Z) | stage (cchunk * Z).
template <int VEC>
__global__ __launch_bounds__(256) void k_frustum_to_voxel(FrustumGeom g, const float* __restrict__ l2c, const float* __restrict__ c2i,
                                                          const int32_t* __restrict__ ishape, const float* __restrict__ feats,
                                                          const float* __restrict__ probs, int cchunk, float* __restrict__ out) {
  extern __shared__ float lds[];
  float* s = lds;
  float* a = s + FR_SCENE_FLOATS;
  int* pixl = reinterpret_cast<int*>(a + 4 * g.Z);
  float* stage = reinterpret_cast<float*>(pixl + 4 * g.Z);
  const int b = blockIdx.y;
  if (threadIdx.x == 0) frustum_scene(g, l2c, c2i, ishape, b, s);
  __syncthreads();
  const int64_t hw = (int64_t)g.H * g.W;
  const float* pb = probs + (int64_t)b * hw * (g.D + 1);
  const float* fb = feats + (int64_t)b * hw * g.C;
  const int ncol = g.X * g.Y;                                      // X * Y * Z < 2^29 is checked by the caller
  for (int col = blockIdx.x; col < ncol; col += gridDim.x) {
    const int y = col / g.X, x = col - y * g.X;
    for (int z = threadIdx.x; z < g.Z; z += blockDim.x) {
      FrustumTaps t;
      frustum_taps(g, s, x, y, z, t);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float ak = 0.f;
        int pk = -1;
        if (t.pix[k] >= 0 && (t.d0 >= 0 || t.d1 >= 0)) {
          const float* pp = pb + (int64_t)t.pix[k] * (g.D + 1);
          const float p0 = t.d0 >= 0 ? t.wd0 * pp[t.d0] : 0.f;
          const float p1 = t.d1 >= 0 ? t.wd1 * pp[t.d1] : 0.f;
          ak = t.w[k] * (p0 + p1);
          pk = t.pix[k];
        }
        a[z * 4 + k] = ak;
        pixl[z * 4 + k] = pk;
      }
    }
    __syncthreads();
    float* ocol = out + ((int64_t)b * ncol + col) * g.C * g.Z;
    for (int c0 = 0; c0 < g.C; c0 += cchunk) {
      const int cc = min(cchunk, g.C - c0);                        // a multiple of VEC
      const int cvc = cc / VEC;
      for (int e = threadIdx.x; e < g.Z * cvc; e += blockDim.x) {
        const int z = e / cvc;
        const int cq = (e - z * cvc) * VEC;
        float acc[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int pk = pixl[z * 4 + k];
          if (pk < 0) continue;
          const float ak = a[z * 4 + k];
          const float* fp = fb + (int64_t)pk * g.C + c0 + cq;
          if constexpr (VEC == 4) {
            const float4 f4 = *reinterpret_cast<const float4*>(fp);
            acc[0] = acc[0] + ak * f4.x; acc[1] = acc[1] + ak * f4.y; acc[2] = acc[2] + ak * f4.z; acc[3] = acc[3] + ak * f4.w;
          } else {
            acc[0] = acc[0] + ak * fp[0];
          }
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) stage[(cq + v) * g.Z + z] = acc[v];
      }
      __syncthreads();
      float* o = ocol + (int64_t)c0 * g.Z;
      for (int i = threadIdx.x; i < cc * g.Z; i += blockDim.x) o[i] = stage[i];
      __syncthreads();
    }
  }
}

// Key 4 * v + t names the pixel of tap t of voxel v = ((b * Y + y) * X + x) * Z + z -- the voxel's position in the output's storage order.  A tap
// outside the map, or of a voxel with both depth taps outside, has no key.
struct FrustumTapRow {
  FrustumGeom g;
  const float* scenes;
  __device__ __forceinline__ int64_t operator()(int64_t key) const {
    const int64_t v = key >> 2;
    const int z = (int)(v % g.Z);
    const int64_t col = v / g.Z;
    const int x = (int)(col % g.X);
    const int y = (int)((col / g.X) % g.Y);
    const int b = (int)(col / ((int64_t)g.X * g.Y));
    FrustumTaps t;
    frustum_taps(g, scenes + (int64_t)b * FR_SCENE_FLOATS, x, y, z, t);
    const int k = (int)(key & 3);
    const int p = k == 0 ? t.pix[0] : k == 1 ? t.pix[1] : k == 2 ? t.pix[2] : t.pix[3];
    if (p < 0 || (t.d0 < 0 && t.d1 < 0)) return -1;
    return (int64_t)b * g.H * g.W + p;
  }
};

// Gradient: one wave per pixel walks the pixel's keys in ascending order; lane l holds the channels l, l + 64 (, ...) of the pixel's feature
// row and of its gradient; the wave's D + 1 depth-bin sums live in LDS and lane 0 alone adds to them.
__global__ __launch_bounds__(256) void k_frustum_grad_gather(FrustumGeom g, const float* __restrict__ scenes, const float* __restrict__ feats,
                                                             const float* __restrict__ probs, const float* __restrict__ gout, int64_t npix,
                                                             SvInvLists L, float* __restrict__ gfeats, float* __restrict__ gprobs) {
  constexpr int MAXV = 2;                                          // channels a lane holds at once: one trip for C <= 128
  extern __shared__ float lds[];
  const int lane = threadIdx.x & 63;
  float* gpl = lds + (threadIdx.x >> 6) * (g.D + 1);
  const int64_t hw = (int64_t)g.H * g.W;
  const int64_t cz = (int64_t)g.C * g.Z;
  const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t p = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); p < npix; p += nwaves) {
    const int b = (int)(p / hw);
    const float* s = scenes + (int64_t)b * FR_SCENE_FLOATS;
    const float* pp = probs + p * (g.D + 1);
    for (int d = lane; d <= g.D; d += 64) gpl[d] = 0.f;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    int32_t n;
    const int32_t* keys = sv_inv_list(L, p, n);
    for (int cb = 0; cb < g.C; cb += 64 * MAXV) {
      float fr[MAXV], acc[MAXV];
#pragma unroll
      for (int u = 0; u < MAXV; ++u) {
        const int c = cb + u * 64 + lane;
        fr[u] = c < g.C ? feats[p * g.C + c] : 0.f;
        acc[u] = 0.f;
      }
      for (int32_t i = 0; i < n; ++i) {
        const int32_t key = __builtin_amdgcn_readfirstlane(keys[i]);
        const int64_t v = key >> 2;
        const int z = (int)(v % g.Z);
        const int64_t col = v / g.Z;
        const int x = (int)(col % g.X);
        const int y = (int)((col / g.X) % g.Y);
        FrustumTaps t;
        frustum_taps(g, s, x, y, z, t);
        const int k = key & 3;
        const float w = k == 0 ? t.w[0] : k == 1 ? t.w[1] : k == 2 ? t.w[2] : t.w[3];
        const float p0 = t.d0 >= 0 ? t.wd0 * pp[t.d0] : 0.f;
        const float p1 = t.d1 >= 0 ? t.wd1 * pp[t.d1] : 0.f;
        const float ak = w * (p0 + p1);
        const float* go = gout + col * cz + z;
        float dot = 0.f;
#pragma unroll
        for (int u = 0; u < MAXV; ++u) {
          const int c = cb + u * 64 + lane;
          if (c < g.C) {
            const float gv = go[(int64_t)c * g.Z];
            acc[u] = acc[u] + ak * gv;
            dot = dot + gv * fr[u];
          }
        }
        dot = sv_wave_reduce_sum(dot);
        if (lane == 0) {
          if (t.d0 >= 0) gpl[t.d0] = gpl[t.d0] + (w * t.wd0) * dot;
          if (t.d1 >= 0) gpl[t.d1] = gpl[t.d1] + (w * t.wd1) * dot;
        }
      }
#pragma unroll
      for (int u = 0; u < MAXV; ++u) {
        const int c = cb + u * 64 + lane;
        if (c < g.C) gfeats[p * g.C + c] = acc[u];
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int d = lane; d <= g.D; d += 64) gprobs[p * (g.D + 1) + d] = gpl[d];          // the ignored last bin was never added to: +0.0f
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

bool frustum_geom(FrustumGeom& g, int B, int C, int D, int H, int W, int X, int Y, int Z, const float* pc_range_host, int mode, double depth_min,
                  double depth_max) {
  if (!(B > 0 && C > 0 && D > 0 && H > 0 && W > 0 && X > 0 && Y > 0 && Z > 0 && pc_range_host) || mode < FR_UD || mode > FR_SID) return false;
  g.B = B; g.C = C; g.D = D; g.H = H; g.W = W; g.X = X; g.Y = Y; g.Z = Z;
  const int gs[3] = {X, Y, Z};
  for (int k = 0; k < 3; ++k) {
    g.pc_min[k] = pc_range_host[k];
    g.vsize[k] = (pc_range_host[3 + k] - pc_range_host[k]) / (float)gs[k];
  }
  g.mode = mode;
  if (mode == FR_UD) {
    g.depth_min = (float)depth_min;
    g.bin_size = (float)((depth_max - depth_min) / D);
  } else if (mode == FR_LID) {
    g.depth_min = (float)depth_min;
    g.bin_size = (float)(2.0 * (depth_max - depth_min) / ((double)D * (1.0 + D)));
  } else {
    g.depth_min = (float)log(1.0 + depth_min);
    g.bin_size = (float)(log(1.0 + depth_max) - log(1.0 + depth_min));
  }
  return true;
}

bool frustum_fits(int B, int H, int W, int X, int Y, int Z) {
  return (int64_t)B * H * W < ((int64_t)1 << 31) && 4 * (int64_t)B * X * Y * Z < ((int64_t)1 << 31);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

constexpr int FR_STAGE_FLOATS = 8192;       // the forward's staging run: 32 KB
constexpr int FR_MAX_Z = 512, FR_MAX_D = 4095;

}  // namespace

extern "C" int sv_frustum_grid(const float* lidar_to_cam, const float* cam_to_img, const int32_t* image_shape, int batch, int X, int Y, int Z,
                               const float* pc_range_host, int mode, double depth_min, double depth_max, int num_bins, float* out, void* stream) {
  FrustumGeom g;
  SV_CHECK_ARG(frustum_geom(g, batch, 1, num_bins, 1, 1, X, Y, Z, pc_range_host, mode, depth_min, depth_max), "frustum_grid: bad arguments");
  SV_CHECK_ARG(lidar_to_cam && cam_to_img && image_shape && out, "frustum_grid: null pointer");
  SV_CHECK_ARG(sv_on_device(lidar_to_cam) && sv_on_device(cam_to_img) && sv_on_device(image_shape) && sv_on_device(out),
               "frustum_grid: host pointer");
  SV_CHECK_ARG(batch < 65536 && 4 * (int64_t)batch * X * Y * Z < ((int64_t)1 << 31), "frustum_grid: voxel index exceeds int32");
  hipLaunchKernelGGL(k_frustum_grid, dim3(sv_grid_1d((int64_t)X * Y * Z, 256), batch), dim3(256), 0, sv_stream(stream), g, lidar_to_cam, cam_to_img,
                     image_shape, out);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_frustum_to_voxel(const float* image_features, const float* depth_probs, const float* lidar_to_cam, const float* cam_to_img,
                                   const int32_t* image_shape, int batch, int C, int D, int H, int W, int X, int Y, int Z,
                                   const float* pc_range_host, int mode, double depth_min, double depth_max, float* out, void* stream) {
  FrustumGeom g;
  SV_CHECK_ARG(frustum_geom(g, batch, C, D, H, W, X, Y, Z, pc_range_host, mode, depth_min, depth_max), "frustum_to_voxel: bad arguments");
  SV_CHECK_ARG(image_features && depth_probs && lidar_to_cam && cam_to_img && image_shape && out, "frustum_to_voxel: null pointer");
  SV_CHECK_ARG(sv_on_device(image_features) && sv_on_device(depth_probs) && sv_on_device(lidar_to_cam) && sv_on_device(cam_to_img) &&
                   sv_on_device(image_shape) && sv_on_device(out), "frustum_to_voxel: host pointer");
  SV_CHECK_ARG(batch < 65536 && frustum_fits(batch, H, W, X, Y, Z), "frustum_to_voxel: pixel index or tap key exceeds int32");
  SV_CHECK_ARG(Z <= FR_MAX_Z, "frustum_to_voxel: more than %d voxels in a column", FR_MAX_Z);
  const bool vec = C % 4 == 0 && aligned16(image_features);
  const int unit = vec ? 4 : 1;
  int cchunk = C;
  if ((int64_t)C * Z > FR_STAGE_FLOATS) cchunk = max(unit, FR_STAGE_FLOATS / Z / unit * unit);
  const size_t lds = (size_t)(FR_SCENE_FLOATS + 8 * Z + cchunk * Z) * sizeof(float);
  const dim3 grid(sv_grid_1d((int64_t)X * Y * 256, 256, 256 * 16), batch);
  if (vec)
    hipLaunchKernelGGL(k_frustum_to_voxel<4>, grid, dim3(256), lds, sv_stream(stream), g, lidar_to_cam, cam_to_img, image_shape, image_features,
                       depth_probs, cchunk, out);
  else
    hipLaunchKernelGGL(k_frustum_to_voxel<1>, grid, dim3(256), lds, sv_stream(stream), g, lidar_to_cam, cam_to_img, image_shape, image_features,
                       depth_probs, cchunk, out);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// the scene table, then an SvInvLists of 4 * B * X * Y * Z keys over B * H * W rows
extern "C" size_t sv_frustum_to_voxel_grad_scratch_bytes(int batch, int H, int W, int X, int Y, int Z) {
  if (batch <= 0 || H <= 0 || W <= 0 || X <= 0 || Y <= 0 || Z <= 0 || !frustum_fits(batch, H, W, X, Y, Z)) return 0;
  const size_t scenes = ((size_t)batch * FR_SCENE_FLOATS * sizeof(float) + 255) / 256 * 256;
  return scenes + sv_inv_lists_bytes(4 * (int64_t)batch * X * Y * Z, (int64_t)batch * H * W);
}

extern "C" int sv_frustum_to_voxel_grad(const float* image_features, const float* depth_probs, const float* lidar_to_cam, const float* cam_to_img,
                                        const int32_t* image_shape, const float* grad_out, int batch, int C, int D, int H, int W, int X, int Y, int Z,
                                        const float* pc_range_host, int mode, double depth_min, double depth_max, void* scratch,
                                        float* grad_features, float* grad_probs, void* stream) {
  FrustumGeom g;
  SV_CHECK_ARG(frustum_geom(g, batch, C, D, H, W, X, Y, Z, pc_range_host, mode, depth_min, depth_max), "frustum_to_voxel_grad: bad arguments");
  SV_CHECK_ARG(frustum_fits(batch, H, W, X, Y, Z), "frustum_to_voxel_grad: pixel index or tap key exceeds int32");
  SV_CHECK_ARG(D <= FR_MAX_D, "frustum_to_voxel_grad: more than %d depth bins", FR_MAX_D);
  SV_CHECK_ARG(image_features && depth_probs && lidar_to_cam && cam_to_img && image_shape && grad_out && scratch && grad_features && grad_probs,
               "frustum_to_voxel_grad: null pointer");
  SV_CHECK_ARG(sv_on_device(image_features) && sv_on_device(depth_probs) && sv_on_device(lidar_to_cam) && sv_on_device(cam_to_img) &&
                   sv_on_device(image_shape) && sv_on_device(grad_out) && sv_on_device(scratch) && sv_on_device(grad_features) &&
                   sv_on_device(grad_probs), "frustum_to_voxel_grad: host pointer");
  hipStream_t st = sv_stream(stream);
  float* scenes = reinterpret_cast<float*>(scratch);
  const size_t scene_bytes = ((size_t)batch * FR_SCENE_FLOATS * sizeof(float) + 255) / 256 * 256;
  const int64_t nkeys = 4 * (int64_t)batch * X * Y * Z, npix = (int64_t)batch * H * W;
  const SvInvLists L = sv_inv_lists_view(reinterpret_cast<char*>(scratch) + scene_bytes, nkeys, npix);
  hipLaunchKernelGGL(k_frustum_scenes, dim3(sv_div_up(batch, 64)), dim3(64), 0, st, g, lidar_to_cam, cam_to_img, image_shape, scenes);
  if (int rc = sv_inv_lists_build(nkeys, npix, FrustumTapRow{g, scenes}, L, st)) return rc;
  hipLaunchKernelGGL(k_frustum_grad_gather, dim3(sv_grid_1d(npix * 64, 256, 256 * 16)), dim3(256), (size_t)4 * (D + 1) * sizeof(float), st, g, scenes,
                     image_features, depth_probs, grad_out, npix, L, grad_features, grad_probs);
  SV_LAUNCH_CHECK();
  return SV_OK;
}
