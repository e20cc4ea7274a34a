// PointNet++ batch-layout primitives and the 3-NN interpolation of both layouts — the remaining wrappers of the reference's
// pointnet2_batch_cuda / pointnet2_stack_cuda extensions (detector3d/pcdet/ops/pointnet2/pointnet2_batch/src/*.cu,
// pointnet2_stack/src/interpolate_gpu.cu; pybind names in pointnet2_api.cpp).  Same results as the reference kernels
// (scan order, strict comparisons, fp32 arithmetic without contraction); gradient kernels use float atomics like theirs and
// zero-fill their output themselves; their *_ordered twins sum in a stated order without float atomics (opt-in).
#include "common.h"
#include "inverse_lists.h"

#define PB_TILE 512

// ball_query_kernel_fast (ball_query_gpu.cu:13-48): first `nsample` points with d2 < r2 in index order; the first hit fills every slot
__global__ __launch_bounds__(256) void k_ball_query_batch(int n, int m, float radius2, int nsample, const float* __restrict__ new_xyz,
                                                        const float* __restrict__ xyz, int32_t* __restrict__ idx) {
  __shared__ float buf[PB_TILE * 3];
  const int b = blockIdx.y, q = blockIdx.x * 256 + threadIdx.x;
  const bool live = q < m;
  const float* p = new_xyz + ((size_t)b * m + (live ? q : 0)) * 3;
  const float nx = p[0], ny = p[1], nz = p[2];
  int32_t* out = idx + ((size_t)b * m + (live ? q : 0)) * nsample;
  int cnt = live ? 0 : nsample;
  for (int k0 = 0; k0 < n; k0 += PB_TILE) {
    const int c = min(n - k0, PB_TILE);
    __syncthreads();
    for (int t = threadIdx.x; t < c * 3; t += 256) buf[t] = xyz[((size_t)b * n + k0) * 3 + t];
    __syncthreads();
    if (cnt >= nsample) continue;
    for (int k = 0; k < c; ++k) {
      const float dx = nx - buf[k * 3], dy = ny - buf[k * 3 + 1], dz = nz - buf[k * 3 + 2];
      const float d2 = dx * dx + dy * dy + dz * dz;
      if (d2 < radius2) {
        if (cnt == 0)
          for (int l = 0; l < nsample; ++l) out[l] = k0 + k;
        out[cnt] = k0 + k;
        if (++cnt >= nsample) break;
      }
    }
  }
}

// group_points_kernel_fast / gather_points_kernel_fast: out[b][c][j] = points[b][c][idx[b][j]]   (j over npoint*nsample)
__global__ __launch_bounds__(256) void k_gather_cn(int c, int n, int64_t per_batch, const float* __restrict__ points,
                                                 const int32_t* __restrict__ idx, float* __restrict__ out) {
  const int b = blockIdx.z, ch = blockIdx.y;
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= per_batch) return;
  out[((size_t)b * c + ch) * per_batch + j] = points[((size_t)b * c + ch) * n + idx[(size_t)b * per_batch + j]];
}

__global__ __launch_bounds__(256) void k_gather_cn_grad(int c, int n, int64_t per_batch, const float* __restrict__ grad_out,
                                                      const int32_t* __restrict__ idx, float* __restrict__ grad_points) {
  const int b = blockIdx.z, ch = blockIdx.y;
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= per_batch) return;
  atomicAdd(&grad_points[((size_t)b * c + ch) * n + idx[(size_t)b * per_batch + j]], grad_out[((size_t)b * c + ch) * per_batch + j]);
}

// three_nn_kernel_fast / three_nn_kernel_stack: squared distances in float, running bests in double (1e40), strict '<' cascade.
// `known` points of the query's batch element are [k_start, k_start + k_cnt); returned indices are k_start-relative + idx_base.
__device__ __forceinline__ void three_nn_scan(float ux, float uy, float uz, const float* __restrict__ known, int k_cnt, int idx_base,
                                              float* dist2, int32_t* idx) {
  double best1 = 1e40, best2 = 1e40, best3 = 1e40;
  int b1 = 0, b2 = 0, b3 = 0;
  for (int k = 0; k < k_cnt; ++k) {
    const float x = known[k * 3], y = known[k * 3 + 1], z = known[k * 3 + 2];
    const float d = (ux - x) * (ux - x) + (uy - y) * (uy - y) + (uz - z) * (uz - z);
    if (d < best1) {
      best3 = best2, b3 = b2;
      best2 = best1, b2 = b1;
      best1 = d, b1 = k;
    } else if (d < best2) {
      best3 = best2, b3 = b2;
      best2 = d, b2 = k;
    } else if (d < best3) {
      best3 = d, b3 = k;
    }
  }
  dist2[0] = (float)best1, dist2[1] = (float)best2, dist2[2] = (float)best3;
  idx[0] = b1 + idx_base, idx[1] = b2 + idx_base, idx[2] = b3 + idx_base;
}

__global__ __launch_bounds__(256) void k_three_nn_batch(int n, int m, const float* __restrict__ unknown, const float* __restrict__ known,
                                                      float* __restrict__ dist2, int32_t* __restrict__ idx) {
  const int b = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const float* u = unknown + ((size_t)b * n + p) * 3;
  three_nn_scan(u[0], u[1], u[2], known + (size_t)b * m * 3, m, 0, dist2 + ((size_t)b * n + p) * 3, idx + ((size_t)b * n + p) * 3);
}

// three_interpolate: batch layout points (B,C,M) -> out (B,C,N)
__global__ __launch_bounds__(256) void k_three_interp_batch(int c, int m, int n, const float* __restrict__ points, const int32_t* __restrict__ idx,
                                                          const float* __restrict__ w, float* __restrict__ out) {
  const int b = blockIdx.z, ch = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const int32_t* i3 = idx + ((size_t)b * n + p) * 3;
  const float* w3 = w + ((size_t)b * n + p) * 3;
  const float* src = points + ((size_t)b * c + ch) * m;
  out[((size_t)b * c + ch) * n + p] = w3[0] * src[i3[0]] + w3[1] * src[i3[1]] + w3[2] * src[i3[2]];
}

__global__ __launch_bounds__(256) void k_three_interp_grad_batch(int c, int n, int m, const float* __restrict__ grad_out,
                                                               const int32_t* __restrict__ idx, const float* __restrict__ w,
                                                               float* __restrict__ grad_points) {
  const int b = blockIdx.z, ch = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const int32_t* i3 = idx + ((size_t)b * n + p) * 3;
  const float* w3 = w + ((size_t)b * n + p) * 3;
  const float g = grad_out[((size_t)b * c + ch) * n + p];
  float* dst = grad_points + ((size_t)b * c + ch) * m;
  atomicAdd(&dst[i3[0]], g * w3[0]), atomicAdd(&dst[i3[1]], g * w3[1]), atomicAdd(&dst[i3[2]], g * w3[2]);
}

// ------------------------------------------------------------------------------------------------
// The two scatter gradients above with a fixed summation order and no float atomics (opt-in): inverse lists (inverse_lists.h) over the dense
// batch, then one gather.  Key k of the flat idx array belongs to batch element k / per and names row (k / per) * rows + idx[k]; an index
// outside [0, rows) names nothing -- it must not reach into the neighbouring batch element's rows.
//   grouping / gather:  per = npoints * nsample, rows = n      three-interpolate:  per = 3 * n (key 3 p + t), rows = m
// ------------------------------------------------------------------------------------------------
struct SvBatchRow {
  const int32_t* idx;
  int64_t per;
  int rows;
  __device__ __forceinline__ int64_t operator()(int64_t key) const {
    const int32_t i = idx[key];
    if (i < 0 || i >= rows) return -1;
    return (key / per) * rows + i;
  }
};

constexpr int BG_CT = 4;   // channels a thread keeps in registers: a key (and its weight) is read once per 4 channels

// grad_points[b][ch][i] = +0.0f + the terms of row i's keys, ascending; lanes along the destination rows (coalesced store, the layout is
// channel-major), each thread walks its own list for BG_CT channels.  WEIGHTED: term = fp32(grad_out[b][ch][p] * weight[key]), key = 3 p + t
// (+ b * per); else term = grad_out[b][ch][key - b * per].  The channels past c of the last tile read channel c - 1 again and store nothing.
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void k_batch_grad_gather(int c, int rows, int64_t per, const float* __restrict__ grad_out,
                                                         const float* __restrict__ weight, SvInvLists L, float* __restrict__ grad_points) {
  const int b = blockIdx.z, ch0 = blockIdx.y * BG_CT, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= rows) return;
  const int nch = min(BG_CT, c - ch0);
  const int64_t src_per = WEIGHTED ? per / 3 : per;                   // elements of one (b, ch) plane of grad_out
  const float* g = grad_out + ((size_t)b * c + ch0) * src_per;
  const int64_t key0 = (int64_t)b * per;
  size_t plane[BG_CT];
#pragma unroll
  for (int t = 0; t < BG_CT; ++t) plane[t] = (size_t)min(t, nch - 1) * src_per;
  int32_t cnt;
  const int32_t* keys = sv_inv_list(L, (int64_t)b * rows + i, cnt);
  float a[BG_CT];
#pragma unroll
  for (int t = 0; t < BG_CT; ++t) a[t] = 0.f;
  for (int32_t k = 0; k < cnt; ++k) {
    const int32_t key = keys[k];
    const int64_t local = key - key0;
    const int64_t j = WEIGHTED ? local / 3 : local;
    const float w = WEIGHTED ? weight[key] : 1.f;
#pragma unroll
    for (int t = 0; t < BG_CT; ++t) {
      const float v = g[plane[t] + j];
      a[t] = __fadd_rn(a[t], WEIGHTED ? __fmul_rn(v, w) : v);
    }
  }
  float* dst = grad_points + ((size_t)b * c + ch0) * rows + i;
#pragma unroll
  for (int t = 0; t < BG_CT; ++t)
    if (t < nch) dst[(size_t)t * rows] = a[t];
}

// keys = batch * per and rows_all = batch * rows, both below 2^31 (per alone is tested first: batch * per could leave int64)
static inline bool bg_fit(int batch, int64_t per, int rows) {
  const int64_t lim = (int64_t)1 << 31;
  return batch >= 0 && per >= 0 && rows >= 0 && per < lim && (int64_t)batch * per < lim && (int64_t)batch * rows < lim;
}

static int bg_ordered(const char* who, bool weighted, int batch, int c, int rows, int64_t per, const float* grad_out, const int32_t* idx,
                      const float* weight, void* scratch, float* grad_points, void* stream) {
  SV_CHECK_ARG(per >= 0, "%s: bad sizes", who);
  if (batch <= 0 || c <= 0 || rows <= 0) return SV_OK;
  SV_CHECK_ARG(bg_fit(batch, per, rows), "%s: the keys (%d * %lld) or the rows (%d * %d) exceed int32", who, batch, (long long)per, batch, rows);
  SV_CHECK_ARG(batch <= 65535 && sv_div_up(c, BG_CT) <= 65535, "%s: batch %d or c %d exceeds the launch grid", who, batch, c);
  SV_CHECK_ARG(grad_points && scratch && (per == 0 || (grad_out && idx && (weight || !weighted))), "%s: null pointer", who);
  hipStream_t st = sv_stream(stream);
  const int64_t nkeys = (int64_t)batch * per, nrows = (int64_t)batch * rows;
  const SvInvLists L = sv_inv_lists_view(scratch, nkeys, nrows);
  if (int rc = sv_inv_lists_build(nkeys, nrows, SvBatchRow{idx, per > 0 ? per : 1, rows}, L, st)) return rc;
  const dim3 grid(sv_div_up(rows, 256), sv_div_up(c, BG_CT), batch);
  if (weighted)
    hipLaunchKernelGGL(k_batch_grad_gather<true>, grid, dim3(256), 0, st, c, rows, per, grad_out, weight, L, grad_points);
  else
    hipLaunchKernelGGL(k_batch_grad_gather<false>, grid, dim3(256), 0, st, c, rows, per, grad_out, weight, L, grad_points);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_ball_query_batch(int batch, int n, int m, float radius, int nsample, const float* new_xyz, const float* xyz, int32_t* idx,
                                   void* stream) {
  SV_CHECK_ARG(batch >= 0 && n >= 0 && m >= 0 && nsample >= 1, "sv_ball_query_batch: bad sizes");
  if (batch == 0 || m == 0) return SV_OK;
  SV_CHECK_ARG(new_xyz && idx && (xyz || n == 0), "sv_ball_query_batch: null pointer");
  hipLaunchKernelGGL(k_ball_query_batch, dim3(sv_div_up(m, 256), batch), dim3(256), 0, sv_stream(stream), n, m, radius * radius, nsample,
                     new_xyz, xyz, idx);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_group_points_batch(int batch, int c, int n, int npoints, int nsample, const float* points, const int32_t* idx, float* out,
                                     void* stream) {
  const int64_t per = (int64_t)npoints * nsample;
  if (batch <= 0 || c <= 0 || per <= 0) return SV_OK;
  SV_CHECK_ARG(points && idx && out, "sv_group_points_batch: null pointer");
  hipLaunchKernelGGL(k_gather_cn, dim3(sv_div_up(per, 256), c, batch), dim3(256), 0, sv_stream(stream), c, n, per, points, idx, out);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_group_points_grad_batch(int batch, int c, int n, int npoints, int nsample, const float* grad_out, const int32_t* idx,
                                          float* grad_points, void* stream) {
  const int64_t per = (int64_t)npoints * nsample;
  if (batch <= 0 || c <= 0 || n <= 0) return SV_OK;
  SV_CHECK_ARG(grad_points && (per == 0 || (grad_out && idx)), "sv_group_points_grad_batch: null pointer");
  SV_HIP(hipMemsetAsync(grad_points, 0, (size_t)batch * c * n * sizeof(float), sv_stream(stream)));
  if (per == 0) return SV_OK;
  hipLaunchKernelGGL(k_gather_cn_grad, dim3(sv_div_up(per, 256), c, batch), dim3(256), 0, sv_stream(stream), c, n, per, grad_out, idx,
                     grad_points);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_gather_points_batch(int batch, int c, int n, int npoints, const float* points, const int32_t* idx, float* out,
                                      void* stream) {
  return sv_group_points_batch(batch, c, n, npoints, 1, points, idx, out, stream);
}

extern "C" int sv_gather_points_grad_batch(int batch, int c, int n, int npoints, const float* grad_out, const int32_t* idx,
                                           float* grad_points, void* stream) {
  return sv_group_points_grad_batch(batch, c, n, npoints, 1, grad_out, idx, grad_points, stream);
}

extern "C" size_t sv_group_points_grad_batch_ordered_scratch_bytes(int batch, int n, int npoints, int nsample) {
  const int64_t per = (int64_t)npoints * nsample;
  if (npoints < 0 || nsample < 0 || !bg_fit(batch, per, n)) return 0;
  return sv_inv_lists_bytes((int64_t)batch * per, (int64_t)batch * n);
}

extern "C" int sv_group_points_grad_batch_ordered(int batch, int c, int n, int npoints, int nsample, const float* grad_out, const int32_t* idx,
                                                  void* scratch, float* grad_points, void* stream) {
  SV_CHECK_ARG(npoints >= 0 && nsample >= 0, "sv_group_points_grad_batch_ordered: bad sizes");
  return bg_ordered("sv_group_points_grad_batch_ordered", false, batch, c, n, (int64_t)npoints * nsample, grad_out, idx, nullptr, scratch,
                    grad_points, stream);
}

extern "C" size_t sv_gather_points_grad_batch_ordered_scratch_bytes(int batch, int n, int npoints) {
  return sv_group_points_grad_batch_ordered_scratch_bytes(batch, n, npoints, 1);
}

extern "C" int sv_gather_points_grad_batch_ordered(int batch, int c, int n, int npoints, const float* grad_out, const int32_t* idx,
                                                   void* scratch, float* grad_points, void* stream) {
  return sv_group_points_grad_batch_ordered(batch, c, n, npoints, 1, grad_out, idx, scratch, grad_points, stream);
}

extern "C" int sv_three_nn_batch(int batch, int n, int m, const float* unknown, const float* known, float* dist2, int32_t* idx,
                                 void* stream) {
  if (batch <= 0 || n <= 0) return SV_OK;
  SV_CHECK_ARG(unknown && dist2 && idx && (known || m == 0), "sv_three_nn_batch: null pointer");
  hipLaunchKernelGGL(k_three_nn_batch, dim3(sv_div_up(n, 256), batch), dim3(256), 0, sv_stream(stream), n, m, unknown, known, dist2, idx);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_three_interpolate_batch(int batch, int c, int m, int n, const float* points, const int32_t* idx, const float* weight,
                                          float* out, void* stream) {
  if (batch <= 0 || c <= 0 || n <= 0) return SV_OK;
  SV_CHECK_ARG(points && idx && weight && out, "sv_three_interpolate_batch: null pointer");
  hipLaunchKernelGGL(k_three_interp_batch, dim3(sv_div_up(n, 256), c, batch), dim3(256), 0, sv_stream(stream), c, m, n, points, idx, weight,
                     out);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_three_interpolate_grad_batch(int batch, int c, int n, int m, const float* grad_out, const int32_t* idx,
                                               const float* weight, float* grad_points, void* stream) {
  if (batch <= 0 || c <= 0 || m <= 0) return SV_OK;
  SV_CHECK_ARG(grad_points && (n == 0 || (grad_out && idx && weight)), "sv_three_interpolate_grad_batch: null pointer");
  SV_HIP(hipMemsetAsync(grad_points, 0, (size_t)batch * c * m * sizeof(float), sv_stream(stream)));
  if (n <= 0) return SV_OK;
  hipLaunchKernelGGL(k_three_interp_grad_batch, dim3(sv_div_up(n, 256), c, batch), dim3(256), 0, sv_stream(stream), c, n, m, grad_out, idx,
                     weight, grad_points);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" size_t sv_three_interpolate_grad_batch_ordered_scratch_bytes(int batch, int n, int m) {
  if (n < 0 || !bg_fit(batch, (int64_t)n * 3, m)) return 0;
  return sv_inv_lists_bytes((int64_t)batch * n * 3, (int64_t)batch * m);
}

extern "C" int sv_three_interpolate_grad_batch_ordered(int batch, int c, int n, int m, const float* grad_out, const int32_t* idx,
                                                       const float* weight, void* scratch, float* grad_points, void* stream) {
  SV_CHECK_ARG(n >= 0, "sv_three_interpolate_grad_batch_ordered: bad sizes");
  return bg_ordered("sv_three_interpolate_grad_batch_ordered", true, batch, c, m, (int64_t)n * 3, grad_out, idx, weight, scratch, grad_points,
                    stream);
}
