// Chamfer distance (nearest neighbour both ways + its gradient): the `chamfer` extension of the reference's VCN training loss
// (see/surface_completion/models/vcn/extensions/chamfer_dist/chamfer.cu:15-201, bound at chamfer_cuda.cpp:36-39).
// dist[b][j] = min_k |xyz1[b][j] - xyz2[b][k]|^2 (fp32, (dx*dx + dy*dy) + dz*dz), idx = first k attaining it.
#include "common.h"

#define CH_TILE 512

__global__ __launch_bounds__(256) void k_chamfer_nn(const float* __restrict__ xyz1, int n, const float* __restrict__ xyz2, int m,
                                                  float* __restrict__ dist, int32_t* __restrict__ idx) {
  __shared__ float buf[CH_TILE * 3];
  const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
  const bool live = j < n;
  const float* p = xyz1 + ((size_t)b * n + (live ? j : 0)) * 3;
  const float x1 = p[0], y1 = p[1], z1 = p[2];
  float best = 0.f;
  int best_k = 0;
  for (int k2 = 0; k2 < m; k2 += CH_TILE) {
    const int cnt = min(m - k2, CH_TILE);
    __syncthreads();
    for (int t = threadIdx.x; t < cnt * 3; t += 256) buf[t] = xyz2[((size_t)b * m + k2) * 3 + t];
    __syncthreads();
    for (int k = 0; k < cnt; ++k) {
      const float x2 = buf[k * 3] - x1, y2 = buf[k * 3 + 1] - y1, z2 = buf[k * 3 + 2] - z1;
      const float d = x2 * x2 + y2 * y2 + z2 * z2;
      if ((k2 == 0 && k == 0) || d < best) best = d, best_k = k2 + k;      // strict <: the first minimum wins, as in the reference
    }
  }
  if (live) dist[(size_t)b * n + j] = best, idx[(size_t)b * n + j] = best_k;
}

// grad_xyz1[j] += 2 g (p1 - p2[idx]),  grad_xyz2[idx] -= 2 g (p1 - p2[idx])   (chamfer.cu:134-166; float atomics like the reference)
__global__ __launch_bounds__(256) void k_chamfer_grad(const float* __restrict__ xyz1, int n, const float* __restrict__ xyz2, int m,
                                                    const float* __restrict__ grad_dist, const int32_t* __restrict__ idx,
                                                    float* __restrict__ grad1, float* __restrict__ grad2) {
  const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const size_t a = ((size_t)b * n + j) * 3;
  const int j2 = idx[(size_t)b * n + j];
  const size_t c = ((size_t)b * m + j2) * 3;
  const float g = grad_dist[(size_t)b * n + j] * 2;
  const float gx = g * (xyz1[a] - xyz2[c]), gy = g * (xyz1[a + 1] - xyz2[c + 1]), gz = g * (xyz1[a + 2] - xyz2[c + 2]);
  atomicAdd(&grad1[a], gx), atomicAdd(&grad1[a + 1], gy), atomicAdd(&grad1[a + 2], gz);
  atomicAdd(&grad2[c], -gx), atomicAdd(&grad2[c + 1], -gy), atomicAdd(&grad2[c + 2], -gz);
}

extern "C" int sv_chamfer_forward(const float* xyz1, const float* xyz2, int batch, int n, int m, float* dist1, float* dist2,
                                  int32_t* idx1, int32_t* idx2, void* stream) {
  SV_CHECK_ARG(batch >= 0 && n >= 1 && m >= 1, "sv_chamfer_forward: bad sizes (batch %d, n %d, m %d)", batch, n, m);
  if (batch == 0) return SV_OK;
  SV_CHECK_ARG(xyz1 && xyz2 && dist1 && dist2 && idx1 && idx2, "sv_chamfer_forward: null pointer");
  hipStream_t st = sv_stream(stream);
  hipLaunchKernelGGL(k_chamfer_nn, dim3(sv_div_up(n, 256), batch), dim3(256), 0, st, xyz1, n, xyz2, m, dist1, idx1);
  hipLaunchKernelGGL(k_chamfer_nn, dim3(sv_div_up(m, 256), batch), dim3(256), 0, st, xyz2, m, xyz1, n, dist2, idx2);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_chamfer_backward(const float* xyz1, const float* xyz2, const int32_t* idx1, const int32_t* idx2,
                                   const float* grad_dist1, const float* grad_dist2, int batch, int n, int m, float* grad_xyz1,
                                   float* grad_xyz2, void* stream) {
  SV_CHECK_ARG(batch >= 0 && n >= 1 && m >= 1, "sv_chamfer_backward: bad sizes");
  if (batch == 0) return SV_OK;
  SV_CHECK_ARG(xyz1 && xyz2 && idx1 && idx2 && grad_dist1 && grad_dist2 && grad_xyz1 && grad_xyz2, "sv_chamfer_backward: null pointer");
  hipStream_t st = sv_stream(stream);
  SV_HIP(hipMemsetAsync(grad_xyz1, 0, (size_t)batch * n * 3 * sizeof(float), st));
  SV_HIP(hipMemsetAsync(grad_xyz2, 0, (size_t)batch * m * 3 * sizeof(float), st));
  hipLaunchKernelGGL(k_chamfer_grad, dim3(sv_div_up(n, 256), batch), dim3(256), 0, st, xyz1, n, xyz2, m, grad_dist1, idx1, grad_xyz1,
                     grad_xyz2);
  hipLaunchKernelGGL(k_chamfer_grad, dim3(sv_div_up(m, 256), batch), dim3(256), 0, st, xyz2, m, xyz1, n, grad_dist2, idx2, grad_xyz2,
                     grad_xyz1);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// The same gradient with a fixed summation order and no float atomics: every output element is written once.  For point (b, i) of cloud A and
// coordinate d:   +0.0f + (2 g_a[i]) * (A[i][d] - B[idx_a[i]][d])            the point's own term (k_chamfer_grad's gx)
//                       + -((2 g_b[k]) * (B[k][d] - A[i][d]))                for every k of cloud B with idx_b[k] == i, in ascending k (its -gx),
// every product and sum rounded to fp32.  The hits are found by a scan of cloud B's idx through LDS in tiles, like k_chamfer_nn's scan of its
// coordinates: a thread per point of A, no lists, no scratch.
__global__ __launch_bounds__(256) void k_chamfer_grad_ordered(const float* __restrict__ pa, int n, const float* __restrict__ pb, int m,
                                                            const float* __restrict__ ga, const int32_t* __restrict__ ia,
                                                            const float* __restrict__ gb, const int32_t* __restrict__ ib, float* __restrict__ grad_a) {
  __shared__ float s_p[CH_TILE * 3];
  __shared__ float s_g[CH_TILE];
  __shared__ int32_t s_i[CH_TILE];
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  const bool live = i < n;
  const size_t a = ((size_t)b * n + (live ? i : 0)) * 3;
  const float x = pa[a], y = pa[a + 1], z = pa[a + 2];
  float ax = 0.f, ay = 0.f, az = 0.f;
  if (live) {
    const size_t c = ((size_t)b * m + ia[(size_t)b * n + i]) * 3;
    const float g = ga[(size_t)b * n + i] * 2;
    ax = ax + g * (x - pb[c]), ay = ay + g * (y - pb[c + 1]), az = az + g * (z - pb[c + 2]);
  }
  for (int k2 = 0; k2 < m; k2 += CH_TILE) {
    const int cnt = min(m - k2, CH_TILE);
    __syncthreads();
    for (int t = threadIdx.x; t < cnt * 3; t += 256) s_p[t] = pb[((size_t)b * m + k2) * 3 + t];
    for (int t = threadIdx.x; t < cnt; t += 256) s_g[t] = gb[(size_t)b * m + k2 + t], s_i[t] = ib[(size_t)b * m + k2 + t];
    __syncthreads();
    for (int k = 0; k < cnt; ++k) {
      if (s_i[k] != i) continue;
      const float g = s_g[k] * 2;
      ax = ax + -(g * (s_p[k * 3] - x)), ay = ay + -(g * (s_p[k * 3 + 1] - y)), az = az + -(g * (s_p[k * 3 + 2] - z));
    }
  }
  if (live) grad_a[a] = ax, grad_a[a + 1] = ay, grad_a[a + 2] = az;
}

extern "C" size_t sv_chamfer_backward_ordered_scratch_bytes(int batch, int n, int m) {
  (void)batch, (void)n, (void)m;
  return 0;                                                            // the hits are found by a scan: no lists
}

extern "C" int sv_chamfer_backward_ordered(const float* xyz1, const float* xyz2, const int32_t* idx1, const int32_t* idx2, const float* grad_dist1,
                                           const float* grad_dist2, int batch, int n, int m, void* scratch, float* grad_xyz1, float* grad_xyz2,
                                           void* stream) {
  (void)scratch;
  SV_CHECK_ARG(batch >= 0 && n >= 1 && m >= 1, "sv_chamfer_backward_ordered: bad sizes");
  SV_CHECK_ARG(batch <= 65535, "sv_chamfer_backward_ordered: at most 65535 objects a call (got %d)", batch);
  if (batch == 0) return SV_OK;
  SV_CHECK_ARG(xyz1 && xyz2 && idx1 && idx2 && grad_dist1 && grad_dist2 && grad_xyz1 && grad_xyz2, "sv_chamfer_backward_ordered: null pointer");
  hipStream_t st = sv_stream(stream);
  hipLaunchKernelGGL(k_chamfer_grad_ordered, dim3(sv_div_up(n, 256), batch), dim3(256), 0, st, xyz1, n, xyz2, m, grad_dist1, idx1, grad_dist2, idx2,
                     grad_xyz1);
  hipLaunchKernelGGL(k_chamfer_grad_ordered, dim3(sv_div_up(m, 256), batch), dim3(256), 0, st, xyz2, m, xyz1, n, grad_dist2, idx2, grad_dist1, idx1,
                     grad_xyz2);
  SV_LAUNCH_CHECK();
  return SV_OK;
}
