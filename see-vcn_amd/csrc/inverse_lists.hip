// Inverse neighbour lists of an (idx, row_start) pair -- see inverse_lists.h.
#include "inverse_lists.h"

// FILL == 0: cnt[row] += 1 per key.  FILL == 1: raw[seg[row]++] = key.
template <int FILL>
__global__ __launch_bounds__(256) void k_inv_keys(const int32_t* __restrict__ idx, const int32_t* __restrict__ row_start, int64_t nkeys, int nsample,
                                                  int64_t N, int skip_empty_balls, SvInvLists L) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nkeys; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t m = e / nsample;
    const int32_t j = idx[e];
    if (j < 0 || (skip_empty_balls && idx[m * nsample] < 0)) continue;
    const int64_t row = (int64_t)row_start[m] + j;
    if (row < 0 || row >= N) continue;
    if (FILL) L.raw[atomicAdd(&L.seg[row], 1)] = (int32_t)e;
    else atomicAdd(&L.cnt[row], 1);
  }
}

// seg[row] = start of a segment of cnt[row] keys.  The segments need not lie in row order (nothing reads across them), so a workgroup sums its
// 1024 rows and takes its range with ONE integer atomic instead of a device-wide scan.
__global__ __launch_bounds__(256) void k_inv_segments(int64_t N, SvInvLists L) {
  __shared__ int32_t wave_sum[4];
  __shared__ int32_t block_base;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t p0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  int32_t c[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) c[j] = p0 + j < N ? L.cnt[p0 + j] : 0;
  const int32_t mine = c[0] + c[1] + c[2] + c[3];
  int32_t incl = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int32_t up = __shfl_up(incl, d);
    if (lane >= d) incl += up;
  }
  if (lane == 63) wave_sum[wave] = incl;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int32_t all = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
    block_base = all ? atomicAdd(L.total, all) : 0;
  }
  __syncthreads();
  int32_t at = block_base + incl - mine;
  for (int w = 0; w < wave; ++w) at += wave_sum[w];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (p0 + j < N) L.seg[p0 + j] = at;
    at += c[j];
  }
}

// One wave per row: keys[rank of a key among the row's keys] = key.  The keys of a row are distinct, so the ranks are a permutation; a list of
// c keys costs c * ceil(c / 64) reads a lane.
__global__ __launch_bounds__(256) void k_inv_sort(int64_t N, SvInvLists L) {
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t n = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); n < N; n += nwaves) {
    const int32_t c = L.cnt[n];
    const int64_t s0 = L.seg[n] - c;
    const int32_t* in = L.raw + s0;
    int32_t* out = L.keys + s0;
    for (int32_t i = lane; i < c; i += 64) {
      const int32_t k = in[i];
      int32_t rank = 0;
      for (int32_t j = 0; j < c; ++j) rank += in[j] < k;
      out[rank] = k;
    }
  }
}

int sv_inv_lists_build(const int32_t* idx, const int32_t* row_start, int64_t M, int nsample, int64_t N, bool skip_empty_balls, const SvInvLists& L,
                       hipStream_t st) {
  if (N == 0) return SV_OK;
  SV_HIP(hipMemsetAsync(L.total, 0, 16 + (size_t)N * 4, st));          // the allocator and the counts
  const int64_t nkeys = M * nsample;
  if (nkeys > 0) {
    const dim3 key_grid(sv_grid_1d(nkeys, 256));
    hipLaunchKernelGGL(k_inv_keys<0>, key_grid, dim3(256), 0, st, idx, row_start, nkeys, nsample, N, (int)skip_empty_balls, L);
    hipLaunchKernelGGL(k_inv_segments, dim3((unsigned)((N + 1023) / 1024)), dim3(256), 0, st, N, L);
    hipLaunchKernelGGL(k_inv_keys<1>, key_grid, dim3(256), 0, st, idx, row_start, nkeys, nsample, N, (int)skip_empty_balls, L);
    hipLaunchKernelGGL(k_inv_sort, dim3(sv_grid_1d(N * 64, 256, 256 * 16)), dim3(256), 0, st, N, L);
  } else {
    SV_HIP(hipMemsetAsync(L.seg, 0, (size_t)N * 4, st));
  }
  SV_LAUNCH_CHECK();
  return SV_OK;
}
