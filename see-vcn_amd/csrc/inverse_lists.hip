// Inverse lists: the kernels that do not depend on how a key finds its row -- see inverse_lists.h.
#include "inverse_lists.h"
#include "wave.h"

// seg[row] = start of a segment of cnt[row] keys.  The segments need not lie in row order (nothing reads across them), so a workgroup sums its
// 1024 rows and takes its range with ONE integer atomic instead of a device-wide scan.
__global__ __launch_bounds__(256) void k_inv_segments(int64_t N, SvInvLists L) {
  __shared__ int32_t wave_sum[4];
  __shared__ int32_t block_base;
  const int64_t p0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  int32_t c[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) c[j] = p0 + j < N ? L.cnt[p0 + j] : 0;
  int32_t all;
  const int32_t before = sv_block_excl_scan<256>(c[0] + c[1] + c[2] + c[3], &all, wave_sum);
  if (threadIdx.x == 0) block_base = all ? atomicAdd(L.total, all) : 0;
  __syncthreads();
  int32_t at = block_base + before;
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

void sv_inv_lists_launch_segments(int64_t nrows, const SvInvLists& L, hipStream_t st) {
  hipLaunchKernelGGL(k_inv_segments, dim3((unsigned)((nrows + 1023) / 1024)), dim3(256), 0, st, nrows, L);
}

void sv_inv_lists_launch_sort(int64_t nrows, const SvInvLists& L, hipStream_t st) {
  hipLaunchKernelGGL(k_inv_sort, dim3(sv_grid_1d(nrows * 64, 256, 256 * 16)), dim3(256), 0, st, nrows, L);
}
