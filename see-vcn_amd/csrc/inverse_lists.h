// Inverse lists: for every row n the keys that name it, each row's keys in ASCENDING order.  The order-fixed gradients walk these lists instead
// of scattering with float atomics: sv_group_points_grad_stack_ordered and sv_sa_train_backward_ordered (key m * nsample + s names support row
// row_start[m] + idx[m][s]) and sv_bev_interpolate_grad_nhwc (key 4 * m + t names the pixel of tap t of keypoint m).  Count with integer atomics,
// one atomic per workgroup to place the segments, fill in arrival order; then every segment is sorted, so nothing a reader sees depends on the
// arrival order.
#pragma once
#include "common.h"

struct SvInvLists {
  int32_t* total;   // 1 word (+3 of padding): the segment allocator
  int32_t* cnt;     // (N) keys per row
  int32_t* seg;     // (N) END of the row's segment (the fill advances it from the start)
  int32_t* raw;     // (K) keys in arrival order
  int32_t* keys;    // (K) keys, every segment ascending
};

// layout: total (16 bytes) | cnt (N int32) | seg (N int32) | raw (K int32) | keys (K int32), K = the number of keys
static inline size_t sv_inv_lists_bytes(int64_t nkeys, int64_t nrows) { return 16 + ((size_t)nrows * 2 + (size_t)nkeys * 2) * sizeof(int32_t); }

static inline SvInvLists sv_inv_lists_view(void* scratch, int64_t nkeys, int64_t nrows) {
  SvInvLists L;
  L.total = reinterpret_cast<int32_t*>(scratch);
  L.cnt = L.total + 4;
  L.seg = L.cnt + nrows;
  L.raw = L.seg + nrows;
  L.keys = L.raw + nkeys;
  return L;
}

static inline bool sv_inv_lists_fit(int64_t M, int nsample, int64_t N) {
  return M >= 0 && N >= 0 && nsample > 0 && M * (int64_t)nsample < ((int64_t)1 << 31) && N < ((int64_t)1 << 31);
}

// The two kernels that do not depend on how a key finds its row, behind launch functions (inverse_lists.hip): the segments of the counted rows,
// and keys[] = every segment of raw[] sorted.
void sv_inv_lists_launch_segments(int64_t nrows, const SvInvLists& L, hipStream_t st);
void sv_inv_lists_launch_sort(int64_t nrows, const SvInvLists& L, hipStream_t st);

#ifdef __HIPCC__
// FILL == 0: cnt[row] += 1 per key.  FILL == 1: raw[seg[row]++] = key.  row_of(key): the key's row, negative to skip the key.
template <int FILL, class RowOf>
__global__ __launch_bounds__(256) void k_inv_keys(int64_t nkeys, int64_t nrows, RowOf row_of, SvInvLists L) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nkeys; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = row_of(e);
    if (row < 0 || row >= nrows) continue;
    if (FILL) L.raw[atomicAdd(&L.seg[row], 1)] = (int32_t)e;
    else atomicAdd(&L.cnt[row], 1);
  }
}

// The lists of the keys 0 .. nkeys - 1 over nrows rows; the caller has checked that both fit int32.  Four launches and one memset on st.
template <class RowOf>
int sv_inv_lists_build(int64_t nkeys, int64_t nrows, RowOf row_of, const SvInvLists& L, hipStream_t st) {
  if (nrows == 0) return SV_OK;
  SV_HIP(hipMemsetAsync(L.total, 0, 16 + (size_t)nrows * 4, st));      // the allocator and the counts
  if (nkeys > 0) {
    const dim3 key_grid(sv_grid_1d(nkeys, 256));
    hipLaunchKernelGGL((k_inv_keys<0, RowOf>), key_grid, dim3(256), 0, st, nkeys, nrows, row_of, L);
    sv_inv_lists_launch_segments(nrows, L, st);
    hipLaunchKernelGGL((k_inv_keys<1, RowOf>), key_grid, dim3(256), 0, st, nkeys, nrows, row_of, L);
    sv_inv_lists_launch_sort(nrows, L, st);
  } else {
    SV_HIP(hipMemsetAsync(L.seg, 0, (size_t)nrows * 4, st));
  }
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// Key m * nsample + s names support row row_start[m] + idx[m][s]; it counts when its idx is not negative and -- skip_empty_balls -- its ball is
// not marked empty (idx[m][0] < 0).
struct SvBallRow {
  const int32_t* idx;
  const int32_t* row_start;
  int nsample;
  bool skip_empty_balls;
  __device__ __forceinline__ int64_t operator()(int64_t key) const {
    const int64_t m = key / nsample;
    const int32_t j = idx[key];
    if (j < 0 || (skip_empty_balls && idx[m * nsample] < 0)) return -1;
    return (int64_t)row_start[m] + j;
  }
};

// the ascending keys of row n
__device__ __forceinline__ const int32_t* sv_inv_list(const SvInvLists& L, int64_t n, int32_t& count) {
  count = L.cnt[n];
  return L.keys + (L.seg[n] - count);
}
#endif
