// Inverse neighbour lists: for every support row n the keys  m * nsample + s  of the (query, slot) pairs that name it
// (row_start[m] + idx[m][s] == n), each row's keys in ASCENDING order.  The order-fixed gradients (sv_group_points_grad_stack_ordered,
// sv_sa_train_backward_ordered) walk these lists instead of scattering with float atomics.  Same method as BevLists in head.hip: count with
// integer atomics, one atomic per workgroup to place the segments, fill in arrival order; then every segment is sorted, so nothing a reader
// sees depends on the arrival order.
#pragma once
#include "common.h"

struct SvInvLists {
  int32_t* total;   // 1 word (+3 of padding): the segment allocator
  int32_t* cnt;     // (N) keys per row
  int32_t* seg;     // (N) END of the row's segment (the fill advances it from the start)
  int32_t* raw;     // (K) keys in arrival order
  int32_t* keys;    // (K) keys, every segment ascending
};

// layout: total (16 bytes) | cnt (N int32) | seg (N int32) | raw (K int32) | keys (K int32), K = M * nsample
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

// A key counts when its idx is not negative, its row lies in [0, N) and -- skip_empty_balls -- its ball is not marked empty (idx[m][0] < 0).
// The caller has checked sv_inv_lists_fit.  Four launches and one memset on st; implemented in inverse_lists.hip.
int sv_inv_lists_build(const int32_t* idx, const int32_t* row_start, int64_t M, int nsample, int64_t N, bool skip_empty_balls, const SvInvLists& L,
                       hipStream_t st);

#ifdef __HIPCC__
// the ascending keys of row n
__device__ __forceinline__ const int32_t* sv_inv_list(const SvInvLists& L, int64_t n, int32_t& count) {
  count = L.cnt[n];
  return L.keys + (L.seg[n] - count);
}
#endif
