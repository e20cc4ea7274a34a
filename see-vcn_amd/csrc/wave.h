// Wave- and workgroup-level scan and reduce helpers (device only, 64-lane waves).  Integer results are exact; the float sum adds in the butterfly's fixed order.
#pragma once
#include "common.h"

#ifdef __HIPCC__
// Inclusive scan over every aligned group of WIDTH lanes.  T: int, int32_t, unsigned.
template <int WIDTH = SV_WAVE, class T>
__device__ __forceinline__ T sv_wave_incl_scan(T v) {
  const int lane = threadIdx.x & (WIDTH - 1);
#pragma unroll
  for (int d = 1; d < WIDTH; d <<= 1) {
    const T t = __shfl_up(v, d, WIDTH);
    if (lane >= d) v += t;
  }
  return v;
}

// Exclusive scan of one value per thread over a 1-D workgroup of THREADS; *total = the sum.  wave_sums: THREADS / 64 words of LDS from the caller.
// ONE barrier, between writing the wave totals and reading them: a caller that uses wave_sums again puts a barrier in between.
template <int THREADS, class T>
__device__ __forceinline__ T sv_block_excl_scan(T v, T* total, T* wave_sums) {
  const int lane = threadIdx.x & (SV_WAVE - 1), wid = threadIdx.x / SV_WAVE;
  const T incl = sv_wave_incl_scan(v);
  if (lane == SV_WAVE - 1) wave_sums[wid] = incl;
  __syncthreads();
  T base = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < THREADS / SV_WAVE; ++i) {
    const T s = wave_sums[i];
    if (i < wid) base += s;
    tot += s;
  }
  *total = tot;
  return base + incl - v;
}

// Exclusive scan of in[0 .. n) into out by ONE 1-D workgroup of THREADS, in tiles of THREADS with the carry in a register; returns the grand total
// in every thread.  in == out is allowed: a thread reads only the elements it writes.  Every thread of the workgroup takes every round; each round
// ends with a barrier, so wave_sums (THREADS / 64 words of LDS) is free again afterwards and out is visible to the whole workgroup.
template <int THREADS, class T>
__device__ __forceinline__ T sv_block_excl_scan_array(const T* in, T* out, int64_t n, T* wave_sums) {
  T carry = 0;
  for (int64_t base = 0; base < n; base += THREADS) {
    const int64_t k = base + threadIdx.x;
    const T v = k < n ? in[k] : 0;
    T total;
    const T ex = sv_block_excl_scan<THREADS>(v, &total, wave_sums);
    if (k < n) out[k] = carry + ex;
    carry += total;
    __syncthreads();
  }
  return carry;
}

// Exclusive scan of one flag per lane through a ballot: the number of set flags in the lanes below this one; *total = set flags in the wave (the
// same in every lane).  sv_wave_ballot_first: the lowest lane whose flag is set (-1: none).  Every lane of the wave must be active.
__device__ __forceinline__ int sv_wave_ballot_rank(bool flag, int* total) {
  const unsigned long long m = __ballot(flag);
  *total = __popcll(m);
  return __popcll(m & ((1ull << (threadIdx.x & (SV_WAVE - 1))) - 1ull));
}
__device__ __forceinline__ int sv_wave_ballot_first(bool flag) { return __ffsll((long long)__ballot(flag)) - 1; }

// A float's bits as an unsigned integer that orders as the float does (negative values inverted, the others with the sign bit set), and back:
// what integer atomicMin / atomicMax need to reduce floats without depending on the order.
__device__ __forceinline__ uint32_t sv_ordered_f32(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sv_unordered_f32(uint32_t e) { return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e); }

// One xor butterfly over the wave's 64 lanes, d = 32 -> 1; every lane gets the result.  A 64-bit value travels as two 32-bit halves.
__device__ __forceinline__ unsigned long long sv_shfl_xor(unsigned long long v, int d) {
  const unsigned lo = __shfl_xor((unsigned)v, d, SV_WAVE), hi = __shfl_xor((unsigned)(v >> 32), d, SV_WAVE);
  return ((unsigned long long)hi << 32) | lo;
}
template <class T>
__device__ __forceinline__ T sv_shfl_xor(T v, int d) { return __shfl_xor(v, d, SV_WAVE); }

template <class T, class Op>
__device__ __forceinline__ T sv_wave_reduce(T v, Op op) {
#pragma unroll
  for (int d = SV_WAVE / 2; d >= 1; d >>= 1) v = op(v, sv_shfl_xor(v, d));
  return v;
}

__device__ __forceinline__ float sv_min2(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ float sv_max2(float a, float b) { return fmaxf(a, b); }
template <class T> __device__ __forceinline__ T sv_min2(T a, T b) { return b < a ? b : a; }
template <class T> __device__ __forceinline__ T sv_max2(T a, T b) { return a < b ? b : a; }

template <class T> __device__ __forceinline__ T sv_wave_reduce_sum(T v) { return sv_wave_reduce(v, [](T a, T b) { return a + b; }); }
template <class T> __device__ __forceinline__ T sv_wave_reduce_min(T v) { return sv_wave_reduce(v, [](T a, T b) { return sv_min2(a, b); }); }
template <class T> __device__ __forceinline__ T sv_wave_reduce_max(T v) { return sv_wave_reduce(v, [](T a, T b) { return sv_max2(a, b); }); }
template <class T> __device__ __forceinline__ T sv_wave_reduce_and(T v) { return sv_wave_reduce(v, [](T a, T b) { return a & b; }); }
template <class T> __device__ __forceinline__ T sv_wave_reduce_or(T v) { return sv_wave_reduce(v, [](T a, T b) { return a | b; }); }
#endif
