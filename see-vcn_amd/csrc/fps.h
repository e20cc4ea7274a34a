// What the farthest-point-sampling kernels share (pointnet2.hip, spc_sampling.hip): the workgroup shape and the key that orders candidates.
#pragma once
#include "common.h"

#ifdef __HIPCC__
constexpr int FPS_THREADS = 512;   // 8 waves = 2 per SIMD: 256 VGPRs per lane, so 48 points per thread stay in registers (1024 threads
                                   // capped the kernel at 128 VGPRs: the 16- and 24-point variants spilled ~700 / ~2500 registers to scratch
                                   // and a round took 39 us instead of ~2)
constexpr int FPS_MAXP = 48;       // points per thread held in registers -> n <= 24576 on the register path

__device__ __forceinline__ unsigned long long fps_key(float d, int k, int log2t) {
  // larger key wins: distance first (non-negative floats order as their bit patterns), then the tie rule
  const unsigned int lo = (unsigned int)k & ((1u << log2t) - 1u);
  const unsigned int rev = log2t ? (__brev(lo) >> (32 - log2t)) : 0u;
  const unsigned int tie = (rev << (31 - log2t)) | ((unsigned int)k >> log2t);   // smaller tie = preferred
  return ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)(0x7FFFFFFFu - tie);
}

// the point index a key was made from
__device__ __forceinline__ int fps_key_index(unsigned long long key, int log2t) {
  const unsigned int tie = 0x7FFFFFFFu - (unsigned int)(key & 0xFFFFFFFFull);
  const unsigned int rev = log2t ? (tie >> (31 - log2t)) : 0u;
  const unsigned int lo = log2t ? (__brev(rev) >> (32 - log2t)) : 0u;
  return (int)(((tie & ((1u << (31 - log2t)) - 1u)) << log2t) | lo);
}
#endif
