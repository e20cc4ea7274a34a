// What the exhaustive farthest-point-sampling kernels share (fps.hip): the workgroup shape, the key that orders candidates, and the sampling
// round -- per-thread scan, wave-winner publication, and the round loops of the register and the HBM-temp form.
// The distance expression, the fminf running minimum, the tie rule and the parity slots below are the index-exactness contract with the
// reference (sampling_gpu.cu:55-134, :188-319); they are stated here once.
#pragma once
#include "common.h"
#include "wave.h"

#ifdef __HIPCC__
constexpr int FPS_THREADS = 512;   // 8 waves = 2 per SIMD: 256 VGPRs per lane, so 48 points per thread stay in registers (1024 threads
                                   // capped the kernel at 128 VGPRs: the 16- and 24-point variants spilled ~700 / ~2500 registers to scratch
                                   // and a round took 39 us instead of ~2)
constexpr int FPS_MAXP = 48;       // points per thread held in registers -> n <= 24576 on the register path
constexpr int FPS_WAVES = FPS_THREADS / 64;

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

// T = 2^floor(log2 n), capped at 1024: the width of the reference's reduction tree for a scene of n points (sampling_gpu.cu:16-21)
__device__ __forceinline__ int fps_log2t(int n) {
  int log2t = 0;
  while ((2 << log2t) <= n && log2t < 10) ++log2t;
  return log2t;
}

struct FpsBest {                   // a thread's candidate of one round: key 0 = the thread holds no point
  unsigned long long key;
  float x, y, z;
};

// One round over the P points a thread keeps in registers, point i being k0 + i * STRIDE: updates the running minima against the previous pick
// (x1, y1, z1) and returns the thread's winner.  l2: the tie width.  How the callers load the arrays and whether k0 / l2 are made opaque decides
// hipcc's register allocation for a whole kernel (profiles/fps_isa_registers.txt): check the table after any change here.
// The tie rule is only evaluated on an exact distance tie, so nothing per point is kept in registers beyond x, y, z and the running minimum
// distance (hoisted tie keys cost 5 more registers per point and spilled).
template <int P, int STRIDE>
__device__ __forceinline__ FpsBest fps_scan(const float (&px)[P], const float (&py)[P], const float (&pz)[P], float (&pt)[P], int k0, int n, int l2,
                                            float x1, float y1, float z1) {
  float bd = -1.f, bx = 0.f, by = 0.f, bz = 0.f;
  int bk = -1;
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const int k = k0 + i * STRIDE;
    // same expression order as the reference (sampling_gpu.cu:62, :243); fp contraction is off for this library
    const float d = (px[i] - x1) * (px[i] - x1) + (py[i] - y1) * (py[i] - y1) + (pz[i] - z1) * (pz[i] - z1);
    const float d2 = fminf(d, pt[i]);
    pt[i] = d2;
    bool up = k < n && d2 > bd;
    if (k < n && d2 == bd) up = fps_key(d2, k, l2) > fps_key(bd, bk, l2);
    bd = up ? d2 : bd;
    bk = up ? k : bk;
    bx = up ? px[i] : bx; by = up ? py[i] : by; bz = up ? pz[i] : bz;
  }
  return FpsBest{bk >= 0 ? fps_key(bd, bk, l2) : 0ull, bx, by, bz};
}

// The lane that holds the wave's winner publishes key + coordinates (keys are unique per point) into the round's parity slot; a wave without
// points must still clear its slot.  Slots alternate by parity, which leaves ONE workgroup barrier per round (the caller's, after this).
__device__ __forceinline__ void fps_publish(const FpsBest& b, int par, unsigned long long (&skey)[2][FPS_WAVES], float (&sxyz)[2][FPS_WAVES][3]) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const unsigned long long wbest = sv_wave_reduce_max(b.key);
  if (b.key == wbest && b.key != 0ull) {
    skey[par][wid] = wbest;
    sxyz[par][wid][0] = b.x; sxyz[par][wid][1] = b.y; sxyz[par][wid][2] = b.z;
  } else if (wbest == 0ull && lane == 0) {
    skey[par][wid] = 0ull;
  }
}

// m picks of one workgroup over n <= P * FPS_THREADS points kept in registers: idx[j] = base + position of pick j.  Point k is row ord[k] of
// xyz, or row first + k when ord is null; the first pick is point 0 (sampling_gpu.cu:44-46, :224-225).  n, m > 0.
template <int P, int LOG2T>
__device__ __forceinline__ void fps_rounds_reg(const float* __restrict__ xyz, const int32_t* __restrict__ ord, int first, int n, int m, int log2t,
                                               int32_t* __restrict__ idx, int base) {
  __shared__ unsigned long long skey[2][FPS_WAVES];
  __shared__ float sxyz[2][FPS_WAVES][3];
  const int tid = threadIdx.x, lane = tid & 63;
  float px[P], py[P], pz[P], pt[P];
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const int k = tid + i * FPS_THREADS;
    const bool ok = k < n;
    const int64_t row = ok ? (ord ? ord[k] : first + k) : 0;     // a select per coordinate: loaded under one branch, k_fps_reg<16> loses a wave
    px[i] = ok ? xyz[row * 3] : 0.f;
    py[i] = ok ? xyz[row * 3 + 1] : 0.f;
    pz[i] = ok ? xyz[row * 3 + 2] : 0.f;
    pt[i] = 1e10f;
  }
  if (tid == 0) idx[0] = base;
  const int64_t row0 = ord ? ord[0] : first;
  float x1 = xyz[row0 * 3], y1 = xyz[row0 * 3 + 1], z1 = xyz[row0 * 3 + 2];
  for (int j = 1; j < m; ++j) {
    const int par = j & 1;
    int tid_r = tid, l2 = LOG2T >= 0 ? LOG2T : log2t;
    // opaque per round: keeps hipcc from hoisting P point indices / tie keys into registers
    if constexpr (LOG2T >= 0) asm volatile("" : "+v"(tid_r));
    else asm volatile("" : "+v"(tid_r), "+s"(l2));
    fps_publish(fps_scan<P, FPS_THREADS>(px, py, pz, pt, tid_r, n, l2, x1, y1, z1), par, skey, sxyz);
    __syncthreads();                                            // the only barrier of the round
    const int sl = lane & (FPS_WAVES - 1);
    const unsigned long long mine = skey[par][sl];
    const unsigned long long w = sv_wave_reduce_max(mine);     // every wave reduces the partials redundantly
    const int src = sv_wave_ballot_first(mine == w);
    x1 = __shfl(sxyz[par][sl][0], src, 64);
    y1 = __shfl(sxyz[par][sl][1], src, 64);
    z1 = __shfl(sxyz[par][sl][2], src, 64);
    if (tid == 0) idx[j] = base + fps_key_index(w, LOG2T >= 0 ? LOG2T : log2t);
  }
}

// the same for scenes past the register file: the running minima live in HBM (temp, n floats, one per point at its position)
template <int LOG2T>
__device__ __forceinline__ void fps_rounds_stream(const float* __restrict__ xyz, const int32_t* __restrict__ ord, int first, int n, int m, int log2t,
                                                  float* __restrict__ temp, int32_t* __restrict__ idx, int base) {
  __shared__ unsigned long long slot[2][FPS_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int l2 = LOG2T >= 0 ? LOG2T : log2t;
  for (int k = tid; k < n; k += FPS_THREADS) temp[k] = 1e10f;
  if (tid == 0) idx[0] = base;
  int old = 0;
  __syncthreads();
  for (int j = 1; j < m; ++j) {
    const int par = j & 1;
    const int64_t ro = ord ? ord[old] : first + old;
    const float x1 = xyz[ro * 3], y1 = xyz[ro * 3 + 1], z1 = xyz[ro * 3 + 2];
    unsigned long long best = 0ull;
    for (int k = tid; k < n; k += FPS_THREADS) {
      const int64_t row = ord ? ord[k] : first + k;
      const float x2 = xyz[row * 3], y2 = xyz[row * 3 + 1], z2 = xyz[row * 3 + 2];
      const float d = (x2 - x1) * (x2 - x1) + (y2 - y1) * (y2 - y1) + (z2 - z1) * (z2 - z1);
      const float d2 = fminf(d, temp[k]);
      temp[k] = d2;
      const unsigned long long key = fps_key(d2, k, l2);
      best = key > best ? key : best;
    }
    best = sv_wave_reduce_max(best);
    if (lane == 0) slot[par][wid] = best;
    __syncthreads();
    unsigned long long w = slot[par][lane & (FPS_WAVES - 1)];
    w = sv_wave_reduce_max(w);
    old = fps_key_index(w, l2);
    if (tid == 0) idx[j] = base + old;
  }
}
#endif
