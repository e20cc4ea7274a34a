// Plan of a rulebook table for the MFMA sparse convolution (k_spconv_rs3 in sparse_conv.hip): regions, mask classes, the regrouped row-major table
// and the deal of tiles to waves.  The header comment of sparse_conv.hip says what a plan is for.
#include <stdlib.h>

#include "sparse_conv.h"
#include "wave.h"

// ================================================================================================
// Plan of a rulebook table for the MFMA kernel
// ================================================================================================

// Mask class.  A 16-row tile executes offset k when ANY of its rows has neighbour k, so rows should share tiles with rows of (nearly) the
// same mask.  Measured on the rulebooks of the bench scenes (useful / executed MFMA steps, 8 regions): tiles of consecutive rows 0.21-0.58,
// a hash of the mask (round 1) 0.48-0.74, this key 0.72-0.87, an exact sort by mask 0.70-0.85.  The key is the MIDDLE z-plane of the mask
// (bits 9..17: the 9 in-plane neighbours, the bulk of a LiDAR surface's neighbourhood) + which of the other two planes are occupied; rows
// with an empty middle plane (the input-major table of a stride-2 conv: the mask is a function of coordinate parity) are keyed by their
// first occupied plane instead.  Equal keys -> equal in-plane pattern; the other planes only add the offsets some row actually has.
__host__ __device__ inline int class_key(unsigned m) {
  const unsigned bot = m & 0x1ffu, mid = (m >> 9) & 0x1ffu, top = (m >> 18) & 0x1ffu;
  const unsigned zs = (bot != 0u ? 1u : 0u) | (top != 0u ? 2u : 0u);
  return mid ? (int)((zs << 9) | mid) : (int)(2048u | (zs << 9) | (bot ? bot : top));
}

// "for every distinct key among the live lanes": this lane's rank inside its key group, the group's size and its first lane
__device__ __forceinline__ void wave_key_groups(int key, bool live, int& rank, int& size, int& first_lane) {
  unsigned long long todo = __ballot(live);
  const int lane = threadIdx.x & 63;
  rank = 0, size = 0, first_lane = lane;
  while (todo) {
    const int first = __ffsll((long long)todo) - 1;
    const int k0 = __shfl(key, first);
    const unsigned long long same = __ballot(live && key == k0);
    if (live && key == k0) {
      rank = __popcll(same & ((1ull << lane) - 1));
      size = __popcll(same);
      first_lane = first;
    }
    todo &= ~same;
  }
}

// The same three answers for keys of at most BITS bits in a FIXED number of steps: lanes with an equal key are the intersection, over the key's bits,
// of the lanes that agree with this lane on that bit (one ballot per bit) -- 12 ballots for a class key whatever the number of distinct keys among the
// 64 rows (the loop above runs once per distinct key: ~20 on consecutive rows of a LiDAR table, and the deterministic plan runs it for every row).
template <int BITS>
__device__ __forceinline__ void wave_key_groups_bits(int key, bool live, int& rank, int& size, int& first_lane) {
  const int lane = threadIdx.x & 63;
  unsigned long long same = __ballot(live);
#pragma unroll
  for (int b = 0; b < BITS; ++b) {
    const bool bit = (key >> b) & 1;
    const unsigned long long m = __ballot(bit);
    same &= bit ? m : ~m;
  }
  rank = __popcll(same & ((1ull << lane) - 1ull));
  size = __popcll(same);
  first_lane = live ? __ffsll((long long)same) - 1 : lane;
}

struct PlanArgs {
  const int32_t* masks;   // (n_rows) neighbour mask of every row (written by the rulebook builders)
  int64_t n_rows;
  int32_t* hist;          // persistent: [0 .. R*C) class counts (zero between calls), [R*C .. 2R*C) class starts, [2R*C .. 3R*C) cursors
  int32_t* perm;          // out: (n_pad) row at each position, -1 in the padding of the last tile; n_pad = 16 * ceil(n_rows / 16)
  int32_t* masks_p;       // out: (n_pad) mask of the row at each position
};

__device__ __forceinline__ int plan_region_of_row(int64_t n_rows, int64_t row) {
  int r = 0;
#pragma unroll
  for (int q = 1; q < PL_REGIONS; ++q) r += row >= plan_region_start(n_rows, q) ? 1 : 0;   // starts are non-decreasing
  return r;
}

// pass 1: per-(region, class) histogram.  One row per thread; counts go wave -> LDS -> global, so the hottest class (one mask covers
// ~20 % of the rows) sees one global atomic per 1024 rows.  A workgroup lies inside one region.
// (Tried: letting the last workgroup to arrive -- release fence + ticket -- do the scan below, and the same for the BatchNorm statistics:
// one launch less each, but 24 us instead of 7 + 6.5: every workgroup's agent-scope release writes back its XCD's L2.  A kernel boundary
// costs 1.5 us on this GPU; separate launches it is.)
__global__ __launch_bounds__(PL_WG) void k_plan_hist(PlanArgs a) {
  __shared__ int s_hist[PL_CLASSES];
  for (int i = threadIdx.x; i < PL_CLASSES; i += PL_WG) s_hist[i] = 0;
  __syncthreads();
  const int64_t row = (int64_t)blockIdx.x * PL_WG + threadIdx.x;
  const bool live = row < a.n_rows;
  const unsigned m = live ? (unsigned)a.masks[row] : 0u;
  int rank, size, first_lane;
  const int key = class_key(m);
  wave_key_groups(key, live, rank, size, first_lane);
  if (live && rank == 0) atomicAdd(&s_hist[key], size);
  __syncthreads();
  const int region = plan_region_of_row(a.n_rows, (int64_t)blockIdx.x * PL_WG);
  int32_t* gh = a.hist + (size_t)region * PL_CLASSES;
  for (int i = threadIdx.x; i < PL_CLASSES; i += PL_WG)
    if (s_hist[i]) atomicAdd(&gh[i], s_hist[i]);
}

// pass 2: counts -> class starts: exclusive scan per region, counts and cursors back to zero.  One 128-thread workgroup per region, 32
// consecutive classes per thread (a single 1024-thread workgroup for all regions took 17 us: one CU moving 0.5 MB).
__global__ __launch_bounds__(128) void k_plan_scan(PlanArgs a) {
  constexpr int RC = PL_REGIONS * PL_CLASSES;
  const int r = blockIdx.x, tid = threadIdx.x, g = r * 128 + tid;      // g: global 32-class group
  int32_t* cnt = a.hist + (size_t)g * 32;
  int v[32], sum = 0;
  {
    const i32x4* c4 = reinterpret_cast<const i32x4*>(cnt);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const i32x4 t = c4[q];
      v[4 * q] = t.x, v[4 * q + 1] = t.y, v[4 * q + 2] = t.z, v[4 * q + 3] = t.w;
    }
#pragma unroll
    for (int u = 0; u < 32; ++u) sum += v[u];
  }
  const int incl = sv_wave_incl_scan(sum);
  __shared__ int s_wave0;
  if (tid == 63) s_wave0 = incl;
  __syncthreads();
  int run = (int)plan_region_start(a.n_rows, r) + incl - sum + (tid >= 64 ? s_wave0 : 0);
  i32x4* st4 = reinterpret_cast<i32x4*>(a.hist + RC + g * 32);
  i32x4* cu4 = reinterpret_cast<i32x4*>(a.hist + 2 * RC + g * 32);
  i32x4* cn4 = reinterpret_cast<i32x4*>(cnt);
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    i32x4 t;
    t.x = run, run += v[4 * q];
    t.y = run, run += v[4 * q + 1];
    t.z = run, run += v[4 * q + 2];
    t.w = run, run += v[4 * q + 3];
    st4[q] = t;
    cu4[q] = (i32x4){0, 0, 0, 0};
    cn4[q] = (i32x4){0, 0, 0, 0};
  }
}

// pass 3: placement.  position = class start + (rows of the class placed by earlier workgroups: one global atomic per (workgroup, class))
// + (rows of the class in earlier waves of this workgroup: LDS) + rank inside the wave.  Threads past n_rows fill the padding of the last tile.
__global__ __launch_bounds__(PL_WG) void k_plan_place(PlanArgs a) {
  __shared__ int s_cnt[PL_CLASSES];
  constexpr int RC = PL_REGIONS * PL_CLASSES;
  for (int i = threadIdx.x; i < PL_CLASSES; i += PL_WG) s_cnt[i] = 0;
  __syncthreads();
  const int64_t row = (int64_t)blockIdx.x * PL_WG + threadIdx.x;
  const int64_t n_pad = (a.n_rows + 15) / 16 * 16;
  const bool live = row < a.n_rows;
  const unsigned m = live ? (unsigned)a.masks[row] : 0u;
  const int key = live ? class_key(m) : 0;
  int rank, size, first_lane;
  wave_key_groups(key, live, rank, size, first_lane);
  int wave_off = 0;
  if (live && rank == 0) wave_off = atomicAdd(&s_cnt[key], size);
  wave_off = __shfl(wave_off, first_lane);
  __syncthreads();
  const int region = plan_region_of_row(a.n_rows, (int64_t)blockIdx.x * PL_WG);
  for (int i = threadIdx.x; i < PL_CLASSES; i += PL_WG) {
    const int c = s_cnt[i];
    if (c) s_cnt[i] = a.hist[RC + region * PL_CLASSES + i] + atomicAdd(&a.hist[2 * RC + region * PL_CLASSES + i], c);
  }
  __syncthreads();
  int64_t pos = -1;
  if (live) pos = (int64_t)s_cnt[key] + wave_off + rank;
  else if (row < n_pad) pos = row;
  if (pos < 0 || pos >= n_pad) return;            // the range check only matters if the persistent counters were clobbered
  a.perm[pos] = live ? (int32_t)row : -1;
  a.masks_p[pos] = (int32_t)m;
}

extern "C" size_t sv_conv_plan_persistent_bytes(void) { return (size_t)3 * PL_REGIONS * PL_CLASSES * sizeof(int32_t); }
extern "C" size_t sv_conv_plan_perm_bytes(int64_t n_rows) {
  const int64_t n_pad = ((n_rows > 0 ? n_rows : 0) + 15) / 16 * 16;
  return (size_t)(n_pad > 0 ? n_pad : 16) * sizeof(int32_t);
}

extern "C" int sv_conv_plan_build(const int32_t* masks, int64_t n_rows, void* persistent, int32_t* perm, int32_t* masks_p, void* stream) {
  SV_CHECK_ARG(n_rows >= 0 && n_rows < (int64_t)1 << 30, "sv_conv_plan_build: 0 <= n_rows < 2^30");
  if (n_rows == 0) return SV_OK;
  SV_CHECK_ARG(masks && persistent && perm && masks_p, "sv_conv_plan_build: null pointer");
  PlanArgs a;
  a.masks = masks, a.n_rows = n_rows, a.hist = static_cast<int32_t*>(persistent), a.perm = perm, a.masks_p = masks_p;
  const int wgs = sv_div_up(n_rows, PL_WG);      // covers the <= 15 padding positions too: n_pad <= wgs * PL_WG
  hipStream_t st = sv_stream(stream);
  hipLaunchKernelGGL(k_plan_hist, dim3(wgs), dim3(PL_WG), 0, st, a);
  hipLaunchKernelGGL(k_plan_scan, dim3(PL_REGIONS), dim3(128), 0, st, a);
  hipLaunchKernelGGL(k_plan_place, dim3(wgs), dim3(PL_WG), 0, st, a);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// neighbour masks of a k-major table (for tables that did not come with masks from their builder)
__global__ __launch_bounds__(256) void k_row_masks(const int32_t* __restrict__ nbr, int64_t n_rows, int K, int32_t* __restrict__ masks) {
  for (int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x; row < n_rows; row += (int64_t)gridDim.x * 256) {
    unsigned m = 0;
    for (int k0 = 0; k0 < K; k0 += 9) {
      int32_t j[9];
#pragma unroll
      for (int u = 0; u < 9; ++u) j[u] = k0 + u < K ? nbr[(int64_t)(k0 + u) * n_rows + row] : -1;
#pragma unroll
      for (int u = 0; u < 9; ++u) m |= j[u] >= 0 ? (1u << (k0 + u)) : 0u;
    }
    masks[row] = (int32_t)m;
  }
}
// k-major (K, n_rows) -> row-major (n_rows, 32) + masks, for tables that did not come with them from their builder
__global__ __launch_bounds__(256) void k_table_rows(const int32_t* __restrict__ nbr, int64_t n_rows, int K, int32_t* __restrict__ tab, int32_t* __restrict__ masks) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= n_rows) return;
  int32_t e[PL_ROW];
#pragma unroll
  for (int k = 0; k < PL_ROW; ++k) e[k] = -1;
  unsigned m = 0;
#pragma unroll
  for (int k = 0; k < RS3_KMAX; ++k)
    if (k < K) {
      e[k] = nbr[(int64_t)k * n_rows + row];
      m |= e[k] >= 0 ? (1u << k) : 0u;
    }
  masks[row] = (int32_t)m;
  i32x4* dst = reinterpret_cast<i32x4*>(tab + row * PL_ROW);
#pragma unroll
  for (int q = 0; q < PL_ROW / 4; ++q) dst[q] = (i32x4){e[4 * q], e[4 * q + 1], e[4 * q + 2], e[4 * q + 3]};
}
extern "C" int sv_conv_table_rows(const int32_t* nbr, int64_t n_rows, int K, int32_t* table_rows, int32_t* masks, void* stream) {
  SV_CHECK_ARG(n_rows >= 0 && K > 0 && K <= RS3_KMAX, "sv_conv_table_rows: 1 <= K <= %d (got %d)", RS3_KMAX, K);
  if (n_rows == 0) return SV_OK;
  SV_CHECK_ARG(nbr && table_rows && masks, "sv_conv_table_rows: null pointer");
  hipLaunchKernelGGL(k_table_rows, dim3(sv_div_up(n_rows, 256)), dim3(256), 0, sv_stream(stream), nbr, n_rows, K, table_rows, masks);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ------------------------------------------------------------------------------------------------ tiles -> waves
// A conv launch is ONE resident round of PL_WAVES_PER_SIMD waves on every SIMD: 8 regions x 128 workgroups of 4 waves.  Observed placement
// (tools/conv_trace.py, MAP=1; speed only, never correctness): workgroup b runs on XCD b % 8; inside an XCD the dispatcher walks the 4 shader
// engines and their CUs in turn, so workgroups j, j + 32, j + 64, j + 96 of a region stack up on one CU; the 4 waves of a workgroup go to the
// CU's 4 SIMDs in a rotation whose start varies.  A launch lasts as long as its busiest SIMD; a 16-row tile costs as many MFMA steps as it
// has kernel offsets with at least one neighbour (3 .. 27) and cannot be split.  So the deal balances CUs, and gives the 4 waves of a
// workgroup equal work (whichever SIMD each lands on): the region's tiles are counting-sorted by cost and taken in QUADS of 4 consecutive
// (near-equal) tiles; round after round the next 32 quads go to the 32 CU bins in snake order; inside a bin the rounds walk the four
// workgroups in snake order as well (one tile of the quad per wave), tile slot round / 4.  A wave works through its slots G tiles at a time
// (n_pass passes).  With >= 16 rounds (the bench's 64-channel layers have 16-34) the busiest CU carries 1.04-1.09x its XCD's mean; a
// region with a few 27-offset tiles and only ~7 rounds of 5-9-offset ones ends at up to 1.45x, because every CU gets one quad per round
// whatever it already holds.  Ranking the bins by load every round (sorted rounds) measured the same there and cost 14 us per deal
// instead of 4; a true longest-processing-time deal needs unequal tile counts per wave -- not built.
// Measured on the 64->64 layers with per-wave stamps: the round-1 snake deal of whole waves left the busiest SIMD at 1.19x (139 k rows) to
// 1.65x (66 k rows) the mean and 16 % of the SIMDs with a wave less than the others.
// Order inside a cost bucket is arbitrary: every output row is still produced by one wave with the same summation order, results do not
// depend on the deal.  One workgroup per region, everything in LDS.
// Round 6: on SUBMANIFOLD tables whose waves work on four tiles at a time (the 16- and 32-channel layers) those tiles are CONSECUTIVE in the
// cost-sorted list (units of G quads dealt together) instead of one tile from each of G different rounds.  A wave walks the union of its tiles' offsets and issues every tile's gather and the offset's weight loads in each step,
// whether the tile has the offset or not: with tiles of cost 27 / 12 / 8 / 5 the union is the 27 and a step carries 1.7 of 4 tiles on average
// (32 -> 32 at 250 k rows), with four tiles of one cost -- neighbours in the sorted list, mostly one mask class -- 3.0; steps per launch 82 k -> 47 k
// there (an emulation of the plan on the bench's tables); measured 68.6 -> 59 us on that layer, 23.8 -> 22.1 us at 16 -> 16.  NOT for the others: a
// wave of G costly tiles is also the launch's longest wave, and the strided tables' equal-cost tiles do not share masks -- 16 -> 32 strided 24.7 -> 28.1 us,
// 32 -> 64 strided 44 -> 50 us, 64 -> 64 on two tiles 112 -> 116 us when every table was dealt this way (profiles/r06_adj_ab.txt).  A region takes its
// table for submanifold when every row has the centre offset of a 27-offset kernel (bit 13 of every mask).

// The deal of a region's sorted tiles (descending cost) to its waves; called by every thread of the plan workgroup behind a barrier.
// Every round of 32 quads goes to the bins in order of the load they already hold (round 6; rounds 1-5 dealt in plain snake order) -- the lightest bin takes the round's
// costliest quad (longest-processing-time dealing under "one quad per bin and round", which the slot layout needs).  The costs are skewed (a few
// 27-offset tiles, many of 5-9): snake order gives the bin of rank b the ranks b, 63 - b, 64 + b, ... whatever they cost, and the busiest CU carried
// 1.14x (139 k rows), 1.26x (66 k rows), 1.41x (strided 64 -> 64) the mean of the launch (per-wave stamps, profiles/r06_conv_trace_raw.txt; an
// emulation of the plan on the same tables reproduces 1.138 / 1.251 / 1.395 and gives 1.08 / 1.115 / 1.29 for this rule).  One wave does it: bins in
// lanes 0..31, a round = 32 readlanes to rank the loads + the slot writes.  Deterministic (ties by bin index): a table still has one plan.
// AND of a region's masks: lanes hand in the AND of their rows' masks (all ones without a row), one LDS atomic per wave
__device__ __forceinline__ void plan_and_masks(unsigned* s_and, unsigned mine) {
  mine = sv_wave_reduce_and(mine);
  if ((threadIdx.x & 63) == 0) atomicAnd(s_and, mine);
}
// ... and only with at least four rounds of units to deal (a bin takes one unit per round whatever it costs: with two or three rounds a unit of four
// 27-offset tiles leaves its CU at 2-3x the mean; at the bench's four rounds the busiest CU of a region carries 1.0-1.2x (32 -> 32) / 1.4-1.8x (16 -> 16) the mean
// and the launches are still 14 % / 7 % shorter -- these layers are bound by their steps, not by the matrix pipe)
__device__ __forceinline__ bool plan_adjacent(int G, unsigned and_all, int nt) {
  const int units = ((nt + PL_QUAD - 1) / PL_QUAD + G - 1) / G;
  return G == 4 && ((and_all >> 13) & 1u) && (units + PL_BINS - 1) / PL_BINS >= 4;
}

template <typename CostOf>
__device__ __forceinline__ void plan_deal_quads(const uint16_t* s_sorted, CostOf cost_of, int nt, int tile0, int slots, int G, bool adjacent, int32_t* __restrict__ out, uint8_t* s_bin) {
  // s_bin: one byte of LDS per unit (the caller's: a table that is dead by now) -- the unit's cost, then its bin
  const int tid = threadIdx.x;
  const int nq = (nt + PL_QUAD - 1) / PL_QUAD;
  const int UG = adjacent ? G : 1;               // quads per unit
  const int nu = (nq + UG - 1) / UG;
  // unit u of round j = u / 32 goes to `bin`; inside a bin the rounds walk its workgroups in snake order; the unit's quads fill the G slots of one pass
  // (not adjacent: a unit is one quad and a round fills one SLOT of the bin's workgroups, as in rounds 2-5)
  auto put = [&](int u, int j, int bin) {
    const int jm = j % PL_WAVES_PER_SIMD, wg = ((j / PL_WAVES_PER_SIMD) & 1) ? PL_WAVES_PER_SIMD - 1 - jm : jm;
    const int slot0 = (j / PL_WAVES_PER_SIMD) * UG;
    for (int g = 0; g < UG; ++g) {
      const int qd = u * UG + g;
#pragma unroll
      for (int part = 0; part < PL_QUAD; ++part) {
        const int p = qd * PL_QUAD + part;
        if (p < nt) out[(int64_t)((bin + PL_BINS * wg) * 4 + part) * slots + slot0 + g] = tile0 + s_sorted[p];
      }
    }
  };
  for (int u = tid; u < nu; u += 1024) s_bin[u] = (uint8_t)cost_of(s_sorted[u * UG * PL_QUAD]);      // the unit's first tile is its costliest (its quads cost about the same)
  __syncthreads();
  if (tid < 64) {                                                   // the serial part: one wave, nothing but the ranking and two LDS bytes per round
    const int lane = tid;
    int key = lane;                                                 // (load << 5) | bin: unique, so a bin's rank is the number of smaller keys
    for (int j = 0; j * PL_BINS < nu; ++j) {
      int rank = 0;
#pragma unroll
      for (int o = 0; o < PL_BINS; ++o) rank += __builtin_amdgcn_readlane(key, o) < key ? 1 : 0;
      const int u = j * PL_BINS + rank;                            // the bin with the rank-th lightest load takes the round's rank-th costliest unit
      if (lane < PL_BINS && u < nu) {
        key += (int)s_bin[u] << 5;
        s_bin[u] = (uint8_t)lane;
      }
    }
  }
  __syncthreads();
  for (int u = tid; u < nu; u += 1024) put(u, u / PL_BINS, s_bin[u]);
}

__global__ __launch_bounds__(1024) void k_plan_deal(const int32_t* __restrict__ masks_p, PlanDims d, int32_t* __restrict__ tile_of) {
  __shared__ uint8_t s_cost[PL_MAX_REGION_TILES];
  __shared__ uint16_t s_sorted[PL_MAX_REGION_TILES];     // tiles of the region in descending cost order
  __shared__ int s_cnt[32], s_start[32];
  __shared__ unsigned s_and_w;
  const int tid = threadIdx.x, r = blockIdx.x;
  const int nt = d.tiles[r], slots = d.n_pass * d.G;
  int32_t* out = tile_of + (int64_t)r * PL_REGION_WAVES * slots;
  for (int i = tid; i < PL_REGION_WAVES * slots; i += 1024) out[i] = -1;
  if (tid < 32) s_cnt[tid] = 0;
  if (tid == 0) s_and_w = 0xFFFFFFFFu;
  __syncthreads();
  unsigned andm = 0xFFFFFFFFu;
  for (int t = tid; t < nt; t += 1024) {
    const i32x4* mp = reinterpret_cast<const i32x4*>(masks_p + ((int64_t)d.tile0[r] + t) * 16);
    unsigned m = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const i32x4 v = mp[q];
      m |= (unsigned)v.x | (unsigned)v.y | (unsigned)v.z | (unsigned)v.w;
      andm &= (v.x ? (unsigned)v.x : ~0u) & (v.y ? (unsigned)v.y : ~0u) & (v.z ? (unsigned)v.z : ~0u) & (v.w ? (unsigned)v.w : ~0u);     // padding positions carry mask 0
    }
    const int c = __popc(m) > 31 ? 31 : __popc(m);
    s_cost[t] = (uint8_t)c;
    atomicAdd(&s_cnt[c], 1);
  }
  __syncthreads();
  if (tid == 0) {                          // descending cost: the most expensive bucket first
    int acc = 0;
    for (int c = 31; c >= 0; --c) s_start[c] = acc, acc += s_cnt[c];
  }
  __syncthreads();
  if (tid < 32) s_cnt[tid] = 0;
  __syncthreads();
  for (int t = tid; t < nt; t += 1024) {
    const int c = s_cost[t];
    s_sorted[s_start[c] + atomicAdd(&s_cnt[c], 1)] = (uint16_t)t;
  }
  plan_and_masks(&s_and_w, andm);
  __syncthreads();
  const unsigned s_and = s_and_w;
  // quads of 4 consecutive tiles of the sorted list, dealt to the 32 CU bins (plan_deal_quads)
  __shared__ uint8_t s_bin[PL_MAX_REGION_TILES / PL_QUAD];
  plan_deal_quads(s_sorted, [&](int t) { return (int)s_cost[t]; }, nt, d.tile0[r], slots, d.G, plan_adjacent(d.G, s_and, nt), out, s_bin);
}

// The whole plan of a table in ONE launch: the 8 regions are independent (own classes, own positions, own tiles, own waves), so one
// 1024-thread workgroup per region runs the four passes above back to back out of LDS -- class histogram, exclusive scan, placement
// (perm / masks_p and the OR of each tile's masks), cost sort + deal -- with workgroup barriers between them instead of kernel boundaries
// and no global counters at all.  A step of the bench builds 12 plans: 12 launches instead of 48, and none of the ~5 us kernels whose
// cost is their launch.  Same placement rule (class start + rows of the class placed before), same deal; the order of the rows inside a
// class depends on LDS atomic order, as it depended on global atomic order before -- results do not depend on it.
// LDS: 2 x 16 KB class tables + 6 bytes per tile of the largest region.
struct PlanFusedArgs {
  const int32_t* masks;
  int64_t n_rows;
  int32_t* perm;
  int32_t* masks_p;
  int32_t* tile_of;
  PlanDims d;
  int max_tiles;          // tiles of the largest region (LDS layout)
#if SEEVCN_MEASURE
  int debug;              // SEEVCN_PLAN_DEBUG (results are wrong): 1 no histogram pass, 2 no perm / masks_p stores, 4 no deal
#else
  static constexpr int debug = 0;
#endif
  int stable;             // every region has <= 65535 rows: the deterministic body (plan_region_body_stable)
};

// LDS of one plan workgroup and whether the deterministic body takes the table (sets a.stable)
static size_t plan_lds_bytes(PlanFusedArgs& a) {
  static const int force_atomic = getenv("SEEVCN_PLAN_ATOMIC") ? atoi(getenv("SEEVCN_PLAN_ATOMIC")) : 0;   // 1: the LDS-atomic placement (A/B runs, tests)
  int64_t big = 0;
  for (int r = 0; r < PL_REGIONS; ++r) {
    const int64_t s0 = plan_region_start(a.n_rows, r), s1 = r + 1 < PL_REGIONS ? plan_region_start(a.n_rows, r + 1) : a.n_rows;
    if (s1 - s0 > big) big = s1 - s0;
  }
  a.stable = (big <= 65535 && !force_atomic) ? 1 : 0;
  return (size_t)(a.stable ? 8 : 2) * PL_CLASSES * 4 + (size_t)a.max_tiles * 6;
}
static size_t plan_lds_bytes_for(const PlanFusedArgs& a) { return (size_t)(a.stable ? 8 : 2) * PL_CLASSES * 4 + (size_t)a.max_tiles * 6; }

// The deterministic body needs 128 KB + tiles of dynamic LDS: above 48 KB a kernel's limit has to be raised, PER DEVICE (the attribute belongs to the
// function's code object on the current device).  Returns false when this device cannot give the kernel that much (the caller then takes the body with
// LDS atomics); `which` = 0 k_plan_region, 1 k_plan_region_batch.
static bool plan_raise_lds(const void* fn, int which) {
  constexpr int MAX_DEV = 64;
  static signed char state[2][MAX_DEV] = {};                          // 0 unknown, 1 raised, -1 refused
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEV) return false;
  if (state[which][dev] == 0) {
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024);
    if (e != hipSuccess) (void)hipGetLastError();                       // not an error of the call: the atomic body runs instead
    state[which][dev] = e == hipSuccess ? 1 : -1;
  }
  return state[which][dev] > 0;
}

__device__ __forceinline__ void plan_region_body(const PlanFusedArgs& a, const int r) {
  extern __shared__ int32_t s_dyn[];
  int32_t* s_start = s_dyn;                                   // [PL_CLASSES] counts, then class starts
  int32_t* s_cur = s_dyn + PL_CLASSES;                        // [PL_CLASSES] rows of the class placed so far
  uint32_t* s_tmask = reinterpret_cast<uint32_t*>(s_dyn + 2 * PL_CLASSES);            // [max_tiles] OR of the tile's 16 masks
  uint16_t* s_sorted = reinterpret_cast<uint16_t*>(s_tmask + a.max_tiles);            // [max_tiles] tiles in descending cost order
  __shared__ int s_wsum[16], s_cnt[32], s_cstart[32];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int64_t row0 = plan_region_start(a.n_rows, r);
  const int64_t row1 = r + 1 < PL_REGIONS ? plan_region_start(a.n_rows, r + 1) : a.n_rows;
  const int64_t n_pad = (a.n_rows + 15) / 16 * 16;
  const int nt = a.d.tiles[r], slots = a.d.n_pass * a.d.G;
  int32_t* out = a.tile_of + (int64_t)r * PL_REGION_WAVES * slots;
  __shared__ unsigned s_and_w;
  unsigned andm = 0xFFFFFFFFu;
  if (tid == 0) s_and_w = 0xFFFFFFFFu;
  for (int i = tid; i < PL_CLASSES; i += 1024) s_start[i] = 0, s_cur[i] = 0;
  for (int i = tid; i < nt; i += 1024) s_tmask[i] = 0u;
  for (int i = tid; i < PL_REGION_WAVES * slots; i += 1024) out[i] = -1;
  if (tid < 32) s_cnt[tid] = 0;
  __syncthreads();
  // pass 1: class histogram of the region.  PLR_B masks per thread are requested before the first is used: one workgroup has ~31 rows per
  // thread and nothing else to hide the load latency behind (one load at a time: 30 us per plan, most of it waiting)
  constexpr int PLR_B = 8;
  for (int64_t base = row0; base < row1 && !(a.debug & 1); base += 1024 * PLR_B) {
    unsigned m[PLR_B];
#pragma unroll
    for (int u = 0; u < PLR_B; ++u) {
      const int64_t row = base + u * 1024 + tid;
      m[u] = row < row1 ? (unsigned)a.masks[row] : 0xFFFFFFFFu;            // bit 31 is never set in a mask: marks "no row"
    }
#pragma unroll
    for (int u = 0; u < PLR_B; ++u)
      if (m[u] != 0xFFFFFFFFu) atomicAdd(&s_start[class_key(m[u])], 1);    // LDS atomic per row: cheaper here than grouping the wave's keys first
  }
  __syncthreads();
  // pass 2: counts -> starts (4 consecutive classes per thread)
  {
    int v[4], sum = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = s_start[tid * 4 + u], sum += v[u];
    const int incl = sv_wave_incl_scan(sum);
    if (lane == 63) s_wsum[wid] = incl;
    __syncthreads();
    int run = (int)row0 + incl - sum;
    for (int w = 0; w < wid; ++w) run += s_wsum[w];
#pragma unroll
    for (int u = 0; u < 4; ++u) s_start[tid * 4 + u] = run, run += v[u];
  }
  __syncthreads();
  // pass 3: placement + the OR of every tile's masks.  The last region also writes the padding of the last tile.
  const int64_t end = r + 1 < PL_REGIONS ? row1 : n_pad;
  for (int64_t base = row0; base < end; base += 1024 * PLR_B) {
    unsigned m[PLR_B];
#pragma unroll
    for (int u = 0; u < PLR_B; ++u) {
      const int64_t row = base + u * 1024 + tid;
      m[u] = row < row1 ? (unsigned)a.masks[row] : 0xFFFFFFFFu;
    }
#pragma unroll
    for (int u = 0; u < PLR_B; ++u) {
      const int64_t row = base + u * 1024 + tid;
      const bool live = m[u] != 0xFFFFFFFFu;
      int64_t pos = -1;
      if (live) {
        const int key = class_key(m[u]);
        pos = (int64_t)s_start[key] + atomicAdd(&s_cur[key], 1);
      } else if (row < end) {
        pos = row;                                            // padding positions n_rows .. n_pad - 1
      }
      if (pos >= row0 && pos < n_pad) {
        if (!(a.debug & 2)) {
          a.perm[pos] = live ? (int32_t)row : -1;
          a.masks_p[pos] = live ? (int32_t)m[u] : 0;
        }
        if (live && m[u]) atomicOr(&s_tmask[(pos - row0) >> 4], m[u]);
      }
      if (live && m[u]) andm &= m[u];
    }
  }
  plan_and_masks(&s_and_w, andm);
  __syncthreads();
  const unsigned s_and = s_and_w;
  if (a.debug & 4) return;
  // pass 4: tiles by descending cost, quads dealt to the 32 CU bins in snake order (k_plan_deal).  Neighbouring tiles are of neighbouring
  // classes and cost about the same: a wave's 64 tiles hit 2-4 of the 32 counters, so the wave groups its keys before the LDS atomic
  for (int base = 0; base < nt; base += 1024) {
    const int t = base + tid;
    const bool live = t < nt;
    const int c = live ? min(__popc(s_tmask[t]), 31) : 0;
    int rank, size, first_lane;
    wave_key_groups(c, live, rank, size, first_lane);
    if (live && rank == 0) atomicAdd(&s_cnt[c], size);
  }
  __syncthreads();
  if (tid == 0) {
    int acc = 0;
    for (int c = 31; c >= 0; --c) s_cstart[c] = acc, acc += s_cnt[c];
  }
  __syncthreads();
  if (tid < 32) s_cnt[tid] = 0;
  __syncthreads();
  for (int base = 0; base < nt; base += 1024) {
    const int t = base + tid;
    const bool live = t < nt;
    const int c = live ? min(__popc(s_tmask[t]), 31) : 0;
    int rank, size, first_lane;
    wave_key_groups(c, live, rank, size, first_lane);
    int off = 0;
    if (live && rank == 0) off = atomicAdd(&s_cnt[c], size);
    off = __shfl(off, first_lane);
    if (live) s_sorted[s_cstart[c] + off + rank] = (uint16_t)t;
  }
  __syncthreads();
  plan_deal_quads(s_sorted, [&](int t) { return min(__popc(s_tmask[t]), 31); }, nt, a.d.tile0[r], slots, a.d.G, plan_adjacent(a.d.G, s_and, nt), out, reinterpret_cast<uint8_t*>(s_start));   // the class starts are dead: placement is over
}

// The same plan with a DETERMINISTIC order: inside a class the rows keep their table order, inside a cost bucket the tiles theirs, so a table has
// exactly one plan.  (With the LDS-atomic placement above the rows of a class land in arrival order; every output row is still computed by one wave
// in a fixed summation order, but the BatchNorm column sums the conv epilogue leaves per workgroup -- and with them the batch statistics, to ~1e-7
// -- depended on which rows shared a tile: two builds of the same table could flip the ReLU branch of an activation within an ulp of zero.)
// Every wave owns a contiguous run of the region's rows and counts / places them into ITS OWN 16-bit counter per class (16 waves x 4096 classes x
// 2 B = 128 KB of LDS, two waves per 32-bit word, updated with packed atomic adds that cannot carry while the region has <= 65535 rows); the
// counters turn into positions relative to the region start by one scan over (class, wave).  Regions of more than 65535 rows take the body above.
__device__ __forceinline__ void plan_region_body_stable(const PlanFusedArgs& a, const int r) {
  extern __shared__ int32_t s_dyn[];
  uint32_t* s_wc = reinterpret_cast<uint32_t*>(s_dyn);                                // [8][PL_CLASSES]: wave w -> half w & 1 of word [w >> 1][class]
  uint32_t* s_tmask = reinterpret_cast<uint32_t*>(s_dyn + 8 * PL_CLASSES);            // [max_tiles] OR of the tile's 16 masks
  uint16_t* s_sorted = reinterpret_cast<uint16_t*>(s_tmask + a.max_tiles);            // [max_tiles] tiles in descending cost order
  __shared__ int s_wsum[16], s_cstart[32];
  __shared__ int s_wcnt[16][32];                                                      // tiles of cost c owned by wave w (then: placed so far)
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int64_t row0 = plan_region_start(a.n_rows, r);
  const int64_t row1 = r + 1 < PL_REGIONS ? plan_region_start(a.n_rows, r + 1) : a.n_rows;
  const int64_t n_pad = (a.n_rows + 15) / 16 * 16;
  const int nt = a.d.tiles[r], slots = a.d.n_pass * a.d.G;
  int32_t* out = a.tile_of + (int64_t)r * PL_REGION_WAVES * slots;
  __shared__ unsigned s_and_w;
  unsigned andm = 0xFFFFFFFFu;
  if (tid == 0) s_and_w = 0xFFFFFFFFu;
  for (int i = tid; i < 8 * PL_CLASSES; i += 1024) s_wc[i] = 0u;
  for (int i = tid; i < nt; i += 1024) s_tmask[i] = 0u;
  for (int i = tid; i < PL_REGION_WAVES * slots; i += 1024) out[i] = -1;
  if (tid < 512) (&s_wcnt[0][0])[tid] = 0;
  __syncthreads();
  // this wave's rows: a contiguous run, a multiple of 64 long
  const int64_t per_wave = (((row1 - row0) + 15) / 16 + 63) / 64 * 64;
  const int64_t w0 = row0 + (int64_t)wid * per_wave, w1 = min(w0 + per_wave, row1);
  uint32_t* my_wc = s_wc + (size_t)(wid >> 1) * PL_CLASSES;
  const int sh = 16 * (wid & 1);
  constexpr int PLR_B = 8;
  // pass 1: per-(wave, class) counts
  for (int64_t base = w0; base < w1; base += 64 * PLR_B) {
    unsigned m[PLR_B];
#pragma unroll
    for (int u = 0; u < PLR_B; ++u) {
      const int64_t row = base + u * 64 + lane;
      m[u] = row < w1 ? (unsigned)a.masks[row] : 0xFFFFFFFFu;              // bit 31 is never set in a mask: marks "no row"
    }
#pragma unroll
    for (int u = 0; u < PLR_B; ++u)
      if (m[u] != 0xFFFFFFFFu) atomicAdd(&my_wc[class_key(m[u])], 1u << sh);
  }
  __syncthreads();
  // pass 2: counts -> positions relative to the region start, class-major then wave-major (4 consecutive classes per thread)
  {
    uint32_t wd[4][8];
    int tot[4], sum = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      tot[u] = 0;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        wd[u][q] = s_wc[q * PL_CLASSES + tid * 4 + u];
        tot[u] += (int)(wd[u][q] & 0xffffu) + (int)(wd[u][q] >> 16);
      }
      sum += tot[u];
    }
    const int incl = sv_wave_incl_scan(sum);
    if (lane == 63) s_wsum[wid] = incl;
    __syncthreads();
    int run = incl - sum;
    for (int w = 0; w < wid; ++w) run += s_wsum[w];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int lo = (int)(wd[u][q] & 0xffffu), hi = (int)(wd[u][q] >> 16);
        s_wc[q * PL_CLASSES + tid * 4 + u] = (uint32_t)run | ((uint32_t)(run + lo) << 16);
        run += lo + hi;
      }
    }
  }
  __syncthreads();
  // pass 3: placement in table order + the OR of every tile's masks
  for (int64_t base = w0; base < w1; base += 64 * PLR_B) {
    unsigned m[PLR_B];
#pragma unroll
    for (int u = 0; u < PLR_B; ++u) {
      const int64_t row = base + u * 64 + lane;
      m[u] = row < w1 ? (unsigned)a.masks[row] : 0xFFFFFFFFu;
    }
#pragma unroll
    for (int u = 0; u < PLR_B; ++u) {
      const int64_t row = base + u * 64 + lane;
      const bool live = m[u] != 0xFFFFFFFFu;
      const int key = live ? class_key(m[u]) : 0;
      int rank, size, first_lane;
      wave_key_groups_bits<12>(key, live, rank, size, first_lane);
      uint32_t old = 0;
      if (live && rank == 0) old = atomicAdd(&my_wc[key], (uint32_t)size << sh);
      old = (uint32_t)__shfl((int)old, first_lane);
      if (live) {
        const int64_t pos = row0 + (int64_t)((old >> sh) & 0xffffu) + rank;
        a.perm[pos] = (int32_t)row;
        a.masks_p[pos] = (int32_t)m[u];
        if (m[u]) atomicOr(&s_tmask[(pos - row0) >> 4], m[u]), andm &= m[u];
      }
    }
  }
  plan_and_masks(&s_and_w, andm);
  if (r + 1 == PL_REGIONS && a.n_rows + tid < n_pad) a.perm[a.n_rows + tid] = -1, a.masks_p[a.n_rows + tid] = 0;    // padding of the last tile
  __syncthreads();
  const unsigned s_and = s_and_w;
  // pass 4: tiles by descending cost (stable: ascending tile inside a cost), quads dealt to the 32 CU bins in snake order (k_plan_deal)
  const int tiles_per_wave = ((nt + 15) / 16 + 63) / 64 * 64;
  const int t0 = wid * tiles_per_wave, t1 = min(t0 + tiles_per_wave, nt);
  for (int base = t0; base < t1; base += 64) {
    const int t = base + lane;
    const bool live = t < t1;
    const int c = live ? min(__popc(s_tmask[t]), 31) : 0;
    int rank, size, first_lane;
    wave_key_groups_bits<5>(c, live, rank, size, first_lane);
    if (live && rank == 0) s_wcnt[wid][c] += size;                     // the wave's own row of counters: no other wave touches it
  }
  __syncthreads();
  if (tid < 32) {                                                       // cost tid: exclusive prefix over the waves; then the bucket starts, most expensive first
    int run = 0;
    for (int w = 0; w < 16; ++w) {
      const int c = s_wcnt[w][tid];
      s_wcnt[w][tid] = run;
      run += c;
    }
    s_cstart[tid] = run;                                                // total of the cost, turned into its start below
  }
  __syncthreads();
  if (tid == 0) {
    int acc = 0;
    for (int c = 31; c >= 0; --c) {
      const int n = s_cstart[c];
      s_cstart[c] = acc, acc += n;
    }
  }
  __syncthreads();
  for (int base = t0; base < t1; base += 64) {
    const int t = base + lane;
    const bool live = t < t1;
    const int c = live ? min(__popc(s_tmask[t]), 31) : 0;
    int rank, size, first_lane;
    wave_key_groups_bits<5>(c, live, rank, size, first_lane);
    int off = 0;
    if (live && rank == 0) off = s_wcnt[wid][c], s_wcnt[wid][c] = off + size;
    off = __shfl(off, first_lane);
    if (live) s_sorted[s_cstart[c] + off + rank] = (uint16_t)t;
  }
  __syncthreads();
  plan_deal_quads(s_sorted, [&](int t) { return min(__popc(s_tmask[t]), 31); }, nt, a.d.tile0[r], slots, a.d.G, plan_adjacent(a.d.G, s_and, nt), out, reinterpret_cast<uint8_t*>(s_wc));      // the class counters are dead: placement is over
}

__device__ __forceinline__ void plan_region_dispatch(const PlanFusedArgs& a, const int r) {
  if (a.stable) plan_region_body_stable(a, r);
  else plan_region_body(a, r);
}
__global__ __launch_bounds__(1024) void k_plan_region(PlanFusedArgs a) { plan_region_dispatch(a, blockIdx.x); }

// The plans of SEVERAL tables in one launch: workgroup b builds region b % 8 of table b / 8.  A step of the bench needs 12 plans; one
// workgroup per region and table is 96 workgroups side by side instead of 12 launches of 8 (29 us each, 8 of 256 CUs busy).
constexpr int PL_BATCH_MAX = 16;
struct PlanBatchArgs {
  PlanFusedArgs j[PL_BATCH_MAX];
};
static_assert(sizeof(PlanBatchArgs) <= 3900, "kernel argument block");
__global__ __launch_bounds__(1024) void k_plan_region_batch(PlanBatchArgs b) { plan_region_dispatch(b.j[blockIdx.x / PL_REGIONS], blockIdx.x % PL_REGIONS); }

// Tiles a wave holds in registers at a time: 2 for the 64-column kernels (113 VGPRs: four waves per SIMD), 4 for the narrow ones (their
// MFMA work per weight load is small).  The weight loads are shared by the G tiles of a pass.
static int conv_tiles_per_wave(int64_t n_rows, int Kd, int Nc) {
  (void)Kd;
  if (Nc <= 32) return 4;
  // 64-column kernels: 2 tiles per pass, but a table with no more tiles than the launch has waves (8 x 512) gives every wave ONE tile --
  // with 2 per wave half the SIMD slots stay empty and the waves that run have nobody to hide their load latency behind
  constexpr int64_t G1_TILES = (int64_t)PL_REGIONS * PL_REGION_WAVES * 9 / 8;
  return (n_rows + 15) / 16 <= G1_TILES ? 1 : 2;
}
extern "C" int sv_conv_tiles_per_wave(int64_t n_rows, int Kd, int Nc) { return conv_tiles_per_wave(n_rows < 0 ? 0 : n_rows, Kd, Nc); }
extern "C" size_t sv_conv_plan_tiles_bytes(int64_t n_rows, int tiles_per_wave) {
  if (tiles_per_wave < 1) tiles_per_wave = 1;
  const PlanDims d = plan_dims(n_rows < 0 ? 0 : n_rows, tiles_per_wave);
  return (size_t)PL_REGIONS * PL_REGION_WAVES * d.n_pass * d.G * sizeof(int32_t);
}

extern "C" int sv_conv_plan_tiles(const int32_t* masks_p, int64_t n_rows, int tiles_per_wave, int32_t* tile_of, void* stream) {
  SV_CHECK_ARG(n_rows >= 0 && tiles_per_wave >= 1 && tiles_per_wave <= 4, "sv_conv_plan_tiles: bad sizes (tiles_per_wave %d)", tiles_per_wave);
  if (n_rows == 0) return SV_OK;
  SV_CHECK_ARG(masks_p && tile_of, "sv_conv_plan_tiles: null pointer");
  const PlanDims d = plan_dims(n_rows, tiles_per_wave);
  for (int r = 0; r < PL_REGIONS; ++r) SV_CHECK_ARG(d.tiles[r] <= PL_MAX_REGION_TILES, "sv_conv_plan_tiles: at most %d tiles per region", PL_MAX_REGION_TILES);
  hipLaunchKernelGGL(k_plan_deal, dim3(PL_REGIONS), dim3(1024), 0, sv_stream(stream), masks_p, d, tile_of);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// perm + masks_p + tile_of(tiles_per_wave) of a table in one launch (k_plan_region); same outputs as sv_conv_plan_build followed by
// sv_conv_plan_tiles up to the order of the rows inside a class
extern "C" int sv_conv_plan_build_dealt(const int32_t* masks, int64_t n_rows, int tiles_per_wave, int32_t* perm, int32_t* masks_p, int32_t* tile_of,
                                        void* stream) {
  SV_CHECK_ARG(n_rows >= 0 && n_rows < (int64_t)1 << 30 && tiles_per_wave >= 1 && tiles_per_wave <= 4, "sv_conv_plan_build_dealt: bad sizes");
  if (n_rows == 0) return SV_OK;
  SV_CHECK_ARG(masks && perm && masks_p && tile_of, "sv_conv_plan_build_dealt: null pointer");
  PlanFusedArgs a;
  a.masks = masks, a.n_rows = n_rows, a.perm = perm, a.masks_p = masks_p, a.tile_of = tile_of;
  a.d = plan_dims(n_rows, tiles_per_wave);
#if SEEVCN_MEASURE
  static const int plan_debug = getenv("SEEVCN_PLAN_DEBUG") ? atoi(getenv("SEEVCN_PLAN_DEBUG")) : 0;
  a.debug = plan_debug;
#endif
  a.max_tiles = 1;
  for (int r = 0; r < PL_REGIONS; ++r) {
    SV_CHECK_ARG(a.d.tiles[r] <= PL_MAX_REGION_TILES, "sv_conv_plan_build_dealt: at most %d tiles per region", PL_MAX_REGION_TILES);
    if (a.d.tiles[r] > a.max_tiles) a.max_tiles = a.d.tiles[r];
  }
  a.max_tiles = (a.max_tiles + 1) & ~1;                                  // keeps the uint16 array 4-byte aligned
  size_t lds = plan_lds_bytes(a);
  if (lds > 48 * 1024 && !plan_raise_lds(reinterpret_cast<const void*>(k_plan_region), 0)) {
    a.stable = 0;                                                       // no large LDS on this device: the body with LDS atomics (32 KB + tiles)
    lds = plan_lds_bytes_for(a);
  }
  hipLaunchKernelGGL(k_plan_region, dim3(PL_REGIONS), dim3(1024), lds, sv_stream(stream), a);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// jobs_host: n_jobs rows of 8 int64 = {masks, n_rows, tiles_per_wave, perm, masks_p, tile_of, 0, 0}: sv_conv_plan_build_dealt for every row, all
// in one launch (groups of PL_BATCH_MAX tables)
extern "C" int sv_conv_plan_build_dealt_batch(const int64_t* jobs_host, int n_jobs, void* stream) {
  SV_CHECK_ARG(n_jobs >= 0 && (jobs_host || n_jobs == 0), "sv_conv_plan_build_dealt_batch: bad arguments");
  hipStream_t st = sv_stream(stream);
  PlanBatchArgs b;
  int nb = 0;
  size_t lds = 0;
  auto flush = [&]() -> int {
    if (nb == 0) return SV_OK;
    if (lds > 48 * 1024 && !plan_raise_lds(reinterpret_cast<const void*>(k_plan_region_batch), 1)) {
      lds = 0;
      for (int q = 0; q < nb; ++q) {
        b.j[q].stable = 0;
        const size_t need = plan_lds_bytes_for(b.j[q]);
        if (need > lds) lds = need;
      }
    }
    hipLaunchKernelGGL(k_plan_region_batch, dim3(PL_REGIONS * nb), dim3(1024), lds, st, b);
    nb = 0, lds = 0;
    return SV_OK;
  };
  for (int q = 0; q < n_jobs; ++q) {
    const int64_t* r = jobs_host + 8 * q;
    const int64_t n_rows = r[1];
    const int g = (int)r[2];
    SV_CHECK_ARG(n_rows >= 0 && n_rows < (int64_t)1 << 30 && g >= 1 && g <= 4, "sv_conv_plan_build_dealt_batch: job %d: bad sizes", q);
    if (n_rows == 0) continue;
    SV_CHECK_ARG(r[0] && r[3] && r[4] && r[5], "sv_conv_plan_build_dealt_batch: job %d: null pointer", q);
    PlanFusedArgs& a = b.j[nb];
    a.masks = reinterpret_cast<const int32_t*>(r[0]), a.n_rows = n_rows, a.perm = reinterpret_cast<int32_t*>(r[3]);
    a.masks_p = reinterpret_cast<int32_t*>(r[4]), a.tile_of = reinterpret_cast<int32_t*>(r[5]);
    a.d = plan_dims(n_rows, g);
#if SEEVCN_MEASURE
    a.debug = 0;
#endif
    a.max_tiles = 1;
    for (int rg = 0; rg < PL_REGIONS; ++rg) {
      SV_CHECK_ARG(a.d.tiles[rg] <= PL_MAX_REGION_TILES, "sv_conv_plan_build_dealt_batch: at most %d tiles per region", PL_MAX_REGION_TILES);
      if (a.d.tiles[rg] > a.max_tiles) a.max_tiles = a.d.tiles[rg];
    }
    a.max_tiles = (a.max_tiles + 1) & ~1;
    const size_t need = plan_lds_bytes(a);
    if (need > lds) lds = need;
    if (++nb == PL_BATCH_MAX) {
      int rc = flush();
      if (rc) return rc;
    }
  }
  int rc = flush();
  if (rc) return rc;
  SV_LAUNCH_CHECK();
  return SV_OK;
}
