// Exhaustive farthest point sampling: every kernel that evaluates all points of a scene each round, and their entries.  (fps_bucket.hip is a
// different algorithm with the same picks.)
//
// Reference kernels (legacy stream, exit(-1) on error):
//   detector3d/pcdet/ops/pointnet2/pointnet2_stack/src/sampling_gpu.cu:24-140   (FPS, one scene per block)
//   detector3d/pcdet/ops/pointnet2/pointnet2_stack/src/sampling_gpu.cu:188-319  (the ragged FPS kernel: 1024 threads, temp in HBM every round)
// Re-designed for 64-wide wavefronts: a scene's points and running distances stay in registers (no HBM traffic inside the M sequential rounds)
// and a round needs one barrier.
//
// Selection rule reproduced exactly (index-exact, including ties):
//   round j picks argmax_k temp[k] where temp[k] = min over picked p of |x_k - x_p|^2 (temp starts at 1e10),
//   first index is 0.  Ties: the reference reduces per-thread strided maxima (strict '>' keeps the smallest k of a
//   stride class) through a power-of-two tree that keeps the LOWER slot on ties (sampling_gpu.cu:16-21,55-134),
//   i.e. among equal maxima the winner minimises (bitreverse(k mod T), k div T), T = 2^floor(log2 n) <= 1024.
// The round itself -- distance, running minimum, key, publication -- is fps.h.
#include <stdlib.h>

#include "common.h"
#include "wave.h"
#include "fps.h"

// one workgroup per scene; idx (m) output: scene-local indices, + start when add_offset
template <int P>
__global__ __launch_bounds__(FPS_THREADS) void k_fps_reg(const float* __restrict__ xyz_all, const int32_t* __restrict__ starts,
                                                         const int32_t* __restrict__ counts, int fixed_n, int m,
                                                         int32_t* __restrict__ idx_all, int add_offset) {
  const int b = blockIdx.x;
  const int start = starts ? starts[b] : b * fixed_n;
  const int n = counts ? counts[b] : fixed_n;
  if (n <= 0 || m <= 0) return;
  fps_rounds_reg<P, -1>(xyz_all, nullptr, start, n, m, fps_log2t(n), idx_all + (int64_t)b * m, add_offset ? start : 0);
}

// streaming variant for scenes too large for the register file: temp lives in HBM (n floats, caller-provided)
__global__ __launch_bounds__(FPS_THREADS) void k_fps_stream(const float* __restrict__ xyz_all, const int32_t* __restrict__ starts,
                                                            const int32_t* __restrict__ counts, int fixed_n, int m,
                                                            float* __restrict__ temp_all, int32_t* __restrict__ idx_all, int add_offset) {
  const int b = blockIdx.x;
  const int start = starts ? starts[b] : b * fixed_n;
  const int n = counts ? counts[b] : fixed_n;
  if (n <= 0 || m <= 0) return;
  fps_rounds_stream<-1>(xyz_all, nullptr, start, n, m, fps_log2t(n), temp_all + start, idx_all + (int64_t)b * m, add_offset ? start : 0);
}

// ---- several workgroups per scene.  One workgroup per scene leaves 252 of 256 CUs idle at batch 4 and pays ~4 us per round for its
// 34-40 points per thread (16 ms for the 4096 keypoints of the SEE-VCN PV-RCNN, source-nuscenes/pvrcnn.yaml:111).  Here FPS_W workgroups
// share a scene (2-3 points per thread); every round each publishes its best candidate as two self-tagged 16-byte granules
// {key, x, tag} {y, z, tag} -- one `sc1` store each, no drain, no flag, no fence (MI355X_MICROARCH.md, "data-tagged granules") -- and every wave
// polls the 2 x FPS_W granules of its scene (one per lane, `sc1` loads) until all carry the round's tag.  The records alternate between two
// banks by round parity so that a fast workgroup cannot overwrite a granule a slow one still has to read; the per-wave candidates in LDS
// alternate the same way, which leaves ONE workgroup barrier per round.  Same keys, same tie rule, same winners as the single-workgroup
// kernel.  The FPS_W workgroups of a scene must be resident together (batch * FPS_W <= 256 workgroups, checked by the host); the poll is
// bounded and raises *err instead of hanging.  one_xcd: the scene's workgroups are dealt to ONE XCD (workgroup i runs on XCD i % 8) and
// the granules are plain stores that stay in that XCD's L2, where the `sc1` polls of the same XCD find them: 1.9 us per round instead of
// 2.8 with write-through (`sc1`) granules that any XCD may read (measured, 4 x 17k points -> 4096: 7.9 / 11.3 ms; one workgroup per
// scene 16.4 ms).
constexpr int FPS_W = 16;
struct FpsRecord {
  unsigned int h0[4];          // key lo, key hi, x, tag
  unsigned int h1[4];          // y, z, tag, 0
};
typedef unsigned int fps_u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void fps_store16(void* p, fps_u32x4 v) { asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory"); }
__device__ __forceinline__ void fps_store16_l2(void* p, fps_u32x4 v) { asm volatile("global_store_dwordx4 %0, %1, off" ::"v"(p), "v"(v) : "memory"); }
__device__ __forceinline__ fps_u32x4 fps_load16(const void* p) {
  fps_u32x4 v;
  asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=&v"(v) : "v"(p) : "memory");
  return v;
}

template <int P>
__global__ __launch_bounds__(FPS_THREADS) void k_fps_multi(const float* __restrict__ xyz_all, const int32_t* __restrict__ starts,
                                                           const int32_t* __restrict__ counts, int fixed_n, int m, int32_t* __restrict__ idx_all,
                                                           int add_offset, FpsRecord* __restrict__ records, unsigned nonce, int32_t* __restrict__ err,
                                                           int batch, int one_xcd, int spin_limit) {
  constexpr int NW = FPS_WAVES;
  static_assert(2 * FPS_W <= 64 && (NW & (NW - 1)) == 0, "one granule per lane");
  __shared__ unsigned long long skey[2][NW];
  __shared__ float sxyz[2][NW][3];
  int b = blockIdx.x / FPS_W, w = blockIdx.x % FPS_W;
  if (one_xcd) {                                                // workgroup i runs on XCD i % 8: a scene's workgroups all on one
    const int slot = blockIdx.x >> 3;
    b = (slot / FPS_W) * 8 + (blockIdx.x & 7);
    w = slot % FPS_W;
    if (b >= batch) return;
  }
  const int start = starts ? starts[b] : b * fixed_n;
  const int n = counts ? counts[b] : fixed_n;
  const float* xyz = xyz_all + (int64_t)start * 3;
  int32_t* idx = idx_all + (int64_t)b * m;
  if (n <= 0 || m <= 0) return;
  const int log2t = fps_log2t(n);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  FpsRecord* rec = records + (size_t)b * 2 * FPS_W;            // [parity][workgroup]
  // this workgroup's share of the scene: point i of a thread is (i * FPS_W + w) * FPS_THREADS + tid.  Loaded under ONE branch: with a select per
  // coordinate hipcc keeps a second, packed copy of x and y in k_fps_multi<8> (84 VGPRs instead of 76, a wave of occupancy less)
  float px[P], py[P], pz[P], pt[P];
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const int k = (i * FPS_W + w) * FPS_THREADS + tid;
    const bool ok = k < n;
    float x = 0.f, y = 0.f, z = 0.f;
    if (ok) { x = xyz[k * 3]; y = xyz[k * 3 + 1]; z = xyz[k * 3 + 2]; }
    px[i] = x; py[i] = y; pz[i] = z;
    pt[i] = 1e10f;
  }
  if (w == 0 && tid == 0) idx[0] = add_offset ? start : 0;
  float x1 = xyz[0], y1 = xyz[1], z1 = xyz[2];
  for (int j = 1; j < m; ++j) {
    const int par = j & 1;
    fps_publish(fps_scan<P, FPS_W * FPS_THREADS>(px, py, pz, pt, w * FPS_THREADS + tid, n, log2t, x1, y1, z1), par, skey, sxyz);
    __syncthreads();
    const unsigned tag = (nonce << 16) | (unsigned)j;
    FpsRecord* bank = rec + (size_t)par * FPS_W;
    if (wid == 0) {                                             // this workgroup's candidate -> its record
      const int sl = lane & (NW - 1);
      const unsigned long long mine = skey[par][sl];
      const unsigned long long wg_best = sv_wave_reduce_max(mine);
      const int src = sv_wave_ballot_first(mine == wg_best);
      if (lane == src || lane == src + NW) {                    // two lanes hold the winner (NW < 64): one stores each granule
        fps_u32x4 v;
        if (lane == src) v = fps_u32x4{(unsigned)(wg_best & 0xffffffffull), (unsigned)(wg_best >> 32), __float_as_uint(sxyz[par][sl][0]), tag};
        else v = fps_u32x4{__float_as_uint(sxyz[par][sl][1]), __float_as_uint(sxyz[par][sl][2]), tag, 0u};
        if (one_xcd) fps_store16_l2(lane == src ? (void*)bank[w].h0 : (void*)bank[w].h1, v);
        else fps_store16(lane == src ? (void*)bank[w].h0 : (void*)bank[w].h1, v);
      }
    }
    // every wave: poll the 2 x FPS_W granules of the scene, one per lane
    const bool poller = lane < 2 * FPS_W;
    const int half = lane / FPS_W;
    const void* gp = half == 0 ? (const void*)bank[lane & (FPS_W - 1)].h0 : (const void*)bank[lane & (FPS_W - 1)].h1;
    fps_u32x4 g = fps_u32x4{0u, 0u, 0u, 0u};
    bool ready = !poller;
    int spins = 0;
    while (true) {
      if (!ready) {
        g = fps_load16(gp);
        ready = (half == 0 ? g.w : g.z) == tag;
      }
      if (__ballot(!ready) == 0ull) break;
      if (++spins > spin_limit) {                                // ~ seconds: a missing partner (not co-resident) must not hang the GPU
        if (lane == 0) *err = 1;
        return;
      }
      __builtin_amdgcn_s_sleep(1);
    }
    const unsigned long long key = lane < FPS_W ? ((unsigned long long)g.y << 32) | g.x : 0ull;
    const unsigned long long win = sv_wave_reduce_max(key);
    const int wl = sv_wave_ballot_first(lane < FPS_W && key == win);
    x1 = __uint_as_float(__shfl(g.z, wl, 64));
    y1 = __uint_as_float(__shfl(g.x, wl + FPS_W, 64));
    z1 = __uint_as_float(__shfl(g.y, wl + FPS_W, 64));
    if (w == 0 && tid == 0) {
      const int old = fps_key_index(win, log2t);
      idx[j] = add_offset ? start + old : old;
    }
  }
}

// async_mode < 0: the multi-workgroup path ends synchronised (error word read back, retry with write-through records).  async_mode 0 / 1: ONE
// attempt (0: one-XCD records, 1: write-through records), nothing is read back -- the caller reads the error word at the end of multi_scratch
// (sv_fps_multi_error_offset) whenever it next synchronises and re-runs with mode 1 if it is non-zero.
static int fps_launch(const float* xyz, const int32_t* starts, const int32_t* counts, int batch, int fixed_n, int max_n, int m,
                      float* temp, int32_t* idx, int add_offset, hipStream_t st, void* multi_scratch = nullptr, int async_mode = -1) {
  if (batch <= 0 || m <= 0) return SV_OK;
  static unsigned nonce = 0;
  static const bool multi_off = getenv("SEEVCN_FPS_MULTI") && atoi(getenv("SEEVCN_FPS_MULTI")) == 0;
  // several workgroups per scene when the scene is large enough to keep them busy, they all fit the chip at once and m fits the 16-bit tag
  if (multi_scratch && !multi_off && batch * FPS_W <= 256 && max_n >= 4096 && max_n <= 8 * FPS_W * FPS_THREADS && m < 65536) {
    FpsRecord* rec = reinterpret_cast<FpsRecord*>(multi_scratch);
    int32_t* err = reinterpret_cast<int32_t*>(rec + (size_t)batch * 2 * FPS_W);
    static const int first_mode = getenv("SEEVCN_FPS_MULTI") && atoi(getenv("SEEVCN_FPS_MULTI")) == 1 ? 0 : 1;
    const int p = (max_n + FPS_W * FPS_THREADS - 1) / (FPS_W * FPS_THREADS);
    // first with the scene's workgroups on one XCD and its L2 as the meeting point (1.9 us per round); were the dispatch order ever not
    // "workgroup i -> XCD i % 8" a partner would poll a stale line of its own L2, time out and raise the error word: then once more with
    // write-through records, which hold for any placement (2.8 us per round).  The error word is read back, so this path ends synchronised.
    for (int one_xcd = async_mode < 0 ? first_mode : 1 - async_mode; one_xcd >= 0; --one_xcd) {
      SV_HIP(hipMemsetAsync(err, 0, 4, st));
      nonce = (nonce + 1) & 0xffffu;
      if (nonce == 0) nonce = 1;
      const int spin_limit = one_xcd ? 1 << 17 : 1 << 21;
      dim3 grid(one_xcd ? (batch + 7) / 8 * 8 * FPS_W : batch * FPS_W), block(FPS_THREADS);
      if (p <= 1) hipLaunchKernelGGL(k_fps_multi<1>, grid, block, 0, st, xyz, starts, counts, fixed_n, m, idx, add_offset, rec, nonce, err, batch, one_xcd, spin_limit);
      else if (p <= 2) hipLaunchKernelGGL(k_fps_multi<2>, grid, block, 0, st, xyz, starts, counts, fixed_n, m, idx, add_offset, rec, nonce, err, batch, one_xcd, spin_limit);
      else if (p <= 4) hipLaunchKernelGGL(k_fps_multi<4>, grid, block, 0, st, xyz, starts, counts, fixed_n, m, idx, add_offset, rec, nonce, err, batch, one_xcd, spin_limit);
      else hipLaunchKernelGGL(k_fps_multi<8>, grid, block, 0, st, xyz, starts, counts, fixed_n, m, idx, add_offset, rec, nonce, err, batch, one_xcd, spin_limit);
      SV_LAUNCH_CHECK();
      if (async_mode >= 0) return SV_OK;
      int32_t host_err = 0;
      SV_HIP(hipMemcpyAsync(&host_err, err, 4, hipMemcpyDeviceToHost, st));
      SV_HIP(hipStreamSynchronize(st));
      if (host_err == 0) return SV_OK;
    }
    sv_set_error("farthest_point_sampling: a partner workgroup never arrived (GPU shared with another process?); SEEVCN_FPS_MULTI=0 selects one workgroup per scene");
    return SV_ERR_HIP;
  }
  if (async_mode >= 0 && multi_scratch)      // the single-workgroup kernels cannot fail: the error word the caller will read is 0
    SV_HIP(hipMemsetAsync(reinterpret_cast<char*>(multi_scratch) + (size_t)batch * 2 * FPS_W * sizeof(FpsRecord), 0, 4, st));
  const int p = (max_n + FPS_THREADS - 1) / FPS_THREADS;
  dim3 grid(batch), block(FPS_THREADS);
  if (p <= 4) hipLaunchKernelGGL(k_fps_reg<4>, grid, block, 0, st, xyz, starts, counts, fixed_n, m, idx, add_offset);
  else if (p <= 8) hipLaunchKernelGGL(k_fps_reg<8>, grid, block, 0, st, xyz, starts, counts, fixed_n, m, idx, add_offset);
  else if (p <= 16) hipLaunchKernelGGL(k_fps_reg<16>, grid, block, 0, st, xyz, starts, counts, fixed_n, m, idx, add_offset);
  else if (p <= 32) hipLaunchKernelGGL(k_fps_reg<32>, grid, block, 0, st, xyz, starts, counts, fixed_n, m, idx, add_offset);
  else if (p <= 40) hipLaunchKernelGGL(k_fps_reg<40>, grid, block, 0, st, xyz, starts, counts, fixed_n, m, idx, add_offset);
  else if (p <= FPS_MAXP) hipLaunchKernelGGL(k_fps_reg<FPS_MAXP>, grid, block, 0, st, xyz, starts, counts, fixed_n, m, idx, add_offset);
  else {
    SV_CHECK_ARG(temp, "farthest_point_sampling: scenes with more than %d points need the temp buffer", FPS_MAXP * FPS_THREADS);
    hipLaunchKernelGGL(k_fps_stream, grid, block, 0, st, xyz, starts, counts, fixed_n, m, temp, idx, add_offset);
  }
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// scratch of the multi-workgroup path: 2 x FPS_W records per scene + an error word (read it back to detect a missing partner; 0 = fine)
extern "C" size_t sv_fps_multi_scratch_bytes(int batch) { return (size_t)(batch > 0 ? batch : 0) * 2 * FPS_W * sizeof(FpsRecord) + 64; }

extern "C" size_t sv_fps_multi_error_offset(int batch) { return (size_t)(batch > 0 ? batch : 0) * 2 * FPS_W * sizeof(FpsRecord); }

extern "C" int sv_farthest_point_sampling(const float* xyz, int b, int n, int m, float* temp, int32_t* idx, void* stream) {
  SV_CHECK_ARG(b >= 0 && n > 0 && m >= 0 && (b == 0 || (xyz && idx)), "farthest_point_sampling: bad arguments");
  SV_CHECK_ARG((int64_t)n < (1ll << 30), "farthest_point_sampling: n too large");
  return fps_launch(xyz, nullptr, nullptr, b, n, n, m, temp, idx, 0, sv_stream(stream));
}

extern "C" int sv_stack_farthest_point_sampling(const float* xyz, const int32_t* xyz_batch_start, const int32_t* xyz_batch_cnt, int batch,
                                                int max_n, int m, float* temp, int32_t* idx, void* stream) {
  SV_CHECK_ARG(batch >= 0 && m >= 0 && max_n >= 0, "stack_farthest_point_sampling: bad arguments");
  if (batch == 0 || m == 0) return SV_OK;
  SV_CHECK_ARG(xyz && xyz_batch_start && xyz_batch_cnt && idx, "stack_farthest_point_sampling: null pointer");
  return fps_launch(xyz, xyz_batch_start, xyz_batch_cnt, batch, 0, max_n, m, temp, idx, 1, sv_stream(stream));
}

extern "C" int sv_stack_farthest_point_sampling_multi(const float* xyz, const int32_t* xyz_batch_start, const int32_t* xyz_batch_cnt, int batch,
                                                      int max_n, int m, float* temp, void* multi_scratch, int32_t* idx, void* stream) {
  SV_CHECK_ARG(batch >= 0 && m >= 0 && max_n >= 0, "stack_farthest_point_sampling: bad arguments");
  if (batch == 0 || m == 0) return SV_OK;
  SV_CHECK_ARG(xyz && xyz_batch_start && xyz_batch_cnt && idx, "stack_farthest_point_sampling: null pointer");
  return fps_launch(xyz, xyz_batch_start, xyz_batch_cnt, batch, 0, max_n, m, temp, idx, 1, sv_stream(stream), multi_scratch);
}

extern "C" int sv_stack_farthest_point_sampling_multi_async(const float* xyz, const int32_t* xyz_batch_start, const int32_t* xyz_batch_cnt, int batch,
                                                            int max_n, int m, float* temp, void* multi_scratch, int32_t* idx, int write_through,
                                                            void* stream) {
  SV_CHECK_ARG(batch >= 0 && m >= 0 && max_n >= 0, "stack_farthest_point_sampling: bad arguments");
  if (batch == 0 || m == 0) return SV_OK;
  SV_CHECK_ARG(xyz && xyz_batch_start && xyz_batch_cnt && idx && multi_scratch, "stack_farthest_point_sampling: null pointer");
  return fps_launch(xyz, xyz_batch_start, xyz_batch_cnt, batch, 0, max_n, m, temp, idx, 1, sv_stream(stream), multi_scratch, write_through ? 1 : 0);
}

// ------------------------------------------------------------------------------------------------
// Ragged farthest point sampling (the segments of spc_sampling.hip): one workgroup per segment, n / m / offsets from the device tables.  The
// reference's stacked kernel always reduces over 1024 slots (sampling_gpu.cu:340), so the tie key is fps_key with log2t = 10 for every n.
// Picks are kept as positions in the segment during the rounds and turned into global rows through `order` at the end, so the row list is off
// the rounds' critical path.
// ------------------------------------------------------------------------------------------------
constexpr int FPS_RAGGED_LOG2T = 10;

// MAXP: the largest register-resident instantiation this kernel carries (the host picks it from its upper bound of a segment's size); the branch on
// the segment's own n is workgroup-uniform, so a 3 000-point segment pays for 8 points per thread and round, not for 48.  Three tiers (8, 32, 48): a
// kernel is allocated for its largest instantiation, and the 48-point one does not fit 256 VGPRs without scratch (as k_fps_reg<48>), so bounds
// up to 16 384 points get a kernel of their own that carries nothing above 32.
template <int MAXP, bool STREAM>
__global__ __launch_bounds__(FPS_THREADS) void k_fps_ragged(const float* __restrict__ xyz, const int32_t* __restrict__ order,
                                                            const int32_t* __restrict__ seg_start, const int32_t* __restrict__ seg_cnt,
                                                            const int32_t* __restrict__ seg_m, const int32_t* __restrict__ seg_out_start,
                                                            int64_t n_rows, int64_t idx_len, float* __restrict__ temp, int32_t* __restrict__ idx_all) {
  constexpr int L = FPS_RAGGED_LOG2T;
  const int g = blockIdx.x;
  const int n = seg_cnt[g], m = seg_m[g];
  if (n <= 0 || m <= 0) return;                                    // nothing of such a segment is read or written
  const int first = seg_start[g], out = seg_out_start[g];
  // tables that do not fit the buffers they index write nothing
  if (first < 0 || (int64_t)first + n > n_rows || out < 0 || (int64_t)out + m > idx_len) return;
  const int32_t* ord = order ? order + first : nullptr;
  int32_t* idx = idx_all + out;
  bool ran = true;                                                 // workgroup-uniform
  if (n <= 2 * FPS_THREADS) fps_rounds_reg<2, L>(xyz, ord, first, n, m, L, idx, 0);
  else if (n <= 4 * FPS_THREADS) fps_rounds_reg<4, L>(xyz, ord, first, n, m, L, idx, 0);
  else if (n <= 8 * FPS_THREADS) fps_rounds_reg<8, L>(xyz, ord, first, n, m, L, idx, 0);
  else if (MAXP >= 32 && n <= 16 * FPS_THREADS) fps_rounds_reg<(MAXP >= 32 ? 16 : 2), L>(xyz, ord, first, n, m, L, idx, 0);
  else if (MAXP >= 32 && n <= 32 * FPS_THREADS) fps_rounds_reg<(MAXP >= 32 ? 32 : 2), L>(xyz, ord, first, n, m, L, idx, 0);
  else if (MAXP >= FPS_MAXP && n <= FPS_MAXP * FPS_THREADS) fps_rounds_reg<(MAXP >= FPS_MAXP ? FPS_MAXP : 2), L>(xyz, ord, first, n, m, L, idx, 0);
  else if (STREAM) fps_rounds_stream<L>(xyz, ord, first, n, m, L, temp + first, idx, 0);
  else ran = false;                                                // a segment above the host's bound: left unwritten
  if (!ran) return;
  __syncthreads();                                                 // tid 0's positions are visible to the workgroup
  for (int j = threadIdx.x; j < m; j += FPS_THREADS) {
    const int k = idx[j];
    idx[j] = ord ? ord[k] : first + k;
  }
}

extern "C" int sv_stack_farthest_point_sampling_ragged(const float* xyz, int64_t n_rows, const int32_t* order, const int32_t* seg_start,
                                                       const int32_t* seg_cnt, const int32_t* seg_m, const int32_t* seg_out_start,
                                                       int num_segments, int max_n, float* temp, int32_t* idx, int64_t idx_len, void* stream) {
  SV_CHECK_ARG(num_segments >= 0 && max_n >= 0 && n_rows >= 0 && n_rows < (1ll << 31) && idx_len >= 0, "stack_farthest_point_sampling_ragged: bad arguments");
  if (num_segments == 0 || max_n == 0 || idx_len == 0) return SV_OK;
  SV_CHECK_ARG(xyz && seg_start && seg_cnt && seg_m && seg_out_start && idx, "stack_farthest_point_sampling_ragged: null pointer");
  dim3 grid(num_segments), block(FPS_THREADS);
  hipStream_t st = sv_stream(stream);
  if (max_n <= 8 * FPS_THREADS)
    hipLaunchKernelGGL((k_fps_ragged<8, false>), grid, block, 0, st, xyz, order, seg_start, seg_cnt, seg_m, seg_out_start, n_rows, idx_len, temp, idx);
  else if (max_n <= 32 * FPS_THREADS)
    hipLaunchKernelGGL((k_fps_ragged<32, false>), grid, block, 0, st, xyz, order, seg_start, seg_cnt, seg_m, seg_out_start, n_rows, idx_len, temp, idx);
  else if (max_n <= FPS_MAXP * FPS_THREADS)
    hipLaunchKernelGGL((k_fps_ragged<FPS_MAXP, false>), grid, block, 0, st, xyz, order, seg_start, seg_cnt, seg_m, seg_out_start, n_rows, idx_len, temp, idx);
  else {
    SV_CHECK_ARG(temp, "stack_farthest_point_sampling_ragged: segments of more than %d points need the temp buffer (n_rows floats)",
                 FPS_MAXP * FPS_THREADS);
    hipLaunchKernelGGL((k_fps_ragged<FPS_MAXP, true>), grid, block, 0, st, xyz, order, seg_start, seg_cnt, seg_m, seg_out_start, n_rows, idx_len, temp, idx);
  }
  SV_LAUNCH_CHECK();
  return SV_OK;
}
