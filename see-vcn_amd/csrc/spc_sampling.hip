// Sectorized proposal-centric (SPC) keypoint sampling of PV-RCNN++ and its RoI neighbour filter, for a whole batch in three launches.
//
// Reference (per scene, in Python):
//   detector3d/pcdet/models/backbones_3d/pfe/voxel_set_abstraction.py:45-75    sample_points_with_roi: an (N, M) distance matrix, min, mask
//   detector3d/pcdet/models/backbones_3d/pfe/voxel_set_abstraction.py:78-121   sector_fps: atan2 sectors, one boolean mask + .sum().item() per
//                                                                             sector, host-built count tensors, one ragged FPS launch
// Here: k_spc_select (mask + sector per point, RoIs in LDS) and k_spc_partition (stable rows per (scene, sector), quotas, output offsets; one
// workgroup per scene, no atomics); the third launch is k_fps_ragged (fps.hip: one workgroup per segment, points gathered through the row list
// into registers).
#include "common.h"
#include "wave.h"

constexpr int SPC_SELECT_THREADS = 256;
constexpr int SPC_PART_THREADS = 1024;
constexpr int SPC_MAX_SECTORS = 63;        // buckets 0..S live one per lane
constexpr int SPC_MAX_ROIS = 2048;         // 16 B of LDS per RoI: 32 KB, half of what a launch may ask for without an attribute (the yaml's largest block is 512)

// atan2f(y, x) with the axis cases written out (IEEE 754 values, fp32(pi) and fp32(pi / 2)): they do not depend on the device atan2f
__device__ __forceinline__ float spc_angle(float x, float y) {
  const float pi = 3.14159274101257324f, half_pi = 1.57079637050628662f;
  if (y == 0.f) {
    const bool xneg = x < 0.f || (x == 0.f && __builtin_signbit(x));
    return __builtin_copysignf(xneg ? pi : 0.f, y);
  }
  if (x == 0.f) return __builtin_copysignf(half_pi, y);
  return atan2f(y, x);
}

// sector_fps (voxel_set_abstraction.py:88-90): floor((atan2(y, x) + pi) / sector_size) clamped to [0, S] -- S itself is reachable
__device__ __forceinline__ int spc_sector(float x, float y, float sector_size, int S) {
  const float pi = 3.14159274101257324f;
  float q = floorf((spc_angle(x, y) + pi) / sector_size);
  q = fminf(fmaxf(q, 0.f), (float)S);
  return (int)q;
}

// One thread per point, blockIdx.y = scene.  sector[row] = -1 (not selected) | 0..S; with S == 0: 0 (selected) | -1.
__global__ __launch_bounds__(SPC_SELECT_THREADS) void k_spc_select(const float* __restrict__ xyz, const int32_t* __restrict__ start,
                                                                   const int32_t* __restrict__ cnt, const float* __restrict__ rois, int M,
                                                                   int roi_stride, float radius, int S, float sector_size,
                                                                   int32_t* __restrict__ sector) {
  extern __shared__ float4 sroi[];                                // centre + threshold of every RoI of the scene
  const int b = blockIdx.y;
  const int n = cnt[b];
  if ((int64_t)blockIdx.x * SPC_SELECT_THREADS >= n) return;
  const float* r = rois + (int64_t)b * M * roi_stride;
  for (int j = threadIdx.x; j < M; j += SPC_SELECT_THREADS) {
    const float* q = r + (int64_t)j * roi_stride;
    const float hl = q[3] / 2.f, hw = q[4] / 2.f, hh = q[5] / 2.f;
    const float md = sqrtf(hl * hl + hw * hw + hh * hh);         // (rois[:, 3:6] / 2).norm(dim=-1)
    sroi[j] = make_float4(q[0], q[1], q[2], md + radius);
  }
  __syncthreads();
  // grid-stride over the scene's rows: the host's max_n only sizes the grid, a scene larger than it is still written row for row
  for (int k = blockIdx.x * SPC_SELECT_THREADS + threadIdx.x; k < n; k += gridDim.x * SPC_SELECT_THREADS) {
    const int64_t row = (int64_t)start[b] + k;
    const float x = xyz[row * 3], y = xyz[row * 3 + 1], z = xyz[row * 3 + 2];
    // nearest RoI by the square-rooted distance, lowest index among equals.  sqrt is monotone, so a candidate whose squared distance is not below
    // the best one's cannot have a smaller root: only the others pay for the correctly rounded sqrt.
    float best_d = __builtin_inff(), best_d2 = __builtin_inff(), best_thr = 0.f;
    for (int j = 0; j < M; ++j) {
      const float4 c = sroi[j];
      const float dx = x - c.x, dy = y - c.y, dz = z - c.z;
      const float d2 = dx * dx + dy * dy + dz * dz;
      if (d2 < best_d2) {
        const float d = sqrtf(d2);
        if (d < best_d) { best_d = d; best_d2 = d2; best_thr = c.w; }
      }
    }
    const bool sel = M > 0 && best_d < best_thr;
    sector[row] = !sel ? -1 : (S > 0 ? spc_sector(x, y, sector_size, S) : 0);
  }
}

// One workgroup per scene.  Every wave owns a contiguous range of the scene's rows and walks it twice, 64 rows at a time: first counting the
// rows of every bucket (lane s keeps bucket s), then -- the counts of the waves before it known -- writing every row behind the rows of its
// bucket that precede it.  Buckets 0..S-1 are the sectors, bucket S holds the selected rows of no sector (S == 0: bucket 0 = the selected rows).
__global__ __launch_bounds__(SPC_PART_THREADS) void k_spc_partition(const int32_t* __restrict__ sector, const float* __restrict__ xyz,
                                                                    const int32_t* __restrict__ start, const int32_t* __restrict__ cnt, int K,
                                                                    int S, float sector_size, int out_stride, int32_t* __restrict__ order,
                                                                    int32_t* __restrict__ seg_start, int32_t* __restrict__ seg_cnt,
                                                                    int32_t* __restrict__ seg_m, int32_t* __restrict__ seg_out_start,
                                                                    int32_t* __restrict__ kp_cnt) {
  constexpr int NW = SPC_PART_THREADS / SV_WAVE;
  __shared__ int wcnt[NW][SV_WAVE];
  __shared__ int base[SV_WAVE + 1];
  const int b = blockIdx.x, st = start[b], n = cnt[b];
  const int nb = S + 1;                                            // S == 0: one bucket
  const int tid = threadIdx.x, lane = tid & (SV_WAVE - 1), wid = tid / SV_WAVE;
  const int per = ((n + NW - 1) / NW + SV_WAVE - 1) / SV_WAVE * SV_WAVE;
  const int r0 = min(n, wid * per), r1 = min(n, r0 + per);
  const int32_t* sec = sector + st;
  int c = 0;
  for (int r = r0; r < r1; r += SV_WAVE) {
    const int v = r + lane < r1 ? sec[r + lane] : -1;
    for (int s = 0; s < nb; ++s) {
      const int t = __popcll(__ballot(v == s));
      if (lane == s) c += t;
    }
  }
  wcnt[wid][lane] = c;
  __syncthreads();
  if (tid < nb) {                                                  // exclusive prefix over the waves, per bucket
    int run = 0;
    for (int w = 0; w < NW; ++w) {
      const int t = wcnt[w][tid];
      wcnt[w][tid] = run;
      run += t;
    }
    base[tid] = run;                                               // the bucket's total for now
  }
  __syncthreads();
  if (tid == 0) {
    int n_sel = 0, n_in = 0;
    for (int s = 0; s < nb; ++s) {
      const int t = base[s];
      base[s] = n_sel;
      n_sel += t;
      if (s < S) n_in += t;
    }
    base[nb] = n_sel;
    if (S == 0) {
      seg_start[b] = st; seg_cnt[b] = n_sel; seg_m[b] = 0; seg_out_start[b] = 0; kp_cnt[b] = n_sel;
    } else {
      int out = b * out_stride, total = 0;
      // the two fallbacks of the reference: nothing selected -> points[:1] (voxel_set_abstraction.py:73); nothing in a sector -> one segment
      // of all selected points with the whole quota (:105-109)
      int one_slot = -1, one_start = st, one_cnt = 0, one_m = 0;
      if (n > 0 && n_sel == 0) {
        const int s0 = spc_sector(xyz[(int64_t)st * 3], xyz[(int64_t)st * 3 + 1], sector_size, S);
        order[st] = st;
        one_slot = s0 < S ? s0 : 0; one_cnt = 1; one_m = s0 < S ? 1 : K;
      } else if (n > 0 && n_in == 0) {
        one_slot = 0; one_start = st + base[S]; one_cnt = n_sel; one_m = K;
      }
      for (int s = 0; s < S; ++s) {
        int s_start = st, s_cnt = 0, m = 0;
        if (one_slot >= 0) {
          if (s == one_slot) { s_start = one_start; s_cnt = one_cnt; m = one_m; }
        } else if (n > 0) {
          s_start = st + base[s];
          s_cnt = base[s + 1] - base[s];
          // min(cnt, ceil(cnt / n_sel * K)) in float64, the reference's three operations (:100-103)
          const double ratio = (double)s_cnt / (double)n_sel;
          const double q = ceil(ratio * (double)K);
          m = q < (double)s_cnt ? (int)q : s_cnt;
        }
        seg_start[b * S + s] = s_start; seg_cnt[b * S + s] = s_cnt; seg_m[b * S + s] = m; seg_out_start[b * S + s] = out + total;
        total += m;
      }
      kp_cnt[b] = total;
    }
  }
  __syncthreads();
  int off = lane < nb ? st + base[lane] + wcnt[wid][lane] : 0;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int r = r0; r < r1; r += SV_WAVE) {
    const int v = r + lane < r1 ? sec[r + lane] : -1;
    for (int s = 0; s < nb; ++s) {
      const unsigned long long m = __ballot(v == s);
      const int o = __shfl(off, s, SV_WAVE);
      if (v == s) order[o + __popcll(m & below)] = st + r + lane;
      if (lane == s) off += __popcll(m);
    }
  }
}

extern "C" int sv_spc_select(const float* xyz, const int32_t* xyz_batch_start, const int32_t* xyz_batch_cnt, int batch, int max_n,
                             const float* rois, int num_rois, int roi_stride, float radius, int num_sectors, int32_t* sector, void* stream) {
  SV_CHECK_ARG(batch >= 0 && max_n >= 0 && num_rois >= 0 && num_rois <= SPC_MAX_ROIS && roi_stride >= 6, "spc_select: bad arguments");
  SV_CHECK_ARG(num_sectors >= 0 && num_sectors <= SPC_MAX_SECTORS, "spc_select: num_sectors must be in [0, %d]", SPC_MAX_SECTORS);
  if (batch == 0 || max_n == 0) return SV_OK;
  SV_CHECK_ARG(xyz && xyz_batch_start && xyz_batch_cnt && sector && (rois || num_rois == 0), "spc_select: null pointer");
  const float sector_size = num_sectors > 0 ? (float)(3.141592653589793 * 2 / num_sectors) : 1.f;
  dim3 grid(sv_div_up(max_n, SPC_SELECT_THREADS), batch), block(SPC_SELECT_THREADS);
  hipLaunchKernelGGL(k_spc_select, grid, block, (size_t)(num_rois > 0 ? num_rois : 1) * sizeof(float4), sv_stream(stream), xyz, xyz_batch_start,
                     xyz_batch_cnt, rois, num_rois, roi_stride, radius, num_sectors, sector_size, sector);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_spc_partition(const int32_t* sector, const float* xyz, const int32_t* xyz_batch_start, const int32_t* xyz_batch_cnt, int batch,
                                int num_keypoints, int num_sectors, int32_t* order, int32_t* seg_start, int32_t* seg_cnt, int32_t* seg_m,
                                int32_t* seg_out_start, int32_t* kp_cnt, void* stream) {
  SV_CHECK_ARG(batch >= 0 && num_keypoints >= 0, "spc_partition: bad arguments");
  SV_CHECK_ARG(num_sectors >= 0 && num_sectors <= SPC_MAX_SECTORS, "spc_partition: num_sectors must be in [0, %d]", SPC_MAX_SECTORS);
  SV_CHECK_ARG((int64_t)batch * (num_keypoints + num_sectors) < (1ll << 31), "spc_partition: batch * (num_keypoints + num_sectors) too large");
  if (batch == 0) return SV_OK;
  SV_CHECK_ARG(sector && xyz_batch_start && xyz_batch_cnt && order && seg_start && seg_cnt && seg_m && seg_out_start && kp_cnt &&
                   (xyz || num_sectors == 0), "spc_partition: null pointer");
  const float sector_size = num_sectors > 0 ? (float)(3.141592653589793 * 2 / num_sectors) : 1.f;
  hipLaunchKernelGGL(k_spc_partition, dim3(batch), dim3(SPC_PART_THREADS), 0, sv_stream(stream), sector, xyz, xyz_batch_start, xyz_batch_cnt,
                     num_keypoints, num_sectors, sector_size, num_keypoints + num_sectors, order, seg_start, seg_cnt, seg_m, seg_out_start, kp_cnt);
  SV_LAUNCH_CHECK();
  return SV_OK;
}
