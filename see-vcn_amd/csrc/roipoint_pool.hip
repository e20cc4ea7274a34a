// PointRCNN's RoI point pooling (detector3d/pcdet/ops/roipoint_pool3d/src/roipoint_pool3d_kernel.cu:38-165), redesigned: the reference allocates a
// (B, N, M) int table on every call, fills it, gives ONE THREAD per box a serial walk over every point of the scene (:63-100) and gathers in a third
// launch.  Here a workgroup owns one (scene, box): it streams the scene once in ascending order, lists the first S inside rows in LDS, and writes
// the box's S rows itself.  The result is the reference's element for element; every element of both outputs is written.
#include "box_test.h"
#include "common.h"
#include "wave.h"

constexpr int RP_THREADS = 256;
constexpr int RP_WAVES = RP_THREADS / SV_WAVE;
constexpr int RP_SUB = 4;                          // sub-chunks of RP_THREADS consecutive points per trip: one barrier pair per 1024 points
constexpr int RP_MAX_SAMPLED = 4096;               // the list of one box in LDS: 16 KB
constexpr int RP_GATHER = 8;                       // elements a thread loads before it stores them

// ------------------------------------------------------------------------------------------------
// Listing.  A trip looks at RP_SUB * 256 consecutive points; sub-chunk u gives lane t the point c0 + 256 u + t, so a wave reads 64 consecutive
// points.  Every lane tests its point (sv_pt_in_box3d); the rank of an inside point among the trip's inside points is its ballot rank in the wave
// plus the totals of the (sub-chunk, wave) pairs before it, which go through LDS.  That is the ascending row order.  The trip count depends on
// cnt, which is the same in every thread, and the walk ends as soon as S rows are listed (the reference's `break`, :85).
// Padding (:92-99): slot k >= cnt repeats slot k % cnt.
// Gather (:103-134).  The box's S rows are S * (3 + C) consecutive floats; thread t writes elements t, t + 256, ... and keeps (slot, column) of its
// element without a division.  It issues RP_GATHER loads before it stores them: a batch has only B * M workgroups, one or two per CU, so a wave
// needs several loads in flight.  canonical: the three xyz columns hold (lx, ly) as sv_pt_in_box3d leaves them and z - cz, all fp32.  An empty
// box gets zeros and flag 1.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RP_THREADS) void k_roipoint_pool(const float* __restrict__ xyz, const float* __restrict__ feat,
                                                              const float* __restrict__ boxes, int n_pts, int n_boxes, int C, int S, int canonical,
                                                              float* __restrict__ pooled, int32_t* __restrict__ empty_flag) {
  __shared__ int32_t list[RP_MAX_SAMPLED];
  __shared__ int32_t wave_cnt[RP_SUB][RP_WAVES];
  const int tid = threadIdx.x, lane = tid & (SV_WAVE - 1), wid = tid / SV_WAVE;
  const int64_t bm = (int64_t)blockIdx.y * n_boxes + blockIdx.x;
  const float* b = boxes + bm * 7;
  const float cx = b[0], cy = b[1], cz = b[2], dx = b[3], dy = b[4], dz = b[5];
  const float cosa = cosf(-b[6]), sina = sinf(-b[6]);
  const float* pts = xyz + (int64_t)blockIdx.y * n_pts * 3;

  int cnt = 0;                                                         // the same in every thread
  for (int c0 = 0; c0 < n_pts && cnt < S; c0 += RP_SUB * RP_THREADS) {
    bool in[RP_SUB];
    int rank[RP_SUB];
#pragma unroll
    for (int u = 0; u < RP_SUB; ++u) {
      const int p = c0 + u * RP_THREADS + tid;
      in[u] = false;
      if (p < n_pts) {
        float lx, ly;
        in[u] = sv_pt_in_box3d(pts[(int64_t)p * 3], pts[(int64_t)p * 3 + 1], pts[(int64_t)p * 3 + 2], cx, cy, cz, dx, dy, dz, cosa, sina, 1e-5f, lx, ly);
      }
      int total;
      rank[u] = sv_wave_ballot_rank(in[u], &total);
      if (lane == 0) wave_cnt[u][wid] = total;
    }
    __syncthreads();
    int run = cnt;
#pragma unroll
    for (int u = 0; u < RP_SUB; ++u) {
#pragma unroll
      for (int w = 0; w < RP_WAVES; ++w) {
        if (w == wid) rank[u] += run;
        run += wave_cnt[u][w];
      }
      if (in[u] && rank[u] < S) list[rank[u]] = c0 + u * RP_THREADS + tid;
    }
    cnt = run;
    __syncthreads();                                                   // wave_cnt is written again by the next trip; list is read below
  }
  cnt = min(cnt, S);
  if (tid == 0) empty_flag[bm] = cnt == 0;

  const int W = 3 + C;
  const int64_t total = (int64_t)S * W;
  float* out = pooled + bm * total;
  if (cnt == 0) {
    for (int64_t e = tid; e < total; e += RP_THREADS) out[e] = 0.f;
    return;
  }
  if (cnt < S) {
    for (int k = cnt + tid; k < S; k += RP_THREADS) list[k] = list[k % cnt];
    __syncthreads();
  }
  const float* f = feat + (int64_t)blockIdx.y * n_pts * C;
  const int step_s = RP_THREADS / W, step_j = RP_THREADS % W;
  int s = tid / W, j = tid % W;
  for (int64_t e0 = tid; e0 < total; e0 += RP_THREADS * RP_GATHER) {   // RP_GATHER independent loads in flight per thread, then their stores
    float v[RP_GATHER];
#pragma unroll
    for (int u = 0; u < RP_GATHER; ++u) {
      v[u] = 0.f;
      if (e0 + (int64_t)u * RP_THREADS < total) {
        const int64_t p = list[s];
        if (j >= 3) {
          v[u] = f[p * C + (j - 3)];
        } else if (!canonical) {
          v[u] = pts[p * 3 + j];
        } else {
          const float z = pts[p * 3 + 2];
          float lx = 0.f, ly = 0.f;
          (void)sv_pt_in_box3d(pts[p * 3], pts[p * 3 + 1], z, cx, cy, cz, dx, dy, dz, cosa, sina, 1e-5f, lx, ly);
          v[u] = j == 0 ? lx : j == 1 ? ly : z - cz;
        }
      }
      s += step_s;
      j += step_j;
      if (j >= W) {
        j -= W;
        ++s;
      }
    }
#pragma unroll
    for (int u = 0; u < RP_GATHER; ++u)
      if (e0 + (int64_t)u * RP_THREADS < total) out[e0 + (int64_t)u * RP_THREADS] = v[u];
  }
}

extern "C" int sv_roipoint_pool3d(const float* xyz, const float* pts_feature, const float* boxes3d, int batch, int n_pts, int n_boxes, int C,
                                  int n_sampled, int canonical, float* pooled, int32_t* empty_flag, void* stream) {
  SV_CHECK_ARG(batch >= 0 && n_pts >= 0 && n_boxes >= 0 && C >= 0, "roipoint_pool3d: negative size");
  SV_CHECK_ARG(n_sampled >= 1 && n_sampled <= RP_MAX_SAMPLED, "roipoint_pool3d: n_sampled %d must lie in 1..%d", n_sampled, RP_MAX_SAMPLED);
  SV_CHECK_ARG(canonical == 0 || canonical == 1, "roipoint_pool3d: canonical %d is neither 0 nor 1", canonical);
  SV_CHECK_ARG(batch <= 65535, "roipoint_pool3d: batch %d, at most 65535", batch);
  if (batch == 0 || n_boxes == 0) return SV_OK;
  SV_CHECK_ARG(boxes3d && pooled && empty_flag && (n_pts == 0 || (xyz && (C == 0 || pts_feature))), "roipoint_pool3d: null pointer");
  SV_CHECK_ARG(sv_on_device(boxes3d) && sv_on_device(pooled) && sv_on_device(empty_flag) &&
                   (n_pts == 0 || (sv_on_device(xyz) && (C == 0 || sv_on_device(pts_feature)))),
               "roipoint_pool3d: a pointer is not device memory");
  hipLaunchKernelGGL(k_roipoint_pool, dim3(n_boxes, batch), dim3(RP_THREADS), 0, sv_stream(stream), xyz, pts_feature, boxes3d, n_pts, n_boxes, C,
                     n_sampled, canonical, pooled, empty_flag);
  SV_LAUNCH_CHECK();
  return SV_OK;
}
