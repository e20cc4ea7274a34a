// The VC training transforms on the device (reference: see/surface_completion/models/vcn/datasets/data_transforms.py).  Objects are stacked:
// points (sum N, 3) fp32 with start / cnt (B) int32.  Every ring transform there is a selection of input rows in input order (its spherical round
// trip moves a float64 component by about 1e-15 r, which no float32 cast sees unless |c| < 2^-24 r), so the kernels here compute ring indices,
// copy rows and apply the point-wise arithmetic; every random draw is made on the host, from the integer table sv_vc_rings returns.
// Integer atomics in LDS only, no float atomics: equal bits run to run.
#include "common.h"
#include "wave.h"

#define VC_THREADS 256
#define VC_WAVES (VC_THREADS / SV_WAVE)
#define VC_RMAX SV_VC_MAX_RINGS
#define VC_PLAN SV_VC_PLAN_WORDS

// cart2sph's elevation (utils/misc.py:284): arctan2(norm(xy), z) of float64 rows; numpy rounds the two products and their sum one by one
// (the library is built with -ffp-contract=off).
__device__ __forceinline__ double vc_elevation(const float* __restrict__ q) {
  const double x = q[0], y = q[1], z = q[2];
  return atan2(sqrt(x * x + y * y), z);
}

// np.linspace(lo, hi, nb + 1)[k]: k * step + lo with the last edge set to hi
__device__ __forceinline__ double vc_edge(int k, int nb, double lo, double hi, double step) { return k == nb ? hi : (double)k * step + lo; }

// np.histogram's bin of e over nb equal bins on [lo, hi] (lo < hi): the b with edge(b) <= e < edge(b + 1), the last bin closed.  The same guess
// and the same two corrections as numpy makes.
__device__ __forceinline__ int vc_bin(double e, int nb, double lo, double hi, double step) {
  int k = (int)(((e - lo) / (hi - lo)) * (double)nb);
  if (k >= nb) k = nb - 1;
  if (k < 0) k = 0;
  if (k > 0 && e < vc_edge(k, nb, lo, hi, step)) --k;
  if (k != nb - 1 && e >= vc_edge(k + 1, nb, lo, hi, step)) ++k;
  return k;
}

// ------------------------------------------------------------------ ring indices (data_transforms.py:131-133, 162-164)
// One workgroup per object: elevations and their min / max, the histogram in LDS, the rank of every non-empty bin, the ring index per point.
__global__ __launch_bounds__(VC_THREADS) void k_vc_rings(const float* __restrict__ points, const int32_t* __restrict__ start,
                                                         const int32_t* __restrict__ cnt, int fixed_bins, int min_in_pts,
                                                         int32_t* __restrict__ ring, int32_t* __restrict__ num_rings,
                                                         int32_t* __restrict__ ring_cnt, double* __restrict__ elev) {
  __shared__ int32_t hist[VC_RMAX];       // points per bin, then per ring
  __shared__ int32_t rank[VC_RMAX];       // 1-based rank of a non-empty bin among the non-empty bins
  __shared__ int32_t by_ring[VC_RMAX];
  __shared__ double red[2 * VC_WAVES];
  __shared__ int32_t wave_sums[VC_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x, n = cnt[b];
  const int64_t s = start[b];
  int32_t* out_cnt = ring_cnt + (int64_t)b * VC_RMAX;
  if (n < min_in_pts || n < 1) {                    // the reference returns pts before it looks at them
    for (int k = tid; k < VC_RMAX; k += VC_THREADS) out_cnt[k] = 0;
    for (int i = tid; i < n; i += VC_THREADS) ring[s + i] = 0;
    if (tid == 0) num_rings[b] = 0;
    return;
  }
  for (int k = tid; k < VC_RMAX; k += VC_THREADS) hist[k] = 0, by_ring[k] = 0;
  double lo = 1e300, hi = -1e300;
  for (int i = tid; i < n; i += VC_THREADS) {
    const double e = vc_elevation(points + (s + i) * 3);
    if (elev) elev[s + i] = e;
    lo = sv_min2(lo, e), hi = sv_max2(hi, e);
  }
  lo = sv_wave_reduce_min(lo), hi = sv_wave_reduce_max(hi);
  if ((tid & (SV_WAVE - 1)) == 0) red[tid / SV_WAVE] = lo, red[VC_WAVES + tid / SV_WAVE] = hi;
  __syncthreads();                                  // also orders the zeroed histogram before the atomics
#pragma unroll
  for (int w = 0; w < VC_WAVES; ++w) lo = sv_min2(lo, red[w]), hi = sv_max2(hi, red[VC_WAVES + w]);
  if (!(lo < hi)) {                                 // all elevations equal: one non-empty bin whatever the bin count
    for (int k = tid; k < VC_RMAX; k += VC_THREADS) out_cnt[k] = k == 0 ? n : 0;
    for (int i = tid; i < n; i += VC_THREADS) ring[s + i] = 1;
    if (tid == 0) num_rings[b] = 1;
    return;
  }
  // bins = 'sqrt': width = ptp / sqrt(n) and ceil(ptp / width) bins, in numpy's float64 steps (a square n can give sqrt(n) + 1 bins)
  int nb = fixed_bins > 0 ? fixed_bins : (int)ceil((hi - lo) / ((hi - lo) / sqrt((double)n)));
  nb = nb < 1 ? 1 : (nb > VC_RMAX ? VC_RMAX : nb);
  const double step = (hi - lo) / (double)nb;
  for (int i = tid; i < n; i += VC_THREADS) {
    const double e = elev ? elev[s + i] : vc_elevation(points + (s + i) * 3);
    const int k = vc_bin(e, nb, lo, hi, step);
    atomicAdd(&hist[k], 1);
    ring[s + i] = k;                                // the bin for now; this thread reads it back below
  }
  __syncthreads();
  // rank scan over the bins: VC_RMAX / VC_THREADS consecutive bins a thread
  constexpr int PER = VC_RMAX / VC_THREADS;
  int mine = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) mine += hist[tid * PER + j] > 0;
  int total;
  int r = sv_block_excl_scan<VC_THREADS>(mine, &total, wave_sums);
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int c = hist[tid * PER + j];
    if (c > 0) {
      rank[tid * PER + j] = r + 1;
      by_ring[r] = c;
      ++r;
    }
  }
  __syncthreads();
  for (int k = tid; k < VC_RMAX; k += VC_THREADS) out_cnt[k] = by_ring[k];
  for (int i = tid; i < n; i += VC_THREADS) ring[s + i] = rank[ring[s + i]];
  if (tid == 0) num_rings[b] = total;
}

extern "C" int sv_vc_rings(const float* points, const int32_t* start, const int32_t* cnt, int batch, int fixed_bins, int min_in_pts, int32_t* ring,
                           int32_t* num_rings, int32_t* ring_cnt, double* elevation, void* stream) {
  SV_CHECK_ARG(batch >= 0 && fixed_bins >= 0 && fixed_bins <= VC_RMAX && min_in_pts >= 0, "vc_rings: bad arguments");
  if (batch == 0) return SV_OK;
  SV_CHECK_ARG(points && start && cnt && ring && num_rings && ring_cnt, "vc_rings: null pointer");
  hipLaunchKernelGGL(k_vc_rings, dim3(batch), dim3(VC_THREADS), 0, sv_stream(stream), points, start, cnt, fixed_bins, min_in_pts, ring, num_rings,
                     ring_cnt, elevation);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ------------------------------------------------------------------ selection (data_transforms.py:63-73, 134-138, 171-194)
// sph_pts[mask][first::step] per object, in input order.  plan row (VC_PLAN int32): 0 pass-through, 1 use the ring bitmask, 2 use the per-point keep
// bytes, 3 first, 4 step, 5 out_start, 6 out_len, 7 unused, 8.. the bitmask of chosen rings (bit r - 1 of ring r).  The position of a kept row is a
// function of its rank among the kept rows, so one scan serves; rows beyond out_len (a plan that does not fit its table) are not written.
__global__ __launch_bounds__(VC_THREADS) void k_vc_select(const float* __restrict__ points, const int32_t* __restrict__ start,
                                                          const int32_t* __restrict__ cnt, const int32_t* __restrict__ ring,
                                                          const uint8_t* __restrict__ keep, const int32_t* __restrict__ plan,
                                                          float* __restrict__ out) {
  __shared__ uint32_t bits[VC_RMAX / 32];
  __shared__ int32_t wave_sums[VC_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x, n = cnt[b];
  const int64_t s = start[b];
  const int32_t* pl = plan + (int64_t)b * VC_PLAN;
  const bool pass = pl[0] != 0, use_rings = pl[1] != 0 && ring, use_keep = pl[2] != 0 && keep;
  const int first = pl[3] < 0 ? 0 : pl[3], step = pl[4] < 1 ? 1 : pl[4], out_len = pl[6];
  float* dst = out + (int64_t)pl[5] * 3;
  if (pass) {
    const int m = n < out_len ? n : out_len;
    for (int i = tid; i < m * 3; i += VC_THREADS) dst[i] = points[s * 3 + i];
    return;
  }
  if (tid < VC_RMAX / 32) bits[tid] = (uint32_t)pl[8 + tid];
  __syncthreads();
  int base = 0;
  for (int i0 = 0; i0 < n; i0 += VC_THREADS) {
    const int i = i0 + tid;
    bool flag = i < n;
    if (flag && use_rings) {
      const int r = ring[s + i] - 1;
      flag = r >= 0 && r < VC_RMAX && ((bits[r >> 5] >> (r & 31)) & 1u);
    }
    if (flag && use_keep) flag = keep[s + i] != 0;
    int total;
    const int k = base + sv_block_excl_scan<VC_THREADS>((int)flag, &total, wave_sums) - first;
    if (flag && k >= 0 && k % step == 0 && k / step < out_len) {
      const float* q = points + (s + i) * 3;
      float* o = dst + (int64_t)(k / step) * 3;
      o[0] = q[0], o[1] = q[1], o[2] = q[2];
    }
    base += total;
    __syncthreads();                                // wave_sums is written again in the next round
  }
}

extern "C" int sv_vc_select(const float* points, const int32_t* start, const int32_t* cnt, int batch, const int32_t* ring, const uint8_t* keep,
                            const int32_t* plan, float* out, void* stream) {
  SV_CHECK_ARG(batch >= 0, "vc_select: bad arguments");
  if (batch == 0) return SV_OK;
  SV_CHECK_ARG(points && start && cnt && plan && out, "vc_select: null pointer");
  hipLaunchKernelGGL(k_vc_select, dim3(batch), dim3(VC_THREADS), 0, sv_stream(stream), points, start, cnt, ring, keep, plan, out);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ------------------------------------------------------------------ ResamplePoints (data_transforms.py:254-262)
// tiled[choice[:n_points]] with tiled[i] = pts[i % len(pts)]: out[b, j] = points[start_b + index[b, j] % cnt_b].
__global__ __launch_bounds__(VC_THREADS) void k_vc_resample(const float* __restrict__ points, const int32_t* __restrict__ start,
                                                            const int32_t* __restrict__ cnt, const int32_t* __restrict__ index, int n_points,
                                                            float* __restrict__ out) {
  const int b = blockIdx.y, j = blockIdx.x * VC_THREADS + threadIdx.x, n = cnt[b];
  if (j >= n_points) return;
  float* o = out + ((int64_t)b * n_points + j) * 3;
  if (n < 1) {
    o[0] = o[1] = o[2] = 0.f;
    return;
  }
  int k = index[(int64_t)b * n_points + j] % n;
  if (k < 0) k += n;
  const float* q = points + ((int64_t)start[b] + k) * 3;
  o[0] = q[0], o[1] = q[1], o[2] = q[2];
}

extern "C" int sv_vc_resample(const float* points, const int32_t* start, const int32_t* cnt, int batch, const int32_t* index, int n_points, float* out,
                              void* stream) {
  SV_CHECK_ARG(batch >= 0 && batch <= 65535 && n_points >= 0, "vc_resample: bad arguments or batch > 65535");
  if (batch == 0 || n_points == 0) return SV_OK;
  SV_CHECK_ARG(points && start && cnt && index && out, "vc_resample: null pointer");
  hipLaunchKernelGGL(k_vc_resample, dim3(sv_div_up(n_points, VC_THREADS), batch), dim3(VC_THREADS), 0, sv_stream(stream), points, start, cnt, index,
                     n_points, out);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ------------------------------------------------------------------ Jitter and AddGNSpherical (data_transforms.py:214-217, 232-245)
// mode 0: p + noise, noise (total, 3) fp64.  mode 1: sph2cart of (r + noise, azimuth, elevation) = p * ((r + noise) / r), noise (total) fp64; r == 0
// has azimuth = elevation = 0 there, which gives (0, 0, noise).  Float64 arithmetic, one rounding to fp32.
__global__ __launch_bounds__(VC_THREADS) void k_vc_pointwise(float* __restrict__ points, int64_t total, const double* __restrict__ noise, int mode) {
  for (int64_t i = (int64_t)blockIdx.x * VC_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * VC_THREADS) {
    float* q = points + i * 3;
    const double x = q[0], y = q[1], z = q[2];
    double ox, oy, oz;
    if (mode == 0) {
      ox = x + noise[i * 3], oy = y + noise[i * 3 + 1], oz = z + noise[i * 3 + 2];
    } else {
      const double r = sqrt((x * x + y * y) + z * z), nz = noise[i];
      if (r == 0.0) {
        ox = 0.0, oy = 0.0, oz = nz;
      } else {
        const double f = (r + nz) / r;
        ox = x * f, oy = y * f, oz = z * f;
      }
    }
    q[0] = (float)ox, q[1] = (float)oy, q[2] = (float)oz;
  }
}

extern "C" int sv_vc_pointwise(float* points, int64_t total, const double* noise, int mode, void* stream) {
  SV_CHECK_ARG(total >= 0 && (mode == 0 || mode == 1), "vc_pointwise: bad arguments");
  if (total == 0) return SV_OK;
  SV_CHECK_ARG(points && noise, "vc_pointwise: null pointer");
  hipLaunchKernelGGL(k_vc_pointwise, dim3(sv_grid_1d(total, VC_THREADS)), dim3(VC_THREADS), 0, sv_stream(stream), points, total, noise, mode);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ------------------------------------------------------------------ RandomObjectScaling (data_transforms.py:302-316)
// params (batch, 8) fp64: enable, the box centre, its heading, the three scale factors.  The reference's steps with their number formats: p - centre
// in float64, cast to fp32; the fp32 rotation by -heading (utils/transform.py:33-58); the float64 product with the scale, cast to fp32; the fp32
// rotation by +heading; + centre in float64.
__global__ __launch_bounds__(VC_THREADS) void k_vc_object_scale(float* __restrict__ points, const int32_t* __restrict__ start,
                                                                const int32_t* __restrict__ cnt, const double* __restrict__ params) {
  const int b = blockIdx.y, i = blockIdx.x * VC_THREADS + threadIdx.x;
  const double* pr = params + (int64_t)b * 8;
  if (i >= cnt[b] || pr[0] == 0.0) return;
  float* q = points + ((int64_t)start[b] + i) * 3;
  const float x0 = (float)((double)q[0] - pr[1]), y0 = (float)((double)q[1] - pr[2]), z0 = (float)((double)q[2] - pr[3]);
  const float a = (float)(-pr[4]), c0 = cosf(a), s0 = sinf(a);
  const float x1 = x0 * c0 + y0 * (-s0), y1 = x0 * s0 + y0 * c0;
  const float x2 = (float)((double)x1 * pr[5]), y2 = (float)((double)y1 * pr[6]), z2 = (float)((double)z0 * pr[7]);
  const float h = (float)pr[4], c1 = cosf(h), s1 = sinf(h);
  const float x3 = x2 * c1 + y2 * (-s1), y3 = x2 * s1 + y2 * c1;
  q[0] = (float)((double)x3 + pr[1]), q[1] = (float)((double)y3 + pr[2]), q[2] = (float)((double)z2 + pr[3]);
}

extern "C" int sv_vc_object_scale(float* points, const int32_t* start, const int32_t* cnt, int batch, int max_points, const double* params,
                                  void* stream) {
  SV_CHECK_ARG(batch >= 0 && batch <= 65535 && max_points >= 0, "vc_object_scale: bad arguments or batch > 65535");
  if (batch == 0 || max_points == 0) return SV_OK;
  SV_CHECK_ARG(points && start && cnt && params, "vc_object_scale: null pointer");
  hipLaunchKernelGGL(k_vc_object_scale, dim3(sv_div_up(max_points, VC_THREADS), batch), dim3(VC_THREADS), 0, sv_stream(stream), points, start, cnt,
                     params);
  SV_LAUNCH_CHECK();
  return SV_OK;
}
