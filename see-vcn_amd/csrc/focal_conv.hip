// Focal sparse convolution: the learned, data-dependent dilation of the active set between submanifold layers.
//
// Replaces the reference's per-scene Python loops -- focal_sparse_utils.py:89-147 (split_voxels), :39-86 (sort_by_indices, check_repeat) and
// focal_sparse_conv.py:171-197 (combine_out): sort, boolean indexing, repeat, cat, unique_consecutive, index_add_ and scatter_ per scene and
// layer -- by a selection, a mark / count / emit pass over the coordinate index (common.h) and two gathers through the submanifold table
// nbr[k][row] of the INPUT set that conv_imp builds anyway.  No float atomics; every sum has a fixed order.
//
//   s (n, 27) = sigmoid(imps): column 26 is the voxel importance mv, column o < 26 the importance of kernel_offsets[o] (focal_sparse_conv.py:43-44:
//   (dz, dy, dx) in range(-1, 2)^3, z slowest, centre removed), i.e. the 27-offset index k(o) = o for o < 13, else o + 1.
//   1. foreground: topk -- per scene the int(n_b * threshold) rows of largest mv (focal_sparse_utils.py:113-115; equal values: lower row first, where
//      the reference's unstable sort leaves the choice open); else mv > threshold (:117).
//   2. candidates: foreground row j, offset o with s[j, o] >= threshold (:124) -> cell coords[j] + offset[o], kept iff 0 < c < dim on every axis
//      (:130-131; the reference's `> 0` drops coordinate 0 for candidates, kept here).
//   3. output set: input cells and kept candidate cells, each once, ascending ((b*Z + z)*Y + y)*X + x.
//   4. features: a new cell gets 0; input row i gets f[i] * (mv[i] if mask_multi) * w[i], w[i] = (1 + sum s[j, o]) / (1 + c_i) over the c_i kept
//      candidates landing on a foreground i (check_repeat's mean of mask_kernel, :83-85), 1 for background rows and under skip_mask_kernel.
//
// Divergences from the reference.  (a) Its sort_by_indices / check_repeat key cells by z*max(y)*max(x) + y*max(x) + x with the maxima of the set
// at hand (:48, :71), which is not injective once a voxel has y = 0 or x = 0 -- (z, y, max x) and (z, y + 1, 0) collide and distinct voxels are
// merged, their features summed.  The true linear key is used here; the two agree wherever the reference's key is injective.  (b) The reference
// raises on a scene without voxels (max() of an empty tensor); such a scene contributes nothing here.
#include "common.h"
#include "wave.h"

constexpr int FC_THREADS = 256;
constexpr int FC_K = 27;          // columns of s: 26 kernel importances + the voxel importance
constexpr int FC_MV = 26;
constexpr int FC_MAX_BATCH = 1024;

struct FocalGeom {
  int batch;
  int shape[3];   // Z, Y, X
};

__device__ __forceinline__ int64_t fc_key(int b, int z, int y, int x, const FocalGeom& g) {
  return (((int64_t)b * g.shape[0] + z) * g.shape[1] + y) * g.shape[2] + x;
}
__device__ __forceinline__ bool fc_coord_ok(const int4 c, const FocalGeom& g) {
  return c.x >= 0 && c.x < g.batch && c.y >= 0 && c.y < g.shape[0] && c.z >= 0 && c.z < g.shape[1] && c.w >= 0 && c.w < g.shape[2];
}
// kernel_offsets[o] of the reference as (dz, dy, dx)
__device__ __forceinline__ void fc_offset(int o, int& dz, int& dy, int& dx) {
  const int k = o < 13 ? o : o + 1;
  dz = k / 9 - 1; dy = (k / 3) % 3 - 1; dx = k % 3 - 1;
}
// the candidate cell of (c, o) or false: focal_sparse_utils.py:130-131, strictly inside (0, dim) on every axis
__device__ __forceinline__ bool fc_candidate(const int4 c, int o, const FocalGeom& g, int& z, int& y, int& x) {
  int dz, dy, dx;
  fc_offset(o, dz, dy, dx);
  z = c.y + dz; y = c.z + dy; x = c.w + dx;
  return z > 0 && y > 0 && x > 0 && z < g.shape[0] && y < g.shape[1] && x < g.shape[2];
}

// ------------------------------------------------------------------------------------------------ 1. selection
// Order-preserving bits of an fp32 value: a larger float has a larger key.
__device__ __forceinline__ uint32_t fc_float_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(FC_THREADS) void k_focal_select_threshold(const float* __restrict__ s, const int4* __restrict__ coords, int64_t n, int batch,
                                                                       float thr, uint8_t* __restrict__ fore) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int b = coords[i].x;
    fore[i] = (b >= 0 && b < batch && s[i * FC_K + FC_MV] > thr) ? 1 : 0;
  }
}

// Radix select, 8-bit digits from the top.  hist[(pass * batch + b) * 256 + d] counts scene b's rows whose key agrees with the digits chosen so far
// and has digit d next; pass 0's counts add up to n_b, so the scene sizes need no pass of their own.
struct SelState {
  uint32_t prefix;    // the digits chosen so far (after 4 passes: the key of the k_b-th largest value)
  int32_t krem;       // rows still to take among those that agree with prefix; 0: the scene takes none
  int32_t last;       // rows in the last chosen bin (after 4 passes: rows equal to the boundary value)
};

// One WAVE (all 64 lanes active) replays the first `npass` digit choices of scene b from the histograms.
__device__ __forceinline__ SelState fc_select_state(const int32_t* __restrict__ hist, int batch, int b, int npass, double threshold) {
  const int lane = threadIdx.x & 63;
  SelState st{0u, 0, 0};
  for (int q = 0; q < npass; ++q) {
    const int32_t* h = hist + ((int64_t)q * batch + b) * 256;
    int v[4];
    int sum = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) { v[t] = h[255 - 4 * lane - t]; sum += v[t]; }      // lane 0 holds the four largest digits
    const int incl = sv_wave_incl_scan(sum);
    if (q == 0) {
      const int nb = __shfl(incl, 63);
      // int(n_b * threshold) with the product formed in float64, as Python forms it (focal_sparse_utils.py:114)
      const double want = (double)nb * threshold;
      long long k = want >= (double)nb ? (long long)nb : (long long)want;
      if (k < 0) k = 0;
      st.krem = (int32_t)k;
    }
    if (st.krem <= 0) return SelState{0u, 0, 0};
    const int first = sv_wave_ballot_first(incl >= st.krem);          // exists: krem <= rows agreeing with prefix
    int digit = 0, rem = 0, last = 0;
    if (lane == first) {
      int before = incl - sum;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (before + v[t] >= st.krem) { digit = 255 - 4 * lane - t; rem = st.krem - before; last = v[t]; break; }
        before += v[t];
      }
    }
    digit = __shfl(digit, first); rem = __shfl(rem, first); last = __shfl(last, first);
    st.prefix = (st.prefix << 8) | (uint32_t)digit;
    st.krem = rem;
    st.last = last;
  }
  return st;
}

template <int PASS>
__global__ __launch_bounds__(FC_THREADS) void k_focal_select_hist(const float* __restrict__ s, const int4* __restrict__ coords, int64_t n, int batch,
                                                                  double threshold, int32_t* __restrict__ hist) {
  extern __shared__ uint32_t sel_lds[];          // [batch] prefix | [batch] krem
  uint32_t* prefix = sel_lds;
  int32_t* krem = reinterpret_cast<int32_t*>(sel_lds + batch);
  if (PASS > 0) {
    for (int b = threadIdx.x >> 6; b < batch; b += FC_THREADS / 64) {
      const SelState st = fc_select_state(hist, batch, b, PASS, threshold);
      if ((threadIdx.x & 63) == 0) { prefix[b] = st.prefix; krem[b] = st.krem; }
    }
    __syncthreads();
  }
  int32_t* out = hist + (int64_t)PASS * batch * 256;
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t n_up = (n + 63) / 64 * 64;       // whole waves stay in the loop: the ballots below need every lane
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_up; i += stride) {
    bool todo = false;
    uint32_t tag = 0;
    if (i < n) {
      const int b = coords[i].x;
      if (b >= 0 && b < batch) {
        const uint32_t key = fc_float_key(s[i * FC_K + FC_MV]);
        todo = PASS == 0 || (krem[b] > 0 && (key >> ((32 - 8 * PASS) & 31)) == prefix[b]);
        tag = (uint32_t)b * 256u + ((key >> (24 - 8 * PASS)) & 255u);
      }
    }
    // one atomic per distinct (scene, digit) in the wave: importances of one scene crowd into a few top digits
    unsigned long long m = __ballot(todo);
    while (m) {
      const int leader = __ffsll((long long)m) - 1;
      const uint32_t ltag = __shfl(tag, leader);
      const bool same = todo && tag == ltag;
      const unsigned long long sm = __ballot(same);
      if (lane == leader) atomicAdd(&out[ltag], (int32_t)__popcll(sm));
      if (same) todo = false;
      m &= ~sm;
    }
  }
}

// fore[i] from the finished selection; tie_info[b] = {boundary key, ties to take, 1 when only SOME of the rows equal to the boundary value are taken}
__global__ __launch_bounds__(FC_THREADS) void k_focal_select_write(const float* __restrict__ s, const int4* __restrict__ coords, int64_t n, int batch,
                                                                   double threshold, const int32_t* __restrict__ hist, uint8_t* __restrict__ fore,
                                                                   int32_t* __restrict__ tie_info) {
  extern __shared__ uint32_t sel_lds[];          // [batch] boundary key | [batch] krem | [batch] rows equal to the boundary
  uint32_t* bound = sel_lds;
  int32_t* krem = reinterpret_cast<int32_t*>(sel_lds + batch);
  int32_t* equal = reinterpret_cast<int32_t*>(sel_lds + 2 * batch);
  for (int b = threadIdx.x >> 6; b < batch; b += FC_THREADS / 64) {
    const SelState st = fc_select_state(hist, batch, b, 4, threshold);
    if ((threadIdx.x & 63) == 0) {
      bound[b] = st.prefix; krem[b] = st.krem; equal[b] = st.last;
      if (blockIdx.x == 0) {
        tie_info[3 * b] = (int32_t)st.prefix;
        tie_info[3 * b + 1] = st.krem;
        tie_info[3 * b + 2] = (st.krem > 0 && st.krem < st.last) ? 1 : 0;
      }
    }
  }
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int b = coords[i].x;
    uint8_t f = 0;
    if (b >= 0 && b < batch && krem[b] > 0) {
      const uint32_t key = fc_float_key(s[i * FC_K + FC_MV]);
      f = key > bound[b] || (key == bound[b] && krem[b] == equal[b]);
    }
    fore[i] = f;
  }
}

// Scenes that take only some of the rows equal to the boundary value: the first krem of them in row order.  One workgroup per scene walks the rows
// in order; the others leave at once.
__global__ __launch_bounds__(FC_THREADS) void k_focal_select_ties(const float* __restrict__ s, const int4* __restrict__ coords, int64_t n,
                                                                  const int32_t* __restrict__ tie_info, uint8_t* __restrict__ fore) {
  const int b = blockIdx.x;
  if (!tie_info[3 * b + 2]) return;
  const uint32_t bound = (uint32_t)tie_info[3 * b];
  const int krem = tie_info[3 * b + 1];
  __shared__ int wsum[FC_THREADS / SV_WAVE];
  int taken = 0;
  for (int64_t base = 0; base < n && taken < krem; base += FC_THREADS) {
    const int64_t i = base + threadIdx.x;
    const bool tie = i < n && coords[i].x == b && fc_float_key(s[i * FC_K + FC_MV]) == bound;
    int tot;
    const int before = sv_block_excl_scan<FC_THREADS>((int)tie, &tot, wsum);
    if (tie && taken + before < krem) fore[i] = 1;
    taken += tot;
    __syncthreads();                             // wsum is written again in the next round
  }
}

extern "C" size_t sv_focal_select_scratch_bytes(int batch) {
  const size_t b = batch > 0 ? (size_t)batch : 1;
  return b * 4 * 256 * sizeof(int32_t) + b * 3 * sizeof(int32_t);
}

extern "C" int sv_focal_select(const float* s, const int32_t* coords, int64_t n, int batch, int topk, double threshold, void* scratch,
                               uint8_t* fore, void* stream) {
  SV_CHECK_ARG(n >= 0 && batch > 0 && batch <= FC_MAX_BATCH, "focal_select: bad arguments (batch 1..%d)", FC_MAX_BATCH);
  SV_CHECK_ARG(threshold == threshold, "focal_select: threshold is NaN");
  if (n == 0) return SV_OK;
  SV_CHECK_ARG(s && coords && fore, "focal_select: null pointer");
  SV_CHECK_ARG(sv_on_device(s) && sv_on_device(coords) && sv_on_device(fore), "focal_select: host pointer");
  hipStream_t st = sv_stream(stream);
  const int4* c4 = reinterpret_cast<const int4*>(coords);
  const int grid = sv_grid_1d(n, FC_THREADS);
  if (!topk) {
    hipLaunchKernelGGL(k_focal_select_threshold, dim3(grid), dim3(FC_THREADS), 0, st, s, c4, n, batch, (float)threshold, fore);
    SV_LAUNCH_CHECK();
    return SV_OK;
  }
  SV_CHECK_ARG(threshold >= 0.0, "focal_select: top-k needs a threshold >= 0");
  SV_CHECK_ARG(scratch && sv_on_device(scratch), "focal_select: scratch");
  int32_t* hist = reinterpret_cast<int32_t*>(scratch);
  int32_t* tie_info = hist + (size_t)batch * 4 * 256;
  SV_HIP(hipMemsetAsync(hist, 0, (size_t)batch * 4 * 256 * sizeof(int32_t), st));
  const size_t lds2 = (size_t)batch * 2 * sizeof(uint32_t), lds3 = (size_t)batch * 3 * sizeof(uint32_t);
  hipLaunchKernelGGL(k_focal_select_hist<0>, dim3(grid), dim3(FC_THREADS), lds2, st, s, c4, n, batch, threshold, hist);
  hipLaunchKernelGGL(k_focal_select_hist<1>, dim3(grid), dim3(FC_THREADS), lds2, st, s, c4, n, batch, threshold, hist);
  hipLaunchKernelGGL(k_focal_select_hist<2>, dim3(grid), dim3(FC_THREADS), lds2, st, s, c4, n, batch, threshold, hist);
  hipLaunchKernelGGL(k_focal_select_hist<3>, dim3(grid), dim3(FC_THREADS), lds2, st, s, c4, n, batch, threshold, hist);
  hipLaunchKernelGGL(k_focal_select_write, dim3(grid), dim3(FC_THREADS), lds3, st, s, c4, n, batch, threshold, hist, fore, tie_info);
  hipLaunchKernelGGL(k_focal_select_ties, dim3(batch), dim3(FC_THREADS), 0, st, s, c4, n, tie_info, fore);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ------------------------------------------------------------------------------------------------ 2. + 3. mark, count, emit
// One thread per (row, column of s): column 26 stands for the row's own cell, column o < 26 for its candidate.  PHASE 0 marks the cells in the
// coordinate index, 1 (after scan and prefix) writes out_coords[rank] and row_of_in, 2 returns the touched words to zero.
template <int PHASE>
__global__ __launch_bounds__(FC_THREADS) void k_focal_cells(const int4* __restrict__ coords, const float* __restrict__ s, const uint8_t* __restrict__ fore,
                                                            int64_t n, FocalGeom g, float thr, SvIndexView ix, int4* __restrict__ out_coords,
                                                            int32_t* __restrict__ row_of_in, int64_t capacity) {
  const int64_t total = n * FC_K;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = idx / FC_K;
    const int o = (int)(idx - i * FC_K);
    const int4 c = coords[i];
    const bool ok = fc_coord_ok(c, g);
    int z = c.y, y = c.z, x = c.w;
    bool hit = ok;
    if (o != FC_MV) hit = ok && fore[i] && s[idx] >= thr && fc_candidate(c, o, g, z, y, x);
    if (hit) {
      const int64_t key = fc_key(c.x, z, y, x, g);
      if (PHASE == 0) {
        sv_index_mark(ix, key);
      } else if (PHASE == 1) {
        int32_t r = sv_index_lookup(ix, key);
        if (r >= capacity) r = -1;
        if (r >= 0) out_coords[r] = make_int4(c.x, z, y, x);        // identical value from every contributor
        if (o == FC_MV) row_of_in[i] = r;
      } else {
        ix.words[key >> 5] = make_uint2(0u, 0u);
        ix.chunk_cnt[key >> SV_CHUNK_SHIFT] = 0;
      }
    } else if (PHASE == 1 && o == FC_MV) {
      row_of_in[i] = -1;
    }
  }
}

static size_t fc_align256(size_t x) { return (x + 255) / 256 * 256; }

extern "C" size_t sv_focal_expand_scratch_bytes(int64_t ncells) { return fc_align256(sv_index_scan_tmp_bytes(ncells)) + 256; }

extern "C" int sv_focal_expand(const int32_t* coords, const float* s, const uint8_t* fore, int64_t n, int batch, const int32_t* shape_host,
                               double threshold, void* index_ws, void* scratch, int32_t* out_coords, int32_t* row_of_in, int64_t capacity,
                               int32_t* num_out, void* stream) {
  SV_CHECK_ARG(n >= 0 && batch > 0 && capacity >= 0 && shape_host && num_out, "focal_expand: bad arguments");
  SV_CHECK_ARG(shape_host[0] > 0 && shape_host[1] > 0 && shape_host[2] > 0, "focal_expand: bad grid");
  hipStream_t st = sv_stream(stream);
  if (n == 0) {
    SV_HIP(hipMemsetAsync(num_out, 0, 4, st));
    return SV_OK;
  }
  SV_CHECK_ARG(coords && s && fore && index_ws && scratch && row_of_in && (out_coords || capacity == 0), "focal_expand: null pointer");
  SV_CHECK_ARG(sv_on_device(coords) && sv_on_device(s) && sv_on_device(fore) && sv_on_device(row_of_in) && sv_on_device(num_out),
               "focal_expand: host pointer");
  FocalGeom g{batch, {shape_host[0], shape_host[1], shape_host[2]}};
  const int64_t ncells = (int64_t)batch * g.shape[0] * g.shape[1] * g.shape[2];
  SvIndexView ix = sv_index_view(index_ws, ncells);
  const int4* c4 = reinterpret_cast<const int4*>(coords);
  int4* oc4 = reinterpret_cast<int4*>(out_coords);
  const float thr = (float)threshold;
  const int grid = sv_grid_1d(n * FC_K, FC_THREADS, 256 * 16);
  hipLaunchKernelGGL(k_focal_cells<0>, dim3(grid), dim3(FC_THREADS), 0, st, c4, s, fore, n, g, thr, ix, oc4, row_of_in, capacity);
  int rc = sv_index_scan_launch(ix, num_out, scratch, st);
  if (rc) return rc;
  rc = sv_index_prefix_launch(ix, st);
  if (rc) return rc;
  hipLaunchKernelGGL(k_focal_cells<1>, dim3(grid), dim3(FC_THREADS), 0, st, c4, s, fore, n, g, thr, ix, oc4, row_of_in, capacity);
  hipLaunchKernelGGL(k_focal_cells<2>, dim3(grid), dim3(FC_THREADS), 0, st, c4, s, fore, n, g, thr, ix, oc4, row_of_in, capacity);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ------------------------------------------------------------------------------------------------ 4. weigh and place
// A candidate of row j through offset o lands on row i  <=>  coords[j] = coords[i] - offset[o]  <=>  j = nbr[26 - k(o)][i]; it was kept iff
// every spatial coordinate of i is > 0 (it is < dim already).  Offsets in ascending o, fp32.
__global__ __launch_bounds__(FC_THREADS) void k_focal_weigh(const float* __restrict__ s, const int4* __restrict__ coords, const uint8_t* __restrict__ fore,
                                                            const int32_t* __restrict__ nbr, int64_t n, int skip_mask_kernel, float thr,
                                                            float* __restrict__ w, int32_t* __restrict__ cnt) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float acc = 1.0f;
    int c = 0;
    const int4 ci = coords[i];
    if (fore[i] && !skip_mask_kernel && ci.y > 0 && ci.z > 0 && ci.w > 0) {
#pragma unroll
      for (int o = 0; o < FC_MV; ++o) {
        const int k = o < 13 ? o : o + 1;
        const int32_t j = nbr[(int64_t)(26 - k) * n + i];
        if (j >= 0 && fore[j]) {
          const float v = s[(int64_t)j * FC_K + o];
          if (v >= thr) { acc += v; ++c; }
        }
      }
    }
    w[i] = c ? acc / (float)(1 + c) : 1.0f;
    cnt[i] = c;
  }
}

__global__ __launch_bounds__(FC_THREADS) void k_focal_place(const float* __restrict__ f, const float* __restrict__ s, const int32_t* __restrict__ row_of_in,
                                                            const float* __restrict__ w, int64_t n, int C, int mask_multi, float* __restrict__ out) {
  const int64_t total = n * C;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = idx / C;
    const int32_t r = row_of_in[i];
    if (r < 0) continue;
    float v = f[idx];
    if (mask_multi) v *= s[i * FC_K + FC_MV];
    out[(int64_t)r * C + (idx - i * C)] = v * w[i];
  }
}

extern "C" int sv_focal_place(const float* f, const float* s, const int32_t* coords, const uint8_t* fore, const int32_t* nbr,
                              const int32_t* row_of_in, int64_t n, int channels, int mask_multi, int skip_mask_kernel, double threshold,
                              int64_t num_out, float* w, int32_t* cnt, float* out, void* stream) {
  SV_CHECK_ARG(n >= 0 && channels > 0 && num_out >= 0, "focal_place: bad arguments");
  hipStream_t st = sv_stream(stream);
  if (num_out > 0) {
    SV_CHECK_ARG(out && sv_on_device(out), "focal_place: out");
    SV_HIP(hipMemsetAsync(out, 0, (size_t)num_out * channels * sizeof(float), st));
  }
  if (n == 0) return SV_OK;
  SV_CHECK_ARG(f && s && coords && fore && nbr && row_of_in && w && cnt && out, "focal_place: null pointer");
  SV_CHECK_ARG(sv_on_device(f) && sv_on_device(s) && sv_on_device(coords) && sv_on_device(fore) && sv_on_device(nbr) && sv_on_device(row_of_in) &&
               sv_on_device(w) && sv_on_device(cnt), "focal_place: host pointer");
  hipLaunchKernelGGL(k_focal_weigh, dim3(sv_grid_1d(n, FC_THREADS)), dim3(FC_THREADS), 0, st, s, reinterpret_cast<const int4*>(coords), fore, nbr, n,
                     skip_mask_kernel, (float)threshold, w, cnt);
  hipLaunchKernelGGL(k_focal_place, dim3(sv_grid_1d(n * channels, FC_THREADS, 256 * 16)), dim3(FC_THREADS), 0, st, f, s, row_of_in, w, n, channels,
                     mask_multi, out);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ------------------------------------------------------------------------------------------------ 5. backward
// One wave per input row: grad_f[i] = g[row_of_in[i]] * (mv[i]) * w[i] and dots[i] = g[row_of_in[i]] . f[i] (lane-strided partial sums, then the
// butterfly's fixed order).
__global__ __launch_bounds__(FC_THREADS) void k_focal_grad_rows(const float* __restrict__ g, const float* __restrict__ f, const float* __restrict__ s,
                                                                const int32_t* __restrict__ row_of_in, const float* __restrict__ w, int64_t n, int C,
                                                                int mask_multi, float* __restrict__ dots, float* __restrict__ grad_f) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t i = wave; i < n; i += nwaves) {
    const int32_t r = row_of_in[i];
    const float scale = (mask_multi ? s[i * FC_K + FC_MV] : 1.0f) * w[i];
    float d = 0.0f;
    for (int c = lane; c < C; c += 64) {
      const float gv = r >= 0 ? g[(int64_t)r * C + c] : 0.0f;
      grad_f[i * C + c] = gv * scale;
      d += gv * f[i * C + c];
    }
    d = sv_wave_reduce_sum(d);
    if (lane == 0) dots[i] = d;
  }
}

// One thread per (row j, column o): grad_s[j, o] = t_i for the foreground row i = nbr[k(o)][j] that j's kept candidate lands on,
// t_i = dots[i] * (mv[i]) / (1 + c_i); column 26: w[j] * dots[j] under mask_multi.  Everything else 0.
__global__ __launch_bounds__(FC_THREADS) void k_focal_grad_s(const float* __restrict__ s, const int4* __restrict__ coords, const uint8_t* __restrict__ fore,
                                                             const int32_t* __restrict__ nbr, const float* __restrict__ w, const int32_t* __restrict__ cnt,
                                                             const float* __restrict__ dots, int64_t n, int mask_multi, int skip_mask_kernel, float thr,
                                                             float* __restrict__ grad_s) {
  const int64_t total = n * FC_K;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j = idx / FC_K;
    const int o = (int)(idx - j * FC_K);
    float out = 0.0f;
    if (o == FC_MV) {
      if (mask_multi) out = w[j] * dots[j];
    } else if (!skip_mask_kernel && fore[j] && s[idx] >= thr) {
      const int k = o < 13 ? o : o + 1;
      const int32_t i = nbr[(int64_t)k * n + j];
      if (i >= 0 && fore[i]) {
        const int4 ci = coords[i];
        if (ci.y > 0 && ci.z > 0 && ci.w > 0) {
          const float t = dots[i] * (mask_multi ? s[(int64_t)i * FC_K + FC_MV] : 1.0f);
          out = t / (float)(1 + cnt[i]);
        }
      }
    }
    grad_s[idx] = out;
  }
}

extern "C" int sv_focal_backward(const float* g, const float* f, const float* s, const int32_t* coords, const uint8_t* fore, const int32_t* nbr,
                                 const int32_t* row_of_in, const float* w, const int32_t* cnt, int64_t n, int channels, int mask_multi,
                                 int skip_mask_kernel, double threshold, float* dots, float* grad_f, float* grad_s, void* stream) {
  SV_CHECK_ARG(n >= 0 && channels > 0, "focal_backward: bad arguments");
  if (n == 0) return SV_OK;
  SV_CHECK_ARG(g && f && s && coords && fore && nbr && row_of_in && w && cnt && dots && grad_f && grad_s, "focal_backward: null pointer");
  SV_CHECK_ARG(sv_on_device(g) && sv_on_device(f) && sv_on_device(s) && sv_on_device(coords) && sv_on_device(fore) && sv_on_device(nbr) &&
               sv_on_device(row_of_in) && sv_on_device(w) && sv_on_device(cnt) && sv_on_device(dots) && sv_on_device(grad_f) && sv_on_device(grad_s),
               "focal_backward: host pointer");
  hipStream_t st = sv_stream(stream);
  hipLaunchKernelGGL(k_focal_grad_rows, dim3(sv_grid_1d(n * 64, FC_THREADS, 256 * 16)), dim3(FC_THREADS), 0, st, g, f, s, row_of_in, w, n, channels,
                     mask_multi, dots, grad_f);
  hipLaunchKernelGGL(k_focal_grad_s, dim3(sv_grid_1d(n * FC_K, FC_THREADS, 256 * 16)), dim3(FC_THREADS), 0, st, s, reinterpret_cast<const int4*>(coords),
                     fore, nbr, w, cnt, dots, n, mask_multi, skip_mask_kernel, (float)threshold, grad_s);
  SV_LAUNCH_CHECK();
  return SV_OK;
}
