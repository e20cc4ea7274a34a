// PV-RCNN++'s vector-pool local aggregation over stacked batches: the `voxel_random_choice` pooling (+ its gradient), the
// `local_interpolation` 3-NN over a query's local neighbours, and the stacked three-point interpolation (+ its gradient).
//
// Reference kernels (one thread per query scanning its whole scene, legacy stream, exit(-1) on error, host-sized buffers with a retry loop in
// the Python wrappers, grouped_idxs in atomic-arrival order):
//   detector3d/pcdet/ops/pointnet2/pointnet2_stack/src/vector_pool_gpu.cu:19-86    (3-NN over stacked local indices)
//   detector3d/pcdet/ops/pointnet2/pointnet2_stack/src/vector_pool_gpu.cu:122-205  (local neighbour lists)
//   detector3d/pcdet/ops/pointnet2/pointnet2_stack/src/vector_pool_gpu.cu:243-373  (vector pool, pooling_type == 1)
//   detector3d/pcdet/ops/pointnet2/pointnet2_stack/src/vector_pool_gpu.cu:433-458  (vector pool gradient)
//   detector3d/pcdet/ops/pointnet2/pointnet2_stack/src/interpolate_gpu.cu:107-172  (three_interpolate / gradient)
// Re-designed like k_ball_query (pointnet2.hip): a wave per query, candidates 64 at a time from an LDS tile that the workgroup's queries of
// one scene share, order kept with ballot + prefix popcount.  Nothing is sized on the host, nothing is read back, nothing is retried: the
// choice kernel writes one support row per (query, cell) -- which is all the gradient needs -- and the 3-NN keeps a query's neighbour list
// in LDS between the reference's two steps.
#include "common.h"
#include "wave.h"
#include "inverse_lists.h"

constexpr int VP_TILE = 1024;          // candidate points per LDS tile (12 KB)

// The reference's rejection test, negated (vector_pool_gpu.cu:170-183, 299-312): ball: lx^2 + ly^2 + lz^2 > R^2; cube: any |l| > R.
__device__ __forceinline__ bool vp_in_range(float lx, float ly, float lz, float R, float R2, int ball) {
  if (ball) return !(lx * lx + ly * ly + lz * lz > R2);
  return !(fabsf(lx) > R || fabsf(ly) > R || fabsf(lz) > R);
}

// ------------------------------------------------------------------------------------------------
// voxel_random_choice.  The reference's thread walks its scene in row order and takes an in-range row whose cell is still empty, until
// nsample rows or all G cells are taken.  Here a wave walks 64 rows at a time: the lanes whose row is in range and whose cell is empty are
// candidates; the lowest candidate lane is the next row the sequential walk would take, taking it removes the candidates of the same cell,
// and so on -- one trip per TAKEN row, at most G over the whole walk.  cell[q][g] (scene-local row or -1) lives in LDS; the outputs are
// written from it at the end, every element once.  A workgroup = 4 waves x VPC_QPW queries of one scene; it stops streaming tiles as soon as
// all its queries are complete.  LDS: 12 KB tile + 16 * G * 4 bytes (G <= 512: 32 KB).
// ------------------------------------------------------------------------------------------------
constexpr int VPC_QPW = 4;
constexpr int VPC_QPB = VPC_QPW * 4;
constexpr int VPC_MAX_G = 512;

__global__ __launch_bounds__(256) void k_vp_choice(int M, int N, const float* __restrict__ new_xyz, const int32_t* __restrict__ q_start,
                                                   const int32_t* __restrict__ q_cnt, const float* __restrict__ xyz,
                                                   const float* __restrict__ features, const int32_t* __restrict__ p_start,
                                                   const int32_t* __restrict__ p_cnt, int c_in, int c_each, int ny, int nz, int G, float R,
                                                   float gsx, float gsy, float gsz, int limit, int ball, int32_t* __restrict__ choice,
                                                   int32_t* __restrict__ point_cnt, float* __restrict__ new_local_xyz,
                                                   float* __restrict__ new_features) {
  extern __shared__ int32_t s_cell[];                    // [VPC_QPB][G]
  __shared__ float tile[VP_TILE * 3];
  __shared__ int done_cnt;
  const int b = blockIdx.y;
  const int qs = q_start[b];
  const int nq = min(q_cnt[b], M - qs);                  // a scene never reaches past the tensors it was cut from
  const int q0 = blockIdx.x * VPC_QPB;
  if (qs < 0 || q0 >= nq) return;
  const int ps = p_start[b];
  const int np = ps < 0 ? 0 : min(p_cnt[b], N - ps);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const float R2 = R * R;
  int32_t* cell = s_cell + wid * VPC_QPW * G;
  float qx[VPC_QPW], qy[VPC_QPW], qz[VPC_QPW];
  int cnt[VPC_QPW];
  bool live[VPC_QPW];
#pragma unroll
  for (int u = 0; u < VPC_QPW; ++u) {
    const int q = q0 + wid * VPC_QPW + u;
    live[u] = q < nq;
    const float* p = new_xyz + (int64_t)(qs + (live[u] ? q : q0)) * 3;
    qx[u] = p[0]; qy[u] = p[1]; qz[u] = p[2];
    cnt[u] = 0;
  }
  for (int e = lane; e < VPC_QPW * G; e += 64) cell[e] = -1;
  for (int t0 = 0; t0 < np; t0 += VP_TILE) {
    const int tn = min(VP_TILE, np - t0);
    if (tid == 0) done_cnt = 0;
    __syncthreads();
    for (int e = tid; e < tn * 3; e += 256) tile[e] = xyz[(int64_t)(ps + t0) * 3 + e];
    __syncthreads();
    int wave_done = 1;
#pragma unroll
    for (int u = 0; u < VPC_QPW; ++u) {
      if (!live[u] || cnt[u] >= limit) continue;
      int32_t* mine = cell + u * G;
      for (int c0 = 0; c0 < tn && cnt[u] < limit; c0 += 64) {
        const int k = c0 + lane;
        bool cand = false;
        int g = 0;
        if (k < tn) {
          const float lx = tile[k * 3] - qx[u], ly = tile[k * 3 + 1] - qy[u], lz = tile[k * 3 + 2] - qz[u];
          if (vp_in_range(lx, ly, lz, R, R2, ball)) {
            const int ix = (int)floorf((lx + R) / gsx), iy = (int)floorf((ly + R) / gsy), iz = (int)floorf((lz + R) / gsz);
            g = min(max(ix * ny * nz + iy * nz + iz, 0), G - 1);      // the clamp is on the COMBINED index (vector_pool_gpu.cu:317-318)
            cand = mine[g] < 0;
          }
        }
        unsigned long long m = __ballot(cand);
        while (m && cnt[u] < limit) {
          const int l = __ffsll((long long)m) - 1;                    // the next row the sequential walk takes
          const int gl = __shfl(g, l, 64);
          if (lane == l) mine[gl] = t0 + k;
          ++cnt[u];
          m &= ~__ballot(cand && g == gl);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      }
      if (cnt[u] < limit) wave_done = 0;
    }
    if (lane == 0 && wave_done) atomicAdd(&done_cnt, 1);
    __syncthreads();
    if (done_cnt == 4) break;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  for (int u = 0; u < VPC_QPW; ++u) {                  // not unrolled: the query is read again instead of indexing the register arrays
    if (q0 + wid * VPC_QPW + u >= nq) break;
    const int64_t m = qs + q0 + wid * VPC_QPW + u;
    const int32_t* mine = cell + u * G;
    for (int g = lane; g < G; g += 64) {
      const int r = mine[g];
      choice[m * G + g] = r >= 0 ? ps + r : -1;
      point_cnt[m * G + g] = r >= 0 ? 1 : 0;
    }
    for (int e = lane; e < 3 * G; e += 64) {
      const int g = e / 3, a = e - g * 3;
      const int r = mine[g];
      const float qa = new_xyz[m * 3 + a];
      new_local_xyz[m * 3 * G + e] = r >= 0 ? xyz[(int64_t)(ps + r) * 3 + a] - qa : 0.f;
    }
    // the reference overwrites channel i % c_each with channel i for every i < c_in: the LAST group is what stays
    for (int e = lane; e < G * c_each; e += 64) {
      const int g = e / c_each, j = e - g * c_each;
      const int r = mine[g];
      new_features[m * G * c_each + e] = r >= 0 ? features[(int64_t)(ps + r) * c_in + (c_in - c_each) + j] : 0.f;
    }
  }
}

extern "C" int sv_vector_pool_choice(int batch, int M, int N, int max_queries_per_scene, const float* new_xyz, const int32_t* new_xyz_batch_start,
                                     const int32_t* new_xyz_batch_cnt, const float* xyz, const float* features, const int32_t* xyz_batch_start,
                                     const int32_t* xyz_batch_cnt, int c_in, int c_each, int nx, int ny, int nz, float max_neighbour_distance,
                                     int nsample, int neighbor_type, int32_t* choice, int32_t* point_cnt, float* new_local_xyz,
                                     float* new_features, void* stream) {
  SV_CHECK_ARG(batch >= 0 && M >= 0 && N >= 0 && nx > 0 && ny > 0 && nz > 0 && c_in > 0 && c_each > 0 && c_in % c_each == 0,
               "vector_pool_choice: bad arguments (c_in a positive multiple of c_each, grid sizes > 0)");
  const int64_t G64 = (int64_t)nx * ny * nz;
  SV_CHECK_ARG(G64 <= VPC_MAX_G, "vector_pool_choice: %lld local cells, at most %d fit the workgroup's LDS", (long long)G64, VPC_MAX_G);
  SV_CHECK_ARG((int64_t)M * G64 * c_each < ((int64_t)1 << 31) && (int64_t)N * c_in < ((int64_t)1 << 31), "vector_pool_choice: outputs exceed int32 indexing");
  if (batch == 0 || M == 0 || max_queries_per_scene <= 0) return SV_OK;
  SV_CHECK_ARG(new_xyz && new_xyz_batch_start && new_xyz_batch_cnt && xyz_batch_start && xyz_batch_cnt && choice && point_cnt && new_local_xyz &&
                   new_features && (N == 0 || (xyz && features)),
               "vector_pool_choice: null pointer");
  const int G = (int)G64;
  const float R = max_neighbour_distance;
  // grid sizes as the reference's launcher computes them, in fp32 (vector_pool_gpu.cu:399-401)
  const float gsx = R * 2 / nx, gsy = R * 2 / ny, gsz = R * 2 / nz;
  const int limit = nsample > 0 ? (nsample < G ? nsample : G) : G;
  dim3 grid(sv_div_up(max_queries_per_scene, VPC_QPB), batch);
  hipLaunchKernelGGL(k_vp_choice, grid, dim3(256), (size_t)VPC_QPB * G * sizeof(int32_t), sv_stream(stream), M, N, new_xyz, new_xyz_batch_start,
                     new_xyz_batch_cnt, xyz, features, xyz_batch_start, xyz_batch_cnt, c_in, c_each, ny, nz, G, R, gsx, gsy, gsz, limit,
                     neighbor_type == 1 ? 1 : 0, choice, point_cnt, new_local_xyz, new_features);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ---- gradient: grad_support[choice[m][g]][c] += grad_new[m][g * c_each + c % c_each] * (1 / max(cnt, 1)) for every c < c_in
// (vector_pool_gpu.cu:433-458: EVERY input channel group receives the gradient, although the forward kept only the last one).
__device__ __forceinline__ float vp_choice_term(const float* __restrict__ grad_new, const int32_t* __restrict__ point_cnt, int64_t key, int c,
                                                int c_each) {
  const float scale = 1 / fmaxf((float)point_cnt[key], 1.0f);
  return grad_new[key * c_each + c % c_each] * scale;
}

// plain: float atomics, lanes along c
__global__ __launch_bounds__(256) void k_vp_choice_grad(int64_t total, int N, int c_in, int c_each, const float* __restrict__ grad_new,
                                                        const int32_t* __restrict__ choice, const int32_t* __restrict__ point_cnt,
                                                        float* __restrict__ grad_support) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t key = e / c_in;
    const int c = (int)(e - key * c_in);
    const int32_t row = choice[key];
    if (row < 0 || row >= N) continue;
    atomicAdd(&grad_support[(int64_t)row * c_in + c], vp_choice_term(grad_new, point_cnt, key, c, c_each));
  }
}

struct SvDirectRow {                   // key k names row rows[k] (negative or out of range: nothing)
  const int32_t* rows;
  __device__ __forceinline__ int64_t operator()(int64_t key) const { return rows[key]; }
};

// ordered: one wave per support row, lanes along c, its keys m * G + g ascending; the sum starts at +0.0f and every element is written once
__global__ __launch_bounds__(256) void k_vp_choice_grad_gather(int64_t N, int c_in, int c_each, const float* __restrict__ grad_new,
                                                               const int32_t* __restrict__ point_cnt, SvInvLists L,
                                                               float* __restrict__ grad_support) {
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t n = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); n < N; n += nwaves) {
    int32_t cnt;
    const int32_t* keys = sv_inv_list(L, n, cnt);
    for (int c = lane; c < c_in; c += 64) {
      float a = 0.f;
      for (int32_t i = 0; i < cnt; ++i) a = a + vp_choice_term(grad_new, point_cnt, keys[i], c, c_each);
      grad_support[n * c_in + c] = a;
    }
  }
}

extern "C" int sv_vector_pool_choice_grad(int M, int N, int G, int c_in, int c_each, const float* grad_new, const int32_t* choice,
                                          const int32_t* point_cnt, float* grad_support, void* stream) {
  SV_CHECK_ARG(M >= 0 && N >= 0 && G > 0 && c_in > 0 && c_each > 0 && c_in % c_each == 0, "vector_pool_choice_grad: bad arguments");
  hipStream_t st = sv_stream(stream);
  if (N > 0) {
    SV_CHECK_ARG(grad_support, "vector_pool_choice_grad: null pointer");
    SV_HIP(hipMemsetAsync(grad_support, 0, (size_t)N * c_in * 4, st));
  }
  if (M == 0 || N == 0) return SV_OK;
  SV_CHECK_ARG(grad_new && choice && point_cnt, "vector_pool_choice_grad: null pointer");
  const int64_t total = (int64_t)M * G * c_in;
  hipLaunchKernelGGL(k_vp_choice_grad, dim3(sv_grid_1d(total, 256, 256 * 16)), dim3(256), 0, st, total, N, c_in, c_each, grad_new, choice, point_cnt,
                     grad_support);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" size_t sv_vector_pool_choice_grad_ordered_scratch_bytes(int M, int N, int G) {
  if (!sv_inv_lists_fit(M, G, N)) return 0;
  return sv_inv_lists_bytes((int64_t)M * G, N);
}

extern "C" int sv_vector_pool_choice_grad_ordered(int M, int N, int G, int c_in, int c_each, const float* grad_new, const int32_t* choice,
                                                  const int32_t* point_cnt, void* scratch, float* grad_support, void* stream) {
  SV_CHECK_ARG(M >= 0 && N >= 0 && G > 0 && c_in > 0 && c_each > 0 && c_in % c_each == 0, "vector_pool_choice_grad_ordered: bad arguments");
  SV_CHECK_ARG(sv_inv_lists_fit(M, G, N), "vector_pool_choice_grad_ordered: the keys M * G (%d * %d) exceed int32", M, G);
  if (N == 0) return SV_OK;
  SV_CHECK_ARG(grad_support && scratch && (M == 0 || (grad_new && choice && point_cnt)), "vector_pool_choice_grad_ordered: null pointer");
  hipStream_t st = sv_stream(stream);
  const SvInvLists L = sv_inv_lists_view(scratch, (int64_t)M * G, N);
  if (int rc = sv_inv_lists_build((int64_t)M * G, N, SvDirectRow{choice}, L, st)) return rc;
  hipLaunchKernelGGL(k_vp_choice_grad_gather, dim3(sv_grid_1d((int64_t)N * 64, 256, 256 * 16)), dim3(256), 0, st, (int64_t)N, c_in, c_each, grad_new,
                     point_cnt, L, grad_support);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ------------------------------------------------------------------------------------------------
// local_interpolation: the reference's two kernels in one launch.  Step 1 (query_stacked_local_neighbor_idxs_kernel): a query's list = the
// first `cap` in-range rows of its scene in row order, cap = min(1000, nsample if nsample > 0).  Step 2
// (query_three_nn_by_stacked_local_idxs_kernel): per grid centre the three list entries smallest under (d, position in list) -- what the
// reference's strict-'<' insertion in list order selects.  The list is split over the lanes (entry p to lane p % 64), every lane keeps its
// own three smallest keys {d bits, p} (d >= 0, so the float's bits order like the float) and three wave minima merge them.
// The list {x, y, z, global row} stays in LDS between the steps: 1000 entries x 16 B = 16 000 B per wave; a workgroup of 3 waves holds
// 3 x 16 000 + the 12 288 B tile = 60 288 B of LDS (two workgroups per CU).
// ------------------------------------------------------------------------------------------------
constexpr int VPN_CAP = 1000;
constexpr int VPN_WAVES = 3;
constexpr unsigned long long VPN_EMPTY = ~0ull;

__global__ __launch_bounds__(VPN_WAVES * 64) void k_vp_three_nn(int M, int N, const float* __restrict__ new_xyz,
                                                                const float* __restrict__ centers, const int32_t* __restrict__ q_start,
                                                                const int32_t* __restrict__ q_cnt, const float* __restrict__ xyz,
                                                                const int32_t* __restrict__ p_start, const int32_t* __restrict__ p_cnt, int G,
                                                                float R, int cap, int ball, int32_t* __restrict__ idx,
                                                                float* __restrict__ dist2) {
  __shared__ float tile[VP_TILE * 3];
  __shared__ float4 s_list[VPN_WAVES][VPN_CAP];
  __shared__ int done_cnt;
  const int b = blockIdx.y;
  const int qs = q_start[b];
  const int nq = min(q_cnt[b], M - qs);
  const int q0 = blockIdx.x * VPN_WAVES;
  if (qs < 0 || q0 >= nq) return;
  const int ps = p_start[b];
  const int np = ps < 0 ? 0 : min(p_cnt[b], N - ps);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const float R2 = R * R;
  float4* list = s_list[wid];
  const bool live = q0 + wid < nq;
  const int64_t m = qs + (live ? q0 + wid : q0);
  const float qx = new_xyz[m * 3], qy = new_xyz[m * 3 + 1], qz = new_xyz[m * 3 + 2];
  int L = 0;
  for (int t0 = 0; t0 < np; t0 += VP_TILE) {
    const int tn = min(VP_TILE, np - t0);
    if (tid == 0) done_cnt = 0;
    __syncthreads();
    for (int e = tid; e < tn * 3; e += VPN_WAVES * 64) tile[e] = xyz[(int64_t)(ps + t0) * 3 + e];
    __syncthreads();
    if (live) {
      for (int c0 = 0; c0 < tn && L < cap; c0 += 64) {
        const int k = c0 + lane;
        bool hit = false;
        float x = 0.f, y = 0.f, z = 0.f;
        if (k < tn) {
          x = tile[k * 3], y = tile[k * 3 + 1], z = tile[k * 3 + 2];
          hit = vp_in_range(x - qx, y - qy, z - qz, R, R2, ball);
        }
        const unsigned long long hm = __ballot(hit);
        if (hm) {
          const int pos = L + __popcll(hm & ((1ull << lane) - 1ull));
          if (hit && pos < cap) list[pos] = make_float4(x, y, z, __int_as_float(ps + t0 + k));
          L = min(cap, L + __popcll(hm));
        }
      }
    }
    if (lane == 0 && (!live || L >= cap)) atomicAdd(&done_cnt, 1);
    __syncthreads();
    if (done_cnt == VPN_WAVES) break;
  }
  if (!live) return;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  for (int g = 0; g < G; ++g) {
    const float* c = centers + (m * G + g) * 3;
    const float cx = c[0], cy = c[1], cz = c[2];
    unsigned long long k1 = VPN_EMPTY, k2 = VPN_EMPTY, k3 = VPN_EMPTY;
    for (int p = lane; p < L; p += 64) {
      const float4 e = list[p];
      const float d = (cx - e.x) * (cx - e.x) + (cy - e.y) * (cy - e.y) + (cz - e.z) * (cz - e.z);
      if (!(d == d)) continue;                                        // a NaN distance never passes the reference's '<'
      const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)p;
      if (key < k1) { k3 = k2; k2 = k1; k1 = key; }
      else if (key < k2) { k3 = k2; k2 = key; }
      else if (key < k3) { k3 = key; }
    }
    unsigned long long best[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      best[r] = sv_wave_reduce_min(k1);
      if (k1 == best[r] && k1 != VPN_EMPTY) { k1 = k2; k2 = k3; k3 = VPN_EMPTY; }      // keys are unique: one lane pops
    }
    if (lane < 3) {
      // one found: slots 2 and 3 repeat slot 1; two found: slot 3 repeats slot 1 (vector_pool_gpu.cu:74-79); none: -1 / 1e40 -> +inf
      unsigned long long w = lane == 0 ? best[0] : (lane == 1 ? best[1] : best[2]);
      if (w == VPN_EMPTY) w = best[0];
      int32_t row = -1;
      float d = __uint_as_float(0x7f800000u);
      if (w != VPN_EMPTY) {
        row = __float_as_int(list[(unsigned)(w & 0xffffffffull)].w);
        d = __uint_as_float((unsigned)(w >> 32));
      }
      idx[(m * G + g) * 3 + lane] = row;
      dist2[(m * G + g) * 3 + lane] = d;
    }
  }
}

extern "C" int sv_vector_pool_three_nn(int batch, int M, int N, int max_queries_per_scene, const float* new_xyz, const float* new_xyz_grid_centers,
                                       const int32_t* new_xyz_batch_start, const int32_t* new_xyz_batch_cnt, const float* xyz,
                                       const int32_t* xyz_batch_start, const int32_t* xyz_batch_cnt, int num_total_grids,
                                       float max_neighbour_distance, int nsample, int neighbor_type, int32_t* idx, float* dist2, void* stream) {
  SV_CHECK_ARG(batch >= 0 && M >= 0 && N >= 0 && num_total_grids > 0, "vector_pool_three_nn: bad arguments");
  SV_CHECK_ARG((int64_t)M * num_total_grids * 3 < ((int64_t)1 << 31), "vector_pool_three_nn: outputs exceed int32 indexing");
  if (batch == 0 || M == 0 || max_queries_per_scene <= 0) return SV_OK;
  SV_CHECK_ARG(new_xyz && new_xyz_grid_centers && new_xyz_batch_start && new_xyz_batch_cnt && xyz_batch_start && xyz_batch_cnt && idx && dist2 &&
                   (N == 0 || xyz),
               "vector_pool_three_nn: null pointer");
  const int cap = nsample > 0 && nsample < VPN_CAP ? nsample : VPN_CAP;
  dim3 grid(sv_div_up(max_queries_per_scene, VPN_WAVES), batch);
  hipLaunchKernelGGL(k_vp_three_nn, grid, dim3(VPN_WAVES * 64), 0, sv_stream(stream), M, N, new_xyz, new_xyz_grid_centers, new_xyz_batch_start,
                     new_xyz_batch_cnt, xyz, xyz_batch_start, xyz_batch_cnt, num_total_grids, max_neighbour_distance, cap,
                     neighbor_type == 1 ? 1 : 0, idx, dist2);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ------------------------------------------------------------------------------------------------
// Stacked three-point interpolation: out[r][c] = w0 * f[i0][c] + w1 * f[i1][c] + w2 * f[i2][c], three rounded products summed left to
// right (interpolate_gpu.cu:123-125); rows x channels, lanes along c.  An index outside [0, n_features) contributes +0.0f (the reference
// would read or add out of bounds).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_three_interp_stack(int64_t total, int C, int n_features, const float* __restrict__ features,
                                                            const int32_t* __restrict__ idx, const float* __restrict__ weight,
                                                            float* __restrict__ out) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = e / C;
    const int c = (int)(e - r * C);
    float t[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      const int32_t i = idx[r * 3 + s];
      t[s] = (i >= 0 && i < n_features) ? weight[r * 3 + s] * features[(int64_t)i * C + c] : 0.f;
    }
    out[e] = t[0] + t[1] + t[2];
  }
}

__global__ __launch_bounds__(256) void k_three_interp_grad_stack(int64_t total, int C, int n_features, const float* __restrict__ grad_out,
                                                                 const int32_t* __restrict__ idx, const float* __restrict__ weight,
                                                                 float* __restrict__ grad_features) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = e / C;
    const int c = (int)(e - r * C);
    const float g = grad_out[e];
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      const int32_t i = idx[r * 3 + s];
      if (i >= 0 && i < n_features) atomicAdd(&grad_features[(int64_t)i * C + c], g * weight[r * 3 + s]);
    }
  }
}

// ordered: key 3 r + t names feature row idx[r][t]; one wave per feature row, lanes along c
__global__ __launch_bounds__(256) void k_three_interp_grad_gather(int64_t n_features, int C, const float* __restrict__ grad_out,
                                                                  const float* __restrict__ weight, SvInvLists L,
                                                                  float* __restrict__ grad_features) {
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t n = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); n < n_features; n += nwaves) {
    int32_t cnt;
    const int32_t* keys = sv_inv_list(L, n, cnt);
    for (int c = lane; c < C; c += 64) {
      float a = 0.f;
      for (int32_t i = 0; i < cnt; ++i) {
        const int32_t key = keys[i];
        a = a + grad_out[(int64_t)(key / 3) * C + c] * weight[key];
      }
      grad_features[n * C + c] = a;
    }
  }
}

extern "C" int sv_three_interpolate_stack(int rows, int C, int n_features, const float* features, const int32_t* idx, const float* weight,
                                          float* out, void* stream) {
  SV_CHECK_ARG(rows >= 0 && C > 0 && n_features >= 0, "three_interpolate_stack: bad arguments");
  if (rows == 0) return SV_OK;
  SV_CHECK_ARG(idx && weight && out && (features || n_features == 0), "three_interpolate_stack: null pointer");
  const int64_t total = (int64_t)rows * C;
  hipLaunchKernelGGL(k_three_interp_stack, dim3(sv_grid_1d(total, 256, 256 * 16)), dim3(256), 0, sv_stream(stream), total, C, n_features, features,
                     idx, weight, out);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_three_interpolate_grad_stack(int rows, int C, int n_features, const float* grad_out, const int32_t* idx, const float* weight,
                                               float* grad_features, void* stream) {
  SV_CHECK_ARG(rows >= 0 && C > 0 && n_features >= 0, "three_interpolate_grad_stack: bad arguments");
  hipStream_t st = sv_stream(stream);
  if (n_features > 0) {
    SV_CHECK_ARG(grad_features, "three_interpolate_grad_stack: null pointer");
    SV_HIP(hipMemsetAsync(grad_features, 0, (size_t)n_features * C * 4, st));
  }
  if (rows == 0 || n_features == 0) return SV_OK;
  SV_CHECK_ARG(grad_out && idx && weight, "three_interpolate_grad_stack: null pointer");
  const int64_t total = (int64_t)rows * C;
  hipLaunchKernelGGL(k_three_interp_grad_stack, dim3(sv_grid_1d(total, 256, 256 * 16)), dim3(256), 0, st, total, C, n_features, grad_out, idx, weight,
                     grad_features);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" size_t sv_three_interpolate_grad_stack_ordered_scratch_bytes(int rows, int n_features) {
  if (!sv_inv_lists_fit(rows, 3, n_features)) return 0;
  return sv_inv_lists_bytes((int64_t)rows * 3, n_features);
}

extern "C" int sv_three_interpolate_grad_stack_ordered(int rows, int C, int n_features, const float* grad_out, const int32_t* idx,
                                                       const float* weight, void* scratch, float* grad_features, void* stream) {
  SV_CHECK_ARG(rows >= 0 && C > 0 && n_features >= 0, "three_interpolate_grad_stack_ordered: bad arguments");
  SV_CHECK_ARG(sv_inv_lists_fit(rows, 3, n_features), "three_interpolate_grad_stack_ordered: the keys 3 * rows (3 * %d) exceed int32", rows);
  if (n_features == 0) return SV_OK;
  SV_CHECK_ARG(grad_features && scratch && (rows == 0 || (grad_out && idx && weight)), "three_interpolate_grad_stack_ordered: null pointer");
  hipStream_t st = sv_stream(stream);
  const SvInvLists L = sv_inv_lists_view(scratch, (int64_t)rows * 3, n_features);
  if (int rc = sv_inv_lists_build((int64_t)rows * 3, n_features, SvDirectRow{idx}, L, st)) return rc;
  hipLaunchKernelGGL(k_three_interp_grad_gather, dim3(sv_grid_1d((int64_t)n_features * 64, 256, 256 * 16)), dim3(256), 0, st, (int64_t)n_features, C,
                     grad_out, weight, L, grad_features);
  SV_LAUNCH_CHECK();
  return SV_OK;
}
