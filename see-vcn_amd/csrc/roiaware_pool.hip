// Part-A2's RoI-aware point feature pooling (detector3d/pcdet/ops/roiaware_pool3d/src/roiaware_pool3d_kernel.cu:16-190 forward, :236-286
// backward), redesigned: the reference writes a (boxes x points) mask to memory and then gives ONE THREAD per box a serial walk over every
// point of the scene (:78-108).  Here a workgroup owns a box, streams the box's point range once, and keeps the cell counters in LDS; the lists
// it leaves are the reference's element for element (slot 0 the count, then the point rows in ascending index), for every scene of a batch in
// one launch.
#include "box_test.h"
#include "common.h"
#include "inverse_lists.h"
#include "wave.h"

constexpr int RA_THREADS = 256;
constexpr int RA_MAX_CELLS = 4096;          // cell counters of one box in LDS: 16 KB
constexpr int RA_MAX_OUT = 255;             // the reference packs a cell into 3 x 8 bits (:72) and silently corrupts beyond

// ------------------------------------------------------------------------------------------------
// Assignment.  Chunks of 256 consecutive points; every lane tests its point (sv_pt_in_box3d) and computes its cell with the reference's fp32
// statements (:57-70).  The inside points of a chunk are compacted IN INDEX ORDER into an LDS staging list (ballot rank in the wave, wave totals
// through LDS).  Staged entry i then counts the entries before it (its rank) and behind it that fall into the same cell -- the staging list is
// read at a wave-uniform address, a broadcast -- reads its cell's counter, and after a barrier writes slot counter + rank; the last entry of a
// cell advances the counter.  Nothing depends on timing, there are no atomics, and a chunk without inside points (most of them: a box holds a
// few per cent of a scene) costs the scan's barriers only.  The counts are written at the end for EVERY cell, so the list tensor needs no
// zero-fill; slots behind a cell's count are never written.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RA_THREADS) void k_roiaware_assign(const float* __restrict__ rois, const float* __restrict__ pts, int n_pts,
                                                                const int32_t* __restrict__ box_pt_range, int out_x, int out_y, int out_z, int cap,
                                                                int32_t* __restrict__ lists) {
  __shared__ int32_t cnt[RA_MAX_CELLS];
  __shared__ int32_t st_pt[RA_THREADS], st_cell[RA_THREADS];
  __shared__ int32_t wave_sum[RA_THREADS / SV_WAVE];
  const int box = blockIdx.x, tid = threadIdx.x;
  const int cells = out_x * out_y * out_z;
  for (int c = tid; c < cells; c += RA_THREADS) cnt[c] = 0;
  const float* b = rois + (int64_t)box * 7;
  const float cx = b[0], cy = b[1], cz = b[2], dx = b[3], dy = b[4], dz = b[5];
  const float cosa = cosf(-b[6]), sina = sinf(-b[6]);
  const float x_res = dx / out_x, y_res = dy / out_y, z_res = dz / out_z;
  int lo = 0, hi = n_pts;
  if (box_pt_range) {
    lo = max(box_pt_range[2 * box], 0);
    hi = min(box_pt_range[2 * box + 1], n_pts);
  }
  int32_t* out = lists + (int64_t)box * cells * cap;
  __syncthreads();
  for (int c0 = lo; c0 < hi; c0 += RA_THREADS) {                       // lo, hi and so the trip count are the same in every thread
    const int p = c0 + tid;
    bool in = false;
    int cell = 0;
    if (p < hi) {
      const float x = pts[(int64_t)p * 3], y = pts[(int64_t)p * 3 + 1], z = pts[(int64_t)p * 3 + 2];
      float lx = 0.f, ly = 0.f;
      in = sv_pt_in_box3d(x, y, z, cx, cy, cz, dx, dy, dz, cosa, sina, 1e-5f, lx, ly);
      if (in) {
        const float lz = z - cz;
        int xi = (int)((lx + dx / 2) / x_res), yi = (int)((ly + dy / 2) / y_res), zi = (int)((lz + dz / 2) / z_res);
        xi = min(max(xi, 0), out_x - 1);
        yi = min(max(yi, 0), out_y - 1);
        zi = min(max(zi, 0), out_z - 1);
        cell = (xi * out_y + yi) * out_z + zi;
      }
    }
    int32_t staged;
    const int32_t at = sv_block_excl_scan<RA_THREADS>((int32_t)in, &staged, wave_sum);
    if (staged == 0) {                                                 // the same in every thread
      __syncthreads();                                                 // wave_sum is written again by the next chunk
      continue;
    }
    if (in) {
      st_pt[at] = p;
      st_cell[at] = cell;
    }
    __syncthreads();
    int before = 0, behind = 0, base = 0, my_cell = 0, my_pt = 0;
    if (tid < staged) {
      my_cell = st_cell[tid];
      my_pt = st_pt[tid];
      for (int j = 0; j < staged; ++j) {
        const bool same = st_cell[j] == my_cell;
        before += same && j < tid;
        behind += same && j > tid;
      }
      base = cnt[my_cell];
    }
    __syncthreads();
    if (tid < staged) {
      const int slot = base + before;
      if (slot < cap - 1) out[(int64_t)my_cell * cap + 1 + slot] = my_pt;   // the later ones are dropped (:97)
      if (behind == 0) cnt[my_cell] = slot + 1;
    }
    __syncthreads();
  }
  for (int c = tid; c < cells; c += RA_THREADS) out[(int64_t)c * cap] = min(cnt[c], cap - 1);
}

extern "C" int sv_roiaware_assign(const float* rois, int n_boxes, const float* pts, int n_pts, const int32_t* box_pt_range, int out_x, int out_y,
                                  int out_z, int max_pts_each_voxel, int32_t* pts_idx_of_voxels, void* stream) {
  SV_CHECK_ARG(n_boxes >= 0 && n_pts >= 0, "roiaware_assign: negative size");
  SV_CHECK_ARG(out_x >= 1 && out_y >= 1 && out_z >= 1 && out_x <= RA_MAX_OUT && out_y <= RA_MAX_OUT && out_z <= RA_MAX_OUT,
               "roiaware_assign: out sizes (%d, %d, %d) must lie in 1..%d", out_x, out_y, out_z, RA_MAX_OUT);
  SV_CHECK_ARG((int64_t)out_x * out_y * out_z <= RA_MAX_CELLS, "roiaware_assign: %lld cells per box, at most %d",
               (long long)out_x * out_y * out_z, RA_MAX_CELLS);
  SV_CHECK_ARG(max_pts_each_voxel >= 2, "roiaware_assign: max_pts_each_voxel %d holds no point (slot 0 is the count)", max_pts_each_voxel);
  if (n_boxes == 0) return SV_OK;
  SV_CHECK_ARG(rois && pts_idx_of_voxels && (n_pts == 0 || pts), "roiaware_assign: null pointer");
  SV_CHECK_ARG(sv_on_device(rois) && sv_on_device(pts_idx_of_voxels) && (n_pts == 0 || sv_on_device(pts)) &&
                   (!box_pt_range || sv_on_device(box_pt_range)),
               "roiaware_assign: a pointer is not device memory");
  hipLaunchKernelGGL(k_roiaware_assign, dim3(n_boxes), dim3(RA_THREADS), 0, sv_stream(stream), rois, pts, n_pts, box_pt_range, out_x, out_y, out_z,
                     max_pts_each_voxel, pts_idx_of_voxels);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ------------------------------------------------------------------------------------------------
// Pooling (:111-190).  One thread per (box, cell, 4 channels): the count is read first, then one 16-byte piece of every listed point's feature
// row (VEC: C % 4 == 0 and aligned rows; else the thread's channels one by one, which is also the tail of C % 4 != 0).  Max: strict > in list
// order from -inf, so the first row of the largest value wins; a cell where nothing compared greater (empty, or all NaN) is 0 with argmax -1.
// Avg: the fp32 sum in list order over the count.
// ------------------------------------------------------------------------------------------------
template <bool VEC, bool MAXP>
__global__ __launch_bounds__(256) void k_roiaware_pool(int64_t total, int C, int cap, const float* __restrict__ feat,
                                                       const int32_t* __restrict__ lists, float* __restrict__ pooled, int32_t* __restrict__ argmax) {
  const int q4 = (C + 3) >> 2;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(e % q4) * 4;
    const int64_t cell = e / q4;
    const int32_t* list = lists + cell * cap;
    const int n = list[0];
    const int w = VEC ? 4 : min(4, C - c);
    float acc[4];
    int32_t arg[4] = {-1, -1, -1, -1};
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = MAXP ? -INFINITY : 0.f;
    for (int k = 1; k <= n; ++k) {
      const int32_t p = list[k];
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (VEC) {
        const float4 f = *reinterpret_cast<const float4*>(feat + (int64_t)p * C + c);
        v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (u < w) v[u] = feat[(int64_t)p * C + c + u];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (MAXP) {
          if (v[u] > acc[u]) { acc[u] = v[u]; arg[u] = p; }
        } else {
          acc[u] = acc[u] + v[u];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (MAXP) acc[u] = arg[u] < 0 ? 0.f : acc[u];
      else acc[u] = n > 0 ? acc[u] / (float)n : 0.f;
    }
    float* o = pooled + cell * C + c;
    if (VEC) {
      *reinterpret_cast<float4*>(o) = make_float4(acc[0], acc[1], acc[2], acc[3]);
      if (MAXP) *reinterpret_cast<int4*>(argmax + cell * C + c) = make_int4(arg[0], arg[1], arg[2], arg[3]);
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (u < w) {
          o[u] = acc[u];
          if (MAXP) argmax[cell * C + c + u] = arg[u];
        }
    }
  }
}

static int ra_check_pool_shape(const char* who, int C, int n_boxes, int cells, int cap) {
  SV_CHECK_ARG(C >= 1 && n_boxes >= 0, "%s: bad arguments", who);
  SV_CHECK_ARG(cells >= 1 && cells <= RA_MAX_CELLS, "%s: %d cells per box, at most %d", who, cells, RA_MAX_CELLS);
  SV_CHECK_ARG(cap >= 2, "%s: max_pts_each_voxel %d holds no point (slot 0 is the count)", who, cap);
  SV_CHECK_ARG((int64_t)n_boxes * cells * (int64_t)(C > cap ? C : cap) < ((int64_t)1 << 31), "%s: more than 2^31 elements", who);
  return SV_OK;
}

extern "C" int sv_roiaware_pool(const float* pts_feature, int C, const int32_t* pts_idx_of_voxels, int n_boxes, int cells, int max_pts_each_voxel,
                                int pool_method, float* pooled, int32_t* argmax, void* stream) {
  if (int rc = ra_check_pool_shape("roiaware_pool", C, n_boxes, cells, max_pts_each_voxel)) return rc;
  SV_CHECK_ARG(pool_method == 0 || pool_method == 1, "roiaware_pool: pool_method %d is neither 0 (max) nor 1 (avg)", pool_method);
  if (n_boxes == 0) return SV_OK;
  SV_CHECK_ARG(pts_idx_of_voxels && pooled && (pool_method == 1 || argmax), "roiaware_pool: null pointer");
  SV_CHECK_ARG(sv_on_device(pts_idx_of_voxels) && sv_on_device(pooled) && (pool_method == 1 || sv_on_device(argmax)) &&
                   (!pts_feature || sv_on_device(pts_feature)),
               "roiaware_pool: a pointer is not device memory");
  // pts_feature may be NULL when there are no points: every count is 0 then and no row is read
  const bool vec = C % 4 == 0 && (((uintptr_t)pts_feature | (uintptr_t)pooled | (uintptr_t)argmax) & 15) == 0;
  const int64_t total = (int64_t)n_boxes * cells * ((C + 3) / 4);
  const dim3 grid(sv_grid_1d(total, 256, 256 * 32)), block(256);
  hipStream_t st = sv_stream(stream);
#define RA_POOL(V, M) \
  hipLaunchKernelGGL((k_roiaware_pool<V, M>), grid, block, 0, st, total, C, max_pts_each_voxel, pts_feature, pts_idx_of_voxels, pooled, argmax)
  if (pool_method == 0) {
    if (vec) RA_POOL(true, true); else RA_POOL(false, true);
  } else {
    if (vec) RA_POOL(true, false); else RA_POOL(false, false);
  }
#undef RA_POOL
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ------------------------------------------------------------------------------------------------
// Backward with float atomics (:236-286): one thread per (box, cell, channel), channels along the lanes so that the adds of a wave to one point
// row are contiguous.  grad_in (n_pts, C) is zero-filled here.
// ------------------------------------------------------------------------------------------------
template <bool MAXP>
__global__ __launch_bounds__(256) void k_roiaware_pool_backward(int64_t total, int C, int cap, int64_t n_pts, const int32_t* __restrict__ lists,
                                                                const int32_t* __restrict__ argmax, const float* __restrict__ grad_out,
                                                                float* __restrict__ grad_in) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(e % C);
    if (MAXP) {
      const int64_t a = argmax[e];
      if (a >= 0 && a < n_pts) atomicAdd(grad_in + a * C + c, grad_out[e]);
    } else {
      const int32_t* list = lists + (e / C) * cap;
      const int n = min(list[0], cap - 1);
      if (n <= 0) continue;
      const float g = grad_out[e] / fmaxf((float)n, 1.f);
      for (int k = 1; k <= n; ++k) {
        const int64_t p = list[k];
        if (p >= 0 && p < n_pts) atomicAdd(grad_in + p * C + c, g);
      }
    }
  }
}

extern "C" int sv_roiaware_pool_backward(const int32_t* pts_idx_of_voxels, const int32_t* argmax, const float* grad_out, int n_boxes, int cells,
                                         int C, int max_pts_each_voxel, int pool_method, int n_pts, float* grad_in, void* stream) {
  if (int rc = ra_check_pool_shape("roiaware_pool_backward", C, n_boxes, cells, max_pts_each_voxel)) return rc;
  SV_CHECK_ARG(n_pts >= 0 && (pool_method == 0 || pool_method == 1), "roiaware_pool_backward: bad arguments");
  if (n_pts == 0) return SV_OK;
  SV_CHECK_ARG(grad_in && sv_on_device(grad_in), "roiaware_pool_backward: grad_in is null or not device memory");
  hipStream_t st = sv_stream(stream);
  SV_HIP(hipMemsetAsync(grad_in, 0, (size_t)n_pts * C * 4, st));
  if (n_boxes == 0) return SV_OK;
  const int32_t* need = pool_method == 0 ? argmax : pts_idx_of_voxels;
  SV_CHECK_ARG(grad_out && need, "roiaware_pool_backward: null pointer");
  SV_CHECK_ARG(sv_on_device(grad_out) && sv_on_device(need), "roiaware_pool_backward: a pointer is not device memory");
  const int64_t total = (int64_t)n_boxes * cells * C;
  const dim3 grid(sv_grid_1d(total, 256, 256 * 32)), block(256);
  if (pool_method == 0)
    hipLaunchKernelGGL((k_roiaware_pool_backward<true>), grid, block, 0, st, total, C, max_pts_each_voxel, (int64_t)n_pts, pts_idx_of_voxels, argmax,
                       grad_out, grad_in);
  else
    hipLaunchKernelGGL((k_roiaware_pool_backward<false>), grid, block, 0, st, total, C, max_pts_each_voxel, (int64_t)n_pts, pts_idx_of_voxels, argmax,
                       grad_out, grad_in);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ------------------------------------------------------------------------------------------------
// The same gradients with a fixed summation order and no float atomics (inverse_lists.h).  Max: key = the flat (box, cell, channel) element,
// row = argmax[key].  Avg: key = the flat (box, cell, slot) element of the list tensor, row = the point listed there (slot 1 .. count).  Every
// point's keys come back ascending, that is in ascending (box, cell); one wave per point, lanes along the channels, sums
//   grad_in[p][c] = +0.0f + (its contributions in that order), each rounded to fp32,
// and writes every element of grad_in once.
// ------------------------------------------------------------------------------------------------
struct RaArgmaxRow {
  const int32_t* argmax;
  __device__ __forceinline__ int64_t operator()(int64_t key) const { return argmax[key]; }
};
struct RaListRow {
  const int32_t* lists;
  int cap;
  __device__ __forceinline__ int64_t operator()(int64_t key) const {
    const int64_t cell = key / cap;
    const int slot = (int)(key - cell * cap);
    if (slot == 0 || slot > lists[cell * cap]) return -1;
    return lists[key];
  }
};

template <bool MAXP>
__global__ __launch_bounds__(256) void k_roiaware_pool_backward_gather(int64_t n_pts, int C, int cap, const int32_t* __restrict__ lists,
                                                                       const float* __restrict__ grad_out, SvInvLists L,
                                                                       float* __restrict__ grad_in) {
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t n = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); n < n_pts; n += nwaves) {
    int32_t cnt;
    const int32_t* keys = sv_inv_list(L, n, cnt);
    for (int c = lane; c < ((C + 63) & ~63); c += 64) {
      float a = 0.f;
      for (int32_t i = 0; i < cnt; ++i) {
        const int32_t key = keys[i];
        if (MAXP) {
          if (key % C == c) a = a + grad_out[key];
        } else {
          const int64_t cell = key / cap;
          const float m = fmaxf((float)min(lists[cell * cap], cap - 1), 1.f);
          if (c < C) a = a + grad_out[cell * C + c] / m;
        }
      }
      if (c < C) grad_in[n * C + c] = a;
    }
  }
}

static int64_t ra_ordered_keys(int n_boxes, int cells, int C, int cap, int pool_method) {
  return (int64_t)n_boxes * cells * (pool_method == 0 ? C : cap);
}

extern "C" size_t sv_roiaware_pool_backward_ordered_scratch_bytes(int n_boxes, int cells, int C, int max_pts_each_voxel, int pool_method, int n_pts) {
  if (n_boxes < 0 || cells < 0 || C < 1 || max_pts_each_voxel < 1 || n_pts < 0) return 0;
  const int64_t keys = ra_ordered_keys(n_boxes, cells, C, max_pts_each_voxel, pool_method);
  if (keys >= ((int64_t)1 << 31)) return 0;
  return sv_inv_lists_bytes(keys, n_pts);
}

extern "C" int sv_roiaware_pool_backward_ordered(const int32_t* pts_idx_of_voxels, const int32_t* argmax, const float* grad_out, int n_boxes,
                                                 int cells, int C, int max_pts_each_voxel, int pool_method, int n_pts, void* scratch, float* grad_in,
                                                 void* stream) {
  if (int rc = ra_check_pool_shape("roiaware_pool_backward_ordered", C, n_boxes, cells, max_pts_each_voxel)) return rc;
  SV_CHECK_ARG(n_pts >= 0 && (pool_method == 0 || pool_method == 1), "roiaware_pool_backward_ordered: bad arguments");
  if (n_pts == 0) return SV_OK;
  SV_CHECK_ARG(grad_in && scratch && sv_on_device(grad_in) && sv_on_device(scratch),
               "roiaware_pool_backward_ordered: grad_in or scratch is null or not device memory");
  const int32_t* need = pool_method == 0 ? argmax : pts_idx_of_voxels;
  SV_CHECK_ARG(n_boxes == 0 || (grad_out && need && sv_on_device(grad_out) && sv_on_device(need)),
               "roiaware_pool_backward_ordered: a pointer is null or not device memory");
  hipStream_t st = sv_stream(stream);
  const int64_t keys = ra_ordered_keys(n_boxes, cells, C, max_pts_each_voxel, pool_method);
  const SvInvLists L = sv_inv_lists_view(scratch, keys, n_pts);
  const dim3 grid(sv_grid_1d((int64_t)n_pts * 64, 256, 256 * 16)), block(256);
  if (pool_method == 0) {
    if (int rc = sv_inv_lists_build(keys, n_pts, RaArgmaxRow{argmax}, L, st)) return rc;
    hipLaunchKernelGGL((k_roiaware_pool_backward_gather<true>), grid, block, 0, st, (int64_t)n_pts, C, max_pts_each_voxel, pts_idx_of_voxels, grad_out,
                       L, grad_in);
  } else {
    if (int rc = sv_inv_lists_build(keys, n_pts, RaListRow{pts_idx_of_voxels, max_pts_each_voxel}, L, st)) return rc;
    hipLaunchKernelGGL((k_roiaware_pool_backward_gather<false>), grid, block, 0, st, (int64_t)n_pts, C, max_pts_each_voxel, pts_idx_of_voxels,
                       grad_out, L, grad_in);
  }
  SV_LAUNCH_CHECK();
  return SV_OK;
}
