// Voxel R-CNN's voxel RoI pooling (detector3d/pcdet/ops/pointnet2/pointnet2_stack/src/voxel_query_gpu.cu:10-89, voxel_pool_modules.py:70-130,
// utils/common_utils.py:235-252): the dense cell -> row volume, the voxel query on it, and the eval-mode tail of one pooling scale.
#include "common.h"
#include "wave.h"

// ------------------------------------------------------------------------------------------------
// generate_voxel2pinds: volume (B, Z, Y, X) int32, -1 everywhere and `row` at [b, z, y, x] of row `row` of coords (N, 4).  A row outside the
// volume writes nothing.  clear = 1 writes -1 instead of the row number: the same N-row scatter returns a persistent volume to all -1.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_voxel2pinds(const int32_t* __restrict__ coords, int64_t N, int B, int Z, int Y, int X, int clear,
                                                     int32_t* __restrict__ volume) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < N; r += (int64_t)gridDim.x * blockDim.x) {
    const int4 c = reinterpret_cast<const int4*>(coords)[r];
    if (c.x < 0 || c.x >= B || c.y < 0 || c.y >= Z || c.z < 0 || c.z >= Y || c.w < 0 || c.w >= X) continue;
    const int64_t off = (((int64_t)c.x * Z + c.y) * Y + c.z) * X + c.w;   // 64-bit: B*Z*Y*X may pass 2^31
    volume[off] = clear ? -1 : (int32_t)r;
  }
}

extern "C" int sv_voxel2pinds(const int32_t* coords, int64_t N, int B, int Z, int Y, int X, int fill, int clear, int32_t* volume, void* stream) {
  SV_CHECK_ARG(N >= 0 && N < (1ll << 31) && B >= 0 && Z >= 0 && Y >= 0 && X >= 0, "voxel2pinds: bad arguments");
  const int64_t cells = (int64_t)B * Z * Y * X;
  if (cells == 0) return SV_OK;
  SV_CHECK_ARG(volume && (N == 0 || coords), "voxel2pinds: null pointer");
  SV_CHECK_ARG(((uintptr_t)coords & 15) == 0, "voxel2pinds: coords must be 16-byte aligned");
  hipStream_t st = sv_stream(stream);
  if (fill) SV_HIP(hipMemsetAsync(volume, 0xFF, (size_t)cells * 4, st));    // every byte 0xFF = int32 -1
  if (N == 0) return SV_OK;
  hipLaunchKernelGGL(k_voxel2pinds, dim3(sv_grid_1d(N, 256)), dim3(256), 0, st, coords, N, B, Z, Y, X, clear, volume);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ------------------------------------------------------------------------------------------------
// voxel_query_kernel_stack.  The reference walks the (2 zr + 1)(2 yr + 1)(2 xr + 1) window with one thread per query: dz outermost, dx
// innermost, cells outside the volume and -1 cells skipped, a neighbour kept unless dist2 > radius2, the first nsample kept ones fill slots
// 0.., the first of them also every later slot, no kept one: idx[0] = -1.  Here one wave owns a query.  The window is clipped to the volume
// first (a clipped box in the same lexicographic order visits the surviving cells in the reference's order), lanes take 64 consecutive cells
// of it per pass, a ballot ranks the kept ones and the wave leaves once nsample slots are full.  No LDS, no atomics; the next pass's cell is
// read while this pass's coordinates are in flight.
// ------------------------------------------------------------------------------------------------
constexpr int VQ_WAVES = 4;

__global__ __launch_bounds__(VQ_WAVES* SV_WAVE) void k_voxel_query(int M, int B, int R1, int R2, int R3, int64_t N, int nsample, float radius2, int zr,
                                                                   int yr, int xr, const float* __restrict__ new_xyz, const float* __restrict__ xyz,
                                                                   const int32_t* __restrict__ new_coords,
                                                                   const int32_t* __restrict__ point_indices, int32_t* __restrict__ idx) {
  const int lane = threadIdx.x & (SV_WAVE - 1);
  const int q = blockIdx.x * VQ_WAVES + (threadIdx.x >> 6);
  if (q >= M) return;                                                     // whole waves leave: q is the same in every lane of a wave
  const float new_x = new_xyz[(int64_t)q * 3], new_y = new_xyz[(int64_t)q * 3 + 1], new_z = new_xyz[(int64_t)q * 3 + 2];
  const int4 nc = reinterpret_cast<const int4*>(new_coords)[q];
  int32_t* out = idx + (int64_t)q * nsample;
  // the clipped window; 64-bit sums: a query far outside may sit next to INT_MAX
  const int z0 = (int)max((int64_t)nc.y - zr, (int64_t)0), z1 = (int)min((int64_t)nc.y + zr, (int64_t)R1 - 1);
  const int y0 = (int)max((int64_t)nc.z - yr, (int64_t)0), y1 = (int)min((int64_t)nc.z + yr, (int64_t)R2 - 1);
  const int x0 = (int)max((int64_t)nc.w - xr, (int64_t)0), x1 = (int)min((int64_t)nc.w + xr, (int64_t)R3 - 1);
  const bool any = nc.x >= 0 && nc.x < B && (int64_t)nc.y + zr >= 0 && (int64_t)nc.y - zr < R1 && (int64_t)nc.z + yr >= 0 &&
                   (int64_t)nc.z - yr < R2 && (int64_t)nc.w + xr >= 0 && (int64_t)nc.w - xr < R3;
  int cnt = 0, first = -1;
  if (any) {
    const int wx = x1 - x0 + 1, wy = y1 - y0 + 1, wz = z1 - z0 + 1;
    const int cells = wz * wy * wx;                                       // <= (2 * 2^10 + 1)^3 is refused by the host: fits
    const int64_t base = (int64_t)nc.x * R1 * R2 * R3;
    auto cell_row = [&](int c) -> int32_t {
      if (c >= cells) return -1;
      const int dx = c % wx, t = c / wx;
      const int dy = t % wy, dz = t / wy;
      return point_indices[base + ((int64_t)(z0 + dz) * R2 + (y0 + dy)) * R3 + (x0 + dx)];
    };
    int32_t nxt = cell_row(lane);
    for (int c0 = 0; c0 < cells; c0 += SV_WAVE) {
      const int32_t nb = nxt;
      bool hit = false;
      float x_per = 0.f, y_per = 0.f, z_per = 0.f;
      const bool valid = nb >= 0 && (int64_t)nb < N;
      if (valid) {
        x_per = xyz[(int64_t)nb * 3];
        y_per = xyz[(int64_t)nb * 3 + 1];
        z_per = xyz[(int64_t)nb * 3 + 2];
      }
      nxt = cell_row(c0 + SV_WAVE + lane);
      if (valid) {
        const float dist2 = (x_per - new_x) * (x_per - new_x) + (y_per - new_y) * (y_per - new_y) + (z_per - new_z) * (z_per - new_z);
        hit = !(dist2 > radius2);
      }
      int total;
      const int pos = cnt + sv_wave_ballot_rank(hit, &total);
      if (total) {
        if (cnt == 0) first = __shfl(nb, sv_wave_ballot_first(hit), SV_WAVE);
        if (hit && pos < nsample) out[pos] = nb;
        cnt += total;
        if (cnt >= nsample) break;                                        // cnt is the same in every lane
      }
    }
  }
  if (cnt == 0) {
    if (lane == 0) out[0] = -1;                                           // the other slots stay as the caller left them
  } else {
    for (int l = cnt + lane; l < nsample; l += SV_WAVE) out[l] = first;   // slots no hit reached repeat the first one
  }
}

extern "C" int sv_voxel_query_stack(int M, int B, int R1, int R2, int R3, int64_t n_points, int nsample, float radius, int z_range, int y_range,
                                    int x_range, const float* new_xyz, const float* xyz, const int32_t* new_coords, const int32_t* point_indices,
                                    int32_t* idx, void* stream) {
  SV_CHECK_ARG(M >= 0 && B >= 0 && R1 >= 0 && R2 >= 0 && R3 >= 0 && n_points >= 0 && nsample > 0, "voxel_query: bad arguments");
  SV_CHECK_ARG(z_range >= 0 && y_range >= 0 && x_range >= 0 && z_range <= 1024 && y_range <= 1024 && x_range <= 1024 &&
                   (int64_t)(2 * z_range + 1) * (2 * y_range + 1) * (2 * x_range + 1) < (1ll << 31) - 64,
               "voxel_query: the window must hold fewer than 2^31 cells");
  if (M == 0) return SV_OK;
  SV_CHECK_ARG(new_xyz && new_coords && idx, "voxel_query: null pointer");
  SV_CHECK_ARG(((uintptr_t)new_coords & 15) == 0, "voxel_query: new_coords must be 16-byte aligned");
  const int64_t cells = (int64_t)B * R1 * R2 * R3;
  SV_CHECK_ARG(cells == 0 || point_indices, "voxel_query: null pointer");
  SV_CHECK_ARG(n_points == 0 || xyz, "voxel_query: null pointer");
  hipLaunchKernelGGL(k_voxel_query, dim3(sv_div_up(M, VQ_WAVES)), dim3(VQ_WAVES * SV_WAVE), 0, sv_stream(stream), M, cells == 0 ? 0 : B, R1, R2, R3,
                     n_points, nsample, radius * radius, z_range, y_range, x_range, new_xyz, xyz, new_coords, point_indices, idx);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ------------------------------------------------------------------------------------------------
// The eval-mode tail of one scale of NeighborVoxelSAModuleMSG.forward without the (M, C1, nsample) and (M, 3, nsample) tensors:
//   out[m][c] = max_s ReLU(f_in[idx[m][s]][c] + Wp[c] . (xyz[idx[m][s]] - new_xyz[m]) + bp[c])
// One thread per (query, 4 channels): a feature row is read in 16-byte pieces by consecutive lanes, the slot's row number and coordinates
// are the same address for the C1 / 4 lanes of a query.  An empty query (idx[m][0] < 0) is ReLU(bp); a slot that names no row is passed over.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_voxel_pool_max(int64_t M, int64_t N, int C1, int nsample, const float* __restrict__ f_in,
                                                        const float* __restrict__ xyz, const float* __restrict__ new_xyz,
                                                        const int32_t* __restrict__ idx, const float* __restrict__ wp,
                                                        const float* __restrict__ bp, float* __restrict__ out) {
  const int q4 = C1 >> 2;
  const int64_t total = M * q4;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(e % q4) * 4;
    const int64_t m = e / q4;
    const float4 b = *reinterpret_cast<const float4*>(bp + c);
    float w[4][3];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      w[u][0] = wp[(c + u) * 3];
      w[u][1] = wp[(c + u) * 3 + 1];
      w[u][2] = wp[(c + u) * 3 + 2];
    }
    const int32_t* id = idx + m * nsample;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};                                  // ReLU's floor: the max of values that are >= 0
    if (id[0] < 0) {
      acc[0] = fmaxf(b.x, 0.f); acc[1] = fmaxf(b.y, 0.f); acc[2] = fmaxf(b.z, 0.f); acc[3] = fmaxf(b.w, 0.f);
    } else {
      const float qx = new_xyz[m * 3], qy = new_xyz[m * 3 + 1], qz = new_xyz[m * 3 + 2];
      for (int s = 0; s < nsample; ++s) {
        const int64_t j = id[s];
        if (j < 0 || j >= N) continue;
        const float dx = xyz[j * 3] - qx, dy = xyz[j * 3 + 1] - qy, dz = xyz[j * 3 + 2] - qz;
        const float4 f = *reinterpret_cast<const float4*>(f_in + j * C1 + c);
        const float fv[4] = {f.x, f.y, f.z, f.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] = fmaxf(acc[u], fv[u] + (w[u][0] * dx + w[u][1] * dy + w[u][2] * dz + bv[u]));
      }
    }
    *reinterpret_cast<float4*>(out + m * C1 + c) = make_float4(acc[0], acc[1], acc[2], acc[3]);
  }
}

extern "C" int sv_voxel_pool_max(const float* f_in, const float* xyz, const float* new_xyz, const int32_t* idx, const float* wp, const float* bp,
                                 int64_t M, int64_t N, int C1, int nsample, float* out, void* stream) {
  SV_CHECK_ARG(M >= 0 && N >= 0, "voxel_pool_max: bad arguments");
  SV_CHECK_ARG(C1 % 16 == 0 && C1 >= 16 && C1 <= 64 && nsample >= 1 && nsample <= 32, "voxel_pool_max: built for C1 in {16, 32, 48, 64} and nsample <= 32");
  if (M == 0) return SV_OK;
  SV_CHECK_ARG(new_xyz && idx && wp && bp && out && (N == 0 || (f_in && xyz)), "voxel_pool_max: null pointer");
  SV_CHECK_ARG((((uintptr_t)f_in | (uintptr_t)bp | (uintptr_t)out) & 15) == 0, "voxel_pool_max: f_in, bp and out must be 16-byte aligned");
  const int64_t total = M * (C1 / 4);
  hipLaunchKernelGGL(k_voxel_pool_max, dim3(sv_grid_1d(total, 256, 256 * 16)), dim3(256), 0, sv_stream(stream), M, N, C1, nsample, f_in, xyz, new_xyz,
                     idx, wp, bp, out);
  SV_LAUNCH_CHECK();
  return SV_OK;
}
