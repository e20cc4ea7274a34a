// Sparse 3-D convolution for half-precision INFERENCE: fp16 activations and weights, fp32 accumulation, fp32 epilogue.
//
//   Y[o][n] = store( epilogue( sum_k sum_c float(X16[nbr[k][o]][c]) * float(W16[k][c][n]) ) )      (rows without a neighbour contribute an exact 0)
//
// k_spconv_h16 is an output-stationary gather-GEMM over the plan of a rulebook table (conv_plan.hip: the row-major table, perm, masks_p), like
// k_spconv_rs3 (sparse_conv.hip), on v_mfma_f32_16x16x32_f16 (C_in >= 32) / v_mfma_f32_16x16x16_f16 (C_in = 16).  What it shares with rs3: 16-row tiles
// of consecutive perm positions, a tile runs the offsets of the OR of its rows' masks, the plan's 8 regions on the workgroups of one XCD each
// (blockIdx.x % 8), whole-row stores through a wave-private staging tile.  What it does not: rs3's deal (tile_of, tiles_per_wave) -- a wave takes
// the tiles w, w + W, w + 2 W ... of its region in perm order (W = waves of the region) -- and rs3's inline-asm operand rings: the loads are plain
// C++ with the next offset's gathered rows requested in front of the current offset's MFMAs.
//
// Numerics.  An fp16 x fp16 product is exact in fp32; the sums are fp32.  Per output element the sequence is: offsets k ascending over the tile's
// mask, inside an offset the channel blocks (32 channels, 16 at C_in = 16) ascending, one MFMA each.  An offset the row itself has no neighbour at
// adds a block of exact zeros, so the row's result does not depend on the tile it was grouped into: bitwise reproducible run to run and plan to plan.
// Epilogue in fp32, in conv_epilogue's order (sparse_conv.hip): + bias[n], ONE fused multiply-add with (scale[n], shift[n]), + float(residual16[o][n]),
// max(., 0).  Store: fp32 as is, or fp16 through v_cvt_f16_f32 (round to nearest even; a finite value beyond 65504 becomes +-inf as that
// instruction defines -- nothing is clamped: an overflow shows as inf instead of a plausible wrong number).
//
// Replaces the half-precision kernels of spconv 2.x behind SubMConv3d / SparseConv3d in eval mode
// (call sites: detector3d/pcdet/models/backbones_3d/spconv_backbone.py:8-27,77-117).
#include <type_traits>

#include "common.h"
#include "norm.h"
#include "sparse_conv.h"

typedef _Float16 h16;
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));

constexpr int H16_REGION_WGS = 128;          // workgroups per region at most: one resident round at four waves per SIMD (32 CUs per XCD)

struct HalfArgs {
  const h16* X;             // (n_src, Kd)
  const int32_t* tab;       // (n_rows, PL_ROW) row-major table
  const int32_t* perm;      // (16 * ceil(n_rows / 16)) row at each position, -1 = padding
  const int32_t* masks_p;   // its mask
  const h16* wfrag;         // sv_conv_weight_fragments_h16
  void* Y;                  // (n_rows, Nc) fp16 or fp32
  const float* bias;        // (Nc) or null
  const float* scale;       // (Nc) or null, with shift
  const float* shift;
  const h16* residual;      // (n_rows, Nc) fp16 or null
  int relu;
  int whole_rows;           // Y and every epilogue term given are 16-byte aligned: 16-byte accesses through the staging tile
  int32_t n_rows;
  uint32_t n_src;
  int K;
  int region_waves;         // waves that share a region's tiles
  int32_t tile0[PL_REGIONS], tiles[PL_REGIONS];
};

__device__ __forceinline__ float h16_epilogue(float v, bool has_bias, float b, bool has_scale, float sc, float sh, bool has_res, float res, bool relu) {
  if (has_bias) v += b;
  if (has_scale) v = bn_act(v, sc, sh);
  if (has_res) v += res;
  if (relu) v = fmaxf(v, 0.f);
  return v;
}

template <int KD, int NT, typename OUT>
// Four waves per SIMD (128 VGPRs); the 128 -> 128 instances hold 32 accumulator, 32 weight and 2 x 16 gathered-row registers in the loop and spill 9-13
// registers at that line: they run at three (168 VGPRs, no scratch).
__global__ __launch_bounds__(256, (KD == 128 && NT == 8) ? 3 : 4) void k_spconv_h16(HalfArgs a) {
  constexpr int E = KD >= 32 ? 8 : 4;                      // halves of one lane's operand: 16x16x32 (8) or 16x16x16 (4)
  constexpr int KQ = KD / (4 * E);                         // channel blocks per offset
  constexpr int NC = NT * 16;
  constexpr int TP = NC + 4;                               // pitch of the staging tile (floats)
  using frag = typename std::conditional<E == 8, h16x8, h16x4>::type;
  __shared__ int32_t s_idx_all[4][PL_ROW - 4][16];         // [k][row of the tile]: source row (table words 0 .. 27; word 27 is the mask, never read as k)
  __shared__ __attribute__((aligned(16))) float s_stage[4][16 * TP];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int li = lane & 15, kk = lane >> 4;
  const int region = blockIdx.x % PL_REGIONS;
  int32_t(*idx)[16] = s_idx_all[wid];
  float* T = s_stage[wid];
  const int n_tiles = a.tiles[region];
  const unsigned kmask = a.K >= 32 ? ~0u : (1u << a.K) - 1u;

  for (int tl = (blockIdx.x / PL_REGIONS) * 4 + wid; tl < n_tiles; tl += a.region_waves) {
    const int64_t p = ((int64_t)a.tile0[region] + tl) * 16 + li;
    int32_t row = a.perm[p];
    if ((uint32_t)row >= (uint32_t)a.n_rows) row = -1;     // padding (and anything a damaged plan could name)
    unsigned m = row >= 0 ? (unsigned)a.masks_p[p] : 0u;
    // the tile's rows of the table -> LDS: lane (row li, kk) brings words 4 kk .. 4 kk + 3 and 16 + 4 kk .. 16 + 4 kk + 3 (< 28)
    {
      i32x4 e0 = (i32x4){-1, -1, -1, -1}, e1 = e0;
      if (row >= 0) {
        const i32x4* rowp = reinterpret_cast<const i32x4*>(a.tab + (int64_t)row * PL_ROW);
        e0 = rowp[kk];
        if (kk < 3) e1 = rowp[4 + kk];
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
#pragma unroll
      for (int c = 0; c < 4; ++c) idx[4 * kk + c][li] = e0[c];
      if (kk < 3) {
#pragma unroll
        for (int c = 0; c < 4; ++c) idx[16 + 4 * kk + c][li] = e1[c];
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) m |= __shfl_xor(m, off, 16);          // OR over the tile's 16 rows (the four kk groups hold the same words)
    unsigned todo = (unsigned)__builtin_amdgcn_readfirstlane((int)m) & kmask;

    f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // gathered row of offset k: the lane's E channels of every channel block, zeros without a neighbour
    auto gather = [&](int k, frag (&A)[KQ]) {
      const int32_t j = idx[k][li];
      const bool has = (uint32_t)j < a.n_src;
      const h16* xr = a.X + (size_t)(uint32_t)(has ? j : 0) * KD + kk * E;
#pragma unroll
      for (int q = 0; q < KQ; ++q) {
        frag z;
#pragma unroll
        for (int u = 0; u < E; ++u) z[u] = (h16)0.f;
        A[q] = has ? *reinterpret_cast<const frag*>(xr + q * 4 * E) : z;
      }
    };
    if (todo) {
      int k = __ffs((int)todo) - 1;
      todo &= todo - 1;
      frag Ac[KQ], An[KQ];
      gather(k, Ac);
      while (true) {
        const int kn = todo ? __ffs((int)todo) - 1 : -1;
        todo &= todo - 1;
        if (kn >= 0) gather(kn, An);                       // requested in front of this offset's MFMAs
        const h16* wk = a.wfrag + ((size_t)k * KQ * NT * 64 + lane) * E;
#pragma unroll
        for (int q = 0; q < KQ; ++q) {
          frag B[NT];
#pragma unroll
          for (int t = 0; t < NT; ++t) B[t] = *reinterpret_cast<const frag*>(wk + (size_t)(q * NT + t) * 64 * E);
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            if constexpr (E == 8) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(Ac[q], B[t], acc[t], 0, 0, 0);
            else acc[t] = __builtin_amdgcn_mfma_f32_16x16x16f16(Ac[q], B[t], acc[t], 0, 0, 0);
          }
        }
        if (kn < 0) break;
        k = kn;
#pragma unroll
        for (int q = 0; q < KQ; ++q) Ac[q] = An[q];
      }
    }

    // D layout (16x16): col = lane & 15, row = 4 * (lane >> 4) + reg
    OUT* Y = static_cast<OUT*>(a.Y);
    if (a.whole_rows) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) T[(kk * 4 + r) * TP + t * 16 + li] = acc[t][r];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      constexpr int C8N = NC / 8;                          // 8-column pieces per row: 16 bytes of fp16, 32 of fp32
#pragma nounroll                                           // unrolled, the four passes of a 128-column tile keep their loads in flight together and spill
      for (int i = 0; i < (16 * C8N + 63) / 64; ++i) {
        const int f = lane + 64 * i, rw = f / C8N, col = (f % C8N) * 8;
        const int32_t orow = __shfl(row, rw & 15);         // lane rw holds row rw of the tile
        if ((16 * C8N % 64 == 0 || f < 16 * C8N) && orow >= 0) {
          const f32x4 v0 = *reinterpret_cast<const f32x4*>(T + rw * TP + col), v1 = *reinterpret_cast<const f32x4*>(T + rw * TP + col + 4);
          float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
          float b[8], sc[8], sh[8], rs[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) b[u] = sc[u] = sh[u] = rs[u] = 0.f;
          if (a.bias) {
            const f32x4 x0 = *reinterpret_cast<const f32x4*>(a.bias + col), x1 = *reinterpret_cast<const f32x4*>(a.bias + col + 4);
#pragma unroll
            for (int u = 0; u < 4; ++u) b[u] = x0[u], b[4 + u] = x1[u];
          }
          if (a.scale) {
            const f32x4 x0 = *reinterpret_cast<const f32x4*>(a.scale + col), x1 = *reinterpret_cast<const f32x4*>(a.scale + col + 4);
            const f32x4 y0 = *reinterpret_cast<const f32x4*>(a.shift + col), y1 = *reinterpret_cast<const f32x4*>(a.shift + col + 4);
#pragma unroll
            for (int u = 0; u < 4; ++u) sc[u] = x0[u], sc[4 + u] = x1[u], sh[u] = y0[u], sh[4 + u] = y1[u];
          }
          if (a.residual) {
            const h16x8 x = *reinterpret_cast<const h16x8*>(a.residual + (int64_t)orow * NC + col);
#pragma unroll
            for (int u = 0; u < 8; ++u) rs[u] = (float)x[u];
          }
#pragma unroll
          for (int u = 0; u < 8; ++u) v[u] = h16_epilogue(v[u], a.bias != nullptr, b[u], a.scale != nullptr, sc[u], sh[u], a.residual != nullptr, rs[u], a.relu != 0);
          OUT* dst = Y + (int64_t)orow * NC + col;
          if constexpr (std::is_same<OUT, float>::value) {
            *reinterpret_cast<f32x4*>(dst) = (f32x4){v[0], v[1], v[2], v[3]};
            *reinterpret_cast<f32x4*>(dst + 4) = (f32x4){v[4], v[5], v[6], v[7]};
          } else {
            h16x8 o;
#pragma unroll
            for (int u = 0; u < 8; ++u) o[u] = (h16)v[u];  // v_cvt_f16_f32: round to nearest even, +-inf beyond the largest finite fp16
            *reinterpret_cast<h16x8*>(dst) = o;
          }
        }
      }
    } else {
      // a pointer that is not 16-byte aligned: straight from the accumulators, one element per access -- the same operations, the same bits
      int32_t orows[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) orows[r] = __shfl(row, kk * 4 + r);       // every lane takes part in all four exchanges before any of them branches
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int32_t orow = orows[r];
        if (orow < 0) continue;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const int col = t * 16 + li;
          const float v = h16_epilogue(acc[t][r], a.bias != nullptr, a.bias ? a.bias[col] : 0.f, a.scale != nullptr, a.scale ? a.scale[col] : 0.f,
                                       a.scale ? a.shift[col] : 0.f, a.residual != nullptr, a.residual ? (float)a.residual[(int64_t)orow * NC + col] : 0.f,
                                       a.relu != 0);
          Y[(int64_t)orow * NC + col] = (OUT)v;
        }
      }
    }
  }
}

static bool h16_channels(int c) { return c == 16 || c == 32 || c == 64 || c == 128; }

extern "C" int sv_conv_h16_applies(int K, int Kd, int Nc, int64_t n_src) {
  // the gathers address X (2 bytes per value) with 32-bit byte offsets, like a buffer descriptor would
  return (K >= 1 && K <= RS3_KMAX && h16_channels(Kd) && h16_channels(Nc) && n_src >= 0 && (uint64_t)n_src * Kd * 2 < 0xfffffff0ull) ? 1 : 0;
}

template <int KD, int NT>
static void launch_h16_out(const HalfArgs& a, int y_is_f32, dim3 grid, hipStream_t st) {
  if (y_is_f32) hipLaunchKernelGGL((k_spconv_h16<KD, NT, float>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((k_spconv_h16<KD, NT, h16>), grid, dim3(256), 0, st, a);
}
template <int KD>
static void launch_h16_nc(const HalfArgs& a, int Nc, int y_is_f32, dim3 grid, hipStream_t st) {
  switch (Nc) {
    case 16: launch_h16_out<KD, 1>(a, y_is_f32, grid, st); break;
    case 32: launch_h16_out<KD, 2>(a, y_is_f32, grid, st); break;
    case 64: launch_h16_out<KD, 4>(a, y_is_f32, grid, st); break;
    default: launch_h16_out<KD, 8>(a, y_is_f32, grid, st); break;
  }
}

extern "C" int sv_sparse_conv_gather_gemm_planned_h16(const void* X16, int64_t n_src, const int32_t* table_rows, const int32_t* perm, const int32_t* masks_p,
                                                      const void* wfrag16, void* Y, int y_is_f32, int64_t n_rows, int K, int Kd, int Nc, const float* bias,
                                                      const float* scale, const float* shift, const void* residual16, int relu, void* stream) {
  SV_CHECK_ARG(n_rows >= 0 && n_rows < 0x7ffffff0ll && K > 0 && Kd > 0 && Nc > 0, "sparse_conv (h16): bad sizes");
  SV_CHECK_ARG(sv_conv_h16_applies(K, Kd, Nc, n_src), "sparse_conv (h16): no fp16 kernel for K %d, C_in %d, C_out %d, %lld source rows (ask sv_conv_h16_applies first)",
               K, Kd, Nc, (long long)n_src);
  SV_CHECK_ARG((scale == nullptr) == (shift == nullptr), "sparse_conv (h16): scale and shift go together");
  if (n_rows == 0) return SV_OK;
  SV_CHECK_ARG(X16 && table_rows && perm && masks_p && wfrag16 && Y, "sparse_conv (h16): null pointer");
  SV_CHECK_ARG((uintptr_t)X16 % 16 == 0 && (uintptr_t)wfrag16 % 16 == 0 && (uintptr_t)table_rows % 16 == 0, "sparse_conv (h16): X, the fragments and the table must be 16-byte aligned");
  SV_CHECK_ARG((uintptr_t)Y % (y_is_f32 ? 4 : 2) == 0 && (uintptr_t)residual16 % 2 == 0 && ((uintptr_t)bias | (uintptr_t)scale | (uintptr_t)shift) % 4 == 0,
               "sparse_conv (h16): a pointer is not aligned to its element");
  HalfArgs a{};
  a.X = static_cast<const h16*>(X16), a.tab = table_rows, a.perm = perm, a.masks_p = masks_p, a.wfrag = static_cast<const h16*>(wfrag16), a.Y = Y;
  a.bias = bias, a.scale = scale, a.shift = shift, a.residual = static_cast<const h16*>(residual16), a.relu = relu ? 1 : 0;
  a.whole_rows = ((((uintptr_t)Y | (uintptr_t)bias | (uintptr_t)scale | (uintptr_t)shift | (uintptr_t)residual16) & 15) == 0) ? 1 : 0;
  a.n_rows = (int32_t)n_rows, a.n_src = (uint32_t)n_src, a.K = K;
  const PlanDims d = plan_dims(n_rows, 1);
  int max_tiles = 0;
  for (int r = 0; r < PL_REGIONS; ++r) {
    a.tile0[r] = d.tile0[r], a.tiles[r] = d.tiles[r];
    if (d.tiles[r] > max_tiles) max_tiles = d.tiles[r];
  }
  int wgs = (max_tiles + 3) / 4;
  wgs = wgs < 1 ? 1 : wgs > H16_REGION_WGS ? H16_REGION_WGS : wgs;
  a.region_waves = wgs * 4;
  const dim3 grid((unsigned)(PL_REGIONS * wgs));
  hipStream_t st = sv_stream(stream);
  switch (Kd) {
    case 16: launch_h16_nc<16>(a, Nc, y_is_f32, grid, st); break;
    case 32: launch_h16_nc<32>(a, Nc, y_is_f32, grid, st); break;
    case 64: launch_h16_nc<64>(a, Nc, y_is_f32, grid, st); break;
    default: launch_h16_nc<128>(a, Nc, y_is_f32, grid, st); break;
  }
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ------------------------------------------------------------------------------------------------ weights in the fp16 kernel's fragment order
// Forward direction only.  One unit = one lane's operand of one (offset k, channel block q, column tile t): E = 8 halves (C_in >= 32) or 4 (C_in = 16),
//   frag[((k * KQ + q) * NT + t) * 64 + lane][j] = half(W[k][c_in = q * 4 E + (lane >> 4) * E + j][c_out = t * 16 + (lane & 15)]),  KQ = C_in / (4 E), NT = C_out / 16
// so a wave's B operand is one contiguous 1 KiB (512 B) read.  float -> half by v_cvt_f16_f32: round to nearest even, as torch.Tensor.half().
struct FragDescH {
  const float* w;
  int64_t sk, si, so, K, Cin, Cout;
  h16* out;
  int64_t reserved;
  int64_t unit0;
};
__device__ __forceinline__ void frag_h16_unit(const float* __restrict__ w, int64_t sk, int64_t si, int64_t so, int Cin, int Cout, h16* __restrict__ out, int64_t e) {
  const int E = Cin >= 32 ? 8 : 4, KQ = Cin / (4 * E), NT = Cout / 16;
  const int lane = (int)(e & 63), li = lane & 15, kk = lane >> 4;
  const int64_t g = e >> 6;
  const int t = (int)(g % NT), q = (int)((g / NT) % KQ);
  const int64_t k = g / ((int64_t)NT * KQ);
  const float* src = w + k * sk + (int64_t)(t * 16 + li) * so + (int64_t)(q * 4 * E + kk * E) * si;
  for (int j = 0; j < E; ++j) out[e * E + j] = (h16)src[j * si];
}
__global__ __launch_bounds__(256) void k_weight_fragments_h16(const float* __restrict__ w, int64_t sk, int64_t si, int64_t so, int Cin, int Cout, h16* __restrict__ out,
                                                              int64_t units) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < units; e += (int64_t)gridDim.x * 256) frag_h16_unit(w, sk, si, so, Cin, Cout, out, e);
}
__global__ __launch_bounds__(256) void k_weight_fragments_h16_batch(const FragDescH* __restrict__ descs, int n, int64_t total_units) {
  for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < total_units; u += (int64_t)gridDim.x * 256) {
    int l = 0;
    while (l + 1 < n && descs[l + 1].unit0 <= u) ++l;
    const FragDescH d = descs[l];
    frag_h16_unit(d.w, d.sk, d.si, d.so, (int)d.Cin, (int)d.Cout, d.out, u - d.unit0);
  }
}

extern "C" int sv_conv_weight_fragments_h16(const float* W, int64_t stride_k, int64_t stride_cin, int64_t stride_cout, int K, int Cin, int Cout, void* frag16,
                                            void* stream) {
  SV_CHECK_ARG(W && frag16 && K > 0, "sv_conv_weight_fragments_h16: null pointer or no offsets");
  SV_CHECK_ARG(h16_channels(Cin) && Cout > 0 && Cout % 16 == 0, "sv_conv_weight_fragments_h16: C_in must be 16, 32, 64 or 128 and C_out a multiple of 16");
  SV_CHECK_ARG((uintptr_t)frag16 % 16 == 0, "sv_conv_weight_fragments_h16: the output must be 16-byte aligned");
  const int64_t units = (int64_t)K * Cin * Cout / (Cin >= 32 ? 8 : 4);
  hipLaunchKernelGGL(k_weight_fragments_h16, dim3(sv_grid_1d(units, 256)), dim3(256), 0, sv_stream(stream), W, stride_k, stride_cin, stride_cout, Cin, Cout,
                     static_cast<h16*>(frag16), units);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_conv_weight_fragments_h16_batch(const void* descs_device, int n_layers, int64_t total_units, void* stream) {
  SV_CHECK_ARG(n_layers >= 0 && total_units >= 0, "sv_conv_weight_fragments_h16_batch: bad sizes");
  if (n_layers == 0 || total_units == 0) return SV_OK;
  SV_CHECK_ARG(descs_device, "sv_conv_weight_fragments_h16_batch: null pointer");
  hipLaunchKernelGGL(k_weight_fragments_h16_batch, dim3(sv_grid_1d(total_units, 256, 2048)), dim3(256), 0, sv_stream(stream),
                     static_cast<const FragDescH*>(descs_device), n_layers, total_units);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ------------------------------------------------------------------------------------------------ fp32 -> fp16 copy of an activation tensor
// The input layer of a half-precision list runs in fp32 (raw point coordinates must not meet fp16's grid); this makes the fp16 copy the next
// layer gathers.  v_cvt_f16_f32: round to nearest even, subnormals kept, +-inf beyond 65504 -- bit for bit torch.Tensor.half().
__global__ __launch_bounds__(256) void k_narrow_h16(const float* __restrict__ x, int64_t n, h16* __restrict__ y, int vec) {
  const int64_t n8 = vec ? n / 8 : 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
    const f32x4 a = reinterpret_cast<const f32x4*>(x)[2 * i], b = reinterpret_cast<const f32x4*>(x)[2 * i + 1];
    h16x8 o;
#pragma unroll
    for (int u = 0; u < 4; ++u) o[u] = (h16)a[u], o[4 + u] = (h16)b[u];
    reinterpret_cast<h16x8*>(y)[i] = o;
  }
  for (int64_t i = n8 * 8 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) y[i] = (h16)x[i];
}

extern "C" int sv_narrow_h16(const float* x_f32, int64_t n_elems, void* y_f16, void* stream) {
  SV_CHECK_ARG(n_elems >= 0, "sv_narrow_h16: bad size");
  if (n_elems == 0) return SV_OK;
  SV_CHECK_ARG(x_f32 && y_f16, "sv_narrow_h16: null pointer");
  SV_CHECK_ARG((uintptr_t)x_f32 % 4 == 0 && (uintptr_t)y_f16 % 2 == 0, "sv_narrow_h16: a pointer is not aligned to its element");
  const int vec = (((uintptr_t)x_f32 | (uintptr_t)y_f16) & 15) == 0 ? 1 : 0;
  hipLaunchKernelGGL(k_narrow_h16, dim3(sv_grid_1d((n_elems + 7) / 8, 256)), dim3(256), 0, sv_stream(stream), x_f32, n_elems, static_cast<h16*>(y_f16), vec);
  SV_LAUNCH_CHECK();
  return SV_OK;
}
