// Sparse 3-D convolution: output-stationary gather-GEMM over the output-major rulebook.
//
//   Y[o][n] = epilogue( sum_k sum_c X[nbr[k][o]][c] * Wt[k][n][c] )       (rows with nbr < 0 contribute 0)
//
// One kernel serves three uses (the caller picks the table and the weight view):
//   forward        X = features,  nbr = output-major table,            Wt[k][n][c] = W[k][c_in=c][c_out=n]
//   backward-data  X = grad_out,  nbr = input-major table (nbr_in),    Wt[k][n][c] = W[k][c_in=n][c_out=c]
// and a second kernel reduces the weight gradient dW[k][c][n] = sum_o X[nbr[k][o]][c] * dY[o][n].
//
// Every output row is produced exactly once, in registers, with a fixed summation order (k ascending):
// no atomics, bitwise reproducible.  The dense per-voxel products run on the fp32 MFMA
// (v_mfma_f32_16x16x4_f32, exact fp32) -- 16-row tiles so that a (tile, offset) pair with no neighbour is skipped.
// Algorithmic traffic per layer: 4*(N_in*C_in + N_out*C_out) + 4*K*C_in*C_out + 4*K*N_out (table) bytes.
//
// The MFMA kernel runs on a PLAN of the table (sv_conv_plan_build, once per rulebook table):
//   * rows are split into 8 contiguous REGIONS (ascending key order = scene / z-slab order), one per XCD: the workgroups of region r are
//     the ones the dispatcher places on XCD r (blockIdx % 8), so a scene's feature rows are gathered through ONE 4 MiB L2 instead of eight;
//   * inside a region rows are regrouped into 16-row tiles of equal NEIGHBOUR-MASK CLASS (counting sort, no comparison sort): a tile executes
//     an offset when any of its rows has that neighbour, so equal-mask tiles waste few MFMA steps;
//   * the regrouped table is rewritten row-major (128 B per row: 27 neighbours, mask, output row): a tile's prologue reads 2 KiB of
//     consecutive bytes instead of 27 x 16 scattered words;
//   * sv_conv_plan_tiles deals a region's tiles to its waves by descending cost in snake order (equal work per wave).
//
// Replaces the third-party spconv kernels behind SubMConv3d / SparseConv3d
// (call sites: detector3d/pcdet/models/backbones_3d/spconv_backbone.py:8-27,77-117).
#include <stdlib.h>

#include "common.h"
#include "norm.h"
#include "sparse_conv.h"

static thread_local InNorm g_next_in;
extern "C" int sv_conv_next_input_norm(const float* coef, int relu) {
  g_next_in.coef = coef, g_next_in.relu = relu ? 1 : 0;
  return SV_OK;
}
InNorm take_input_norm() {
  const InNorm r = g_next_in;
  g_next_in = InNorm{};
  return r;
}

struct ConvArgs {
  const float* X;         // (n_src, Kd)
  const int32_t* nbr;     // (K, n_rows)
  const float* Wt;        // (K, Nc, Kd)
  float* Y;               // (n_rows, Nc)
  const float* bias;      // (Nc) or null        : y += bias
  const float* scale;     // (Nc) or null        : y = y*scale + shift   (folded eval-mode BatchNorm)
  const float* shift;     // (Nc) or null
  const float* residual;  // (n_rows, Nc) or null: y += residual (after scale/shift, before relu)
  int relu;
  int64_t n_rows;
  int K, Kd, Nc;
};

__device__ __forceinline__ float conv_epilogue(float v, int col, int64_t row, const ConvArgs& a) {
  if (a.bias) v += a.bias[col];
  if (a.scale) v = bn_act(v, a.scale[col], a.shift[col]);       // the fused multiply-add of k_bn_apply_fwd: a folded BatchNorm gives the separate pass's bits
  if (a.residual) v += a.residual[row * a.Nc + col];
  if (a.relu) v = fmaxf(v, 0.f);
  return v;
}

// ------------------------------------------------------------------------------------------------
// Register-stationary, barrier-free variant (the default MFMA path).
//   * a wave owns RS_G 16-row output tiles x all Nc columns, accumulators in registers;
//   * no LDS, no workgroup barriers: both MFMA operands are loaded straight into registers — the gathered
//     source rows (A) and the 16-column weight slabs (B, shared by every wave, served by L1/L2);
//   * operands of step (k, q) + 1 are requested before step (k, q) runs on the matrix core, the neighbour
//     indices of the next active offset are fetched one offset ahead;
//   * offsets with no neighbour for any of the wave's rows are skipped entirely (64-bit activity mask from a
//     ballot pre-pass), row tiles with no neighbour skip their MFMAs;
//   * the wave's tiles are taken from RS_G distant parts of the (key-sorted) row range: neighbour density is
//     spatially correlated, striding gives every wave a mix of dense and sparse regions (measured -8 % time).
// Summation order per output element is fixed (k ascending, channels ascending) -> bitwise reproducible.
// Measured (MI355X, 64->64 submanifold layer, 134 580 rows, 1.17 M pairs): 250 us = 38 TFLOP/s algorithmic;
// matrix-core busy 38 % — waves spend their time in issue stalls, see DESIGN.md "sparse conv: what limits it".
// Two LDS-DMA restructurings (global_load_lds row gathers into a ring, offset-major weight slabs) were built, verified
// bit-compatible with the tests and measured slower (304 us with columns split over a workgroup's waves and a barrier per
// position; 266 us wave-private with the next slab prefetched) — they are in the git history (commit "Experimental
// wave-private LDS-DMA sparse conv kernel"), the findings in DESIGN.md.
// ------------------------------------------------------------------------------------------------
template <int NT, int KQ, int RS_G>
__global__ __launch_bounds__(256) void k_spconv_rs(ConvArgs a) {
  constexpr int Kd = KQ * 16, Nc = NT * 16;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int li = lane & 15, kk = lane >> 4;
  const int64_t n_tiles = (a.n_rows + 15) / 16;
  const int64_t n_waves = (n_tiles + RS_G - 1) / RS_G;
  const int64_t wave_id = (int64_t)blockIdx.x * 4 + wid;
  if (wave_id >= n_waves) return;
  auto tile_row0 = [&](int g) { return (wave_id + (int64_t)g * n_waves) * 16; };

  // activity mask of the kernel offsets for this wave's rows
  unsigned long long active = 0ull;
  {
    // lane -> (tile lane>>4, row lane&15); with RS_G < 4 the upper tiles alias tile 0 (harmless for an OR)
    const int64_t r = tile_row0((lane >> 4) % RS_G) + li;
    for (int k = 0; k < a.K; ++k) {
      const int32_t j = r < a.n_rows ? a.nbr[(int64_t)k * a.n_rows + r] : -1;
      if (__ballot(j >= 0)) active |= 1ull << k;
    }
  }

  f32x4 acc[RS_G][NT];
#pragma unroll
  for (int g = 0; g < RS_G; ++g)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[g][t] = (f32x4){0.f, 0.f, 0.f, 0.f};

  auto load_j = [&](int k, int32_t (&j)[RS_G]) {
#pragma unroll
    for (int g = 0; g < RS_G; ++g) {
      const int64_t r = tile_row0(g) + li;
      j[g] = r < a.n_rows ? a.nbr[(int64_t)k * a.n_rows + r] : -1;
    }
  };
  auto load_ab = [&](int k, int q, const int32_t (&j)[RS_G], float4 (&A)[RS_G], float4 (&B)[NT]) {
#pragma unroll
    for (int g = 0; g < RS_G; ++g)
      A[g] = j[g] >= 0 ? *reinterpret_cast<const float4*>(a.X + (int64_t)j[g] * Kd + q * 16 + kk * 4) : make_float4(0, 0, 0, 0);
    const float* w = a.Wt + ((int64_t)k * Nc + li) * Kd + q * 16 + kk * 4;
#pragma unroll
    for (int t = 0; t < NT; ++t) B[t] = *reinterpret_cast<const float4*>(w + (int64_t)t * 16 * Kd);
  };

  if (active) {
    int k = __ffsll((long long)active) - 1;
    active &= active - 1;
    int32_t jc[RS_G], jn[RS_G];
    float4 Ac[RS_G], Bc[NT], An[RS_G], Bn[NT];
    load_j(k, jc);
    load_ab(k, 0, jc, Ac, Bc);
    while (true) {
      const int kn = active ? __ffsll((long long)active) - 1 : -1;
      if (kn >= 0) load_j(kn, jn);
      bool anyg[RS_G];
#pragma unroll
      for (int g = 0; g < RS_G; ++g) anyg[g] = __ballot(jc[g] >= 0) != 0ull;
#pragma unroll
      for (int q = 0; q < KQ; ++q) {
        // request the next step's operands before running this step's MFMAs
        if (q + 1 < KQ) load_ab(k, q + 1, jc, An, Bn);
        else if (kn >= 0) load_ab(kn, 0, jn, An, Bn);
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int g = 0; g < RS_G; ++g)
            if (anyg[g]) {
              acc[g][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(Ac[g].x, Bc[t].x, acc[g][t], 0, 0, 0);
              acc[g][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(Ac[g].y, Bc[t].y, acc[g][t], 0, 0, 0);
              acc[g][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(Ac[g].z, Bc[t].z, acc[g][t], 0, 0, 0);
              acc[g][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(Ac[g].w, Bc[t].w, acc[g][t], 0, 0, 0);
            }
        if (q + 1 < KQ || kn >= 0) {
#pragma unroll
          for (int g = 0; g < RS_G; ++g) Ac[g] = An[g];
#pragma unroll
          for (int t = 0; t < NT; ++t) Bc[t] = Bn[t];
        }
      }
      if (kn < 0) break;
      k = kn;
      active &= active - 1;
#pragma unroll
      for (int g = 0; g < RS_G; ++g) jc[g] = jn[g];
    }
  }
  // D layout (16x16): col = lane&15, row = 4*(lane>>4) + reg
#pragma unroll
  for (int g = 0; g < RS_G; ++g)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row = tile_row0(g) + kk * 4 + r;
        const int col = t * 16 + li;
        if (row < a.n_rows) a.Y[row * Nc + col] = conv_epilogue(acc[g][t][r], col, row, a);
      }
}


template <int NT, int G>
static int launch_rs_kq(const ConvArgs& a, int kq, hipStream_t st) {
  const int64_t n_tiles = (a.n_rows + 15) / 16;
  const int64_t n_waves = (n_tiles + G - 1) / G;
  const dim3 grid((unsigned)((n_waves + 3) / 4));
  switch (kq) {
    case 1: hipLaunchKernelGGL((k_spconv_rs<NT, 1, G>), grid, dim3(256), 0, st, a); return 0;
    case 2: hipLaunchKernelGGL((k_spconv_rs<NT, 2, G>), grid, dim3(256), 0, st, a); return 0;
    case 4: hipLaunchKernelGGL((k_spconv_rs<NT, 4, G>), grid, dim3(256), 0, st, a); return 0;
    case 8: hipLaunchKernelGGL((k_spconv_rs<NT, 8, G>), grid, dim3(256), 0, st, a); return 0;
  }
  return -1;
}

static int try_launch_rs(const ConvArgs& a, hipStream_t st) {
  if (a.Kd % 16 || a.Nc % 16 || a.K > 64) return -1;
  switch (a.Nc / 16) {
    case 1: return launch_rs_kq<1, 4>(a, a.Kd / 16, st);
    case 2: return launch_rs_kq<2, 4>(a, a.Kd / 16, st);
    case 4: return launch_rs_kq<4, 4>(a, a.Kd / 16, st);
    case 8: return launch_rs_kq<8, 4>(a, a.Kd / 16, st);
  }
  return -1;
}


// ------------------------------------------------------------------------------------------------ weights in MFMA fragment order
// One contiguous KiB per (offset, 16-channel step, column tile): the B-operand load of a wave touches 8 whole cache lines instead of 16
// half lines at 16 different rows.  Both directions of a layer in one launch, into caller-owned buffers (cached by the host per weight
// version; round 1 kept ONE device-global buffer, which two streams would have raced on):
//   fwd:  Wt[k][n = c_out][c = c_in]      bwd:  Wt[k][n = c_in][c = c_out]         from W (K, C_in, C_out) given by its element strides
struct WStride {
  int64_t k, i, o;     // element strides of the (K, C_in, C_out) weight view
};
__global__ __launch_bounds__(256) void k_weight_fragments(const float* __restrict__ w, WStride ws, int K, int Cin, int Cout, float* __restrict__ wf_fwd,
                                                          float* __restrict__ wf_bwd) {
  const int total = K * Cin * Cout / 4;                      // float4 units per direction
  for (int i = blockIdx.x * 256 + threadIdx.x; i < 2 * total; i += gridDim.x * 256) {
    const bool bwd = i >= total;
    const int e = bwd ? i - total : i;
    const int Nc = bwd ? Cin : Cout, Kd = bwd ? Cout : Cin;
    const int64_t sn = bwd ? ws.i : ws.o, sc = bwd ? ws.o : ws.i;
    const int KQ = Kd / 16, NT = Nc / 16;
    const int lane = e & 63, t = (e >> 6) % NT, q = ((e >> 6) / NT) % KQ, k = (e >> 6) / (NT * KQ);
    const int li = lane & 15, kk = lane >> 4;
    const float* src = w + k * ws.k + (t * 16 + li) * sn + (q * 16 + kk * 4) * sc;
    float4 v;
    if (sc == 1 && (((uintptr_t)src) & 15) == 0) v = *reinterpret_cast<const float4*>(src);
    else v = make_float4(src[0], src[sc], src[2 * sc], src[3 * sc]);
    float* dst = bwd ? wf_bwd : wf_fwd;
    if (dst) reinterpret_cast<float4*>(dst)[e] = v;
  }
}

extern "C" int sv_conv_weight_fragments(const float* W, int64_t stride_k, int64_t stride_cin, int64_t stride_cout, int K, int Cin, int Cout, float* frag_fwd,
                                        float* frag_bwd, void* stream) {
  SV_CHECK_ARG(W && K > 0 && Cin > 0 && Cout > 0 && Cin % 16 == 0 && Cout % 16 == 0, "sv_conv_weight_fragments: channels must be multiples of 16");
  SV_CHECK_ARG(frag_fwd || frag_bwd, "sv_conv_weight_fragments: no output");
  SV_CHECK_ARG(((uintptr_t)frag_fwd % 16 == 0) && ((uintptr_t)frag_bwd % 16 == 0), "sv_conv_weight_fragments: outputs must be 16-byte aligned");
  const WStride ws{stride_k, stride_cin, stride_cout};
  hipLaunchKernelGGL(k_weight_fragments, dim3(sv_grid_1d((int64_t)K * Cin * Cout / 2, 256)), dim3(256), 0, sv_stream(stream), W, ws, K, Cin, Cout, frag_fwd,
                     frag_bwd);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// All layers of a network in ONE launch: descs (n, 10) int64 on the device = {W, stride_k, stride_cin, stride_cout, K, C_in, C_out, frag_fwd,
// frag_bwd, first float4 unit of the layer in the launch}; a step of the bench re-lays 11 layers (the fragments follow the weights every
// forward, see spconv/functional.py), one 4 us launch each before.
struct FragDesc {
  const float* w;
  int64_t sk, si, so, K, Cin, Cout;
  float* fwd;
  float* bwd;
  int64_t unit0;
};
__global__ __launch_bounds__(256) void k_weight_fragments_batch(const FragDesc* __restrict__ descs, int n, int64_t total_units) {
  for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < total_units; u += (int64_t)gridDim.x * 256) {
    int l = 0;
    while (l + 1 < n && descs[l + 1].unit0 <= u) ++l;
    const FragDesc d = descs[l];
    const int K = (int)d.K, Cin = (int)d.Cin, Cout = (int)d.Cout;
    const int total = K * Cin * Cout / 4;
    const int i = (int)(u - d.unit0);
    const bool bwd = i >= total;
    const int e = bwd ? i - total : i;
    const int Nc = bwd ? Cin : Cout, Kd = bwd ? Cout : Cin;
    const int64_t sn = bwd ? d.si : d.so, sc = bwd ? d.so : d.si;
    const int KQ = Kd / 16, NT = Nc / 16;
    const int lane = e & 63, t = (e >> 6) % NT, q = ((e >> 6) / NT) % KQ, k = (e >> 6) / (NT * KQ);
    const int li = lane & 15, kk = lane >> 4;
    const float* src = d.w + k * d.sk + (t * 16 + li) * sn + (q * 16 + kk * 4) * sc;
    float4 v;
    if (sc == 1 && (((uintptr_t)src) & 15) == 0) v = *reinterpret_cast<const float4*>(src);
    else v = make_float4(src[0], src[sc], src[2 * sc], src[3 * sc]);
    reinterpret_cast<float4*>(bwd ? d.bwd : d.fwd)[e] = v;
  }
}

extern "C" int sv_conv_weight_fragments_batch(const void* descs_device, int n_layers, int64_t total_units, void* stream) {
  SV_CHECK_ARG(n_layers >= 0 && total_units >= 0, "sv_conv_weight_fragments_batch: bad sizes");
  if (n_layers == 0 || total_units == 0) return SV_OK;
  SV_CHECK_ARG(descs_device, "sv_conv_weight_fragments_batch: null pointer");
  hipLaunchKernelGGL(k_weight_fragments_batch, dim3(sv_grid_1d(total_units, 256, 2048)), dim3(256), 0, sv_stream(stream),
                     static_cast<const FragDesc*>(descs_device), n_layers, total_units);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ------------------------------------------------------------------------------------------------
// The MFMA kernel on a plan.  Register-stationary like k_spconv_rs above, plus:
//   * PMC on k_spconv_rs: matrix core busy 38 %, waves waiting for operands that were requested only one 64-MFMA step (~2000 cycles)
//     earlier, less than the gather latency under load; hipcc additionally sinks its own prefetch loads towards their first use.  Here
//     every operand load of the loop is an inline-asm buffer_load_dwordx4 (hipcc can neither move it nor wait for it), issued TWO steps
//     ahead into a 3-deep register ring, and retired with a counted s_waitcnt vmcnt(2 x loads-per-step) that names the stage's registers
//     ("+v", form (ii) of cdna_hip_programming.md 5.7).  Every step issues exactly RS_G + NT loads: rows without a neighbour use an
//     out-of-range buffer offset (the range check returns zeros without a memory access), steps past the end issue out-of-range dummies;
//   * a wave's tiles come from the plan: tile_of[wave][slot] inside the region of its XCD (blockIdx.x % 8), rows + masks + output rows
//     from the regrouped row-major table (one 128-byte line per row);
//   * blockIdx.y selects a block of 64 output columns (C_out = 128 runs as two column blocks that gather the same rows);
//   * the wave's neighbour indices are parked in LDS once, so the loop contains no compiler-visible VMEM load.
// Same ownership, skipping and summation order (k ascending, channels ascending) as k_spconv_rs -> bitwise reproducible, and bit-identical to
// the ungrouped kernels.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ i32x4 make_srd(const void* p, uint32_t bytes) {
  const uint64_t a = (uint64_t)p;
  i32x4 r;
  r.x = __builtin_amdgcn_readfirstlane((int)(uint32_t)a);
  r.y = __builtin_amdgcn_readfirstlane((int)(uint32_t)((a >> 32) & 0xffffu));      // stride 0
  r.z = __builtin_amdgcn_readfirstlane((int)bytes);
  r.w = 0x00020000;
  return r;
}
__device__ __forceinline__ f32x4 buf_load_b128(i32x4 srd, uint32_t voff) {
  f32x4 v;
  asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen" : "=v"(v) : "v"(voff), "s"(srd) : "memory");
  return v;
}
// address = base + soff (SGPR) + voff (VGPR) + IMM; the range check looks at voff + IMM only, so an out-of-range voff still returns zeros
// without a memory access whatever soff is
// (cache-policy bits on these loads -- nt, sc1, sc0 sc1, rows and weights separately -- were measured and changed nothing: DESIGN.md)
template <int IMM>
__device__ __forceinline__ f32x4 buf_load_b128_s(i32x4 srd, uint32_t voff, uint32_t soff) {
  f32x4 v;
  asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen offset:%4" : "=v"(v) : "v"(voff), "s"(srd), "s"(soff), "i"(IMM) : "memory");
  return v;
}

struct PlanView {
  const int32_t* tab;       // (n_rows, PL_ROW) row-major table, natural row order
  const int32_t* perm;      // (n_pad) row at each position (-1 padding)
  const int32_t* masks_p;   // (n_pad) its mask
  const int32_t* tile_of;   // [wave][G]
  PlanDims d;
  int k_flip;               // read table entry K-1-k for offset k (a submanifold table serving its own data gradient)
  int nc_total;             // columns of Y and of the weight fragments (a.Nc is the block's share)
  float* bn_partial;        // (gridDim.x, 2, nc_total) per-workgroup column sums / sums of squares of Y, or null (BatchNorm statistics made here)
  // BatchNorm BACKWARD sums instead (a data-gradient launch whose output Y is the gradient dy of a BatchNorm(+ReLU) output): bn_x = that
  // BatchNorm's input (n_rows, nc_total), its saved batch statistics and affine parameters; the partials are {sum of masked dy, sum of masked
  // dy * xhat} -- what k_bn_reduce<true> makes in a pass of its own.  bn_x null: forward statistics of Y.
  const float* bn_x;
  const float* bn_mean;
  const float* bn_istd;
  const float* bn_gamma;    // may be null (1)
  const float* bn_beta;     // may be null (0)
  int bn_relu;
#if SEEVCN_MEASURE
  int debug;                // SEEVCN_RS3_DEBUG (results are wrong): 1 no gathered-row loads, 2 no weight loads, 4 no MFMAs,
                            // 8 / 16 weight / row loads of a wave all at ONE address (one cache line per load instead of 16)
  unsigned long long* trace;   // sv_debug_conv_trace: 8 words per wave, or null
#else
  static constexpr int debug = 0;                          // the DBG instances exist in the measurement build only
  static constexpr unsigned long long* trace = nullptr;
#endif
  const float* in_coef;     // FIN instances: (2, Kd) scale | shift applied to every gathered X value (+ ReLU when in_relu); see InNorm
  int in_relu;
  int epi_rows;             // a launch with an epilogue stores whole rows through the staging tile (its terms and Y are 16-byte aligned); 0: per accumulator
};

// DBG (measurement build only): 0 production; 1 the measurement switches of PlanView::debug (+ trace); 2 per-wave trace only (the production loop +
// a few s_memtime per pass)
// FIN: the gathered rows go through pv.in_coef (BatchNorm + ReLU of the layer below applied on load) -- production instances only
template <int NT, int KQ, int RS_G, int DBG = 0, bool FIN = false>
__global__ __launch_bounds__(256, PL_WAVES_PER_SIMD) void k_spconv_rs3(ConvArgs a, PlanView pv, const float* __restrict__ wfrag, uint32_t x_bytes,
                                                                        uint32_t w_bytes) {
  constexpr int Kd = KQ * 16;
  __shared__ int32_t s_idx_all[4][RS3_KMAX + 1][64];       // [k][lane]: source row of (tile lane>>4, row lane&15); [27][lane]: its output row
  __shared__ __attribute__((aligned(16))) float s_coef[2][FIN ? Kd : 4];      // (scale | shift) of the input transform
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int li = lane & 15, kk = lane >> 4;
  const int region = blockIdx.x % PL_REGIONS, lw = (blockIdx.x / PL_REGIONS) * 4 + wid;
  const unsigned long long t_start = (DBG && pv.trace) ? __builtin_amdgcn_s_memtime() : 0ull;    // per-wave stamps: debug / trace instances only
  unsigned long long t_pro = 0ull, t_loop = 0ull, t_mark = t_start;      // cycles in pass prologues / main loops, summed over the passes
  unsigned trace_work = 0;
  int32_t(*s_idx)[64] = s_idx_all[wid];
  float in_lo = 0.f;
  if constexpr (FIN) {
    for (int c = threadIdx.x; c < 2 * Kd; c += 256) s_coef[c / Kd][c % Kd] = pv.in_coef[c];
    in_lo = pv.in_relu ? 0.f : -__builtin_inff();
  }
  const int nt_total = pv.nc_total / 16, col_tile0 = blockIdx.y * NT;
  const i32x4 srd_x = make_srd(a.X, x_bytes), srd_w = make_srd(wfrag, w_bytes);
  const int32_t* my_tiles = pv.tile_of + ((int64_t)region * PL_REGION_WAVES + lw) * (pv.d.n_pass * RS_G);
  if constexpr (FIN) __syncthreads();                      // the only workgroup barrier in front of the epilogue

  // BatchNorm statistics: lane c < 16 NT sums column c of every tile the wave stores, read back from the staging tile row by row (fixed order).
  // Two registers carried across the pass loop; the first version summed straight from the accumulators (column 16 t + li in lane (li, kk):
  // 2 NT registers), which hipcc spilled around the main loop at four waves per SIMD.
  float bn0 = 0.f, bn1 = 0.f;
#pragma nounroll
  for (int pass = 0; pass < pv.d.n_pass; ++pass) {
  if (my_tiles[pass * RS_G] < 0) break;                    // slots are filled front to back: an empty first slot ends the wave's list
  // the wave's rows of the regrouped table -> LDS; per-offset tile masks in lane k of maskreg
  unsigned maskreg = 0;
  {
    const int g = lane >> 4;
    const int32_t t = g < RS_G ? my_tiles[pass * RS_G + g] : -1;
    i32x4 e[PL_ROW / 4];
    const int64_t p = (int64_t)t * 16 + li;
    const int32_t row = t >= 0 ? pv.perm[p] : -1;
    unsigned m = row >= 0 ? (unsigned)pv.masks_p[p] : 0u;
    if (row >= 0) {
      const i32x4* rowp = reinterpret_cast<const i32x4*>(pv.tab + (int64_t)row * PL_ROW);
#pragma unroll
      for (int q = 0; q < (RS3_KMAX + 3) / 4; ++q) e[q] = rowp[q];
    } else {
#pragma unroll
      for (int q = 0; q < (RS3_KMAX + 3) / 4; ++q) e[q] = (i32x4){-1, -1, -1, -1};
    }
#pragma unroll
    for (int k = 0; k < RS3_KMAX; ++k)
      s_idx[k][lane] = e[k >> 2][k & 3];            // table order (entries >= K are -1 in the table); a reversed table is read at K-1-k in the loop
    s_idx[RS3_KMAX][lane] = row;                           // output row (-1: padding)
    if (pv.k_flip) m = __brev(m) >> (32 - a.K);
    unsigned mall = m;                                                      // FIN: offsets EVERY row of the tile has (a padding row has none: its tile always clears)
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) m |= __shfl_xor(m, off, 16);      // OR over the tile's 16 rows
    if constexpr (FIN) {
#pragma unroll
      for (int off = 8; off > 0; off >>= 1) mall &= __shfl_xor(mall, off, 16);
    }
    unsigned mk = 0;
#pragma unroll
    for (int t2 = 0; t2 < RS_G; ++t2) {
      const unsigned tm = (unsigned)__builtin_amdgcn_readlane((int)m, 16 * t2);
      mk |= ((tm >> (lane & 31)) & 1u) << t2;
      if constexpr (FIN) {                                                  // bit 8 + t2: tile t2 has a neighbour in every row at this offset
        const unsigned ta = (unsigned)__builtin_amdgcn_readlane((int)mall, 16 * t2);
        mk |= ((ta >> (lane & 31)) & 1u) << (8 + t2);
      }
    }
    maskreg = lane < a.K ? mk : 0u;
  }
  const unsigned long long active = __ballot((maskreg & 0xffu) != 0);
  if constexpr (DBG != 0) {
    if (pv.trace) {
      const unsigned long long t = __builtin_amdgcn_s_memtime();
      t_pro += t - t_mark, t_mark = t;
    }
  }

  f32x4 acc[RS_G][NT];
#pragma unroll
  for (int g = 0; g < RS_G; ++g)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[g][t] = (f32x4){0.f, 0.f, 0.f, 0.f};

  if (active) {
    // Operand rings.  Rows (A): RA stages = RA - 1 steps of gathers in flight (a gathered row comes from HBM / a remote L2 line: ~2 us under load).
    // Weights (B): RB = 2 stages, ONE step ahead -- the 442 KB of fragments are shared by every wave of the launch and sit in L2, a step of four
    // waves' MFMAs (~4 k cycles) covers that latency; the third B stage (16 VGPRs at NT = 4) is what kept the two-tile instances at the
    // 128-register line with spills in every pass prologue, and is what the input transform's (FIN) coefficients now live in.
    // (History: one ring of 3 stages for both operands until round 5.  Tried on it: 5 stages for the one-tile-per-wave instance -- slower,
    // 64->64 at 66 k rows 78 -> 85 us, 64->128 28 -> 39 us: the extra dummy loads of the tail and the longer prologue cost more than the
    // lookahead buys (round 1 found the same on the narrow kernels); 4 stages for it in round 3 (128 VGPRs, no spill): 65.5 -> 67-68 us.)
    constexpr int RA = 3, RB = 2;
    f32x4 A[RA][RS_G], B[RB][NT];
    // defined here so that their live ranges start inside the pass (the asm waits below read-modify them: left undefined, hipcc keeps all
    // stage registers alive across the whole pass loop, prologue and epilogue included, and spills 55 VGPRs at four waves per SIMD)
#pragma unroll
    for (int st = 0; st < RA; ++st)
#pragma unroll
      for (int g = 0; g < RS_G; ++g) A[st][g] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int st = 0; st < RB; ++st)
#pragma unroll
      for (int t = 0; t < NT; ++t) B[st][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    constexpr uint32_t OOB = 0xfffffff0u;
    // the weight loads add immediates of up to 3 KiB to their vector offset: an out-of-range value that cannot wrap around 2^32 with them
    // (the fragment buffer is a few MB)
    constexpr uint32_t WOOB = 0x80000000u;
    constexpr uint32_t WSTEP = 1024u;                                // one (offset, q, column tile) fragment
    const uint32_t wq = (uint32_t)nt_total * WSTEP;                   // q -> q + 1
    const uint32_t wlane = (uint32_t)lane * 16u;
    auto math = [&](f32x4 (&As)[RS_G], f32x4 (&Bs)[NT], const int qc, const unsigned mc, const int32_t (&fin_absent)[RS_G]) {
      // Issue order inside a step: weights of step s + 1, then rows of step s + RA - 1.  The younger of this step's operands is its weight stage
      // (issued one step ago, in front of that step's row loads): behind it in the queue are one step's row loads and one whole step,
      // NWAIT = RS_G + (RS_G + NT) loads that may stay outstanding; loads return in order, so the row stage (older) has arrived as well.
        // FIN: the step's coefficients (channels 16 qc + 4 kk + {0..3} of the lane's four values) and the rows' validity are LDS reads that do not
      // depend on the operands: requested here, in front of the wait, their latency hides behind it (behind it they sat on every step's critical
      // path: the two-tile forward at 139 k rows ran 127 us against 115 without the transform)
      f32x4 fin_sc, fin_sh;
      if constexpr (FIN) fin_sc = *reinterpret_cast<const f32x4*>(&s_coef[0][qc * 16 + kk * 4]), fin_sh = *reinterpret_cast<const f32x4*>(&s_coef[1][qc * 16 + kk * 4]);
      constexpr int NWAIT = RS_G + (RB - 1) * (RS_G + NT);
#define RS3_WAIT(...) asm volatile("s_waitcnt vmcnt(%[nw])" : __VA_ARGS__ : [nw] "n"(NWAIT))
#define V(x) "+v"(x)
      if constexpr (RS_G == 4 && NT == 4) { RS3_WAIT(V(As[0]), V(As[1]), V(As[2]), V(As[3]), V(Bs[0]), V(Bs[1]), V(Bs[2]), V(Bs[3])); }
      else if constexpr (RS_G == 4 && NT == 2) { RS3_WAIT(V(As[0]), V(As[1]), V(As[2]), V(As[3]), V(Bs[0]), V(Bs[1])); }
      else if constexpr (RS_G == 4 && NT == 1) { RS3_WAIT(V(As[0]), V(As[1]), V(As[2]), V(As[3]), V(Bs[0])); }
      else if constexpr (RS_G == 2 && NT == 4) { RS3_WAIT(V(As[0]), V(As[1]), V(Bs[0]), V(Bs[1]), V(Bs[2]), V(Bs[3])); }
      else if constexpr (RS_G == 2 && NT == 2) { RS3_WAIT(V(As[0]), V(As[1]), V(Bs[0]), V(Bs[1])); }
      else if constexpr (RS_G == 1 && NT == 4) { RS3_WAIT(V(As[0]), V(Bs[0]), V(Bs[1]), V(Bs[2]), V(Bs[3])); }
      else {
        static_assert(RS_G == 2 && NT == 1, "no counted wait for this (tiles per wave, column tiles) pair");
        RS3_WAIT(V(As[0]), V(As[1]), V(Bs[0]));
      }
#undef V
#undef RS3_WAIT
      // per tile: 4 passes over the NT column tiles, so that consecutive MFMAs never share an accumulator (a dependent
      // v_mfma_f32_16x16x4_f32 issues 47 cycles after its producer, an independent one after 32).
      // FIN: the transform of a tile's k-th operand register (fused multiply-add, max, and -- unless every row of the tile has this neighbour -- the
      // clearing of the rows without one) is written BEHIND the first MFMA of the register before it: the wave issues it while the matrix pipe works
      // on that MFMA instead of in front of the step's whole MFMA block (12-15 % on every forward launch when it sat there).
      auto fin1 = [&](int g, int i) {
        float v = fmaxf(__fmaf_rn(As[g][i], fin_sc[i], fin_sh[i]), in_lo);
        if (!((mc >> (8 + g)) & 1u)) v = __uint_as_float(__float_as_uint(v) & ~(uint32_t)fin_absent[g]);       // wave-uniform test
        As[g][i] = v;
      };
#pragma unroll
      for (int g = 0; g < RS_G; ++g)
        if (((mc >> g) & 1u) && !(DBG == 1 && (pv.debug & 4))) {
          if constexpr (FIN) fin1(g, 0);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            acc[g][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(As[g][i], Bs[0][i], acc[g][0], 0, 0, 0);
            if constexpr (FIN) {
              if (i + 1 < 4) fin1(g, i + 1);
            }
#pragma unroll
            for (int t = 1; t < NT; ++t) acc[g][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(As[g][i], Bs[t][i], acc[g][t], 0, 0, 0);
          }
        }
    };
    if constexpr (KQ >= 2) {
      // The loop by OFFSET (round 6).  The first form below keeps three iterators (row loads, weight loads, compute) that each test "was this
      // the offset's last 16-channel step" in EVERY step: ~30 scalar instructions and 6-8 taken branches between two MFMA blocks (hipcc keeps
      // a step's MFMAs together, the bookkeeping is not interleaved with them).  With four waves on a SIMD the others' MFMAs cover that; a wave
      // left ALONE does not: per-wave stamps (tools/conv_trace.py, profiles/r06_conv_trace_raw.txt) show every 64 -> 64 launch of <= 74 k rows
      // ending with its 27-offset tiles, each walking 108 steps at ~1080 cycles where its 16 MFMAs need 512 -- the launch lasts as long as
      // that wave (144 k cycles where the busiest SIMD needs 113 k, the mean one 89 k).  Here an iteration is one offset: its KQ steps are
      // unrolled with compile-time q, the rows of step s + 2 and the weights of step s + 1 are "this offset's q + 2 / q + 1 or the next
      // offset's q + 2 - KQ / 0" decided at compile time, and the list advances ONCE per offset (next offset, its gathered-row offsets from
      // LDS, its weight base, its tile mask).  Three offsets per trip make the ring stages compile-time too (KQ steps per offset, 3 row stages).
      // Same loads in the same order, same counted wait, same MFMA order: bit-identical results.
      unsigned long long rest = active;                              // offsets behind k_n
      int k_c = __ffsll((long long)rest) - 1;
      rest &= rest - 1;
      int k_n = rest ? __ffsll((long long)rest) - 1 : -1;
      rest &= rest - 1;
      auto rows_of = [&](int k, uint32_t (&ro)[RS_G]) {              // k >= 0: byte offset of the lane's gathered row (+ its 4-channel column), OOB without a neighbour
#pragma unroll
        for (int g = 0; g < RS_G; ++g) {
          const int32_t j = s_idx[pv.k_flip ? a.K - 1 - k : k][g * 16 + li];
          ro[g] = j >= 0 ? (uint32_t)(j * (Kd * 4) + kk * 16) : OOB;
          if constexpr (DBG == 1) {
            if (pv.debug & 1) ro[g] = OOB;
            else if ((pv.debug & 16) && j >= 0) ro[g] = 0u;
          }
        }
      };
      auto wbase = [&](int k) { return (uint32_t)(k * KQ * nt_total + col_tile0) * WSTEP; };
      uint32_t ro_c[RS_G], ro_n[RS_G], ro_t[RS_G];
      rows_of(k_c, ro_c);
#pragma unroll
      for (int g = 0; g < RS_G; ++g) ro_n[g] = OOB;
      if (k_n >= 0) rows_of(k_n, ro_n);
      uint32_t wv_c = wlane;
      if constexpr (DBG == 1) {
        if (pv.debug & 2) wv_c = WOOB;
        else if (pv.debug & 8) wv_c = 0u;
      }
      uint32_t wv_n = k_n >= 0 ? wv_c : WOOB;                         // past the list's end: out-of-range dummies (exactly NT + RS_G loads per step, always)
      uint32_t sw_c = wbase(k_c), sw_n = k_n >= 0 ? wbase(k_n) : 0u;
      unsigned mc = (unsigned)__builtin_amdgcn_readlane((int)maskreg, k_c);
      auto load_a = [&](f32x4 (&As)[RS_G], const uint32_t (&ro)[RS_G], uint32_t sa) {
#pragma unroll
        for (int g = 0; g < RS_G; ++g) As[g] = buf_load_b128_s<0>(srd_x, ro[g], sa);
      };
      auto load_b = [&](f32x4 (&Bs)[NT], uint32_t wv, uint32_t sw) {
        if constexpr (NT >= 1) Bs[0] = buf_load_b128_s<0>(srd_w, wv, sw);
        if constexpr (NT >= 2) Bs[1] = buf_load_b128_s<1024>(srd_w, wv, sw);
        if constexpr (NT >= 3) Bs[2] = buf_load_b128_s<2048>(srd_w, wv, sw);
        if constexpr (NT >= 4) Bs[3] = buf_load_b128_s<3072>(srd_w, wv, sw);
      };
      constexpr int LA = RA - 1, LB = RB - 1;                         // steps of row / weight loads in flight
      static_assert(LA <= KQ && LB <= LA, "a step's loads reach at most into the next offset");
      constexpr int NTRIP = RA;                                       // offsets per trip: the ring stages of a step are compile-time
      static_assert((KQ * NTRIP) % RA == 0 && (KQ * NTRIP) % RB == 0, "a trip is whole turns of both rings");
      // ring fill, in the loop's own issue order (virtual steps -LA .. -1: weights of step v + LB, then rows of step v + LA; all in the first offset)
#pragma unroll
      for (int v = -LA; v < 0; ++v) {
        if (v + LB >= 0) load_b(B[(v + LB) % RB], wv_c, sw_c + (uint32_t)(v + LB) * wq);
        load_a(A[(v + LA) % RA], ro_c, 64u * (uint32_t)(v + LA));
      }
      for (bool more = true; more;) {
#pragma unroll
        for (int u = 0; u < NTRIP; ++u) {
          int32_t absent[RS_G];
#pragma unroll
          for (int g = 0; g < RS_G; ++g) absent[g] = FIN ? (ro_c[g] == OOB ? -1 : 0) : 0;     // all-ones: the row has no neighbour at this offset
          int k_t = -1;
#pragma unroll
          for (int q = 0; q < KQ; ++q) {
            const int st = u * KQ + q;                               // step inside the trip (compile-time after unrolling)
            if (q + LB < KQ) load_b(B[(st + LB) % RB], wv_c, sw_c + (uint32_t)(q + LB) * wq);
            else load_b(B[(st + LB) % RB], wv_n, sw_n + (uint32_t)(q + LB - KQ) * wq);
            if (q + LA < KQ) load_a(A[(st + LA) % RA], ro_c, 64u * (uint32_t)(q + LA));
            else load_a(A[(st + LA) % RA], ro_n, 64u * (uint32_t)(q + LA - KQ));
            if (q == KQ - 1) {
              // the offset behind the next one: its rows' offsets are requested from LDS here, in front of this step's MFMAs, and first used
              // KQ - LA steps into the next offset
              k_t = rest ? __ffsll((long long)rest) - 1 : -1;
              rest &= rest - 1;
#pragma unroll
              for (int g = 0; g < RS_G; ++g) ro_t[g] = OOB;
              if (k_t >= 0) rows_of(k_t, ro_t);
            }
            math(A[st % RA], B[st % RB], q, mc, absent);
          }
          k_c = k_n, k_n = k_t;
          if (k_c < 0) {
            more = false;
            break;
          }
#pragma unroll
          for (int g = 0; g < RS_G; ++g) ro_c[g] = ro_n[g], ro_n[g] = ro_t[g];
          sw_c = sw_n, sw_n = k_n >= 0 ? wbase(k_n) : 0u;
          wv_n = k_n >= 0 ? wv_c : WOOB;
          mc = (unsigned)__builtin_amdgcn_readlane((int)maskreg, k_c);
        }
      }
    } else {
    // Row-load iterator (RA - 1 steps ahead of the compute iterator).  Per offset: rowoff[g] = byte offset of the lane's gathered row (+ its
    // 4-channel column), or an out-of-range value when the row has no neighbour there / the list has ended.  Per 16-channel step the loads then
    // need NO vector arithmetic: rows at rowoff + (scalar) 64 * q, weights at one constant per-lane offset + (scalar) fragment base of
    // (offset, q) + (immediate) 1 KiB * column tile.  (The first version recomputed every load's offset each step: 74 scalar + 25 vector
    // instructions per step next to its 32 MFMAs.)
    unsigned long long la = active;
    int kl = __ffsll((long long)la) - 1, ql = 0;
    uint32_t rowoff[RS_G];
    uint32_t wvoff = wlane;                                          // OOB once the list has ended (dummy loads)
    auto read_j = [&]() {
#pragma unroll
      for (int g = 0; g < RS_G; ++g) {
        const int32_t j = s_idx[pv.k_flip ? a.K - 1 - kl : kl][g * 16 + li];
        rowoff[g] = j >= 0 ? (uint32_t)(j * (Kd * 4) + kk * 16) : OOB;
        if constexpr (DBG == 1) {
          if (pv.debug & 1) rowoff[g] = OOB;
          else if ((pv.debug & 16) && j >= 0) rowoff[g] = 0u;
        }
      }
    };
    read_j();
    if constexpr (DBG == 1) {
      if (pv.debug & 2) wvoff = WOOB;
      else if (pv.debug & 8) wvoff = 0u;
    }
    // running scalar offsets: sa = 64 * q (rows), sw = fragment base of (offset, q) (weights)
    uint32_t sa = 0u;
    auto issue_a = [&](f32x4 (&As)[RS_G]) {                          // exactly RS_G loads, always
#pragma unroll
      for (int g = 0; g < RS_G; ++g) As[g] = buf_load_b128_s<0>(srd_x, rowoff[g], sa);
      if (kl >= 0) {
        sa += 64u;
        if (++ql == KQ) {
          ql = 0, sa = 0u;
          la &= la - 1;
          kl = la ? __ffsll((long long)la) - 1 : -1;
          if (kl >= 0) read_j();
          else {                                                   // the list has ended: every further load is an out-of-range dummy
#pragma unroll
            for (int g = 0; g < RS_G; ++g) rowoff[g] = OOB;
          }
        }
      }
    };
    // weight-load iterator (one step ahead)
    unsigned long long lb = active;
    int kb = __ffsll((long long)lb) - 1, qb = 0;
    uint32_t sw = (uint32_t)((kb < 0 ? 0 : kb) * KQ * nt_total + col_tile0) * WSTEP;
    auto issue_b = [&](f32x4 (&Bs)[NT]) {                            // exactly NT loads, always
      if constexpr (NT >= 1) Bs[0] = buf_load_b128_s<0>(srd_w, wvoff, sw);
      if constexpr (NT >= 2) Bs[1] = buf_load_b128_s<1024>(srd_w, wvoff, sw);
      if constexpr (NT >= 3) Bs[2] = buf_load_b128_s<2048>(srd_w, wvoff, sw);
      if constexpr (NT >= 4) Bs[3] = buf_load_b128_s<3072>(srd_w, wvoff, sw);
      if (kb >= 0) {
        sw += wq;
        if (++qb == KQ) {
          qb = 0;
          lb &= lb - 1;
          kb = lb ? __ffsll((long long)lb) - 1 : -1;
          if (kb >= 0) sw = (uint32_t)(kb * KQ * nt_total + col_tile0) * WSTEP;
          else wvoff = WOOB;
        }
      }
    };
    // compute iterator
    unsigned long long ca = active;
    int kc = __ffsll((long long)ca) - 1, qc = 0;
    unsigned mc = (unsigned)__builtin_amdgcn_readlane((int)maskreg, kc);
    auto compute = [&](f32x4 (&As)[RS_G], f32x4 (&Bs)[NT]) {
      int32_t fin_absent[RS_G];
#pragma unroll
      for (int g = 0; g < RS_G; ++g) fin_absent[g] = 0;
      if constexpr (FIN) {
#pragma unroll
        for (int g = 0; g < RS_G; ++g) fin_absent[g] = s_idx[pv.k_flip ? a.K - 1 - kc : kc][g * 16 + li] >> 31;     // all-ones: no neighbour
      }
      math(As, Bs, qc, mc, fin_absent);
      if (++qc == KQ) {
        qc = 0;
        ca &= ca - 1;
        kc = ca ? __ffsll((long long)ca) - 1 : -1;
        if (kc >= 0) mc = (unsigned)__builtin_amdgcn_readlane((int)maskreg, kc);
      }
    };
    // the steps in front of the first compute, in the loop's own issue order (virtual steps -(RA - 1) .. -1)
#pragma unroll
    for (int s0 = -(RA - 1); s0 < 0; ++s0) {
      if (s0 + RB - 1 >= 0) issue_b(B[(s0 + RB - 1) % RB]);
      issue_a(A[(s0 + RA - 1) % RA]);
    }
    for (bool more = true; more;) {
#pragma unroll
      for (int u = 0; u < RA * RB; ++u) {                    // whole turns of both rings: the stages of a step are compile-time
        issue_b(B[(u + RB - 1) % RB]);
        issue_a(A[(u + RA - 1) % RA]);
        compute(A[u % RA], B[u % RB]);
        if (kc < 0) {
          more = false;
          break;
        }
      }
    }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // retire the dummy loads before the registers are reused
  }
  if (DBG && pv.trace) {
    const unsigned long long t = __builtin_amdgcn_s_memtime();
    t_loop += t - t_mark, t_mark = t;
    for (int k = 0; k < a.K; ++k) trace_work += __popc((unsigned)__builtin_amdgcn_readlane((int)maskreg, k));
  }
  // D layout (16x16): col = lane&15, row = 4*(lane>>4) + reg
  const bool plain_out = !a.bias && !a.scale && !a.residual && !a.relu;       // the training layers: BatchNorm follows, nothing fused here
  // An opaque copy of the lane id for the epilogue: its addresses (staging tile, output columns) are invariant over the pass loop, hipcc
  // hoists them in front of it and then SPILLS them across the main loop (21 VGPRs, 43 MB of scratch traffic per launch by PMC) -- derived
  // from a value defined here they are computed where they are used.
  int lane_e = lane;
  asm volatile("" : "+v"(lane_e));
  const int li_e = lane_e & 15, kk_e = lane_e >> 4;
  if (plain_out) {
    // Whole rows out: a tile goes through wave-private LDS (rows 0..16 of the neighbour-index block, free now; row RS3_KMAX = the output rows
    // stays) so that the 16 x NT lanes of a row store its 64 * NT bytes with one instruction.  Stored straight from the accumulators a row left
    // as four 64-byte pieces in four instructions: 58 MB written for a 35.7 MB output on the 64-channel layers (PMC WRITE_SIZE, round 2).
    float* T = reinterpret_cast<float*>(&s_idx[0][0]);
    constexpr int TP = NT * 16 + 4;                                 // pitch: 68 floats at NT = 4 (17 index rows of 64 ints hold 16 of them)
    static_assert(16 * TP <= 17 * 64, "the staging tile must fit under the output-row line of the index block");
#pragma unroll
    for (int g = 0; g < RS_G; ++g) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          T[(kk_e * 4 + r) * TP + t * 16 + li_e] = acc[g][t][r];
        }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      if (pv.bn_partial && (NT == 4 || lane_e < NT * 16)) {
        if (pv.bn_x) {
          // backward sums of the BatchNorm whose output gradient this tile is: x rows of the tile (whole 64 NT-byte runs, one per row)
          const int col = col_tile0 * 16 + lane_e;
          const float mean = pv.bn_mean[col], istd = pv.bn_istd[col];
          const float sc = istd * (pv.bn_gamma ? pv.bn_gamma[col] : 1.f), sh = bn_shift(mean, sc, pv.bn_beta ? pv.bn_beta[col] : 0.f);
          float xv[16];
#pragma unroll
          for (int rw = 0; rw < 16; ++rw) {
            const int row = __builtin_amdgcn_readfirstlane(s_idx[RS3_KMAX][g * 16 + rw]);
            xv[rw] = row >= 0 ? pv.bn_x[(int64_t)row * pv.nc_total + col] : 0.f;
          }
#pragma unroll
          for (int rw = 0; rw < 16; ++rw) {
            float d = T[rw * TP + lane_e];                                // padding rows hold zeros
            if (pv.bn_relu) d = bn_act(xv[rw], sc, sh) > 0.f ? d : 0.f;
            bn0 += d, bn1 += d * ((xv[rw] - mean) * istd);
          }
        } else {
#pragma unroll
          for (int rw = 0; rw < 16; ++rw) {
            const float v = T[rw * TP + lane_e];                          // padding rows hold zeros
            bn0 += v, bn1 += v * v;
          }
        }
      }
      constexpr int C4N = NT * 4;                                     // 16-byte pieces per row
#pragma unroll
      for (int i = 0; i < (16 * C4N + 63) / 64; ++i) {
        const int f = lane_e + 64 * i, rw = f / C4N, c4 = f % C4N;
        if (16 * C4N % 64 == 0 || f < 16 * C4N) {
          const int64_t row = s_idx[RS3_KMAX][g * 16 + rw];
          if (row >= 0) *reinterpret_cast<f32x4*>(a.Y + row * pv.nc_total + col_tile0 * 16 + c4 * 4) = *reinterpret_cast<const f32x4*>(T + rw * TP + c4 * 4);
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");          // the next pass refills the index block
  } else if (pv.epi_rows) {
    // Whole rows out with an epilogue (every launch of an eval-mode forward): the same staging tile, then a lane applies the epilogue to its 16-byte
    // piece -- bias / scale / shift of its four columns as one float4 each, the residual row piece as one 16-byte load -- and stores it.  Per
    // element the operations of conv_epilogue in its order (add, one fused multiply-add, add, max): the bits of the per-accumulator form below.
    // Padding rows (row < 0) are neither read nor written.
    float* T = reinterpret_cast<float*>(&s_idx[0][0]);
    constexpr int TP = NT * 16 + 4;
    constexpr int C4N = NT * 4;                                       // 16-byte pieces per row
#pragma unroll
    for (int g = 0; g < RS_G; ++g) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          T[(kk_e * 4 + r) * TP + t * 16 + li_e] = acc[g][t][r];
        }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
#pragma unroll
      for (int i = 0; i < (16 * C4N + 63) / 64; ++i) {
        const int f = lane_e + 64 * i, rw = f / C4N, c4 = f % C4N;
        if (16 * C4N % 64 == 0 || f < 16 * C4N) {
          const int64_t row = s_idx[RS3_KMAX][g * 16 + rw];
          if (row >= 0) {
            const int col = col_tile0 * 16 + c4 * 4;
            f32x4 v = *reinterpret_cast<const f32x4*>(T + rw * TP + c4 * 4);
            if (a.bias) v += *reinterpret_cast<const f32x4*>(a.bias + col);
            if (a.scale) {
              const f32x4 sc = *reinterpret_cast<const f32x4*>(a.scale + col), sh = *reinterpret_cast<const f32x4*>(a.shift + col);
              v = (f32x4){bn_act(v[0], sc[0], sh[0]), bn_act(v[1], sc[1], sh[1]), bn_act(v[2], sc[2], sh[2]), bn_act(v[3], sc[3], sh[3])};
            }
            if (a.residual) v += *reinterpret_cast<const f32x4*>(a.residual + row * pv.nc_total + col);
            if (a.relu) v = (f32x4){fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f)};
            *reinterpret_cast<f32x4*>(a.Y + row * pv.nc_total + col) = v;
          }
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");          // the next pass refills the index block
  } else {
    // epilogue terms that are not 16-byte aligned (or SEEVCN_RS3_EPI_ROWS=0, A/B): straight from the accumulators, 4-byte accesses
#pragma unroll
    for (int g = 0; g < RS_G; ++g)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row = s_idx[RS3_KMAX][g * 16 + kk_e * 4 + r];
        if (row < 0) continue;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const int col = (col_tile0 + t) * 16 + li_e;
          a.Y[row * pv.nc_total + col] = conv_epilogue(acc[g][t][r], col, row, a);
        }
      }
  }
    if (DBG && pv.trace) t_mark = __builtin_amdgcn_s_memtime();          // the pass's epilogue ends here: (life - prologues - loops) is epilogue time
  }   // pass
  if (pv.bn_partial) {
    // BatchNorm statistics of this launch's output: lane c holds column c of its wave -> the workgroup (4 waves, fixed order) -> one partial
    // per workgroup and column, combined by k_bn_finalize in a fixed order
    __shared__ float s_bn[4][2][64];
    if (NT == 4 || lane < NT * 16) s_bn[wid][0][lane] = bn0, s_bn[wid][1][lane] = bn1;
    __syncthreads();
    for (int e = threadIdx.x; e < 2 * NT * 16; e += 256) {
      const int which = e / (NT * 16), c = e % (NT * 16);
      const float v = (s_bn[0][which][c] + s_bn[1][which][c]) + (s_bn[2][which][c] + s_bn[3][which][c]);
      pv.bn_partial[((size_t)blockIdx.x * 2 + which) * pv.nc_total + col_tile0 * 16 + c] = v;
    }
  }
  if (DBG && pv.trace && lane == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned long long t_end = __builtin_amdgcn_s_memtime();
    unsigned hw = 0, xcc = 0;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    const unsigned work = trace_work;
    unsigned long long* o = pv.trace + (((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 4 + wid) * 8;
    o[0] = t_start, o[1] = t_pro, o[2] = t_loop, o[3] = t_end, o[4] = hw, o[5] = xcc, o[6] = work, o[7] = ((unsigned long long)blockIdx.x << 8) | wid;
  }
}

// shapes the plan kernel is instantiated for: C_in in {16, 32, 64, 128}, C_out in {16, 32, 64} or a multiple of 64, K <= 27
static bool rs3_applies(int K, int Kd, int Nc) {
  if (K > RS3_KMAX || K < 1) return false;
  const bool kd_ok = Kd == 16 || Kd == 32 || Kd == 64 || Kd == 128;
  const bool nc_ok = Nc == 16 || Nc == 32 || (Nc >= 64 && Nc % 64 == 0 && Nc <= 512);
  return kd_ok && nc_ok;
}
// workgroups along x of every planned launch = BatchNorm partials its epilogue writes
extern "C" int sv_conv_planned_partials(void) { return PL_REGIONS * PL_REGION_WAVES / 4; }

extern "C" int sv_conv_mfma_kernel_applies(int K, int Kd, int Nc, int64_t n_src) {
  // the gathers address X through a 32-bit buffer descriptor
  return (rs3_applies(K, Kd, Nc) && (uint64_t)(n_src < 0 ? 0 : n_src) * Kd * 4 < 0xfffffff0ull) ? 1 : 0;
}

template <int NT, int KQ>
static void launch_rs3_g(const ConvArgs& a, const PlanView& pv, const float* wfrag, uint32_t xb, uint32_t wb, dim3 grid, hipStream_t st) {
  // tiles per pass: sv_conv_tiles_per_wave (1 or 2 for the 64-column kernels, 4 for the narrow ones)
#if SEEVCN_MEASURE
  // the switches of SEEVCN_RS3_DEBUG live in instances of their own so that the production loop carries none of their tests
  if (pv.debug) {
    if constexpr (NT == 4) {
      if (pv.d.G == 1) hipLaunchKernelGGL((k_spconv_rs3<NT, KQ, 1, 1>), grid, dim3(256), 0, st, a, pv, wfrag, xb, wb);
      else hipLaunchKernelGGL((k_spconv_rs3<NT, KQ, 2, 1>), grid, dim3(256), 0, st, a, pv, wfrag, xb, wb);
    } else {
      hipLaunchKernelGGL((k_spconv_rs3<NT, KQ, 4, 1>), grid, dim3(256), 0, st, a, pv, wfrag, xb, wb);
    }
    return;
  }
  if (pv.trace) {                      // the production loop with time stamps
    if constexpr (NT == 4) {
      if (pv.d.G == 1) hipLaunchKernelGGL((k_spconv_rs3<NT, KQ, 1, 2>), grid, dim3(256), 0, st, a, pv, wfrag, xb, wb);
      else hipLaunchKernelGGL((k_spconv_rs3<NT, KQ, 2, 2>), grid, dim3(256), 0, st, a, pv, wfrag, xb, wb);
    } else {
      hipLaunchKernelGGL((k_spconv_rs3<NT, KQ, 4, 2>), grid, dim3(256), 0, st, a, pv, wfrag, xb, wb);
    }
    return;
  }
#endif
  if (pv.in_coef) {                    // BatchNorm (+ ReLU) of the layer below applied on load
    if constexpr (NT == 4) {
      if (pv.d.G == 1) hipLaunchKernelGGL((k_spconv_rs3<NT, KQ, 1, 0, true>), grid, dim3(256), 0, st, a, pv, wfrag, xb, wb);
      else hipLaunchKernelGGL((k_spconv_rs3<NT, KQ, 2, 0, true>), grid, dim3(256), 0, st, a, pv, wfrag, xb, wb);
    } else {
      hipLaunchKernelGGL((k_spconv_rs3<NT, KQ, 4, 0, true>), grid, dim3(256), 0, st, a, pv, wfrag, xb, wb);
    }
    return;
  }
  if constexpr (NT == 4) {
    if (pv.d.G == 1) hipLaunchKernelGGL((k_spconv_rs3<NT, KQ, 1>), grid, dim3(256), 0, st, a, pv, wfrag, xb, wb);
    else hipLaunchKernelGGL((k_spconv_rs3<NT, KQ, 2>), grid, dim3(256), 0, st, a, pv, wfrag, xb, wb);
  } else {
    hipLaunchKernelGGL((k_spconv_rs3<NT, KQ, 4>), grid, dim3(256), 0, st, a, pv, wfrag, xb, wb);
  }
}
template <int NT>
static void launch_rs3_kq(const ConvArgs& a, const PlanView& pv, const float* wfrag, uint32_t xb, uint32_t wb, dim3 grid, hipStream_t st) {
  switch (a.Kd / 16) {
    case 1: launch_rs3_g<NT, 1>(a, pv, wfrag, xb, wb, grid, st); break;
    case 2: launch_rs3_g<NT, 2>(a, pv, wfrag, xb, wb, grid, st); break;
    case 4: launch_rs3_g<NT, 4>(a, pv, wfrag, xb, wb, grid, st); break;
    default: launch_rs3_g<NT, 8>(a, pv, wfrag, xb, wb, grid, st); break;
  }
}

// measurement build only: per-wave time stamps of the next planned launches go to `buf` (8 x uint64 per wave slot: grid.x * grid.y * 4 slots); null = off
#if SEEVCN_MEASURE
static unsigned long long* g_conv_trace = nullptr;
extern "C" int sv_debug_conv_trace(void* buf) {
  g_conv_trace = static_cast<unsigned long long*>(buf);
  return SV_OK;
}
#else
extern "C" int sv_debug_conv_trace(void*) {
  sv_set_error("sv_debug_conv_trace: only in the measurement build (make measure: libseevcn_hip_measure.so)");
  return SV_ERR_ARG;
}
#endif

struct BnBwdView {            // the BatchNorm whose output gradient a data-gradient launch produces (PlanView's bn_* fields)
  const float *x, *mean, *istd, *gamma, *beta;
  int relu;
};
static int conv_planned(const float* X, int64_t n_src, const int32_t* table_rows, const int32_t* perm, const int32_t* masks_p, const int32_t* tile_of,
                        int tiles_per_wave, const float* wfrag, float* Y, int64_t n_rows, int K, int Kd, int Nc, const float* bias, const float* scale,
                        const float* shift, const float* residual, int relu, int table_k_reversed, float* bn_partial, const BnBwdView* bnb, void* stream) {
  const InNorm in = take_input_norm();
  SV_CHECK_ARG(n_rows >= 0 && K > 0 && Kd > 0 && Nc > 0, "sparse_conv (planned): bad sizes");
  SV_CHECK_ARG(!bn_partial || (!bias && !scale && !residual && !relu), "sparse_conv (planned): BatchNorm partial sums are made by the plain epilogue only");
  if (n_rows == 0) return SV_OK;
  SV_CHECK_ARG(X && table_rows && perm && masks_p && tile_of && wfrag && Y, "sparse_conv (planned): null pointer");
  SV_CHECK_ARG((scale == nullptr) == (shift == nullptr), "sparse_conv: scale and shift go together");
  SV_CHECK_ARG(sv_conv_mfma_kernel_applies(K, Kd, Nc, n_src), "sparse_conv (planned): no MFMA kernel for K %d, C_in %d, C_out %d, %lld source rows "
               "(ask sv_conv_mfma_kernel_applies first)", K, Kd, Nc, (long long)n_src);
  SV_CHECK_ARG(tiles_per_wave == sv_conv_tiles_per_wave(n_rows, Kd, Nc), "sparse_conv (planned): tiles_per_wave must be sv_conv_tiles_per_wave(n_rows, Kd, Nc)");
  SV_CHECK_ARG((uintptr_t)X % 16 == 0 && (uintptr_t)wfrag % 16 == 0 && (uintptr_t)table_rows % 16 == 0, "sparse_conv (planned): 16-byte alignment");
  ConvArgs a{X, nullptr, nullptr, Y, bias, scale, shift, residual, relu, n_rows, K, Kd, Nc};
  PlanView pv;
  pv.tab = table_rows, pv.perm = perm, pv.masks_p = masks_p, pv.tile_of = tile_of, pv.d = plan_dims(n_rows, tiles_per_wave), pv.k_flip = table_k_reversed ? 1 : 0, pv.nc_total = Nc, pv.bn_partial = bn_partial;
  pv.bn_x = pv.bn_mean = pv.bn_istd = pv.bn_gamma = pv.bn_beta = nullptr, pv.bn_relu = 0;
  if (bnb) pv.bn_x = bnb->x, pv.bn_mean = bnb->mean, pv.bn_istd = bnb->istd, pv.bn_gamma = bnb->gamma, pv.bn_beta = bnb->beta, pv.bn_relu = bnb->relu;
#if SEEVCN_MEASURE
  static const int debug = getenv("SEEVCN_RS3_DEBUG") ? atoi(getenv("SEEVCN_RS3_DEBUG")) : 0;
  pv.debug = debug;
  pv.trace = g_conv_trace;
#endif
  pv.in_coef = in.coef, pv.in_relu = in.relu;
  // SEEVCN_RS3_EPI_ROWS=0 (A/B): epilogue launches store per accumulator, as they did before the whole-row form existed
  static const int epi_rows = getenv("SEEVCN_RS3_EPI_ROWS") ? atoi(getenv("SEEVCN_RS3_EPI_ROWS")) : 1;
  pv.epi_rows = (epi_rows && (((uintptr_t)Y | (uintptr_t)bias | (uintptr_t)scale | (uintptr_t)shift | (uintptr_t)residual) & 15) == 0) ? 1 : 0;
  SV_CHECK_ARG(!in.coef || (!pv.debug && !pv.trace && (uintptr_t)in.coef % 16 == 0), "sparse_conv (planned): an input transform needs a production instance and 16-byte aligned coefficients");
  const int nc_blk = Nc > 64 ? 64 : Nc;
  const dim3 grid((unsigned)(PL_REGIONS * PL_REGION_WAVES / 4), (unsigned)(Nc / nc_blk));
  const uint32_t xb = (uint32_t)((uint64_t)n_src * Kd * 4), wb = (uint32_t)((uint64_t)K * Nc * Kd * 4);
  hipStream_t st = sv_stream(stream);
  switch (nc_blk / 16) {
    case 1: launch_rs3_kq<1>(a, pv, wfrag, xb, wb, grid, st); break;
    case 2: launch_rs3_kq<2>(a, pv, wfrag, xb, wb, grid, st); break;
    default: launch_rs3_kq<4>(a, pv, wfrag, xb, wb, grid, st); break;
  }
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_sparse_conv_gather_gemm_planned(const float* X, int64_t n_src, const int32_t* table_rows, const int32_t* perm, const int32_t* masks_p,
                                                  const int32_t* tile_of, int tiles_per_wave,
                                                  const float* wfrag, float* Y, int64_t n_rows, int K, int Kd, int Nc, const float* bias,
                                                  const float* scale, const float* shift, const float* residual, int relu, int table_k_reversed,
                                                  float* bn_partial, void* stream) {
  return conv_planned(X, n_src, table_rows, perm, masks_p, tile_of, tiles_per_wave, wfrag, Y, n_rows, K, Kd, Nc, bias, scale, shift, residual, relu,
                      table_k_reversed, bn_partial, nullptr, stream);
}

// The data gradient of a layer whose INPUT came out of a BatchNorm (+ReLU): Y (n_rows, Nc) is the gradient w.r.t. that BatchNorm's output, and
// the launch's epilogue also leaves the two per-channel sums of the BatchNorm's backward -- sum(dy * branch) and sum(dy * branch * xhat), branch
// = the forward's ReLU decision recomputed from bn_x with the forward's own expression -- as sv_conv_planned_partials() per-workgroup partials in
// bn_partial, laid out like sv_batchnorm_relu_backward's scratch: sv_batchnorm_relu_backward_partial starts at the combine.
extern "C" int sv_sparse_conv_dgrad_planned_bn(const float* dZ, int64_t n_src, const int32_t* table_rows, const int32_t* perm, const int32_t* masks_p,
                                               const int32_t* tile_of, int tiles_per_wave, const float* wfrag, float* dY, int64_t n_rows, int K, int Kd,
                                               int Nc, int table_k_reversed, const float* bn_x, const float* bn_mean, const float* bn_invstd,
                                               const float* bn_gamma, const float* bn_beta, int bn_relu, float* bn_partial, void* stream) {
  SV_CHECK_ARG(bn_x && bn_mean && bn_invstd && bn_partial, "sparse_conv_dgrad_planned_bn: null pointer");
  const BnBwdView bnb{bn_x, bn_mean, bn_invstd, bn_gamma, bn_beta, bn_relu ? 1 : 0};
  return conv_planned(dZ, n_src, table_rows, perm, masks_p, tile_of, tiles_per_wave, wfrag, dY, n_rows, K, Kd, Nc, nullptr, nullptr, nullptr, nullptr, 0,
                      table_k_reversed, bn_partial, &bnb, stream);
}

// Generic VALU path for channel counts the MFMA tiling does not cover (e.g. the C_in = 3 input layer):
// one thread per (row, 4 output columns), weights read through L1/L2.
__global__ __launch_bounds__(256) void k_spconv_valu(ConvArgs a) {
  const int nq = (a.Nc + 3) / 4;
  const int64_t total = a.n_rows * nq;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = idx / nq;
    const int n0 = (int)(idx - row * nq) * 4;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < a.K; ++k) {
      const int32_t j = a.nbr[(int64_t)k * a.n_rows + row];
      if (j < 0) continue;
      const float* x = a.X + (int64_t)j * a.Kd;
      for (int u = 0; u < 4; ++u) {
        if (n0 + u >= a.Nc) break;
        const float* w = a.Wt + ((int64_t)k * a.Nc + n0 + u) * a.Kd;
        float s = acc[u];
        for (int c = 0; c < a.Kd; ++c) s = fmaf(x[c], w[c], s);
        acc[u] = s;
      }
    }
    for (int u = 0; u < 4 && n0 + u < a.Nc; ++u) a.Y[row * a.Nc + n0 + u] = conv_epilogue(acc[u], n0 + u, row, a);
  }
}

// Input layer (C_in = 3 or 4 point features -> 16 channels, spconv_backbone.py:77-81): HBM-bound -- 4*K bytes of neighbour table and
// 4*Nc bytes of output per row against 2*K*Kd*Nc flops.  Same thread mapping and summation order as k_spconv_valu (bit-identical
// results); the weights (K*Nc*Kd floats, 5 KB) are staged in LDS and the K table reads of a row are issued 9 at a time.
constexpr int SC_SMALL_KD = 4, SC_SMALL_LDS = 27 * 32 * SC_SMALL_KD;
template <int KD>
__global__ __launch_bounds__(256) void k_spconv_small_cin(ConvArgs a) {
  __shared__ float s_w[SC_SMALL_LDS];
  for (int i = threadIdx.x; i < a.K * a.Nc * KD; i += 256) s_w[i] = a.Wt[i];
  __syncthreads();
  const int nq = (a.Nc + 3) / 4;
  const int64_t total = a.n_rows * nq;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int64_t row = idx / nq;
    const int n0 = (int)(idx - row * nq) * 4;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < a.K; k0 += 9) {
      int32_t j[9];
#pragma unroll
      for (int u = 0; u < 9; ++u) j[u] = k0 + u < a.K ? a.nbr[(int64_t)(k0 + u) * a.n_rows + row] : -1;
      float x[9][KD];
#pragma unroll
      for (int u = 0; u < 9; ++u)
#pragma unroll
        for (int c = 0; c < KD; ++c) x[u][c] = j[u] >= 0 ? a.X[(int64_t)j[u] * KD + c] : 0.f;
#pragma unroll
      for (int u = 0; u < 9; ++u) {
        if (j[u] < 0) continue;
        const float* w = s_w + (size_t)((k0 + u) * a.Nc + n0) * KD;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          if (n0 + v >= a.Nc) break;
          float t = acc[v];
#pragma unroll
          for (int c = 0; c < KD; ++c) t = fmaf(x[u][c], w[v * KD + c], t);
          acc[v] = t;
        }
      }
    }
    for (int v = 0; v < 4 && n0 + v < a.Nc; ++v) a.Y[row * a.Nc + n0 + v] = conv_epilogue(acc[v], n0 + v, row, a);
  }
}

// Plain entry: packed (K, Nc, Kd) weights, k-major table, no plan -- the register-stationary MFMA kernel for channel multiples of 16, the
// small-C_in kernel for the 3 / 4-channel input layer, the VALU kernel for everything else.
extern "C" int sv_sparse_conv_gather_gemm(const float* X, int64_t n_src, const int32_t* nbr, const float* Wt, float* Y,
                                          int64_t n_rows, int K, int Kd, int Nc, const float* bias, const float* scale, const float* shift,
                                          const float* residual, int relu, void* stream) {
  SV_CHECK_ARG(!take_input_norm().coef, "sparse_conv: the plain entry takes no input transform (sv_conv_next_input_norm is for the planned kernel and the weight gradients)");
  SV_CHECK_ARG(n_rows >= 0 && K > 0 && Kd > 0 && Nc > 0, "sparse_conv: bad sizes");
  if (n_rows == 0) return SV_OK;
  SV_CHECK_ARG(X && nbr && Wt && Y, "sparse_conv: null pointer");
  SV_CHECK_ARG((scale == nullptr) == (shift == nullptr), "sparse_conv: scale and shift go together");
  (void)n_src;
  ConvArgs a{X, nbr, Wt, Y, bias, scale, shift, residual, relu, n_rows, K, Kd, Nc};
  hipStream_t st = sv_stream(stream);
  const int nt = Nc / 16;
  const bool mfma_ok = (Kd % 16 == 0) && (Nc % 16 == 0) && (nt == 1 || nt == 2 || nt == 4 || nt == 8) &&
                       ((uintptr_t)X % 16 == 0) && ((uintptr_t)Wt % 16 == 0);
  if (mfma_ok && try_launch_rs(a, st) == 0) {
    SV_LAUNCH_CHECK();
    return SV_OK;
  }
  if ((Kd == 3 || Kd == 4) && K * Nc * Kd <= SC_SMALL_LDS) {
    const dim3 grid(sv_grid_1d(n_rows * ((Nc + 3) / 4), 256, 256 * 8));
    if (Kd == 3) hipLaunchKernelGGL(k_spconv_small_cin<3>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_spconv_small_cin<4>, grid, dim3(256), 0, st, a);
  } else {
    hipLaunchKernelGGL(k_spconv_valu, dim3(sv_grid_1d(n_rows * ((Nc + 3) / 4), 256, 256 * 16)), dim3(256), 0, st, a);
  }
  SV_LAUNCH_CHECK();
  return SV_OK;
}
