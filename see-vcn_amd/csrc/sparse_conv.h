// What the three sparse-convolution translation units share: conv_plan.hip (the plan of a table), sparse_conv.hip (forward and data gradient),
// sparse_wgrad.hip (weight gradient).
#pragma once
#include "common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// Input transform of the NEXT call (sv_conv_next_input_norm): the convolution / weight gradient reads X through y = [relu](x * scale[c] + shift[c]) --
// X is then the RAW output of the convolution below and (scale, shift) the coefficients of its BatchNorm (sv_batchnorm_finalize_forward), so that the
// normalised activations are never written to memory: the BatchNorm's elementwise pass (one read + one write of every activation tensor) disappears
// into the gathers that read the tensor anyway.  Same expression as k_bn_apply_fwd (bn_act, then fmaxf): the values a consumer sees are bit for bit
// the ones the separate pass would have stored.  Absent neighbours contribute 0, not relu(shift).
struct InNorm {
  const float* coef = nullptr;   // (2, C_in): scale | shift
  int relu = 0;
};
// the transform set for the next call, and back to none (one thread-local slot, defined in sparse_conv.hip)
InNorm take_input_norm();

// ---- plan of a rulebook table (conv_plan.hip builds it, k_spconv_rs3 walks it)
constexpr int PL_REGIONS = 8;          // one region per XCD (MI355X: 8 XCDs, workgroup b runs on XCD b % 8)
constexpr int PL_CLASSES = 4096;       // neighbour-mask classes (class_key)
constexpr int PL_WG = 1024;            // rows per workgroup of the plan kernels; region boundaries are multiples of it (and so of 16)
constexpr int PL_ROW = 32;             // int32 per row of the regrouped table: [0..26] source rows, [27] mask, [28] output row, [29..31] unused
constexpr int RS3_KMAX = 27;

// first row of region r: regions are runs of whole PL_WG-row blocks, as equal as possible
__host__ __device__ inline int64_t plan_region_start(int64_t n_rows, int r) {
  const int64_t nblk = (n_rows + PL_WG - 1) / PL_WG;
  const int64_t s = (nblk * r / PL_REGIONS) * PL_WG;
  return s < n_rows ? s : n_rows;
}

constexpr int PL_WAVES_PER_SIMD = 4;                                // resident waves per SIMD of a conv launch (__launch_bounds__ of k_spconv_rs3)
constexpr int PL_BINS = 32;                                         // CUs per XCD
constexpr int PL_QUAD = 4;                                          // tiles dealt together: one per wave of a workgroup
constexpr int PL_REGION_WAVES = PL_BINS * PL_QUAD * PL_WAVES_PER_SIMD;   // 512 waves = 128 workgroups per region
constexpr int PL_MAX_REGION_TILES = 16384;                          // LDS bound of the deal (2 M rows per launch)
struct PlanDims {
  int32_t tile0[PL_REGIONS];    // first tile of the region
  int32_t tiles[PL_REGIONS];    // tiles of the region
  int32_t G;                    // tiles a wave works on at a time
  int32_t n_pass;               // passes: a wave has n_pass * G tile slots
};
static inline PlanDims plan_dims(int64_t n_rows, int G) {
  PlanDims d{};
  const int64_t n_tiles = (n_rows + 15) / 16;
  int max_tiles = 0;
  d.G = G;
  for (int r = 0; r < PL_REGIONS; ++r) {
    const int64_t s = plan_region_start(n_rows, r), e = r + 1 < PL_REGIONS ? plan_region_start(n_rows, r + 1) : n_rows;
    d.tile0[r] = (int32_t)(s / 16);
    d.tiles[r] = (int32_t)((r + 1 < PL_REGIONS ? e / 16 : n_tiles) - s / 16);
    if (d.tiles[r] > max_tiles) max_tiles = d.tiles[r];
  }
  const int quads = (max_tiles + PL_QUAD - 1) / PL_QUAD;
  // a region deals its tiles one quad per (bin, round) or -- submanifold tables on four tiles per wave, see plan_deal_quads -- in units of G consecutive
  // quads; the slot count covers both
  const int rounds = (quads + PL_BINS - 1) / PL_BINS;                            // quads per CU bin
  const int slots = (rounds + PL_WAVES_PER_SIMD - 1) / PL_WAVES_PER_SIMD;        // tiles per wave
  d.n_pass = slots > 0 ? (slots + G - 1) / G : 1;
  const int units = (quads + G - 1) / G;
  const int urounds = (units + PL_BINS - 1) / PL_BINS;
  const int upass = (urounds + PL_WAVES_PER_SIMD - 1) / PL_WAVES_PER_SIMD;
  if (upass > d.n_pass) d.n_pass = upass;
  return d;
}
