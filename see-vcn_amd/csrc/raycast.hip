// Mesh ray casting for the VCN's "VC" training data: a linear BVH over a scene's triangles, a nearest-hit search, pinhole rays made in the
// kernel and the stable compaction of the hit points with their in-box crop.
//
// Reference (open3d.t.geometry.RaycastingScene = Embree on the CPU): see/surface_completion/models/vcn/vc_shapenet/dataset_functions.py:265-342
// (populate_scene, cast_rays_at_point, raycast_object) and raycast_surface_from_meshes.py:16-52 (generate_views, get_object_surface).
//
// The arithmetic is the one tests/raycast_reference.py states: Moeller-Trumbore without culling in fp32, one rounding per operation (the library
// is built with -ffp-contract=off and a correctly rounded divide), nearest t, ties to the lowest (geometry, primitive).  The hierarchy only
// decides WHICH triangles meet that test; DESIGN.md section 3 "VC ray casting" derives the padding that keeps the culling conservative and the
// bounds of every loop here.
//
// Layout.  nodes: max(T - 1, 1) rows of 16 words -- lo0 hi0 lo1 hi1 (the two children's boxes, 12 floats), child0, child1 (int32: >= 0 an internal
// node, < 0 the leaf ~c, RC_NONE no child), two spare words.  Node 0 is the root.  leaves: T rows of 12 words in key order -- v0, e1 = v1 - v0,
// e2 = v2 - v0 (9 floats), geometry id, primitive id, the triangle's index in the scene (the tie-break order).
#include <math.h>

#include "box_test.h"
#include "common.h"
#include "wave.h"

constexpr int RC_THREADS = 256;
constexpr int RC_WAVE_THREADS = 64;                            // the cast kernels: one wave a workgroup, an 8 x 8 pixel tile or 64 consecutive rays
constexpr int RC_STACK = 64;                                   // >= RC_MAX_DEPTH: one entry per internal node on a root-to-leaf path at most
constexpr int RC_KEY_INDEX_BITS = 24;                          // T <= 2^24: the key's bits that can differ are 30 (Morton) + 24 (index)
constexpr int RC_MAX_DEPTH = 30 + RC_KEY_INDEX_BITS;           // internal nodes on one path: their common-prefix lengths are distinct
constexpr int64_t RC_MAX_TRIANGLES = (int64_t)1 << RC_KEY_INDEX_BITS;
constexpr int RC_NONE = INT32_MIN;
constexpr float RC_PAD = 0x1p-11f;                             // box padding as a share of the largest coordinate magnitude
constexpr float RC_TSLACK = 0x1p-20f;                          // widening of the slab interval: 16 ulp for the 4 roundings of its arithmetic
static_assert(RC_MAX_DEPTH <= RC_STACK, "the traversal stack must hold one entry per level");

struct RcV3 { float x, y, z; };
__device__ __forceinline__ RcV3 rc_sub(RcV3 a, RcV3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ RcV3 rc_cross(RcV3 a, RcV3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ float rc_dot(RcV3 a, RcV3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// ------------------------------------------------------------------ build, part 1: bounds of the centroids and the sort keys
__device__ __forceinline__ RcV3 rc_centroid(const float* __restrict__ t) {
  return {((t[0] + t[3]) + t[6]) / 3.f, ((t[1] + t[4]) + t[7]) / 3.f, ((t[2] + t[5]) + t[8]) / 3.f};
}

// bounds: 6 unsigned words, mins preset to 0xffffffff and maxes to 0 by the launcher; status[0] |= 1 when a vertex is not finite
__global__ __launch_bounds__(RC_THREADS) void k_rc_bounds(const float* __restrict__ tris, int64_t T, unsigned* __restrict__ bounds,
                                                          int32_t* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x;
  unsigned lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
  bool bad = false;
  if (i < T) {
    const float* t = tris + i * 9;
#pragma unroll
    for (int k = 0; k < 9; ++k) bad |= !isfinite(t[k]);
    if (!bad) {
      const RcV3 c = rc_centroid(t);
      lo[0] = hi[0] = sv_ordered_f32(c.x), lo[1] = hi[1] = sv_ordered_f32(c.y), lo[2] = hi[2] = sv_ordered_f32(c.z);
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    lo[k] = sv_wave_reduce_min(lo[k]), hi[k] = sv_wave_reduce_max(hi[k]);
  }
  const unsigned long long any_bad = __ballot(bad);
  if ((threadIdx.x & (SV_WAVE - 1)) == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (lo[k] <= hi[k]) atomicMin(&bounds[k], lo[k]), atomicMax(&bounds[3 + k], hi[k]);
    }
    if (any_bad) atomicOr(&status[0], 1);
  }
}

__device__ __forceinline__ unsigned rc_spread10(unsigned v) {  // 10 bits -> every third bit
  v = (v * 0x00010001u) & 0xFF0000FFu;
  v = (v * 0x00000101u) & 0x0F00F00Fu;
  v = (v * 0x00000011u) & 0xC30C30C3u;
  v = (v * 0x00000005u) & 0x49249249u;
  return v;
}
__device__ __forceinline__ unsigned rc_cell(float c, float lo, float hi) {
  const float f = (c - lo) / (hi - lo) * 1024.f;
  if (!(f >= 0.f)) return 0u;                                  // NaN (no extent, or a vertex that is not finite) and below
  return f >= 1023.f ? 1023u : (unsigned)f;
}

// key = Morton code of the centroid (30 bits) << 32 | the triangle's index: all keys differ, so equal codes still split
__global__ __launch_bounds__(RC_THREADS) void k_rc_keys(const float* __restrict__ tris, int64_t T, const unsigned* __restrict__ bounds,
                                                        int64_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x;
  if (i >= T) return;
  const RcV3 c = rc_centroid(tris + i * 9);
  const unsigned m = (rc_spread10(rc_cell(c.x, sv_unordered_f32(bounds[0]), sv_unordered_f32(bounds[3]))) << 2) |
                     (rc_spread10(rc_cell(c.y, sv_unordered_f32(bounds[1]), sv_unordered_f32(bounds[4]))) << 1) |
                     rc_spread10(rc_cell(c.z, sv_unordered_f32(bounds[2]), sv_unordered_f32(bounds[5])));
  keys[i] = ((int64_t)m << 32) | i;
}

extern "C" size_t sv_bvh_scratch_bytes(int64_t T) {
  if (T <= 0 || T > RC_MAX_TRIANGLES) return 0;
  return 32 + (size_t)(3 * T) * sizeof(int32_t);               // bounds | arrival counters (T) | parents of the internal nodes (T) and of the leaves (T)
}

extern "C" int sv_bvh_keys(const float* tris, int64_t T, int64_t* keys, int32_t* status, void* scratch, void* stream) {
  SV_CHECK_ARG(T >= 0 && T <= RC_MAX_TRIANGLES, "bvh_keys: %lld triangles, the key holds %d index bits (at most %lld)", (long long)T,
               RC_KEY_INDEX_BITS, (long long)RC_MAX_TRIANGLES);
  SV_CHECK_ARG(status, "bvh_keys: null pointer");
  hipStream_t st = sv_stream(stream);
  SV_HIP(hipMemsetAsync(status, 0, 2 * sizeof(int32_t), st));
  if (T == 0) return SV_OK;
  SV_CHECK_ARG(tris && keys && scratch, "bvh_keys: null pointer");
  unsigned* bounds = reinterpret_cast<unsigned*>(scratch);
  SV_HIP(hipMemsetAsync(bounds, 0xff, 3 * sizeof(unsigned), st));
  SV_HIP(hipMemsetAsync(bounds + 3, 0, 3 * sizeof(unsigned), st));
  const int grid = sv_div_up(T, RC_THREADS);
  hipLaunchKernelGGL(k_rc_bounds, dim3(grid), dim3(RC_THREADS), 0, st, tris, T, bounds, status);
  hipLaunchKernelGGL(k_rc_keys, dim3(grid), dim3(RC_THREADS), 0, st, tris, T, bounds, keys);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ------------------------------------------------------------------ build, part 2: the radix tree over the sorted keys (Karras 2012) and the refit
__device__ __forceinline__ int rc_delta(const int64_t* __restrict__ keys, int64_t T, int64_t i, int64_t j) {
  if (j < 0 || j >= T) return -1;
  return __clzll(keys[i] ^ keys[j]);                           // the keys differ, so this is at most 63
}

__global__ __launch_bounds__(RC_THREADS) void k_rc_tree(const int64_t* __restrict__ keys, int64_t T, int32_t* __restrict__ nodes,
                                                        int32_t* __restrict__ parent_node, int32_t* __restrict__ parent_leaf) {
  const int64_t i = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x;
  if (i >= T - 1) return;
  const int d = rc_delta(keys, T, i, i + 1) > rc_delta(keys, T, i, i - 1) ? 1 : -1;
  const int dmin = rc_delta(keys, T, i, i - d);
  int64_t lmax = 2;
  for (int s = 0; s < 32 && rc_delta(keys, T, i, i + lmax * d) > dmin; ++s) lmax <<= 1;     // lmax <= 2 T <= 2^25
  int64_t l = 0;
  for (int64_t t = lmax >> 1; t >= 1; t >>= 1)
    if (rc_delta(keys, T, i, i + (l + t) * d) > dmin) l += t;
  const int64_t j = i + l * d;
  const int dnode = rc_delta(keys, T, i, j);
  int64_t s = 0;
  for (int64_t t = (l + 1) >> 1;; t = (t + 1) >> 1) {                                         // halves until 1: at most 26 rounds
    if (rc_delta(keys, T, i, i + (s + t) * d) > dnode) s += t;
    if (t == 1) break;
  }
  const int64_t gamma = i + s * d + (d < 0 ? -1 : 0);
  const int64_t first = i < j ? i : j, last = i < j ? j : i;
  int32_t c0, c1;
  if (first == gamma) c0 = ~(int32_t)gamma, parent_leaf[gamma] = (int32_t)i; else c0 = (int32_t)gamma, parent_node[gamma] = (int32_t)i;
  if (last == gamma + 1) c1 = ~(int32_t)(gamma + 1), parent_leaf[gamma + 1] = (int32_t)i; else c1 = (int32_t)(gamma + 1), parent_node[gamma + 1] = (int32_t)i;
  nodes[i * 16 + 12] = c0, nodes[i * 16 + 13] = c1, nodes[i * 16 + 14] = 0, nodes[i * 16 + 15] = 0;
  if (i == 0) parent_node[0] = -1;
}

// One thread per leaf writes its row and its box into the parent's slot, then climbs: the first of a node's two children to arrive stops, the
// second unites the two boxes and carries the union on.  Every word another workgroup reads travels through agent-scope atomics around the
// counter's release / acquire, so no cache holds a stale copy.  The climb ends at the root, after RC_MAX_DEPTH nodes at most.
__device__ __forceinline__ void rc_put(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float rc_get(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(RC_THREADS) void k_rc_leaves(const float* __restrict__ tris, const int32_t* __restrict__ geom_ids,
                                                          const int32_t* __restrict__ prim_ids, int64_t T, const int64_t* __restrict__ keys,
                                                          float* nodes, float* __restrict__ leaves, int32_t* counters,
                                                          const int32_t* __restrict__ parent_node, const int32_t* __restrict__ parent_leaf) {
  const int64_t i = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x;
  if (i >= T) return;
  const int64_t src = min((int64_t)(keys[i] & 0xffffffffll), T - 1);   // a key of sv_bvh_keys holds an index below T; never read beyond tris
  const float* t = tris + src * 9;
  float* row = leaves + i * 12;
  float lo[3], hi[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    row[k] = t[k], row[3 + k] = t[3 + k] - t[k], row[6 + k] = t[6 + k] - t[k];
    lo[k] = fminf(fminf(t[k], t[3 + k]), t[6 + k]), hi[k] = fmaxf(fmaxf(t[k], t[3 + k]), t[6 + k]);
  }
  int32_t* irow = reinterpret_cast<int32_t*>(row);
  irow[9] = geom_ids[src], irow[10] = prim_ids[src], irow[11] = (int32_t)src;
  if (T == 1) {                                                // no internal node: row 0 stands in for the root, with one child
    int32_t* n = reinterpret_cast<int32_t*>(nodes);
#pragma unroll
    for (int k = 0; k < 3; ++k) nodes[k] = lo[k], nodes[3 + k] = hi[k], nodes[6 + k] = 0.f, nodes[9 + k] = 0.f;
    n[12] = ~0, n[13] = RC_NONE, n[14] = 0, n[15] = 0;
    return;
  }
  int32_t child = ~(int32_t)i, p = parent_leaf[i];
  for (int level = 0; level <= RC_MAX_DEPTH && p >= 0; ++level) {
    float* n = nodes + (int64_t)p * 16;
    const int slot = reinterpret_cast<const int32_t*>(n)[12] == child ? 0 : 1;   // the child words come from the launch before: plain reads
#pragma unroll
    for (int k = 0; k < 3; ++k) rc_put(n + slot * 6 + k, lo[k]), rc_put(n + slot * 6 + 3 + k, hi[k]);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    const int32_t arrived = __hip_atomic_fetch_add(&counters[p], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (arrived == 0) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const int other = 1 - slot;
#pragma unroll
    for (int k = 0; k < 3; ++k) lo[k] = fminf(lo[k], rc_get(n + other * 6 + k)), hi[k] = fmaxf(hi[k], rc_get(n + other * 6 + 3 + k));
    child = p, p = parent_node[p];
  }
}

extern "C" int sv_bvh_build(const float* tris, const int32_t* geom_ids, const int32_t* prim_ids, int64_t T, const int64_t* sorted_keys, float* nodes,
                            float* leaves, void* scratch, void* stream) {
  SV_CHECK_ARG(T >= 0 && T <= RC_MAX_TRIANGLES, "bvh_build: %lld triangles, at most %lld", (long long)T, (long long)RC_MAX_TRIANGLES);
  if (T == 0) return SV_OK;
  SV_CHECK_ARG(tris && geom_ids && prim_ids && sorted_keys && nodes && leaves && scratch, "bvh_build: null pointer");
  hipStream_t st = sv_stream(stream);
  int32_t* counters = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(scratch) + 32);
  int32_t* parent_node = counters + T;
  int32_t* parent_leaf = parent_node + T;
  SV_HIP(hipMemsetAsync(counters, 0, (size_t)T * sizeof(int32_t), st));
  if (T > 1)
    hipLaunchKernelGGL(k_rc_tree, dim3(sv_div_up(T - 1, RC_THREADS)), dim3(RC_THREADS), 0, st, sorted_keys, T, reinterpret_cast<int32_t*>(nodes),
                       parent_node, parent_leaf);
  hipLaunchKernelGGL(k_rc_leaves, dim3(sv_div_up(T, RC_THREADS)), dim3(RC_THREADS), 0, st, tris, geom_ids, prim_ids, T, sorted_keys, nodes, leaves,
                     counters, parent_node, parent_leaf);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ------------------------------------------------------------------ the nearest-hit search
struct RcRay {
  RcV3 o, d, inv;
  float mag;                                                   // the origin's largest coordinate magnitude
};
struct RcHit {
  float t, u, v;
  int32_t geom, prim, index;
};

__device__ __forceinline__ RcRay rc_make_ray(RcV3 o, RcV3 d) {
  RcRay r;
  r.o = o, r.d = d;
  r.inv = {1.f / d.x, 1.f / d.y, 1.f / d.z};
  r.mag = fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fabsf(o.z));
  return r;
}

// The padded slab test: does the ray meet the box, grown by RC_PAD times the largest coordinate magnitude in play, at a parameter in [0, t_best]?
// fminf / fmaxf drop a NaN (0 * inf: the origin on a padded face of a slab the ray is parallel to), which keeps that slab open.
__device__ __forceinline__ bool rc_meets_box(const RcRay& r, const float* __restrict__ b, float t_best, float* t_enter) {
  float mag = r.mag;
#pragma unroll
  for (int k = 0; k < 6; ++k) mag = fmaxf(mag, fabsf(b[k]));
  const float pad = RC_PAD * mag;
  const float x0 = ((b[0] - pad) - r.o.x) * r.inv.x, x1 = ((b[3] + pad) - r.o.x) * r.inv.x;
  const float y0 = ((b[1] - pad) - r.o.y) * r.inv.y, y1 = ((b[4] + pad) - r.o.y) * r.inv.y;
  const float z0 = ((b[2] - pad) - r.o.z) * r.inv.z, z1 = ((b[5] + pad) - r.o.z) * r.inv.z;
  float t0 = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fmaxf(fminf(z0, z1), 0.f));
  float t1 = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fminf(fmaxf(z0, z1), t_best));
  t0 -= fabsf(t0) * RC_TSLACK, t1 += fabsf(t1) * RC_TSLACK;
  *t_enter = t0;
  return t0 <= t1;
}

// The stated test (tests/raycast_reference.py), statement for statement.
__device__ __forceinline__ void rc_triangle(const RcRay& r, const float* __restrict__ leaf, RcHit& best) {
  const RcV3 v0 = {leaf[0], leaf[1], leaf[2]}, e1 = {leaf[3], leaf[4], leaf[5]}, e2 = {leaf[6], leaf[7], leaf[8]};
  const RcV3 p = rc_cross(r.d, e2);
  const float det = rc_dot(e1, p);
  const float inv = 1.f / det;
  const RcV3 s = rc_sub(r.o, v0);
  const float u = rc_dot(s, p) * inv;
  const RcV3 q = rc_cross(s, e1);
  const float v = rc_dot(r.d, q) * inv;
  const float t = rc_dot(e2, q) * inv;
  if (det != 0.f && u >= 0.f && v >= 0.f && (u + v) <= 1.f && t >= 0.f) {
    const int32_t* il = reinterpret_cast<const int32_t*>(leaf);
    if (t < best.t || (t == best.t && il[11] < best.index)) best = {t, u, v, il[9], il[10], il[11]};
  }
}

// stack: RC_STACK rows of 64 lanes in LDS, lane-contiguous (no bank conflicts, no scratch memory).  Every internal node is entered once at most,
// so the walk ends within T steps; a path pushes one node per level at most, so RC_MAX_DEPTH entries suffice (status[1] |= 1 were that ever
// untrue: the push is then dropped instead of written out of bounds).
__device__ __forceinline__ RcHit rc_trace(const RcRay& r, const float* __restrict__ nodes, const float* __restrict__ leaves, int64_t T,
                                          int32_t (*stack)[RC_WAVE_THREADS], int lane, int32_t* __restrict__ status) {
  RcHit best = {INFINITY, 0.f, 0.f, -1, -1, INT32_MAX};
  if (T == 0) return best;
  int sp = 0;
  int32_t node = 0;
  for (int64_t step = 0; step < T; ++step) {
    const float4* n4 = reinterpret_cast<const float4*>(nodes + (int64_t)node * 16);
    const float4 a = n4[0], b = n4[1], c = n4[2], d = n4[3];
    const float box[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
    const int32_t c0 = __float_as_int(d.x), c1 = __float_as_int(d.y);
    float t0, t1;
    bool h0 = rc_meets_box(r, box, best.t, &t0);
    if (h0 && c0 < 0) {
      rc_triangle(r, leaves + (int64_t)(~c0) * 12, best);
      h0 = false;
    }
    bool h1 = c1 != RC_NONE && rc_meets_box(r, box + 6, best.t, &t1);
    if (h1 && c1 < 0) {
      rc_triangle(r, leaves + (int64_t)(~c1) * 12, best);
      h1 = false;
    }
    if (h0 && h1) {                                            // both are internal nodes: the nearer first, the other waits
      const bool swap = t1 < t0;
      const int32_t far_node = swap ? c0 : c1;
      node = swap ? c1 : c0;
      if (sp < RC_STACK) stack[sp++][lane] = far_node; else atomicOr(&status[1], 1);
    } else if (h0 || h1) {
      node = h0 ? c0 : c1;
    } else {
      if (sp == 0) break;
      node = stack[--sp][lane];
    }
  }
  return best;
}

__device__ __forceinline__ void rc_store(const RcHit& h, int64_t i, float* __restrict__ t_hit, int32_t* __restrict__ geom, int32_t* __restrict__ prim,
                                         float* __restrict__ uvs) {
  t_hit[i] = h.t, geom[i] = h.geom, prim[i] = h.prim;
  uvs[2 * i] = h.u, uvs[2 * i + 1] = h.v;
}

__global__ __launch_bounds__(RC_WAVE_THREADS) void k_rc_cast_rays(const float* __restrict__ nodes, const float* __restrict__ leaves, int64_t T,
                                                                  const float* __restrict__ rays, int64_t N, float* __restrict__ t_hit,
                                                                  int32_t* __restrict__ geom, int32_t* __restrict__ prim, float* __restrict__ uvs,
                                                                  int32_t* __restrict__ status) {
  __shared__ int32_t stack[RC_STACK][RC_WAVE_THREADS];
  const int64_t i = (int64_t)blockIdx.x * RC_WAVE_THREADS + threadIdx.x;
  if (i >= N) return;
  const float* q = rays + i * 6;
  const RcRay r = rc_make_ray({q[0], q[1], q[2]}, {q[3], q[4], q[5]});
  rc_store(rc_trace(r, nodes, leaves, T, stack, threadIdx.x, status), i, t_hit, geom, prim, uvs);
}

// cams: rows of 12 doubles, M = R^-1 K^-1 row-major and the eye.  Pixel (x, y): direction M (x + 0.5, y + 0.5, 1), three products summed left to
// right in fp64 and rounded once; origin = the eye rounded.
struct RcOriginDir { RcV3 o, d; };
__device__ __forceinline__ RcOriginDir rc_pinhole(const double* __restrict__ cam, int x, int y) {
  const double px = x + 0.5, py = y + 0.5;
  RcOriginDir r;
  r.d.x = (float)((cam[0] * px + cam[1] * py) + cam[2] * 1.0);
  r.d.y = (float)((cam[3] * px + cam[4] * py) + cam[5] * 1.0);
  r.d.z = (float)((cam[6] * px + cam[7] * py) + cam[8] * 1.0);
  r.o = {(float)cam[9], (float)cam[10], (float)cam[11]};
  return r;
}

// one wave per 8 x 8 pixel tile: neighbours in the image walk the same subtree
__global__ __launch_bounds__(RC_WAVE_THREADS) void k_rc_cast_pinhole(const float* __restrict__ nodes, const float* __restrict__ leaves, int64_t T,
                                                                     const double* __restrict__ cams, int W, int H, int tiles_x,
                                                                     float* __restrict__ t_hit, int32_t* __restrict__ geom,
                                                                     int32_t* __restrict__ prim, float* __restrict__ uvs,
                                                                     int32_t* __restrict__ status) {
  __shared__ int32_t stack[RC_STACK][RC_WAVE_THREADS];
  const int cam = blockIdx.y, tile = blockIdx.x, lane = threadIdx.x;
  const int x = (tile % tiles_x) * 8 + (lane & 7), y = (tile / tiles_x) * 8 + (lane >> 3);
  if (x >= W || y >= H) return;
  const RcOriginDir r = rc_pinhole(cams + (int64_t)cam * 12, x, y);
  const int64_t i = ((int64_t)cam * H + y) * W + x;
  rc_store(rc_trace(rc_make_ray(r.o, r.d), nodes, leaves, T, stack, lane, status), i, t_hit, geom, prim, uvs);
}

extern "C" int sv_cast_rays(const float* nodes, const float* leaves, int64_t T, const float* rays, int64_t N, float* t_hit, int32_t* geometry_ids,
                            int32_t* primitive_ids, float* primitive_uvs, int32_t* status, void* stream) {
  SV_CHECK_ARG(T >= 0 && T <= RC_MAX_TRIANGLES && N >= 0 && N < ((int64_t)1 << 31) * RC_WAVE_THREADS, "cast_rays: bad arguments");
  if (N == 0) return SV_OK;
  SV_CHECK_ARG(rays && t_hit && geometry_ids && primitive_ids && primitive_uvs && status && (T == 0 || (nodes && leaves)), "cast_rays: null pointer");
  hipLaunchKernelGGL(k_rc_cast_rays, dim3(sv_div_up(N, RC_WAVE_THREADS)), dim3(RC_WAVE_THREADS), 0, sv_stream(stream), nodes, leaves, T, rays, N, t_hit,
                     geometry_ids, primitive_ids, primitive_uvs, status);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

static bool rc_image_ok(int C, int W, int H) {
  return C >= 0 && C <= 65535 && W >= 1 && H >= 1 && (int64_t)sv_div_up(W, 8) * sv_div_up(H, 8) < ((int64_t)1 << 31) &&
         (int64_t)C * W * H < ((int64_t)1 << 31);
}

extern "C" int sv_cast_pinhole(const float* nodes, const float* leaves, int64_t T, const double* cams, int C, int W, int H, float* t_hit,
                               int32_t* geometry_ids, int32_t* primitive_ids, float* primitive_uvs, int32_t* status, void* stream) {
  SV_CHECK_ARG(T >= 0 && T <= RC_MAX_TRIANGLES && rc_image_ok(C, W, H), "cast_pinhole: bad arguments (C <= 65535, C * W * H < 2^31)");
  if (C == 0) return SV_OK;
  SV_CHECK_ARG(cams && t_hit && geometry_ids && primitive_ids && primitive_uvs && status && (T == 0 || (nodes && leaves)), "cast_pinhole: null pointer");
  const int tiles_x = sv_div_up(W, 8), tiles_y = sv_div_up(H, 8);
  hipLaunchKernelGGL(k_rc_cast_pinhole, dim3(tiles_x * tiles_y, C), dim3(RC_WAVE_THREADS), 0, sv_stream(stream), nodes, leaves, T, cams, W, H, tiles_x,
                     t_hit, geometry_ids, primitive_ids, primitive_uvs, status);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ------------------------------------------------------------------ the ray tensor itself (create_rays_pinhole)
__global__ __launch_bounds__(RC_THREADS) void k_rc_rays_pinhole(const double* __restrict__ cams, int W, int H, float* __restrict__ out) {
  const int cam = blockIdx.y;
  const int64_t p = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x;
  if (p >= (int64_t)W * H) return;
  const RcOriginDir r = rc_pinhole(cams + (int64_t)cam * 12, (int)(p % W), (int)(p / W));
  float* q = out + ((int64_t)cam * W * H + p) * 6;
  q[0] = r.o.x, q[1] = r.o.y, q[2] = r.o.z, q[3] = r.d.x, q[4] = r.d.y, q[5] = r.d.z;
}

extern "C" int sv_rays_pinhole(const double* cams, int C, int W, int H, float* out, void* stream) {
  SV_CHECK_ARG(rc_image_ok(C, W, H), "rays_pinhole: bad arguments (C <= 65535, C * W * H < 2^31)");
  if (C == 0) return SV_OK;
  SV_CHECK_ARG(cams && out, "rays_pinhole: null pointer");
  hipLaunchKernelGGL(k_rc_rays_pinhole, dim3(sv_div_up((int64_t)W * H, RC_THREADS), C), dim3(RC_THREADS), 0, sv_stream(stream), cams, W, H, out);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ------------------------------------------------------------------ hit points: one stable compaction per camera, with the in-box crop
// Segment c owns rays c * R .. (c + 1) * R (R = W * H; with a ray tensor W = R and H = 1).  A chunk is the RC_THREADS rays of one workgroup.
// Pass 1 makes every ray's code (bit 0 hit, bit 1 inside the segment's box) and the chunk's two counts; pass 2, one workgroup, scans the counts
// segment-major and writes the per-segment totals; pass 3 scatters.  Integer sums only: equal bits run to run.
__device__ __forceinline__ RcOriginDir rc_segment_ray(const float* __restrict__ rays, const double* __restrict__ cams, int c, int64_t p, int W,
                                                      int64_t R) {
  if (!rays) return rc_pinhole(cams + (int64_t)c * 12, (int)(p % W), (int)(p / W));
  const float* q = rays + ((int64_t)c * R + p) * 6;
  return {{q[0], q[1], q[2]}, {q[3], q[4], q[5]}};
}
__device__ __forceinline__ RcV3 rc_hit_point(RcV3 o, RcV3 d, float t) { return {o.x + d.x * t, o.y + d.y * t, o.z + d.z * t}; }

__global__ __launch_bounds__(RC_THREADS) void k_rc_hit_codes(const float* __restrict__ rays, const double* __restrict__ cams, int W, int64_t R,
                                                             const float* __restrict__ t_hit, const float* __restrict__ boxes,
                                                             int32_t* __restrict__ codes, int32_t* __restrict__ chunk_cnt, int64_t chunks_total) {
  __shared__ int32_t wave_sums[RC_THREADS / SV_WAVE];
  const int c = blockIdx.y;
  const int64_t p = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x;
  int32_t hit = 0, inside = 0;
  if (p < R) {
    const float t = t_hit[(int64_t)c * R + p];
    hit = t < INFINITY;                                        // isfinite for a t that is never negative; NaN is no hit
    if (hit && boxes) {
      const RcOriginDir r = rc_segment_ray(rays, cams, c, p, W, R);
      const RcV3 h = rc_hit_point(r.o, r.d, t);
      const float* b = boxes + (int64_t)c * 7;
      float lx, ly;
      inside = sv_pt_in_box3d(h.x, h.y, h.z, b[0], b[1], b[2], b[3], b[4], b[5], cosf(-b[6]), sinf(-b[6]), 0.f, lx, ly);
    }
    codes[(int64_t)c * R + p] = hit | (inside << 1);
  }
  int32_t n_hit, n_in;
  sv_block_excl_scan<RC_THREADS>(hit, &n_hit, wave_sums);
  __syncthreads();
  sv_block_excl_scan<RC_THREADS>(inside, &n_in, wave_sums);
  if (threadIdx.x == 0) {
    const int64_t k = (int64_t)c * gridDim.x + blockIdx.x;
    chunk_cnt[k] = n_hit, chunk_cnt[chunks_total + k] = n_in;
  }
}

// chunk_cnt (2, n) -> chunk_off (2, n) exclusive; counts (2, C): hits per segment, then in-box hits per segment
__global__ __launch_bounds__(1024) void k_rc_scan_chunks(const int32_t* __restrict__ chunk_cnt, int32_t* __restrict__ chunk_off, int64_t n,
                                                         int chunks_per_segment, int C, int32_t* __restrict__ counts) {
  __shared__ int32_t wave_sums[1024 / SV_WAVE];
  __shared__ int32_t totals[2];
  for (int which = 0; which < 2; ++which) {
    const int32_t total = sv_block_excl_scan_array<1024>(chunk_cnt + which * n, chunk_off + which * n, n, wave_sums);
    if (threadIdx.x == 0) totals[which] = total;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < 2 * C; k += 1024) {
    const int which = k / C, c = k - which * C;
    const int32_t* off = chunk_off + which * n;
    const int32_t end = c + 1 < C ? off[(int64_t)(c + 1) * chunks_per_segment] : totals[which];
    counts[k] = end - off[(int64_t)c * chunks_per_segment];
  }
}

__global__ __launch_bounds__(RC_THREADS) void k_rc_hit_scatter(const float* __restrict__ rays, const double* __restrict__ cams, int W, int64_t R,
                                                               const float* __restrict__ t_hit, const int32_t* __restrict__ codes,
                                                               const int32_t* __restrict__ chunk_off, int64_t chunks_total,
                                                               float* __restrict__ points, int32_t* __restrict__ flags, float* __restrict__ obj_points) {
  __shared__ int32_t wave_sums[RC_THREADS / SV_WAVE];
  const int c = blockIdx.y;
  const int64_t p = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x, k = (int64_t)c * gridDim.x + blockIdx.x;
  const int32_t code = p < R ? codes[(int64_t)c * R + p] : 0;
  int32_t total;
  const int32_t rank = sv_block_excl_scan<RC_THREADS>(code & 1, &total, wave_sums);
  __syncthreads();
  const int32_t rank_in = sv_block_excl_scan<RC_THREADS>(code >> 1, &total, wave_sums);
  if (!(code & 1)) return;
  const RcOriginDir r = rc_segment_ray(rays, cams, c, p, W, R);
  const RcV3 h = rc_hit_point(r.o, r.d, t_hit[(int64_t)c * R + p]);
  const int64_t row = (int64_t)chunk_off[k] + rank;
  points[row * 3] = h.x, points[row * 3 + 1] = h.y, points[row * 3 + 2] = h.z;
  flags[row] = code >> 1;
  if (code >> 1) {
    const int64_t orow = (int64_t)chunk_off[chunks_total + k] + rank_in;
    obj_points[orow * 3] = h.x, obj_points[orow * 3 + 1] = h.y, obj_points[orow * 3 + 2] = h.z;
  }
}

static bool rc_segments_ok(int C, int W, int H) { return rc_image_ok(C, W, H) && C >= 1; }

extern "C" size_t sv_ray_hit_points_scratch_bytes(int C, int W, int H) {
  if (!rc_segments_ok(C, W, H)) return 0;
  const int64_t R = (int64_t)W * H, chunks = (int64_t)C * sv_div_up(R, RC_THREADS);
  return (size_t)(C * R + 4 * chunks) * sizeof(int32_t);      // codes | chunk counts (2, chunks) | chunk offsets (2, chunks)
}

extern "C" int sv_ray_hit_points(const float* rays, const double* cams, int C, int W, int H, const float* t_hit, const float* boxes, void* scratch,
                                 float* points, int32_t* flags, float* obj_points, int32_t* counts, void* stream) {
  SV_CHECK_ARG(rc_segments_ok(C, W, H), "ray_hit_points: bad arguments (1 <= C <= 65535, C * W * H < 2^31)");
  SV_CHECK_ARG((rays != nullptr) != (cams != nullptr), "ray_hit_points: give the ray tensor or the cameras, not both");
  SV_CHECK_ARG(t_hit && scratch && points && flags && obj_points && counts, "ray_hit_points: null pointer");
  hipStream_t st = sv_stream(stream);
  const int64_t R = (int64_t)W * H;
  const int per = sv_div_up(R, RC_THREADS);
  const int64_t chunks = (int64_t)C * per;
  int32_t* codes = reinterpret_cast<int32_t*>(scratch);
  int32_t* chunk_cnt = codes + (int64_t)C * R;
  int32_t* chunk_off = chunk_cnt + 2 * chunks;
  hipLaunchKernelGGL(k_rc_hit_codes, dim3(per, C), dim3(RC_THREADS), 0, st, rays, cams, W, R, t_hit, boxes, codes, chunk_cnt, chunks);
  hipLaunchKernelGGL(k_rc_scan_chunks, dim3(1), dim3(1024), 0, st, chunk_cnt, chunk_off, chunks, per, C, counts);
  hipLaunchKernelGGL(k_rc_hit_scatter, dim3(per, C), dim3(RC_THREADS), 0, st, rays, cams, W, R, t_hit, codes, chunk_off, chunks, points, flags,
                     obj_points);
  SV_LAUNCH_CHECK();
  return SV_OK;
}
