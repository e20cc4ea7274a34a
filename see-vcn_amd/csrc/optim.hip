// Fused multi-tensor Adam step with gradient-norm clipping (include/seevcn_hip.h, "optimizer step").  Replaces, per train step, the host loops of
// detector3d/tools/train_utils/optimization/fastai_optim.py:135-152 (one mul_ per parameter), torch.nn.utils.clip_grad_norm_ (per-tensor norms,
// stack, norm, clamp, per-tensor scale; detector3d/tools/train_utils/train_utils.py:53) and torch.optim.Adam's passes (:54) by at most three launches
// over a chunk table kept on the device.
//
// Order of the gradient norm (sv_optim_grad_sqnorm), the same whatever the alignment of the gradient:
//   chunk c holds elements [0, n) of one tensor's slice, n <= SV_OPTIM_CHUNK.  Thread t of 256 takes the groups of four elements 4i .. 4i+3 for
//   i = t, t + 256, ... and adds (double)g * (double)g (exact) to ONE float64 accumulator, elements ascending.  The 64 accumulators of a wave are
//   summed by the xor butterfly of wave.h (distance 32, 16, .. 1), the four wave totals in ascending wave order by thread 0: partial[c], float64.
//   The finalize launch adds the partials in ascending chunk order, in 256 blocks: thread j of its one workgroup adds partials [j B, (j + 1) B),
//   B = ceil(nchunks / 256), ascending, to one float64; thread 0 adds the 256 block sums, ascending; then the float64 square root, rounded to fp32.
//   (One thread adding all partials costs about 10 ns a partial: 12 us of a 45 us step at 1301 chunks.)
// No atomics anywhere, so equal inputs at equal chunking give equal bits.
//
// Order of the update (sv_optim_adam_step), fp32, every operation rounded once (-ffp-contract=off, correctly rounded divide and sqrt):
//   g = grad * clip
//   g = g + wd * p                         mode 1 (L2, OPTIMIZER: adam)
//   p = p * decay                          mode 2 (decoupled: true_wd / AdamW), decay = fp32(1 - lr * wd) from float64
//   m = b1 * m + omb1 * g                  b1 = fp32(beta1), omb1 = fp32(1 - beta1) from float64
//   v = b2 * v + (omb2 * g) * g
//   p = p - (step * m) / (sqrt(v) / rbc2 + eps)
// step = fp32(lr / bc1), rbc2 = fp32(sqrt(bc2)), bc1 = 1 - beta1^t, bc2 = 1 - beta2^t in float64 with the tensor's own t (advanced by the finalize
// launch before the update reads it) and the CURRENT beta1: torch's semantics under a schedule that moves beta1.
#include "common.h"
#include "wave.h"

#define SV_OPTIM_THREADS 256
#define SV_OPTIM_VECS (SV_OPTIM_CHUNK / 4 / SV_OPTIM_THREADS)      // dwordx4 per thread and stream in a whole chunk
static_assert(SV_OPTIM_VECS * 4 * SV_OPTIM_THREADS == SV_OPTIM_CHUNK, "a chunk is a whole number of vectors per thread");

struct SvOptimChunk {          // 48 bytes, the host packs the same layout (seevcn_amd/optim.py)
  float* p;
  float* g;
  float* m;
  float* v;
  int32_t n;
  int32_t tensor;
  int32_t group;
  int32_t pad;
};
static_assert(sizeof(SvOptimChunk) == 48, "chunk table layout");

struct SvOptimGroupsD {        // finalize: float64 scalars by value
  double lr[SV_OPTIM_MAX_GROUPS], b1[SV_OPTIM_MAX_GROUPS], b2[SV_OPTIM_MAX_GROUPS];
};
struct SvOptimGroupsF {        // update: fp32 scalars by value
  float b1[SV_OPTIM_MAX_GROUPS], omb1[SV_OPTIM_MAX_GROUPS], b2[SV_OPTIM_MAX_GROUPS], omb2[SV_OPTIM_MAX_GROUPS];
  float eps[SV_OPTIM_MAX_GROUPS], wd[SV_OPTIM_MAX_GROUPS], decay[SV_OPTIM_MAX_GROUPS];
  int32_t mode[SV_OPTIM_MAX_GROUPS];
};

static __device__ __forceinline__ bool sv_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

__global__ __launch_bounds__(SV_OPTIM_THREADS) void optim_sqnorm_kernel(const SvOptimChunk* __restrict__ chunks, double* __restrict__ partials) {
  __shared__ double wave_tot[SV_OPTIM_THREADS / SV_WAVE];
  const SvOptimChunk ch = chunks[blockIdx.x];
  const float* __restrict__ g = ch.g;
  const int n = ch.n, n4 = n >> 2;
  double acc = 0.0;
  if (sv_aligned16(g)) {
    const float4* g4 = reinterpret_cast<const float4*>(g);
    for (int i = threadIdx.x; i < n4; i += SV_OPTIM_THREADS) {
      const float4 x = g4[i];
      acc += (double)x.x * (double)x.x;
      acc += (double)x.y * (double)x.y;
      acc += (double)x.z * (double)x.z;
      acc += (double)x.w * (double)x.w;
    }
  } else {
    for (int i = threadIdx.x; i < n4; i += SV_OPTIM_THREADS) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const double x = (double)g[4 * i + k];
        acc += x * x;
      }
    }
  }
  // the last n % 4 elements belong to group n4, i.e. to thread n4 % 256, after its whole groups
  if ((int)threadIdx.x == (n4 % SV_OPTIM_THREADS))
    for (int e = 4 * n4; e < n; ++e) {
      const double x = (double)g[e];
      acc += x * x;
    }
  acc = sv_wave_reduce_sum(acc);
  if ((threadIdx.x & (SV_WAVE - 1)) == 0) wave_tot[threadIdx.x / SV_WAVE] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = wave_tot[0];
#pragma unroll
    for (int w = 1; w < SV_OPTIM_THREADS / SV_WAVE; ++w) s += wave_tot[w];
    partials[blockIdx.x] = s;
  }
}

// One workgroup.  norm_out[0] = total_norm, norm_out[1] = clip; t[tensor] += 1 and tensor_scal[2 tensor] = {step, rbc2} for the present tensors.
__global__ __launch_bounds__(SV_OPTIM_THREADS) void optim_finalize_kernel(const double* __restrict__ partials, int nparts, float max_norm,
                                                                           const int32_t* __restrict__ present, int npresent, SvOptimGroupsD gs,
                                                                           int32_t* __restrict__ t, float* __restrict__ tensor_scal,
                                                                           float* __restrict__ norm_out) {
  __shared__ double tile[SV_OPTIM_THREADS];
  if (partials != nullptr) {
    // thread j adds its block of ceil(nparts / 256) consecutive partials in ascending order, thread 0 the 256 block sums in ascending order
    const int per = (nparts + SV_OPTIM_THREADS - 1) / SV_OPTIM_THREADS;
    const int lo = min((int)threadIdx.x * per, nparts), hi = min(lo + per, nparts);
    double acc = 0.0;
    for (int k = lo; k < hi; ++k) acc += partials[k];
    tile[threadIdx.x] = acc;
    __syncthreads();
    double total = 0.0;
    if (threadIdx.x == 0)
      for (int j = 0; j < SV_OPTIM_THREADS; ++j) total += tile[j];
    if (threadIdx.x == 0) {
      const float norm = (float)sqrt(total);
      const float c = max_norm / (norm + 1e-6f);
      norm_out[0] = norm;
      norm_out[1] = c > 1.0f ? 1.0f : c;          // a NaN coefficient stays NaN, as torch.clamp keeps it
    }
  } else if (threadIdx.x == 0) {
    norm_out[0] = 0.0f;
    norm_out[1] = 1.0f;
  }
  for (int i = threadIdx.x; i < npresent; i += SV_OPTIM_THREADS) {
    const int tensor = present[2 * i], group = present[2 * i + 1];
    const int32_t step = t[tensor] + 1;
    t[tensor] = step;
    const double bc1 = 1.0 - pow(gs.b1[group], (double)step), bc2 = 1.0 - pow(gs.b2[group], (double)step);
    tensor_scal[2 * tensor] = (float)(gs.lr[group] / bc1);
    tensor_scal[2 * tensor + 1] = (float)sqrt(bc2);
  }
}

struct SvOptimScalars {
  float clip, b1, omb1, b2, omb2, eps, wd, decay, step, rbc2;
  int mode;
};

static __device__ __forceinline__ void sv_adam_element(float& p, float g, float& m, float& v, const SvOptimScalars& s) {
  g = g * s.clip;
  if (s.mode == SV_OPTIM_L2) g = g + s.wd * p;
  if (s.mode == SV_OPTIM_DECOUPLED) p = p * s.decay;
  m = s.b1 * m + s.omb1 * g;
  v = s.b2 * v + (s.omb2 * g) * g;
  const float denom = sqrtf(v) / s.rbc2 + s.eps;
  p = p - (s.step * m) / denom;
}

__global__ __launch_bounds__(SV_OPTIM_THREADS) void optim_adam_kernel(const SvOptimChunk* __restrict__ chunks, SvOptimGroupsF gs,
                                                                       const float* __restrict__ tensor_scal, const float* __restrict__ norm_out,
                                                                       int consume) {
  const SvOptimChunk ch = chunks[blockIdx.x];
  SvOptimScalars s;
  s.clip = norm_out[1];
  s.b1 = gs.b1[ch.group], s.omb1 = gs.omb1[ch.group], s.b2 = gs.b2[ch.group], s.omb2 = gs.omb2[ch.group];
  s.eps = gs.eps[ch.group], s.wd = gs.wd[ch.group], s.decay = gs.decay[ch.group], s.mode = gs.mode[ch.group];
  s.step = tensor_scal[2 * ch.tensor], s.rbc2 = tensor_scal[2 * ch.tensor + 1];
  float* p = ch.p;
  float* g = ch.g;
  float* m = ch.m;
  float* v = ch.v;
  const int n = ch.n;
  int done = 0;
  if (sv_aligned16(p) && sv_aligned16(g) && sv_aligned16(m) && sv_aligned16(v)) {
    // dwordx4 over the whole groups of four; the chunk size is a multiple of four, so only a tensor's last chunk has a tail
    float4* p4 = reinterpret_cast<float4*>(p);
    float4* g4 = reinterpret_cast<float4*>(g);
    float4* m4 = reinterpret_cast<float4*>(m);
    float4* v4 = reinterpret_cast<float4*>(v);
    const int n4 = n >> 2;
    // a whole chunk is SV_OPTIM_VECS vectors a thread: all sixteen loads are issued before the first store, so that no load waits behind a store
    // the compiler cannot prove distinct
    float4 pp[SV_OPTIM_VECS], gg[SV_OPTIM_VECS], mm[SV_OPTIM_VECS], vv[SV_OPTIM_VECS];
#pragma unroll
    for (int k = 0; k < SV_OPTIM_VECS; ++k) {
      const int i = threadIdx.x + k * SV_OPTIM_THREADS;
      if (i < n4) pp[k] = p4[i], gg[k] = g4[i], mm[k] = m4[i], vv[k] = v4[i];
    }
#pragma unroll
    for (int k = 0; k < SV_OPTIM_VECS; ++k) {
      const int i = threadIdx.x + k * SV_OPTIM_THREADS;
      if (i < n4) {
        sv_adam_element(pp[k].x, gg[k].x, mm[k].x, vv[k].x, s);
        sv_adam_element(pp[k].y, gg[k].y, mm[k].y, vv[k].y, s);
        sv_adam_element(pp[k].z, gg[k].z, mm[k].z, vv[k].z, s);
        sv_adam_element(pp[k].w, gg[k].w, mm[k].w, vv[k].w, s);
        p4[i] = pp[k];
        m4[i] = mm[k];
        v4[i] = vv[k];
        if (consume) g4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    done = n4 << 2;
  }
  // scalar path: the tail of an aligned chunk, or all of a chunk with a pointer off a 16-byte boundary (coalesced dwords, nothing past [0, n))
  for (int e = done + threadIdx.x; e < n; e += SV_OPTIM_THREADS) {
    float pp = p[e], mm = m[e], vv = v[e];
    sv_adam_element(pp, g[e], mm, vv, s);
    p[e] = pp;
    m[e] = mm;
    v[e] = vv;
    if (consume) g[e] = 0.f;
  }
}

extern "C" int sv_optim_chunk_elems(void) { return SV_OPTIM_CHUNK; }
extern "C" int sv_optim_chunk_bytes(void) { return (int)sizeof(SvOptimChunk); }
extern "C" int sv_optim_max_groups(void) { return SV_OPTIM_MAX_GROUPS; }

extern "C" int sv_optim_grad_sqnorm(const void* chunks, int nchunks, double* partials, void* stream) {
  SV_CHECK_ARG(nchunks >= 0, "sv_optim_grad_sqnorm: nchunks %d", nchunks);
  if (nchunks == 0) return SV_OK;
  SV_CHECK_ARG(chunks && partials, "sv_optim_grad_sqnorm: null pointer");
  SV_CHECK_ARG(sv_on_device(chunks) && sv_on_device(partials), "sv_optim_grad_sqnorm: the chunk table and the partials must be device memory");
  optim_sqnorm_kernel<<<nchunks, SV_OPTIM_THREADS, 0, sv_stream(stream)>>>(static_cast<const SvOptimChunk*>(chunks), partials);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_optim_adam_step(const void* chunks, int nchunks, const int32_t* present, int npresent, const double* groups, int ngroups,
                                  const double* partials, float max_norm, int consume, int32_t* t, float* tensor_scal, float* norm_out,
                                  void* stream) {
  SV_CHECK_ARG(nchunks >= 0 && npresent >= 0, "sv_optim_adam_step: nchunks %d npresent %d", nchunks, npresent);
  SV_CHECK_ARG(ngroups >= 1 && ngroups <= SV_OPTIM_MAX_GROUPS, "sv_optim_adam_step: %d parameter groups, 1 .. %d are built", ngroups,
               SV_OPTIM_MAX_GROUPS);
  SV_CHECK_ARG(groups && t && tensor_scal && norm_out, "sv_optim_adam_step: null pointer");
  SV_CHECK_ARG((nchunks == 0 || chunks) && (npresent == 0 || present), "sv_optim_adam_step: null table");
  SV_CHECK_ARG(sv_on_device(t) && sv_on_device(tensor_scal) && sv_on_device(norm_out) && (nchunks == 0 || sv_on_device(chunks)) &&
                   (npresent == 0 || sv_on_device(present)) && (!partials || sv_on_device(partials)),
               "sv_optim_adam_step: tables, state and outputs must be device memory");
  SvOptimGroupsD gd;
  SvOptimGroupsF gf;
  for (int i = 0; i < SV_OPTIM_MAX_GROUPS; ++i) {
    const double* q = groups + 6 * (i < ngroups ? i : 0);
    const double lr = q[0], b1 = q[1], b2 = q[2], eps = q[3], wd = q[4];
    const int mode = (int)q[5];
    SV_CHECK_ARG(mode == SV_OPTIM_NO_DECAY || mode == SV_OPTIM_L2 || mode == SV_OPTIM_DECOUPLED, "sv_optim_adam_step: group %d mode %d", i, mode);
    gd.lr[i] = lr, gd.b1[i] = b1, gd.b2[i] = b2;
    gf.b1[i] = (float)b1, gf.omb1[i] = (float)(1.0 - b1), gf.b2[i] = (float)b2, gf.omb2[i] = (float)(1.0 - b2);
    gf.eps[i] = (float)eps, gf.wd[i] = (float)wd, gf.decay[i] = (float)(1.0 - lr * wd), gf.mode[i] = mode;
  }
  const bool clipped = partials != nullptr && max_norm > 0.f;
  optim_finalize_kernel<<<1, SV_OPTIM_THREADS, 0, sv_stream(stream)>>>(clipped ? partials : nullptr, nchunks, max_norm, present, npresent, gd, t,
                                                                       tensor_scal, norm_out);
  SV_LAUNCH_CHECK();
  if (nchunks > 0) {
    optim_adam_kernel<<<nchunks, SV_OPTIM_THREADS, 0, sv_stream(stream)>>>(static_cast<const SvOptimChunk*>(chunks), gf, tensor_scal, norm_out,
                                                                           consume);
    SV_LAUNCH_CHECK();
  }
  return SV_OK;
}
