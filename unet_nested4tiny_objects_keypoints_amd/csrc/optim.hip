// Fused optimizer step: the reference trainer's own optimizers (tools/optimizers/{adamw,adabound,sgdw}.py) as ONE
// multi-tensor launch per step.  Every parameter of every group is a segment of a device table (param, grad, exp_avg,
// exp_avg_sq, aux: five streams); the table, the persistent grid, the chunk walk and the arrival counter of capturable
// launches are multi_tensor.h's and are described there.
//
// Per element the op sequence of the reference's torch calls is restated in their order, each aten op as ONE float32 op
// rounded once as IEEE-754 rounds it: add(a, b, alpha) = fma(alpha, b, a), addcmul(a, b, c, s) = fma(s*b, c, a),
// addcdiv(a, b, c, s) = a + (s*b)/c, sqrt = the correctly rounded sqrtf (NOT __fsqrt_rn: without
// OCML_BASIC_ROUNDED_OPERATIONS the HIP headers map that to the native 1-ulp v_sqrt_f32).  Implicit contraction is off;
// every fma below is one aten op.  aten's CPU kernels (the golden fixtures are CPU runs of the reference) round + - * /
// and fma the same way; their vectorised sqrt is not correctly rounded in the build that made the fixtures, and that is
// the whole of the rounding allowance of tests/test_gpu_optim.py.  tests/test_gpu_optim_elementwise.py holds every
// element of every step to tests/optim_oracle.py, a numpy restatement of this contract, bit for bit.
//   AdamW     m = fma(1-b1, g, m*b1);  v = fma((1-b2)*g, g, v*b2);  [vmax = max(vmax, v)];  denom = sqrt(v|vmax) + eps;
//             [d = p*wd];  p = p + (-step_size*m)/denom;  [p = p - d]
//   AdaBound  [g = fma(wd, p, g)];  m, v, vmax, denom as above;  s = clamp(step_size/denom, lo, hi)*m;  p = p - s
//   SGDW      [buf = first ? 0 + g : fma(1-damp, g, buf*mom)];  [p = fma(-wd, p, p)]   (the reference never applies g)
// Scalars (bias corrections, step size, AdaBound's bounds) are formed in double from the segment's own step count and
// rounded to float once, as the reference forms them in Python floats and hands them to aten as float scalars.
// No floating-point atomics, no cross-workgroup order: every element's result depends on that element alone.
//
// Gradient clipping / non-finite skip (unetpp_grad_norm, unetpp_optim_step_clip, unetpp_grad_scale) over the same table:
//   norm pass   one double per CHUNK: sum of double(g)^2 (the product of two floats is exact in double), per thread in
//               element order, a fixed tree across the wave, the four waves through LDS; plain stores to partials[c].
//               The element -> thread map is the float4 one on every path, so the bits do not depend on the alignment,
//               on the grid size or on which workgroup took which chunk.
//   combine     launch-boundary reduce: every workgroup of the consuming launch sums partials[0..n_chunks) itself, in
//               one fixed order, before its first chunk; workgroup 0 publishes {total_norm, coef, skipped_steps}.
//   consume     total = float(sqrt(sum)); c = max_norm / (total + 1e-6f); coef = c > 1 ? 1 : c (torch's
//               clip_grad_norm_ in fp32: NaN stays NaN, an infinite norm gives 0); g = g * coef as it is read.
#include "common.h"
#include "multi_tensor.h"

#include <math.h>

#pragma clang fp contract(off)

namespace unetpp {
namespace {

enum { H_LR = 0, H_B1 = 1, H_B2 = 2, H_EPS = 3, H_WD = 4, H_FINAL_LR = 5, H_GAMMA = 6 };

struct Scalars {
  float b1, omb1, b2, omb2, eps, wd, neg_step, step, lo, hi;
  bool first;
};

__device__ __forceinline__ Scalars make_scalars(int kind, const double* h, double t) {
  Scalars s;
  s.b1 = static_cast<float>(h[H_B1]);
  s.b2 = static_cast<float>(h[H_B2]);
  s.omb1 = static_cast<float>(1.0 - h[H_B1]);
  s.omb2 = static_cast<float>(1.0 - h[H_B2]);   // SGDW: 1 - dampening
  s.eps = static_cast<float>(h[H_EPS]);
  s.wd = static_cast<float>(h[H_WD]);
  s.first = t <= 1.0;
  s.step = s.neg_step = s.lo = s.hi = 0.f;
  if (kind != UNETPP_OPTIM_SGDW) {
    const double bc1 = 1.0 - pow(h[H_B1], t);
    const double bc2 = 1.0 - pow(h[H_B2], t);
    const double step_size = h[H_LR] * sqrt(bc2) / bc1;
    s.step = static_cast<float>(step_size);
    s.neg_step = static_cast<float>(-step_size);
    if (kind == UNETPP_OPTIM_ADABOUND) {
      const double f = h[H_FINAL_LR], gamma = h[H_GAMMA];
      s.lo = static_cast<float>(f * (1.0 - 1.0 / (gamma * t + 1.0)));
      s.hi = static_cast<float>(f * (1.0 + 1.0 / (gamma * t)));
    }
  }
  return s;
}

// one element of every stream; aux = max_exp_avg_sq (AMS) or momentum_buffer (SGDW)
template <int KIND, bool AMS>
__device__ __forceinline__ void update(float& p, float g, float& m, float& v, float& a, const Scalars& s, bool decay,
                                       bool has_aux) {
  if (KIND == UNETPP_OPTIM_SGDW) {
    if (has_aux) a = s.first ? 0.f + g : fmaf(s.omb2, g, a * s.b1);
    if (decay) p = fmaf(-s.wd, p, p);
    return;
  }
  if (KIND == UNETPP_OPTIM_ADABOUND && decay) g = fmaf(s.wd, p, g);
  m = fmaf(s.omb1, g, m * s.b1);
  v = fmaf(s.omb2 * g, g, v * s.b2);
  float denom;
  if (AMS) {
    a = fmaxf(a, v);
    denom = sqrtf(a) + s.eps;
  } else {
    denom = sqrtf(v) + s.eps;
  }
  if (KIND == UNETPP_OPTIM_ADAMW) {
    const float d = decay ? p * s.wd : 0.f;
    p = p + (s.neg_step * m) / denom;
    if (decay) p = p - d;
  } else {
    float r = s.step / denom;
    r = fminf(fmaxf(r, s.lo), s.hi);
    r = r * m;
    p = p - r;
  }
}

// the step itself; CLIP: every gradient is multiplied by coef (one rounded multiply) as it is read
template <int KIND, bool AMS, bool CLIP>
__device__ __forceinline__ void optim_body(const unetpp_optim_segment* __restrict__ segs, int32_t n_segments,
                                           const int32_t* __restrict__ chunk_seg, int64_t n_chunks,
                                           const double* __restrict__ hyper, const double* __restrict__ steps,
                                           int32_t* done, float coef) {
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const int si = chunk_seg[c];
    const unetpp_optim_segment sg = segs[si];
    // (a capturable SGDW segment without momentum has no counter: its count is never used)
    const double t = sg.step != nullptr ? static_cast<double>(*sg.step) + 1.0 : steps != nullptr ? steps[si] : 2.0;
    const Scalars s = make_scalars(KIND, hyper + int64_t(sg.group) * UNETPP_OPTIM_HYPER, t);
    const bool decay = s.wd != 0.f;
    const bool has_aux = sg.aux != nullptr;
    float* __restrict__ P = sg.param;
    const float* __restrict__ G = sg.grad;
    float* __restrict__ M = sg.exp_avg;
    float* __restrict__ V = sg.exp_avg_sq;
    float* __restrict__ A = sg.aux;
    const bool moments = KIND != UNETPP_OPTIM_SGDW;
    walk_chunk(
        chunk_span(sg.numel, sg.chunk_begin, c), sg.vec != 0,
        [&](int64_t i) __attribute__((always_inline)) {
          f32x4 p = *reinterpret_cast<const f32x4*>(P + i);
          f32x4 g = *reinterpret_cast<const f32x4*>(G + i);
          if (CLIP) g = g * coef;
          f32x4 m = {0.f, 0.f, 0.f, 0.f}, v = m, a = m;
          if (moments) {
            m = *reinterpret_cast<const f32x4*>(M + i);
            v = *reinterpret_cast<const f32x4*>(V + i);
          }
          if (has_aux && (AMS || KIND == UNETPP_OPTIM_SGDW)) a = *reinterpret_cast<const f32x4*>(A + i);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float pe = p[e], me = m[e], ve = v[e], ae = a[e];
            update<KIND, AMS>(pe, g[e], me, ve, ae, s, decay, has_aux);
            p[e] = pe, m[e] = me, v[e] = ve, a[e] = ae;
          }
          if (KIND != UNETPP_OPTIM_SGDW || decay) *reinterpret_cast<f32x4*>(P + i) = p;
          if (moments) {
            *reinterpret_cast<f32x4*>(M + i) = m;
            *reinterpret_cast<f32x4*>(V + i) = v;
          }
          if (has_aux && (AMS || KIND == UNETPP_OPTIM_SGDW)) *reinterpret_cast<f32x4*>(A + i) = a;
        },
        [&](int64_t i) __attribute__((always_inline)) {
          float pe = P[i], me = moments ? M[i] : 0.f, ve = moments ? V[i] : 0.f, ae = has_aux ? A[i] : 0.f;
          update<KIND, AMS>(pe, CLIP ? G[i] * coef : G[i], me, ve, ae, s, decay, has_aux);
          P[i] = pe;
          if (moments) M[i] = me, V[i] = ve;
          if (has_aux) A[i] = ae;
        });
  }
  if (done == nullptr) return;
  // capturable: the device step counters advance once every workgroup has read them
  if (!last_workgroup(done)) return;
  for (int i = threadIdx.x; i < n_segments; i += kMtThreads)
    if (segs[i].step != nullptr) segs[i].step[0] = segs[i].step[0] + 1.f;
  if (threadIdx.x == 0) *done = 0;
}

template <int KIND, bool AMS>
__global__ void __launch_bounds__(kMtThreads) optim_kernel(const unetpp_optim_segment* __restrict__ segs,
                                                           int32_t n_segments, const int32_t* __restrict__ chunk_seg,
                                                           int64_t n_chunks, const double* __restrict__ hyper,
                                                           const double* __restrict__ steps, int32_t* done) {
  optim_body<KIND, AMS, false>(segs, n_segments, chunk_seg, n_chunks, hyper, steps, done, 1.f);
}

// ---- gradient norm, clip coefficient, non-finite skip ---------------------------------------------------------------
constexpr int kOptWaves = kMtThreads / 64;

// sum over the workgroup in one fixed order: a tree across each wave, then ((w0 + w1) + (w2 + w3)); every thread gets it.
// `red` must not be in use by a sum that some wave may still be reading (callers in a loop alternate two buffers).
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = v + __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  static_assert(kOptWaves == 4, "the cross-wave order below is written out for four waves");
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ void __launch_bounds__(kMtThreads) grad_norm_kernel(const unetpp_optim_segment* __restrict__ segs,
                                                               const int32_t* __restrict__ chunk_seg,
                                                               int64_t n_chunks, double* __restrict__ partials) {
  __shared__ double red[2][kOptWaves];
  int slot = 0;
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const unetpp_optim_segment sg = segs[chunk_seg[c]];
    const ChunkSpan sp = chunk_span(sg.numel, sg.chunk_begin, c);
    const int64_t end = sp.end;
    const float* __restrict__ G = sg.grad;
    double acc = 0.0;
    // thread t owns elements (k*256 + t)*4 + e of the chunk, added in (k, e) order -- float4 loads where the segment is
    // aligned and the four are inside it, scalar loads of the same elements otherwise: the same sum either way
#pragma unroll
    for (int k = 0; k < kMtVecPerThread; ++k) {
      const int64_t i = sp.begin + vec_slot_offset(k, threadIdx.x);
      if (i >= end) break;
      if (sg.vec && i + 4 <= end) {
        const f32x4 g = *reinterpret_cast<const f32x4*>(G + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const double d = static_cast<double>(g[e]);
          acc = acc + d * d;
        }
      } else {
        for (int e = 0; e < 4 && i + e < end; ++e) {
          const double d = static_cast<double>(G[i + e]);
          acc = acc + d * d;
        }
      }
    }
    const double sum = block_sum(acc, red[slot]);
    slot ^= 1;
    if (threadIdx.x == 0) partials[c] = sum;
  }
}

struct Clip {
  float coef;
  bool skip;
};

// The launch-boundary reduce: EVERY workgroup sums the norm pass's per-chunk partials in the same fixed order, so all of
// them hold the same bits without exchanging anything inside the launch; workgroup 0 publishes.  max_norm <= 0: no
// clipping (coef = 1), the norm is formed for the skip decision and for the caller.
__device__ __forceinline__ Clip clip_prologue(const double* __restrict__ partials, int64_t n_chunks, float max_norm,
                                              bool skip_nonfinite, unetpp_clip_state* state, double* red) {
  double acc = 0.0;
  for (int64_t j = threadIdx.x; j < n_chunks; j += kMtThreads) acc = acc + partials[j];
  const double sum = block_sum(acc, red);
  const float total = static_cast<float>(sqrt(sum));   // the one fp32 rounding
  Clip cl;
  cl.coef = 1.f;
  if (max_norm > 0.f) {
    const float c = max_norm / (total + 1e-6f);
    cl.coef = c > 1.f ? 1.f : c;                       // NaN stays NaN, as torch.clamp keeps it
  }
  cl.skip = skip_nonfinite && !isfinite(sum);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    state->total_norm = total;
    state->coef = cl.coef;
    if (cl.skip) state->skipped_steps = state->skipped_steps + 1;
  }
  return cl;
}

template <int KIND, bool AMS>
__global__ void __launch_bounds__(kMtThreads) optim_clip_kernel(const unetpp_optim_segment* __restrict__ segs,
                                                                int32_t n_segments,
                                                                const int32_t* __restrict__ chunk_seg,
                                                                int64_t n_chunks, const double* __restrict__ hyper,
                                                                const double* __restrict__ steps, int32_t* done,
                                                                const double* __restrict__ partials,
                                                                unetpp_clip_state* state, int32_t skip_nonfinite) {
  __shared__ double red[kOptWaves];
  const Clip cl = clip_prologue(partials, n_chunks, static_cast<float>(hyper[UNETPP_OPTIM_H_MAX_NORM]),
                                skip_nonfinite != 0, state, red);
  if (cl.skip) return;   // every workgroup decides alike: nothing is stored, the arrival counter stays zero
  optim_body<KIND, AMS, true>(segs, n_segments, chunk_seg, n_chunks, hyper, steps, done, cl.coef);
}

__global__ void __launch_bounds__(kMtThreads) grad_scale_kernel(const unetpp_optim_segment* __restrict__ segs,
                                                                const int32_t* __restrict__ chunk_seg,
                                                                int64_t n_chunks, const double* __restrict__ partials,
                                                                float max_norm, unetpp_clip_state* state) {
  __shared__ double red[kOptWaves];
  const Clip cl = clip_prologue(partials, n_chunks, max_norm, false, state, red);
  if (cl.coef == 1.f) return;   // g * 1 = g bit for bit: nothing to write
  const float coef = cl.coef;
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const unetpp_optim_segment sg = segs[chunk_seg[c]];
    float* __restrict__ G = const_cast<float*>(sg.grad);
    walk_chunk(
        chunk_span(sg.numel, sg.chunk_begin, c), sg.vec != 0,
        [&](int64_t i) __attribute__((always_inline)) {
          const f32x4 g = *reinterpret_cast<const f32x4*>(G + i);
          *reinterpret_cast<f32x4*>(G + i) = g * coef;
        },
        [&](int64_t i) __attribute__((always_inline)) { G[i] = G[i] * coef; });
  }
}

// (kind, AMS flag) -> the template arguments and the kernel labels of the plain and of the clipped step
template <int KIND, bool AMS>
struct Variant {
  static constexpr int kind = KIND;
  static constexpr bool ams = AMS;
  const char *label, *clip_label;
};

template <class F>
void with_variant(int32_t kind, bool ams, F&& f) {
  switch (kind * 2 + (ams ? 1 : 0)) {
    case UNETPP_OPTIM_ADAMW * 2: f(Variant<UNETPP_OPTIM_ADAMW, false>{"optim_adamw", "optim_clip_adamw"}); break;
    case UNETPP_OPTIM_ADAMW * 2 + 1:
      f(Variant<UNETPP_OPTIM_ADAMW, true>{"optim_adamw_amsgrad", "optim_clip_adamw_amsgrad"});
      break;
    case UNETPP_OPTIM_ADABOUND * 2:
      f(Variant<UNETPP_OPTIM_ADABOUND, false>{"optim_adabound", "optim_clip_adabound"});
      break;
    case UNETPP_OPTIM_ADABOUND * 2 + 1:
      f(Variant<UNETPP_OPTIM_ADABOUND, true>{"optim_adabound_amsbound", "optim_clip_adabound_amsbound"});
      break;
    default: f(Variant<UNETPP_OPTIM_SGDW, false>{"optim_sgdw", "optim_clip_sgdw"}); break;
  }
}

}  // namespace
}  // namespace unetpp

using namespace unetpp;

extern "C" int64_t unetpp_optim_chunk_elems(void) { return kMtChunk; }

extern "C" int unetpp_optim_step(int32_t kind, int32_t flags, const unetpp_optim_segment* segments, int32_t n_segments,
                                 const int32_t* chunk_segment, int64_t n_chunks, const double* hyper,
                                 const double* steps, int32_t* done, void* stream) {
  if (!table_args_ok(segments, n_segments, chunk_segment, n_chunks) || hyper == nullptr) return UNETPP_EINVAL;
  if (kind < UNETPP_OPTIM_ADAMW || kind > UNETPP_OPTIM_SGDW) return UNETPP_EINVAL;
  if ((flags & ~(UNETPP_OPTIM_AMS | UNETPP_OPTIM_CAPTURABLE)) != 0) return UNETPP_EINVAL;
  const bool ams = (flags & UNETPP_OPTIM_AMS) != 0, capturable = (flags & UNETPP_OPTIM_CAPTURABLE) != 0;
  if (ams && kind == UNETPP_OPTIM_SGDW) return UNETPP_EINVAL;
  if (capturable ? (done == nullptr || steps != nullptr) : (steps == nullptr || done != nullptr)) return UNETPP_EINVAL;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  with_variant(kind, ams, [&](auto v) {
    hipLaunchKernelGGL((optim_kernel<decltype(v)::kind, decltype(v)::ams>), dim3(persistent_grid(n_chunks)),
                       dim3(kMtThreads), 0, st, segments, n_segments, chunk_segment, n_chunks, hyper, steps, done);
    note_kernel(v.label);
  });
  return launch_status();
}

extern "C" int unetpp_grad_norm(const unetpp_optim_segment* segments, int32_t n_segments, const int32_t* chunk_segment,
                               int64_t n_chunks, double* partials, void* stream) {
  if (!table_args_ok(segments, n_segments, chunk_segment, n_chunks) || partials == nullptr) return UNETPP_EINVAL;
  hipLaunchKernelGGL(grad_norm_kernel, dim3(persistent_grid(n_chunks)), dim3(kMtThreads), 0,
                     static_cast<hipStream_t>(stream), segments, chunk_segment, n_chunks, partials);
  note_kernel("grad_norm");
  return launch_status();
}

extern "C" int unetpp_optim_step_clip(int32_t kind, int32_t flags, const unetpp_optim_segment* segments,
                                      int32_t n_segments, const int32_t* chunk_segment, int64_t n_chunks,
                                      const double* hyper, const double* steps, int32_t* done, const double* partials,
                                      unetpp_clip_state* state, void* stream) {
  if (!table_args_ok(segments, n_segments, chunk_segment, n_chunks) || hyper == nullptr || partials == nullptr ||
      state == nullptr)
    return UNETPP_EINVAL;
  if (kind < UNETPP_OPTIM_ADAMW || kind > UNETPP_OPTIM_SGDW) return UNETPP_EINVAL;
  if ((flags & ~(UNETPP_OPTIM_AMS | UNETPP_OPTIM_CAPTURABLE | UNETPP_OPTIM_SKIP_NONFINITE)) != 0) return UNETPP_EINVAL;
  const bool ams = (flags & UNETPP_OPTIM_AMS) != 0, capturable = (flags & UNETPP_OPTIM_CAPTURABLE) != 0;
  const int32_t skip = (flags & UNETPP_OPTIM_SKIP_NONFINITE) != 0;
  if (ams && kind == UNETPP_OPTIM_SGDW) return UNETPP_EINVAL;
  if (skip && !capturable) return UNETPP_EINVAL;   // an eager caller has advanced its step counts already
  if (capturable ? (done == nullptr || steps != nullptr) : (steps == nullptr || done != nullptr)) return UNETPP_EINVAL;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  with_variant(kind, ams, [&](auto v) {
    hipLaunchKernelGGL((optim_clip_kernel<decltype(v)::kind, decltype(v)::ams>), dim3(persistent_grid(n_chunks)),
                       dim3(kMtThreads), 0, st, segments, n_segments, chunk_segment, n_chunks, hyper, steps, done,
                       partials, state, skip);
    note_kernel(v.clip_label);
  });
  return launch_status();
}

extern "C" int unetpp_grad_scale(const unetpp_optim_segment* segments, int32_t n_segments, const int32_t* chunk_segment,
                                int64_t n_chunks, const double* partials, float max_norm, unetpp_clip_state* state,
                                void* stream) {
  if (!table_args_ok(segments, n_segments, chunk_segment, n_chunks) || partials == nullptr || state == nullptr)
    return UNETPP_EINVAL;
  if (!(max_norm > 0.f)) return UNETPP_EINVAL;
  hipLaunchKernelGGL(grad_scale_kernel, dim3(persistent_grid(n_chunks)), dim3(kMtThreads), 0,
                     static_cast<hipStream_t>(stream), segments, chunk_segment, n_chunks, partials, max_norm, state);
  note_kernel("grad_scale");
  return launch_status();
}

extern "C" int unetpp_optim_upload(void* dst, const void* host_src, int64_t bytes, void* stream) {
  if (dst == nullptr || host_src == nullptr || bytes <= 0) return UNETPP_EINVAL;
  return hipMemcpyAsync(dst, host_src, static_cast<size_t>(bytes), hipMemcpyHostToDevice,
                        static_cast<hipStream_t>(stream)) == hipSuccess ? UNETPP_OK : UNETPP_ELAUNCH;
}
