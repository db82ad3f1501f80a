// Penalty-reduced focal loss (CornerNet / CenterNet), normalised by the number of positives, every deep-supervision
// head against one target in one call.  The rule, element by element over n float32 values of a head p (a sigmoid
// output, in [0, 1]) and the target t (domain [0, 1]); alpha >= 0, beta >= 0, eps in (0, 0.5), positive in (0, 1],
// all float32:
//   lo = float32(eps), hi = float32(1) - lo (one float32 subtraction);  q = min(max(p, lo), hi), a NaN stays a NaN;
//   the gradient passes where lo <= p <= hi (torch.clamp's rule) and is exactly +0.0 elsewhere;
//   an element is positive when t >= positive:
//     positive:   l = -(1 - q)^alpha log(q)
//     otherwise:  l = -(1 - t)^beta q^alpha log(1 - q),   log(1 - q) evaluated as log1pf(-q);
//   0^0 = 1;  n_pos = the positive elements of the target (an exact integer), denom = max(n_pos, 1);
//   loss_h = (sum of l over head h) * (1 / denom),  1 / denom = float32(1) / float32(denom);
//   loss[0] = the mean over heads of loss_h in the trainer's order (loss_heads.h);
//   grad_h = ((dl / dq) * (1 / denom)) * (1 / n_heads): the two float32 products in autograd's order.
// A NaN in p makes the loss NaN (its own gradient element is 0: the gate compares false).  eps below 2^-25 makes hi = 1,
// and the rule itself is then infinite at p = 1.
//
// Three launches, no host synchronisation, no atomics, the same bits on every run:
//   count   reads the target once: at most kPrCountBlocks workgroups, each over chunks of kPrCountChunk elements
//           (kPrCountLoads float4 loads in flight per lane) at a stride of the whole grid -> counts[block], 64-bit
//           integers.  Integer sums are exact in any order.
//   main    the geometry and partial sums of loss_heads.h: the thread's targets are read once for all heads, their
//           weights (1 - t)^beta formed once; every WAVE adds the count partials itself (at most four per lane, then six
//           shuffles), so 1 / denom is known before the first gradient is written and no launch stands between count
//           and main.  Every pred[h] is read once, every grad[h] written once.  Workgroup 0 writes n_pos.
//   finish  loss_heads.h's, a head's sum times 1 / denom (formed from the counts as the main pass forms it).
// alpha and beta in {0, 1, 2, 3, 4} take multiply chains instead of powf.
#include "common.h"
#include "loss_heads.h"

#include <cmath>

namespace unetpp {
namespace {

constexpr int kPrThreads = 256;
constexpr int kPrPerThread = 8;       // main pass: elements per thread, 2 x float4 per tensor
static_assert(kPrThreads == kLossThreads && kPrPerThread == kLossPerThread, "the main pass runs in loss_heads.h's geometry");
constexpr int kPrCountLoads = 4;      // count pass: float4 loads a lane issues before it looks at the first
constexpr int kPrCountChunk = kPrThreads * kPrCountLoads * 4;   // elements of one workgroup trip
constexpr int kPrCountBlocks = 256;   // count partials at most: four per lane of a wave of the main pass
constexpr int kPrGeneral = -1;        // exponent mode: powf

struct PrParams {
  float alpha, beta, lo, hi, positive;
  int amode, bmode;   // alpha / beta when it is 0, 1, 2, 3 or 4 exactly, else kPrGeneral
};

typedef unsigned long long pr_count_t;

// x^e for the weight (1 - t)^beta
__device__ __forceinline__ float pr_pow(float x, int mode, float e) {
  switch (mode) {
    case 0: return 1.f;
    case 1: return x;
    case 2: return x * x;
    case 3: return (x * x) * x;
    case 4: {
      const float s = x * x;
      return s * s;
    }
    default: return powf(x, e);
  }
}

// xe = x^e and xm1 = x^(e-1) for x > 0.  e == 0: xm1 is only ever multiplied by e, so 0 stands for it.
__device__ __forceinline__ void pr_pow_pair(float x, int mode, float e, float& xm1, float& xe) {
  switch (mode) {
    case 0: xm1 = 0.f; xe = 1.f; break;
    case 1: xm1 = 1.f; xe = x; break;
    case 2: xm1 = x; xe = x * x; break;
    case 3: xm1 = x * x; xe = xm1 * x; break;
    case 4: xm1 = (x * x) * x; xe = xm1 * x; break;
    default: xe = powf(x, e); xm1 = xe / x; break;
  }
}

// One element -> its loss term; g = ((dl/dq) * inv_denom) * scale where the clamp passes the gradient, +0.0 elsewhere.
// w: (1 - t)^beta of a negative, 1 of a positive.
__device__ __forceinline__ float pr_element(float p, float w, bool pos, const PrParams& k, float inv_denom, float scale,
                                            float& g) {
  const float q = (p < k.lo) ? k.lo : ((p > k.hi) ? k.hi : p);   // (a NaN fails both tests and stays)
  const bool open = (p >= k.lo) && (p <= k.hi);
  const float omq = 1.f - q;
  float lg;
  if (pos) {
    lg = logf(q);
  } else {
    lg = log1pf(-q);
  }
  const float a = pos ? omq : q;    // the base of the alpha power
  const float b = pos ? q : omq;    // the argument of the logarithm
  float a1, aa;
  pr_pow_pair(a, k.amode, k.alpha, a1, aa);
  const float wa = w * aa;
  const float mag = wa / b - (k.alpha * (w * a1)) * lg;   // |dl/dq|: both terms are >= 0
  const float dq = pos ? -mag : mag;
  g = open ? (dq * inv_denom) * scale : 0.f;
  return -wa * lg;
}

// the sum of the count partials, in every lane of the calling wave (n_counts <= kPrCountBlocks = 4 * 64)
__device__ __forceinline__ pr_count_t pr_total(const pr_count_t* __restrict__ counts, int n_counts) {
  const int lane = threadIdx.x & 63;
  pr_count_t c = 0;
#pragma unroll
  for (int j = 0; j < kPrCountBlocks / 64; ++j) {
    const int i = lane + 64 * j;
    c += (i < n_counts) ? counts[i] : 0ull;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off);
  return c;
}

__device__ __forceinline__ float pr_inv_denom(pr_count_t total) {
  return 1.f / static_cast<float>(total > 0 ? total : 1ull);
}

// counts[block] = the elements t >= positive of the block's chunks (a padded element is 0 and positive > 0)
__global__ __launch_bounds__(kPrThreads) void pr_count_kernel(const float* __restrict__ target, long n, float positive,
                                                              pr_count_t* __restrict__ counts) {
  __shared__ pr_count_t red[kPrThreads / 64];
  const long stride = static_cast<long>(gridDim.x) * kPrCountChunk;
  pr_count_t c = 0;
#pragma unroll 1
  for (long start = static_cast<long>(blockIdx.x) * kPrCountChunk; start < n; start += stride) {
    float v[kPrCountLoads][4];
#pragma unroll
    for (int a = 0; a < kPrCountLoads; ++a)
      load4(target, start + (static_cast<long>(a) * kPrThreads + threadIdx.x) * 4, n, 0.f, v[a]);
    unsigned here = 0;
#pragma unroll
    for (int a = 0; a < kPrCountLoads; ++a)
#pragma unroll
      for (int e = 0; e < 4; ++e) here += (v[a][e] >= positive) ? 1u : 0u;
    c += here;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// kIgnore: an element with a negative target (t < 0.0f: -0.0 and a NaN are not) is ignored -- its term and its gradient
// are +0.0 whatever pred holds (the term is left out by the condition of the addition, so that `sum += le` contracts as
// in the plain instantiation); every other element runs pr_element unchanged.  Such a target is never >= positive, so the
// count pass and n_pos are those of the plain call.
template <bool kIgnore = false>
__global__ __launch_bounds__(kPrThreads) void pr_focal_kernel(const unetpp_focal_heads hd, const float* __restrict__ target,
                                                              long n, const PrParams k, float scale,
                                                              const pr_count_t* __restrict__ counts, int n_counts,
                                                              float* __restrict__ partial, long long* __restrict__ n_pos) {
  __shared__ float red[UNETPP_MAX_HEADS][kPrThreads / 64];
  const long base = (blockIdx.x * static_cast<long>(kPrThreads) + threadIdx.x) * kPrPerThread;
  float w[kPrPerThread / 4][4];
  unsigned pos = 0;   // bit 4 * v + e: the element is positive
  [[maybe_unused]] unsigned ign = 0;   // bit 4 * v + e: the element is ignored (kIgnore)
  float t[kPrPerThread / 4][4];
#pragma unroll
  for (int v = 0; v < kPrPerThread / 4; ++v) load4(target, base + 4 * v, n, 0.f, t[v]);
  const pr_count_t total = pr_total(counts, n_counts);   // (its loads are in flight beside the target's)
  if (blockIdx.x == 0 && threadIdx.x == 0) *n_pos = static_cast<long long>(total);
#pragma unroll
  for (int v = 0; v < kPrPerThread / 4; ++v)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool is_pos = t[v][e] >= k.positive;
      pos |= is_pos ? (1u << (4 * v + e)) : 0u;
      if constexpr (kIgnore) ign |= (t[v][e] < 0.f) ? (1u << (4 * v + e)) : 0u;
      w[v][e] = is_pos ? 1.f : pr_pow(1.f - t[v][e], k.bmode, k.beta);
    }
  const float inv_denom = pr_inv_denom(total);
  for (int h = 0; h < hd.n_heads; ++h) {
    const float* __restrict__ pred = hd.pred[h];
    float* __restrict__ grad = hd.grad[h];
    float p[kPrPerThread / 4][4];
#pragma unroll
    for (int v = 0; v < kPrPerThread / 4; ++v) load4(pred, base + 4 * v, n, 0.5f, p[v]);   // both loads first
    float sum = 0.f;
#pragma unroll
    for (int v = 0; v < kPrPerThread / 4; ++v) {
      const long i = base + 4 * v;
      float g[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float le = pr_element(p[v][e], w[v][e], (pos >> (4 * v + e)) & 1u, k, inv_denom, scale, g[e]);
        bool take = i + e < n;
        if constexpr (kIgnore) {
          if ((ign >> (4 * v + e)) & 1u) take = false, g[e] = 0.f;
        }
        if (take) sum += le;
      }
      if (grad != nullptr) {
        if (i + 4 <= n) {
          *reinterpret_cast<f32x4*>(grad + i) = f32x4{g[0], g[1], g[2], g[3]};
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (i + e < n) grad[i + e] = g[e];
        }
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
    if ((threadIdx.x & 63) == 0) red[h][threadIdx.x >> 6] = sum;
  }
  __syncthreads();
  if (static_cast<int>(threadIdx.x) < hd.n_heads) {
    const float* r = red[threadIdx.x];
    partial[static_cast<long>(threadIdx.x) * gridDim.x + blockIdx.x] = (r[0] + r[1]) + (r[2] + r[3]);
  }
}

// one block: every head's sum times 1 / denom, then the mean over heads
__global__ __launch_bounds__(kFinishThreads) void pr_focal_finish_kernel(const float* __restrict__ partial, long n_blocks,
                                                                         int n_heads, float inv_heads,
                                                                         const pr_count_t* __restrict__ counts, int n_counts,
                                                                         float* __restrict__ loss) {
  // (no contraction: fused into the addition to avg, the product with 1 / denom would not be rounded, and the mean
  // would not be the sum of the values written to loss[1 + h], which is what the loop over single-head calls adds)
#pragma clang fp contract(off)
  __shared__ float red[kFinishThreads];
  const float inv_denom = pr_inv_denom(pr_total(counts, n_counts));
  finish_heads(n_heads, inv_heads, loss,
               [&](int h) { return finish_sum(partial + h * n_blocks, n_blocks, red) * inv_denom; });
}

inline int pr_mode(float e) {
  for (int m = 0; m <= 4; ++m)
    if (e == static_cast<float>(m)) return m;
  return kPrGeneral;
}

inline bool pr_args_ok(int32_t n_heads, int64_t n) {
  return n_heads >= 1 && n_heads <= UNETPP_MAX_HEADS && n >= 1 && loss_blocks(n) <= 0x7fffffffLL;
}

}  // namespace
}  // namespace unetpp

using namespace unetpp;

extern "C" int64_t unetpp_pr_focal_workspace_bytes(int32_t n_heads, int64_t n) {
  if (!pr_args_ok(n_heads, n)) return 0;
  return static_cast<int64_t>(kPrCountBlocks) * static_cast<int64_t>(sizeof(pr_count_t)) +
         static_cast<int64_t>(n_heads) * loss_blocks(n) * 4;
}

namespace {

template <bool kIgnore>
int pr_focal_heads_launch(const unetpp_focal_heads* heads, const float* target, int64_t n, float alpha, float beta, float eps,
                          float positive, void* workspace, int64_t* n_pos, float* loss, void* stream) {
  unetpp_focal_heads hd;
  if (loss_heads_checked(heads, target, hd) != UNETPP_OK) return UNETPP_EINVAL;
  if (workspace == nullptr || n_pos == nullptr || loss == nullptr || !pr_args_ok(hd.n_heads, n)) return UNETPP_EINVAL;
  if (!(alpha >= 0.f) || !(beta >= 0.f) || !(eps > 0.f && eps < 0.5f) || !(positive > 0.f && positive <= 1.f))
    return UNETPP_EINVAL;   // (a NaN fails every comparison)
  if (((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(n_pos)) & 7) != 0) return UNETPP_EINVAL;
  PrParams k;
  k.alpha = alpha;
  k.beta = beta;
  k.lo = eps;
  k.hi = 1.0f - eps;
  k.positive = positive;
  k.amode = pr_mode(alpha);
  k.bmode = pr_mode(beta);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t blocks = loss_blocks(n);
  const int64_t chunks = (n - 1) / kPrCountChunk + 1;
  const int n_counts = static_cast<int>(chunks < kPrCountBlocks ? chunks : kPrCountBlocks);
  pr_count_t* counts = static_cast<pr_count_t*>(workspace);
  float* partial = reinterpret_cast<float*>(counts + kPrCountBlocks);
  const float inv_heads = 1.0f / static_cast<float>(hd.n_heads);
  hipLaunchKernelGGL(pr_count_kernel, dim3(static_cast<unsigned>(n_counts)), dim3(kPrThreads), 0, st, target,
                     static_cast<long>(n), positive, counts);
  hipLaunchKernelGGL(pr_focal_kernel<kIgnore>, dim3(static_cast<unsigned>(blocks)), dim3(kPrThreads), 0, st, hd, target,
                     static_cast<long>(n), k, inv_heads, static_cast<const pr_count_t*>(counts), n_counts, partial,
                     reinterpret_cast<long long*>(n_pos));
  hipLaunchKernelGGL(pr_focal_finish_kernel, dim3(1), dim3(kFinishThreads), 0, st, static_cast<const float*>(partial),
                     static_cast<long>(blocks), hd.n_heads, inv_heads, static_cast<const pr_count_t*>(counts), n_counts, loss);
  return launch_status();
}

}  // namespace

extern "C" int unetpp_pr_focal_heads(const unetpp_focal_heads* heads, const float* target, int64_t n, float alpha, float beta,
                                     float eps, float positive, void* workspace, int64_t* n_pos, float* loss, void* stream) {
  return pr_focal_heads_launch<false>(heads, target, n, alpha, beta, eps, positive, workspace, n_pos, loss, stream);
}

extern "C" int unetpp_pr_focal_heads_ignore(const unetpp_focal_heads* heads, const float* target, int64_t n, float alpha,
                                            float beta, float eps, float positive, void* workspace, int64_t* n_pos,
                                            float* loss, void* stream) {
  return pr_focal_heads_launch<true>(heads, target, n, alpha, beta, eps, positive, workspace, n_pos, loss, stream);
}
