// Self-distillation across the deep-supervision heads (losses.HeadDistillLoss): FocalLoss_BCE_2d of every head against
// the target, plus the same element rule of every shallower head against a deeper head's map -- its teacher, read as data:
// no gradient reaches a head through its role as teacher.  For heads p_0 .. p_{J-1} (shallow to deep), target t, weight w:
//   teacher of head j < J-1:  the deepest head ("last") or head j + 1 ("next");  the deepest head has none;
//   S_j = sum l(p_j, t) / rows,   D_j = sum over the admitted elements of l(p_j, q) / rows  (q: the teacher's element),
//   L_j = S_j + w D_j (one rounded product, one rounded sum),  D_{J-1} = +0.0,
//   loss[0] = the mean over heads of L_j in the trainer's order (loss_heads.h),
//   grad_j = g_s + w g_d per admitted element (one rounded product, one rounded sum); g_s itself, with its bits, on an
//            element that is kept out of D_j and on every element of the deepest head.
// l, g_s and g_d are focal_element.h's rule (distill_element below) with the same inv_rows and scale = float32(1 / J);
// S_j and the supervised gradients are unetpp_focal_bce_heads' bits, D_j without gate and ignore rule is
// unetpp_focal_bce(p_j, q)'s.
// An element is admitted to D_j
//   gate:    where |q - t| < |p - t|, a float32 comparison of the absolute values of the two float32 differences (a NaN on
//            either side compares false and keeps the element out);
//   ignore:  an ignored element (t < 0.0f; S term and g_s are +0.0 as in unetpp_focal_bce_heads_ignore) passes the gate
//            and keeps its distillation term when distill_ignored is set, and is kept out when it is not.
// One main launch in the geometry of loss_heads.h: a thread reads its 8 targets once and walks the heads from the deepest
// to the shallowest with the teacher's 8 values in registers, so every map is read once and every gradient written once.
// Two partial sums per head and block (S, D), each formed as loss_heads.h has it and times inv_rows, then its finish per
// sum.  w is read from device memory, so a captured graph follows a schedule of w.
#include "common.h"
#include "loss_heads.h"

namespace unetpp {
namespace {

constexpr int kVecs = kLossVecs;

// a + w * b in two roundings.  Left to the compiler the pair becomes one fma, which is neither what float32 tensor
// arithmetic over the two stored gradients gives nor the S_j and D_j this call reports.
__device__ __forceinline__ float distill_combine(float a, float w, float b) {
#pragma clang fp contract(off)
  const float wb = w * b;
  return a + wb;
}

struct DistillFlags {
  int next;             // teacher: the head visited before this one (j + 1) instead of the deepest
  int gate;             // teacher_better
  int distill_ignored;  // kIgnore only: an ignored element keeps its distillation term
};

// One element of FocalLoss_BCE_2d with every rounding written out: focal_element.h's statements in their order, compiled
// without contraction, and the loss term handed out as its two factors.  The bits focal_element has in caller.hip are
// not those of a plain inlining here: there the vectoriser pairs u^(gamma-1) u with gamma u^(gamma-1) log e into one
// packed product, which leaves `gamma u^(gamma-1) log e - u^gamma / e` a rounded product and a rounded difference, and the
// only fused operation is `sum += le` (an fma of log e and u^gamma; with kLow, where le goes through a select, a plain sum).
// With two elements per pixel in one loop the vectoriser pairs other products, the backend fuses that difference for some
// elements and not for others, and the term reaches the sum through a select.  Written out, the bits do not depend on
// either: they are unetpp_focal_bce's and unetpp_focal_bce_heads' (tests/test_gpu_distill.py holds them against both).
template <bool kLow>
__device__ __forceinline__ void distill_element(float p, float t, float gamma, bool cube, float inv_rows, float scale,
                                                float& lg, float& ug, float& le, float& g) {
#pragma clang fp contract(off)
  const float d = p - t;
  const float err = (1.f - fabsf(d)) + 1e-20f;
  const float u = 1.f - err;
  lg = logf(err);
  const float ug1 = cube ? u * u : powf(u, gamma - 1.f);  // u^(gamma-1)
  ug = ug1 * u;
  le = -ug * lg;
  float dl_de = gamma * ug1 * lg - ug / err;
  if constexpr (kLow) {
    if (u == 0.f) {
      le = 0.f;
      dl_de = (gamma == 0.f) ? -1.f / err : 0.f;
    }
  }
  const float sgn = (d > 0.f) ? 1.f : ((d < 0.f) ? -1.f : 0.f);
  g = (-dl_de * sgn * inv_rows) * scale;
}

// sum += le as focal_thread (caller.hip) compiles it
template <bool kLow>
__device__ __forceinline__ float distill_add_term(float sum, float lg, float ug, float le) {
  if constexpr (kLow) {
    return sum + le;
  } else {
    return __builtin_fmaf(-lg, ug, sum);
  }
}

// One head of one thread.  kStudent: q holds the teacher's elements and sum_d receives the distillation terms.
template <bool kLow, bool kIgnore, bool kStudent>
__device__ __forceinline__ void distill_head(const float (&p)[kVecs][4], const float (&t)[kVecs][4],
                                             const float (&q)[kVecs][4], float* __restrict__ grad, long base, long n,
                                             float gamma, float inv_rows, float scale, float w, const DistillFlags f,
                                             float& sum_s, float& sum_d) {
#pragma clang fp contract(off)
  const bool cube = gamma == 3.f;
  sum_s = 0.f;
  sum_d = 0.f;
#pragma unroll
  for (int h = 0; h < kVecs; ++h) {
    const long i = base + 4 * h;
    if (i >= n) break;
    float g[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float lg, ug, le, gs;
      distill_element<kLow>(p[h][e], t[h][e], gamma, cube, inv_rows, scale, lg, ug, le, gs);
      const bool inside = i + e < n;
      bool take = inside;
      bool ignored = false;
      if constexpr (kIgnore) {
        if (t[h][e] < 0.f) ignored = true, take = false, gs = 0.f;
      }
      if (take) sum_s = distill_add_term<kLow>(sum_s, lg, ug, le);
      if constexpr (kStudent) {
        float gd;
        distill_element<kLow>(p[h][e], q[h][e], gamma, cube, inv_rows, scale, lg, ug, le, gd);
        bool admit = true;
        if (f.gate) admit = fabsf(q[h][e] - t[h][e]) < fabsf(p[h][e] - t[h][e]);
        if constexpr (kIgnore) {
          if (ignored) admit = f.distill_ignored != 0;
        }
        if (admit && inside) sum_d = distill_add_term<kLow>(sum_d, lg, ug, le);
        g[e] = admit ? distill_combine(gs, w, gd) : gs;   // kept out: the supervised gradient's own bits
      } else {
        g[e] = gs;
      }
    }
    store4(grad, i, n, g);
  }
}

template <bool kLow, bool kIgnore>
__global__ __launch_bounds__(kLossThreads) void distill_heads_kernel(const unetpp_focal_heads hd,
                                                                    const float* __restrict__ target, long n, float gamma,
                                                                    float inv_rows, float scale,
                                                                    const float* __restrict__ weight, const DistillFlags f,
                                                                    float* __restrict__ partial) {
  __shared__ float red[2][UNETPP_MAX_HEADS][kLossThreads / 64];
  const long base = (blockIdx.x * static_cast<long>(kLossThreads) + threadIdx.x) * kLossPerThread;
  const float w = weight[0];
  float t[kVecs][4], p[kVecs][4];
  float q[kVecs][4] = {};   // the teacher's elements (set by the deepest head before a student reads them)
  load_thread(target, base, n, t);
  const int last = hd.n_heads - 1;
  for (int h = last; h >= 0; --h) {
    load_thread(hd.pred[h], base, n, p);
    float sum_s, sum_d;
    if (h == last)
      distill_head<kLow, kIgnore, false>(p, t, q, hd.grad[h], base, n, gamma, inv_rows, scale, w, f, sum_s, sum_d);
    else
      distill_head<kLow, kIgnore, true>(p, t, q, hd.grad[h], base, n, gamma, inv_rows, scale, w, f, sum_s, sum_d);
    if (h == last || f.next) {
#pragma unroll
      for (int v = 0; v < kVecs; ++v)
#pragma unroll
        for (int e = 0; e < 4; ++e) q[v][e] = p[v][e];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      sum_s += __shfl_xor(sum_s, off);
      sum_d += __shfl_xor(sum_d, off);
    }
    if ((threadIdx.x & 63) == 0) {
      red[0][h][threadIdx.x >> 6] = sum_s;
      red[1][h][threadIdx.x >> 6] = sum_d;
    }
  }
  __syncthreads();
  if (static_cast<int>(threadIdx.x) < 2 * hd.n_heads) {
    const int h = threadIdx.x >> 1, k = threadIdx.x & 1;
    const float* r = red[k][h];
    partial[static_cast<long>(threadIdx.x) * gridDim.x + blockIdx.x] = ((r[0] + r[1]) + (r[2] + r[3])) * inv_rows;
  }
}

// one block: S_h and D_h summed, L_h = S_h + w D_h, then the mean over heads.
// loss: [0] the mean, [1 + h] L_h, [1 + H + h] S_h, [1 + 2 H + h] D_h.
__global__ __launch_bounds__(kFinishThreads) void distill_finish_kernel(const float* __restrict__ partial, long n_blocks,
                                                                        int n_heads, float inv_heads,
                                                                        const float* __restrict__ weight,
                                                                        float* __restrict__ loss) {
  __shared__ float red[kFinishThreads];
  const float w = weight[0];
  finish_heads(n_heads, inv_heads, loss, [&](int h) {
    const float s = finish_sum(partial + (2 * h) * n_blocks, n_blocks, red);
    const float d = finish_sum(partial + (2 * h + 1) * n_blocks, n_blocks, red);
    if (threadIdx.x == 0) {
      loss[1 + n_heads + h] = s;
      loss[1 + 2 * n_heads + h] = d;
    }
    return distill_combine(s, w, d);
  });
}

// ---------------------------------------------------------------------------------------------------------------------
// A teacher from outside (losses.TeacherDistillLoss, unetpp_teacher_heads): every head, the deepest included, is held
// against the target and against ONE external map q of the target's shape (another network's output, a stitched scene
// map), read as data.  The element functions, the two combinations and the finish are the ones above, so S_h, D_h, L_h
// and the mean are formed exactly as unetpp_distill_heads forms them, and with the deepest head's own map as q heads
// 0 .. J-2 have unetpp_distill_heads(teacher = last)'s bits.  What is new is the void rule: an element with q < 0.0f
// has no teacher (-0.0 and a NaN are not negative: a NaN teacher element is admitted and reaches the loss, as t < 0
// hides nothing either), so the -1 that fills a window outside its frame keeps the term out there.  A thread keeps its
// 8 targets and its 8 teacher values in registers and walks the heads: 2 + 2 J map-sized streams for J heads.
struct TeacherFlags {
  int gate;             // teacher_better
  int distill_ignored;  // kIgnore only: an ignored element keeps its distillation term
};

template <bool kLow, bool kIgnore>
__device__ __forceinline__ void teacher_head(const float (&p)[kVecs][4], const float (&t)[kVecs][4],
                                             const float (&q)[kVecs][4], float* __restrict__ grad, long base, long n,
                                             float gamma, float inv_rows, float scale, float w, const TeacherFlags f,
                                             float& sum_s, float& sum_d) {
#pragma clang fp contract(off)
  const bool cube = gamma == 3.f;
  sum_s = 0.f;
  sum_d = 0.f;
#pragma unroll
  for (int h = 0; h < kVecs; ++h) {
    const long i = base + 4 * h;
    if (i >= n) break;
    float g[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float lg, ug, le, gs, gd;
      distill_element<kLow>(p[h][e], t[h][e], gamma, cube, inv_rows, scale, lg, ug, le, gs);
      const bool inside = i + e < n;
      bool take = inside;
      bool ignored = false;
      if constexpr (kIgnore) {
        if (t[h][e] < 0.f) ignored = true, take = false, gs = 0.f;
      }
      if (take) sum_s = distill_add_term<kLow>(sum_s, lg, ug, le);
      distill_element<kLow>(p[h][e], q[h][e], gamma, cube, inv_rows, scale, lg, ug, le, gd);
      bool admit = true;
      if (f.gate) admit = fabsf(q[h][e] - t[h][e]) < fabsf(p[h][e] - t[h][e]);
      if constexpr (kIgnore) {
        if (ignored) admit = f.distill_ignored != 0;
      }
      if (q[h][e] < 0.f) admit = false;   // void: no teacher here
      if (admit && inside) sum_d = distill_add_term<kLow>(sum_d, lg, ug, le);
      // kept out: the supervised gradient's own bits.  The same where w g_d is a zero (w = 0, an exact hit of the
      // teacher): g_s + 0 is g_s but for g_s = -0.0 at an exact hit of the target, which a sum with +0.0 would turn into
      // +0.0 -- and weight 0 is unetpp_focal_bce_heads bit for bit.  A NaN product is not a zero and goes through.
      g[e] = (admit && w * gd != 0.f) ? distill_combine(gs, w, gd) : gs;
    }
    store4(grad, i, n, g);
  }
}

template <bool kLow, bool kIgnore>
__global__ __launch_bounds__(kLossThreads) void teacher_heads_kernel(const unetpp_focal_heads hd,
                                                                    const float* __restrict__ target,
                                                                    const float* __restrict__ teacher, long n, float gamma,
                                                                    float inv_rows, float scale,
                                                                    const float* __restrict__ weight, const TeacherFlags f,
                                                                    float* __restrict__ partial) {
  __shared__ float red[2][UNETPP_MAX_HEADS][kLossThreads / 64];
  const long base = (blockIdx.x * static_cast<long>(kLossThreads) + threadIdx.x) * kLossPerThread;
  const float w = weight[0];
  float t[kVecs][4], q[kVecs][4], p[kVecs][4];
  load_thread(target, base, n, t);
  load_thread(teacher, base, n, q);
  for (int h = 0; h < hd.n_heads; ++h) {
    load_thread(hd.pred[h], base, n, p);
    float sum_s, sum_d;
    teacher_head<kLow, kIgnore>(p, t, q, hd.grad[h], base, n, gamma, inv_rows, scale, w, f, sum_s, sum_d);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      sum_s += __shfl_xor(sum_s, off);
      sum_d += __shfl_xor(sum_d, off);
    }
    if ((threadIdx.x & 63) == 0) {
      red[0][h][threadIdx.x >> 6] = sum_s;
      red[1][h][threadIdx.x >> 6] = sum_d;
    }
  }
  __syncthreads();
  if (static_cast<int>(threadIdx.x) < 2 * hd.n_heads) {
    const int h = threadIdx.x >> 1, k = threadIdx.x & 1;
    const float* r = red[k][h];
    partial[static_cast<long>(threadIdx.x) * gridDim.x + blockIdx.x] = ((r[0] + r[1]) + (r[2] + r[3])) * inv_rows;
  }
}

}  // namespace
}  // namespace unetpp

using namespace unetpp;

extern "C" int unetpp_teacher_heads(const unetpp_focal_heads* heads, const float* target, const float* teacher, int64_t n,
                                    int64_t rows, float gamma, const float* weight, int32_t gate, int32_t ignore,
                                    int32_t distill_ignored, float* partial, float* loss, void* stream) {
  unetpp_focal_heads hd;
  if (loss_heads_checked(heads, target, hd) != UNETPP_OK) return UNETPP_EINVAL;
  if (teacher == nullptr || weight == nullptr || partial == nullptr || loss == nullptr || n < 1 || rows < 1)
    return UNETPP_EINVAL;
  if ((gate != 0 && gate != 1) || (ignore != 0 && ignore != 1) || (distill_ignored != 0 && distill_ignored != 1))
    return UNETPP_EINVAL;
  if (!(gamma >= 0.f)) return UNETPP_EINVAL;
  if ((reinterpret_cast<uintptr_t>(teacher) & 15) != 0 || (reinterpret_cast<uintptr_t>(weight) & 3) != 0)
    return UNETPP_EINVAL;
  const int64_t blocks = loss_blocks(n);
  if (blocks > 0x7fffffffLL) return UNETPP_EINVAL;
  const float inv_heads = 1.0f / static_cast<float>(hd.n_heads);
  TeacherFlags f;
  f.gate = gate;
  f.distill_ignored = distill_ignored;
  const bool low = gamma < 1.f;
  const auto kernel = ignore ? (low ? teacher_heads_kernel<true, true> : teacher_heads_kernel<false, true>)
                             : (low ? teacher_heads_kernel<true, false> : teacher_heads_kernel<false, false>);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(blocks)), dim3(kLossThreads), 0, st, hd, target, teacher,
                     static_cast<long>(n), gamma, 1.f / static_cast<float>(rows), inv_heads, weight, f, partial);
  hipLaunchKernelGGL(distill_finish_kernel, dim3(1), dim3(kFinishThreads), 0, st, static_cast<const float*>(partial),
                     static_cast<long>(blocks), hd.n_heads, inv_heads, weight, loss);
  return launch_status();
}

extern "C" int unetpp_distill_heads(const unetpp_focal_heads* heads, const float* target, int64_t n, int64_t rows, float gamma,
                                    const float* weight, int32_t teacher, int32_t gate, int32_t ignore,
                                    int32_t distill_ignored, float* partial, float* loss, void* stream) {
  unetpp_focal_heads hd;
  if (loss_heads_checked(heads, target, hd) != UNETPP_OK) return UNETPP_EINVAL;
  if (weight == nullptr || partial == nullptr || loss == nullptr || n < 1 || rows < 1) return UNETPP_EINVAL;
  if ((teacher != UNETPP_DISTILL_LAST && teacher != UNETPP_DISTILL_NEXT) || (gate != 0 && gate != 1) ||
      (ignore != 0 && ignore != 1) || (distill_ignored != 0 && distill_ignored != 1))
    return UNETPP_EINVAL;
  if (!(gamma >= 0.f)) return UNETPP_EINVAL;
  if ((reinterpret_cast<uintptr_t>(weight) & 3) != 0) return UNETPP_EINVAL;
  const int64_t blocks = loss_blocks(n);
  if (blocks > 0x7fffffffLL) return UNETPP_EINVAL;
  const float inv_heads = 1.0f / static_cast<float>(hd.n_heads);
  DistillFlags f;
  f.next = teacher == UNETPP_DISTILL_NEXT;
  f.gate = gate;
  f.distill_ignored = distill_ignored;
  const bool low = gamma < 1.f;
  const auto kernel = ignore ? (low ? distill_heads_kernel<true, true> : distill_heads_kernel<false, true>)
                             : (low ? distill_heads_kernel<true, false> : distill_heads_kernel<false, false>);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(blocks)), dim3(kLossThreads), 0, st, hd, target, static_cast<long>(n),
                     gamma, 1.f / static_cast<float>(rows), inv_heads, weight, f, partial);
  hipLaunchKernelGGL(distill_finish_kernel, dim3(1), dim3(kFinishThreads), 0, st, static_cast<const float*>(partial),
                     static_cast<long>(blocks), hd.n_heads, inv_heads, weight, loss);
  return launch_status();
}
