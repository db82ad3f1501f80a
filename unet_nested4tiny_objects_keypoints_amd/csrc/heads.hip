// The deep-supervision heads, fp32 and bf16 storage side by side: dropout + 1x1 convolution + sigmoid forward
// (unetpp_head_fwd[_bf16]), the ensemble mean of several heads (unetpp_heads_mean_fwd[_bf16], no dropout), its backward
// (unetpp_heads_mean_bwd[_bf16]: the head maps are recomputed, never read) and the backward of one head
// (unetpp_head_bwd[_bf16]: feature gradient, per-workgroup partial rows of dW and db); fp32 only: one head of a training
// step in one pass (unetpp_head_train) and Monte-Carlo dropout at one head (unetpp_head_mc).  Features are NHWC,
// probabilities fp32 NCHW (the loss stays fp32).  head_select (head_select.h) decides which kernel takes a call; the
// launchers at the end check pointers, ask it and launch.
#include "bf16_common.h"
#include "common.h"
#include "lds_asm.h"
#include "dropout.h"
#include "focal_element.h"
#include "heads_mean.h"
#include "head_select.h"
#include "head_mc_select.h"

#include <type_traits>

namespace unetpp {
namespace {

static_assert(kHeadThreads == kThreads, "head_select sizes its grids for kThreads threads per workgroup");

// ------------------------------------------------------------------ fp32 storage
__global__ __launch_bounds__(kThreads) void head_fwd_kernel(const float* __restrict__ x, const float* __restrict__ weight,
                                                            const float* __restrict__ bias, long pixels, int HW, int C,
                                                            int n_cls, float keep_scale, uint32_t thr16, uint64_t seed,
                                                            const uint8_t* __restrict__ mask, const uint64_t* __restrict__ seed_dev, int use_drop,
                                                            float* __restrict__ out) {
  if (seed_dev != nullptr) seed += *seed_dev;  // graph-captured steps: the varying part of the seed lives in device memory
  __shared__ float wsm[kHeadMaxCls * kHeadMaxC];
  for (int i = threadIdx.x; i < n_cls * C; i += kThreads) wsm[i] = weight[i];
  __syncthreads();
  const int g4n = (C + 3) >> 2;
  for (long p = blockIdx.x * static_cast<long>(kThreads) + threadIdx.x; p < pixels;
       p += static_cast<long>(gridDim.x) * kThreads) {
    float acc[kHeadMaxCls];
#pragma unroll
    for (int k = 0; k < kHeadMaxCls; ++k) acc[k] = (k < n_cls) ? bias[k] : 0.f;
    const float* xp = x + p * C;
    for (int g = 0; g < g4n; ++g) {
      const uint64_t bits = (use_drop && mask == nullptr) ? keep_bits(seed, p, g4n, g) : 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = 4 * g + q;
        if (c < C) {
          float v = xp[c];
          if (use_drop) {
            const bool keep = (mask != nullptr) ? (mask[p * C + c] != 0) : keep_one(bits, q, thr16);
            v = keep ? v * keep_scale : 0.f;
          }
#pragma unroll
          for (int k = 0; k < kHeadMaxCls; ++k)
            if (k < n_cls) acc[k] += v * wsm[k * C + c];
        }
      }
    }
    const long n = p / HW, hw = p - n * HW;
#pragma unroll
    for (int k = 0; k < kHeadMaxCls; ++k)
      if (k < n_cls) out[(n * n_cls + k) * HW + hw] = 1.0f / (1.0f + expf(-acc[k]));
  }
}

// Forward head, coalesced: one wave per workgroup stages 64 pixels x C channels through LDS with full-line
// 16-byte loads (dropout applied on the way in), then lane = pixel reads its row (stride C+1: conflict-free)
// and the class weights come through scalar loads (uniform index).  Output is NCHW, coalesced along pixels.
__global__ __launch_bounds__(64) void head_fwd_tiled_kernel(const float* __restrict__ x, const float* __restrict__ weight,
                                                            const float* __restrict__ bias, long pixels, int HW, int C,
                                                            int n_cls, float keep_scale, uint32_t thr16, uint64_t seed,
                                                            const uint8_t* __restrict__ mask, const uint64_t* __restrict__ seed_dev, int use_drop,
                                                            float* __restrict__ out) {
  if (seed_dev != nullptr) seed += *seed_dev;  // graph-captured steps: the varying part of the seed lives in device memory
  extern __shared__ __attribute__((aligned(16))) float xs[];  // 64 * (C + 1) floats (sized by the launcher)
  const int lane = threadIdx.x;
  const int XS = C + 1, g4n = C >> 2;  // launcher guarantees C % 4 == 0
  const long n_tiles = (pixels + 63) / 64;
  for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long p0 = tile * 64;
    __syncthreads();
    for (int it = lane; it < 64 * g4n; it += 64) {
      const int pl = it / g4n, gq = it - pl * g4n;
      const long p = p0 + pl;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (p < pixels) {
        v = *reinterpret_cast<const f32x4*>(x + p * C + 4 * gq);
        if (use_drop) {
          const uint64_t bits = (mask == nullptr) ? keep_bits(seed, p, g4n, gq) : 0;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const bool keep = (mask != nullptr) ? (mask[p * C + 4 * gq + q] != 0) : keep_one(bits, q, thr16);
            v[q] = keep ? v[q] * keep_scale : 0.f;
          }
        }
      }
      float* dst = &xs[pl * XS + 4 * gq];
      dst[0] = v[0];
      dst[1] = v[1];
      dst[2] = v[2];
      dst[3] = v[3];
    }
    __syncthreads();
    const long p = p0 + lane;
    float acc[kHeadMaxCls];
#pragma unroll
    for (int k = 0; k < kHeadMaxCls; ++k) acc[k] = (k < n_cls) ? bias[k] : 0.f;
    for (int c = 0; c < C; ++c) {
      const float v = xs[lane * XS + c];
#pragma unroll
      for (int k = 0; k < kHeadMaxCls; ++k)
        if (k < n_cls) acc[k] += v * weight[k * C + c];
    }
    if (p < pixels) {
      const long n = p / HW, hw = p - n * HW;
#pragma unroll
      for (int k = 0; k < kHeadMaxCls; ++k)
        if (k < n_cls) out[(n * n_cls + k) * HW + hw] = 1.0f / (1.0f + expf(-acc[k]));
    }
  }
}

// One pixel's logits in the streaming layout (lane = (pixel, channel quad), G = 2^LOG2G lanes per pixel): the P per-class
// partial dot products of the lane's quad, summed over the pixel's lanes by a reduce-scatter in a fixed order.  Returns
// the total (without the bias) of class `cls`, the one this lane ends up with; G / P lanes (at least one) hold each class.
// Shared by head_fwd_stream_kernel and heads_mean_stream_kernel: both produce the same bits for the same operands.
template <int LOG2G, int P>
__device__ __forceinline__ float head_pixel_logit(const f32x4& v, const f32x4 (&wq)[P], int gq, int& cls) {
  constexpr int G = 1 << LOG2G;
  float acc[P];
#pragma unroll
  for (int k = 0; k < P; ++k)
    acc[k] = fmaf(v[0], wq[k][0], fmaf(v[1], wq[k][1], fmaf(v[2], wq[k][2], v[3] * wq[k][3])));
  // reduce-scatter over the G lanes of the pixel: with `live` classes left, a lane keeps the half selected by its
  // bit `off` and adds the partner's partials of that half; once one class is left, a plain butterfly sum
  int c = 0;
  static_for<LOG2G>([&](auto sc) {
    constexpr int step = decltype(sc)::v, off = G >> (1 + step);
    constexpr int live = (P >> step) > 1 ? (P >> step) : 1;  // classes a lane still carries before this step
    if constexpr (live > 1) {
      constexpr int half = live >> 1;
      const bool upper = (gq & off) != 0;
#pragma unroll
      for (int i = 0; i < half; ++i) {
        const float send = upper ? acc[i] : acc[half + i];
        const float keep = upper ? acc[half + i] : acc[i];
        acc[i] = keep + xor_lane<off>(send);
      }
      c += upper ? half : 0;
    } else {
      acc[0] += xor_lane<off>(acc[0]);
    }
  });
  cls = c;
  return acc[0];
}

// Forward head, streaming form for power-of-two channel-quad counts (C = 4 .. 128): lane = (pixel, channel quad), one
// coalesced 16-byte load per item, the class weights of the quad in registers.  The P per-class partial dot products
// of a lane are summed over the C/4 lanes of the pixel by a reduce-scatter (each exchange step halves the classes a
// lane still carries: P-1 + log2(G/P) shuffles instead of P log2 G), fixed order.  No LDS tile, no transposition.
// DROP: 0 = no dropout, 1 = keep flags from the counter hash, 2 = keep flags from a mask tensor -- three instantiations so
// that the loop body is straight-line code (as one kernel it carried ~16 uniform branches per item).  32-bit element
// offsets (the launcher takes this path for tensors below 2^31 elements); C = 4 G, so pixel -> element offset and
// pixel -> hash counter are shifts; the (image, position) pair of the NCHW output is carried along instead of divided
// out per item.
template <int LOG2G, int P, int DROP>  // P = classes padded to a power of two (4 or 8), P <= G
__global__ __launch_bounds__(kThreads) void head_fwd_stream_kernel(const float* __restrict__ x, const float* __restrict__ weight,
                                                                   const float* __restrict__ bias, unsigned pixels, unsigned HW,
                                                                   int n_cls, float keep_scale, uint32_t thr16, uint64_t seed,
                                                                   const uint8_t* __restrict__ mask, const uint64_t* __restrict__ seed_dev, float* __restrict__ out) {
  if (seed_dev != nullptr) seed += *seed_dev;  // graph-captured steps: the varying part of the seed lives in device memory
  constexpr int G = 1 << LOG2G;  // lanes (channel quads) per pixel
  const int gq = threadIdx.x & (G - 1);
  f32x4 wq[P];
#pragma unroll
  for (int k = 0; k < P; ++k)
    wq[k] = (k < n_cls) ? *reinterpret_cast<const f32x4*>(weight + k * 4 * G + 4 * gq) : f32x4{0.f, 0.f, 0.f, 0.f};
  constexpr unsigned ppb = kThreads >> LOG2G;  // pixels per block and slot
  constexpr int U = 4;                         // pixels per thread and iteration: 4 loads in flight
  const unsigned span = gridDim.x * ppb, outer = U * span;
  const unsigned pl = threadIdx.x >> LOG2G;
  // (image, position) of this thread's first pixel and the step of one `span`, kept up to date by adds
  const unsigned span_n = span / HW, span_hw = span - span_n * HW;
  unsigned p0 = blockIdx.x * ppb + pl;
  unsigned n0 = p0 / HW, hw0 = p0 - n0 * HW;
  for (; p0 - pl < pixels; p0 += outer) {  // wave-uniform trip count
    f32x4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const unsigned p = p0 + u * span;
      v[u] = (p < pixels) ? *reinterpret_cast<const f32x4*>(x + ((p << (LOG2G + 2)) + 4 * gq)) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const unsigned p = p0 + u * span;
      const bool valid = p < pixels;
      if constexpr (DROP == 1) {
        const uint64_t bits = keep_bits(seed, p, G, gq);
#pragma unroll
        for (int q = 0; q < 4; ++q) v[u][q] = keep_one(bits, q, thr16) ? v[u][q] * keep_scale : 0.f;
      } else if constexpr (DROP == 2) {
        const uint32_t m4 = valid ? *reinterpret_cast<const uint32_t*>(mask + ((p << (LOG2G + 2)) + 4 * gq)) : 0u;
#pragma unroll
        for (int q = 0; q < 4; ++q) v[u][q] = ((m4 >> (8 * q)) & 0xffu) != 0 ? v[u][q] * keep_scale : 0.f;
      }
      int cls;  // class this lane ends up with
      const float logit = head_pixel_logit<LOG2G, P>(v[u], wq, gq, cls);
      // this item's (image, position): u steps of `span` from the thread's first pixel of the iteration
      unsigned n = n0 + u * span_n, hw = hw0 + u * span_hw;
#pragma unroll
      for (int c = 0; c < U - 1; ++c) {  // at most u carries
        const bool carry = c < u && hw >= HW;
        hw -= carry ? HW : 0u;
        n += carry ? 1u : 0u;
      }
      constexpr int kDup = (G > P) ? G / P : 1;  // lanes that end with the same class total
      if (valid && cls < n_cls && (gq & (kDup - 1)) == 0)
        out[(static_cast<long>(n) * n_cls + cls) * HW + hw] = 1.0f / (1.0f + __expf(-(logit + bias[cls])));
    }
    // advance the carried position by U spans
    n0 += U * span_n;
    hw0 += U * span_hw;
#pragma unroll
    for (int c = 0; c < U; ++c) {
      const bool carry = hw0 >= HW;
      hw0 -= carry ? HW : 0u;
      n0 += carry ? 1u : 0u;
    }
  }
}

// Ensemble head (unetpp_heads_mean_fwd), streaming form: the layout, the loop and the per-pixel logit of
// head_fwd_stream_kernel without dropout, with the heads as an inner loop -- for every iteration's U pixels each head's
// quad is loaded once (16 bytes), its class weights come from the L1-resident [n_cls, C] table (no LDS tile), and the
// sigmoids are added in head order; the mean is stored once.  32-bit element offsets (launcher: < 2^31 elements).
template <int LOG2G, int P>
__global__ __launch_bounds__(kThreads) void heads_mean_stream_kernel(const unetpp_heads_mean hd, unsigned pixels, unsigned HW,
                                                                     int n_cls, float* __restrict__ out) {
  constexpr int G = 1 << LOG2G;
  const int gq = threadIdx.x & (G - 1);
  constexpr unsigned ppb = kThreads >> LOG2G;
  constexpr int U = 4;
  const unsigned span = gridDim.x * ppb, outer = U * span;
  const unsigned pl = threadIdx.x >> LOG2G;
  const unsigned span_n = span / HW, span_hw = span - span_n * HW;
  const int n_heads = hd.n_heads;
  const float count = static_cast<float>(n_heads);
  unsigned p0 = blockIdx.x * ppb + pl;
  unsigned n0 = p0 / HW, hw0 = p0 - n0 * HW;
  for (; p0 - pl < pixels; p0 += outer) {  // wave-uniform trip count
    float sum[U] = {0.f, 0.f, 0.f, 0.f};  // 0 + s_1 is s_1: the sum is ((s_1 + s_2) + ...) in head order
    int cls = 0;
    for (int h = 0; h < n_heads; ++h) {
      const float* __restrict__ x = static_cast<const float*>(hd.head[h].x);
      const float* __restrict__ weight = hd.head[h].weight;
      f32x4 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const unsigned p = p0 + u * span;
        v[u] = (p < pixels) ? *reinterpret_cast<const f32x4*>(x + ((p << (LOG2G + 2)) + 4 * gq)) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
      f32x4 wq[P];
#pragma unroll
      for (int k = 0; k < P; ++k)
        wq[k] = (k < n_cls) ? *reinterpret_cast<const f32x4*>(weight + k * 4 * G + 4 * gq) : f32x4{0.f, 0.f, 0.f, 0.f};
      float logit[U];
#pragma unroll
      for (int u = 0; u < U; ++u) logit[u] = head_pixel_logit<LOG2G, P>(v[u], wq, gq, cls);
      const float b = cls < n_cls ? hd.head[h].bias[cls] : 0.f;
#pragma unroll
      for (int u = 0; u < U; ++u) sum[u] += 1.0f / (1.0f + __expf(-(logit[u] + b)));
    }
    constexpr int kDup = (G > P) ? G / P : 1;  // lanes that end with the same class total
#pragma unroll
    for (int u = 0; u < U; ++u) {
      unsigned n = n0 + u * span_n, hw = hw0 + u * span_hw;
#pragma unroll
      for (int c = 0; c < U - 1; ++c) {  // at most u carries
        const bool carry = c < u && hw >= HW;
        hw -= carry ? HW : 0u;
        n += carry ? 1u : 0u;
      }
      if (p0 + u * span < pixels && cls < n_cls && (gq & (kDup - 1)) == 0)
        out[(static_cast<long>(n) * n_cls + cls) * HW + hw] = sum[u] / count;
    }
    n0 += U * span_n;
    hw0 += U * span_hw;
#pragma unroll
    for (int c = 0; c < U; ++c) {
      const bool carry = hw0 >= HW;
      hw0 -= carry ? HW : 0u;
      n0 += carry ? 1u : 0u;
    }
  }
}

// tile = 64 consecutive pixels.  LDS: x*keep*scale [64][C+1], dlogit [64][8], W [8][C].
__global__ __launch_bounds__(kThreads) void head_bwd_kernel(const float* __restrict__ d_out, const float* __restrict__ outp,
                                                            const float* __restrict__ x, const float* __restrict__ weight,
                                                            long pixels, int HW, int C, int n_cls, float keep_scale,
                                                            uint32_t thr16, uint64_t seed, const uint8_t* __restrict__ mask, const uint64_t* __restrict__ seed_dev,
                                                            int use_drop, float* __restrict__ dx, int accumulate, int gate_x,
                                                            float* __restrict__ partial) {
  if (seed_dev != nullptr) seed += *seed_dev;  // graph-captured steps: the varying part of the seed lives in device memory
  __shared__ float xs[64 * (kHeadMaxC + 1)];
  __shared__ float dl[64 * kHeadMaxCls];
  __shared__ float wsm[kHeadMaxCls * kHeadMaxC];
  const int tid = threadIdx.x;
  const int XS = C + 1;
  const int g4n = (C + 3) >> 2;
  for (int i = tid; i < n_cls * C; i += kThreads) wsm[i] = weight[i];
  float wacc[4] = {0.f, 0.f, 0.f, 0.f};  // dW entries tid, tid+256, ... (n_cls*C <= 1024)
  float bacc = 0.f;                      // db entry tid (< n_cls)
  const long n_tiles = (pixels + 63) / 64;
  for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long p0 = tile * 64;
    __syncthreads();
    // dlogit = d_out * out * (1 - out)
    for (int it = tid; it < 64 * n_cls; it += kThreads) {
      const int pl = it & 63, k = it >> 6;
      const long p = p0 + pl;
      float v = 0.f;
      if (p < pixels) {
        const long n = p / HW, hw = p - n * HW;
        const long o = (n * n_cls + k) * HW + hw;
        const float pr = outp[o];
        v = d_out[o] * pr * (1.f - pr);
      }
      dl[pl * kHeadMaxCls + k] = v;
    }
    // x * keep * scale
    for (int it = tid; it < 64 * C; it += kThreads) {
      const int pl = it / C, c = it - pl * C;
      const long p = p0 + pl;
      float v = 0.f;
      if (p < pixels) {
        v = x[p * C + c];
        if (use_drop) {
          const bool keep = (mask != nullptr) ? (mask[p * C + c] != 0)
                                              : keep_one(keep_bits(seed, p, g4n, c >> 2), c & 3, thr16);
          v = keep ? v * keep_scale : 0.f;
        }
      }
      xs[pl * XS + c] = v;
    }
    __syncthreads();
    // dx[p, c] = keep * scale * sum_k W[k, c] * dlogit[p, k]
    for (int it = tid; it < 64 * C; it += kThreads) {
      const int pl = it / C, c = it - pl * C;
      const long p = p0 + pl;
      if (p < pixels) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < kHeadMaxCls; ++k)
          if (k < n_cls) s += wsm[k * C + c] * dl[pl * kHeadMaxCls + k];
        if (use_drop) {
          const bool keep = (mask != nullptr) ? (mask[p * C + c] != 0)
                                              : keep_one(keep_bits(seed, p, g4n, c >> 2), c & 3, thr16);
          s = keep ? s * keep_scale : 0.f;
        }
        if (accumulate) s += dx[p * C + c];
        if (gate_x) s = (x[p * C + c] > 0.f) ? s : 0.f;
        dx[p * C + c] = s;
      }
    }
    // dW[k, c] += sum_p dlogit[p, k] * xs[p, c];  db[k] += sum_p dlogit[p, k]
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int idx = tid + q * kThreads;
      if (idx < n_cls * C) {
        const int k = idx / C, c = idx - k * C;
        float s = 0.f;
        for (int pl = 0; pl < 64; ++pl) s += dl[pl * kHeadMaxCls + k] * xs[pl * XS + c];
        wacc[q] += s;
      }
    }
    if (tid < n_cls) {
      float s = 0.f;
      for (int pl = 0; pl < 64; ++pl) s += dl[pl * kHeadMaxCls + tid];
      bacc += s;
    }
  }
  float* dst = partial + static_cast<long>(blockIdx.x) * (n_cls * C + n_cls);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int idx = tid + q * kThreads;
    if (idx < n_cls * C) dst[idx] = wacc[q];
  }
  if (tid < n_cls) dst[n_cls * C + tid] = bacc;
}

// Backward head, vectorised (C % 4 == 0): per 64-pixel tile
//   1. dlogit = d_out * out * (1 - out)                    (NCHW reads, coalesced along pixels) -> LDS
//   2. one pass over x in 16-byte pieces: dropout keep mask from ONE hash per piece, x*keep*scale -> LDS for
//      the weight gradient, and dx = keep*scale * (W^T dlogit) (+ old dx, ReLU gate) written straight back
//   3. dW[k, c] += sum_p dlogit[p, k] * xs[p, c]: all 256 threads, two pixel halves per (k, c)
// Dynamic LDS: xs [64][C+1] | dlogit [64][8] | W [8][C] | scratch [2][n_cls*C].
// (launch bound of 4 waves per SIMD: left alone hipcc unrolls the reduction loops into 256 VGPRs and the kernel
// runs at 2 workgroups per CU, latency-bound at 1 TB/s)
__global__ __launch_bounds__(kThreads, 4) void head_bwd_vec_kernel(const float* __restrict__ d_out,
                                                                const float* __restrict__ outp,
                                                                const float* __restrict__ x,
                                                                const float* __restrict__ weight, long pixels, int HW,
                                                                int C, int n_cls, float keep_scale, uint32_t thr16,
                                                                uint64_t seed, const uint8_t* __restrict__ mask, const uint64_t* __restrict__ seed_dev,
                                                                int use_drop, float* __restrict__ dx, int accumulate,
                                                                int gate_x, float* __restrict__ partial) {
  if (seed_dev != nullptr) seed += *seed_dev;  // graph-captured steps: the varying part of the seed lives in device memory
  extern __shared__ __attribute__((aligned(16))) float hsm[];
  const int XS = C + 1, g4n = C >> 2, NW = n_cls * C;
  float* xs = hsm;
  float* dl = xs + 64 * XS;
  float* wsm = dl + 64 * kHeadMaxCls;
  float* scratch = wsm + kHeadMaxCls * C;
  const int tid = threadIdx.x;
  for (int i = tid; i < NW; i += kThreads) wsm[i] = weight[i];
  constexpr int kMaxPairs = (kHeadMaxCls * kHeadMaxC + 127) / 128;  // (k, c) pairs per thread
  float wacc[kMaxPairs];
#pragma unroll
  for (int q = 0; q < kMaxPairs; ++q) wacc[q] = 0.f;
  float bacc = 0.f;
  const int pair0 = tid & 127, half = tid >> 7;
  const long n_tiles = (pixels + 63) / 64;
  for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long p0 = tile * 64;
    __syncthreads();
    for (int it = tid; it < 64 * n_cls; it += kThreads) {
      const int pl = it & 63, k = it >> 6;
      const long p = p0 + pl;
      float v = 0.f;
      if (p < pixels) {
        const long n = p / HW, hw = p - n * HW;
        const long o = (n * n_cls + k) * HW + hw;
        const float pr = outp[o];
        v = d_out[o] * pr * (1.f - pr);
      }
      dl[pl * kHeadMaxCls + k] = v;
    }
    __syncthreads();
    for (int it = tid; it < 64 * g4n; it += kThreads) {
      const int pl = it / g4n, gq = it - pl * g4n;
      const long p = p0 + pl;
      f32x4 xv = {0.f, 0.f, 0.f, 0.f};
      float ms[4] = {1.f, 1.f, 1.f, 1.f};
      if (p < pixels) {
        xv = *reinterpret_cast<const f32x4*>(x + p * C + 4 * gq);
        if (use_drop) {
          const uint64_t bits = (mask == nullptr) ? keep_bits(seed, p, g4n, gq) : 0;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const bool keep = (mask != nullptr) ? (mask[p * C + 4 * gq + q] != 0) : keep_one(bits, q, thr16);
            ms[q] = keep ? keep_scale : 0.f;
          }
        }
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < kHeadMaxCls; ++k) {
          if (k < n_cls) {
            const float dk = dl[pl * kHeadMaxCls + k];
#pragma unroll
            for (int q = 0; q < 4; ++q) s[q] += wsm[k * C + 4 * gq + q] * dk;
          }
        }
        float* dst = dx + p * C + 4 * gq;
        f32x4 old = {0.f, 0.f, 0.f, 0.f};
        if (accumulate) old = *reinterpret_cast<const f32x4*>(dst);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float v = s[q] * ms[q] + old[q];
          if (gate_x) v = (xv[q] > 0.f) ? v : 0.f;
          s[q] = v;
        }
        *reinterpret_cast<f32x4*>(dst) = s;
      }
      float* xd = &xs[pl * XS + 4 * gq];
#pragma unroll
      for (int q = 0; q < 4; ++q) xd[q] = xv[q] * ms[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kMaxPairs; ++q) {
      const int idx = pair0 + q * 128;
      if (idx < NW) {
        const int k = idx / C, c = idx - k * C;
        float s = 0.f;
#pragma unroll 4
        for (int pl = 32 * half; pl < 32 * half + 32; ++pl) s += dl[pl * kHeadMaxCls + k] * xs[pl * XS + c];
        wacc[q] += s;
      }
    }
    if (tid < n_cls) {
      float s = 0.f;
      for (int pl = 0; pl < 64; ++pl) s += dl[pl * kHeadMaxCls + tid];
      bacc += s;
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < kMaxPairs; ++q) {
    const int idx = pair0 + q * 128;
    if (idx < NW) scratch[half * NW + idx] = wacc[q];
  }
  __syncthreads();
  float* dst = partial + static_cast<long>(blockIdx.x) * (NW + n_cls);
  for (int i = tid; i < NW; i += kThreads) dst[i] = scratch[i] + scratch[NW + i];
  if (tid < n_cls) dst[NW + tid] = bacc;
}

// The same for C = 4 * 2^LOG2G channels and tensors below 2^31 elements (every configuration of the reference): the
// index arithmetic is shifts and 32-bit, a thread's channel quad is the same for all its pieces so its class weights
// live in registers (the general kernel re-reads them from LDS per piece: 16 + 4 LDS reads per 16 bytes of x), the
// (class, channel) pairs of the weight-gradient pass are decoded once instead of once per tile, and the dropout mode is
// a template parameter (0 none, 1 counter hash, 2 mask tensor) so that the piece loop is straight-line code.
template <int LOG2G, int DROP, int PCLS>  // PCLS = classes padded to 4 or 8 (zero weights past n_cls: no class branches)
__global__ __launch_bounds__(kThreads, 4) void head_bwd_pow2_kernel(const float* __restrict__ d_out,
                                                                 const float* __restrict__ outp,
                                                                 const float* __restrict__ x,
                                                                 const float* __restrict__ weight, unsigned pixels,
                                                                 unsigned HW, int n_cls, float keep_scale, uint32_t thr16,
                                                                 uint64_t seed, const uint8_t* __restrict__ mask, const uint64_t* __restrict__ seed_dev,
                                                                 float* __restrict__ dx, int accumulate, int gate_x,
                                                                 float* __restrict__ partial) {
  if (seed_dev != nullptr) seed += *seed_dev;  // graph-captured steps: the varying part of the seed lives in device memory
  extern __shared__ __attribute__((aligned(16))) float hsm[];
  constexpr int G = 1 << LOG2G, C = 4 * G, XS = C + 1;
  constexpr int ITEMS = (64 * G + kThreads - 1) / kThreads;  // 16-byte pieces of a 64-pixel tile per thread
  const int NW = n_cls * C;
  float* xs = hsm;
  float* dl = xs + 64 * XS;
  float* scratch = dl + 64 * kHeadMaxCls;
  const int tid = threadIdx.x;
  const int gq = tid & (G - 1);  // channel quad of every piece of this thread (kThreads is a multiple of G)
  f32x4 wq[PCLS];
#pragma unroll
  for (int k = 0; k < PCLS; ++k)
    wq[k] = (k < n_cls) ? *reinterpret_cast<const f32x4*>(weight + k * C + 4 * gq) : f32x4{0.f, 0.f, 0.f, 0.f};
  constexpr int kMaxPairs = (PCLS * C + 127) / 128;  // (k, c) pairs per thread
  float wacc[kMaxPairs];
  int pair_k[kMaxPairs], pair_c[kMaxPairs];
  const int pair0 = tid & 127, half = tid >> 7;
#pragma unroll
  for (int q = 0; q < kMaxPairs; ++q) {
    wacc[q] = 0.f;
    const int idx = pair0 + q * 128;
    pair_k[q] = idx >> (LOG2G + 2);
    pair_c[q] = idx & (C - 1);
  }
  float bacc = 0.f;
  for (int i = tid; i < 64 * kHeadMaxCls; i += kThreads) dl[i] = 0.f;  // classes past n_cls are never written again
  const unsigned n_tiles = (pixels + 63) / 64;
  for (unsigned tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const unsigned p0 = tile * 64;
    __syncthreads();
    for (int it = tid; it < 64 * n_cls; it += kThreads) {
      const int pl = it & 63, k = it >> 6;
      const unsigned p = p0 + pl;
      float v = 0.f;
      if (p < pixels) {
        const unsigned n = p / HW, hw = p - n * HW;
        const long o = (static_cast<long>(n) * n_cls + k) * HW + hw;
        const float pr = outp[o];
        v = d_out[o] * pr * (1.f - pr);
      }
      dl[pl * kHeadMaxCls + k] = v;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < ITEMS; ++u) {
      const int it = tid + u * kThreads;
      if (ITEMS * kThreads != 64 * G && it >= 64 * G) break;
      const int pl = it >> LOG2G;
      const unsigned p = p0 + pl;
      f32x4 xv = {0.f, 0.f, 0.f, 0.f};
      float ms[4] = {1.f, 1.f, 1.f, 1.f};
      if (p < pixels) {
        const unsigned off = (p << (LOG2G + 2)) + 4 * gq;
        xv = *reinterpret_cast<const f32x4*>(x + off);
        if constexpr (DROP == 1) {
          const uint64_t bits = keep_bits(seed, p, G, gq);
#pragma unroll
          for (int q = 0; q < 4; ++q) ms[q] = keep_one(bits, q, thr16) ? keep_scale : 0.f;
        } else if constexpr (DROP == 2) {
          const uint32_t m4 = *reinterpret_cast<const uint32_t*>(mask + off);
#pragma unroll
          for (int q = 0; q < 4; ++q) ms[q] = ((m4 >> (8 * q)) & 0xffu) != 0 ? keep_scale : 0.f;
        }
        f32x4 sacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < PCLS; ++k) {
          const float dk = dl[pl * kHeadMaxCls + k];
#pragma unroll
          for (int q = 0; q < 4; ++q) sacc[q] += wq[k][q] * dk;
        }
        f32x4 old = {0.f, 0.f, 0.f, 0.f};
        if (accumulate) old = *reinterpret_cast<const f32x4*>(dx + off);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float v = sacc[q] * ms[q] + old[q];
          if (gate_x) v = (xv[q] > 0.f) ? v : 0.f;
          sacc[q] = v;
        }
        *reinterpret_cast<f32x4*>(dx + off) = sacc;
      }
      float* xd = &xs[pl * XS + 4 * gq];
#pragma unroll
      for (int q = 0; q < 4; ++q) xd[q] = xv[q] * ms[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kMaxPairs; ++q) {
      if (pair0 + q * 128 < NW) {
        const int k = pair_k[q], c = pair_c[q];
        float sum = 0.f;
#pragma unroll 4
        for (int pl = 32 * half; pl < 32 * half + 32; ++pl) sum += dl[pl * kHeadMaxCls + k] * xs[pl * XS + c];
        wacc[q] += sum;
      }
    }
    if (tid < n_cls) {
      float sum = 0.f;
      for (int pl = 0; pl < 64; ++pl) sum += dl[pl * kHeadMaxCls + tid];
      bacc += sum;
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < kMaxPairs; ++q) {
    const int idx = pair0 + q * 128;
    if (idx < NW) scratch[half * NW + idx] = wacc[q];
  }
  __syncthreads();
  float* dst = partial + static_cast<long>(blockIdx.x) * (NW + n_cls);
  for (int i = tid; i < NW; i += kThreads) dst[i] = scratch[i] + scratch[NW + i];
  if (tid < n_cls) dst[NW + tid] = bacc;
}

// The class head_pixel_logit leaves with the lane of channel quad gq (its `cls`): a function of gq alone.
template <int LOG2G, int P>
__device__ __forceinline__ int head_lane_class(int gq) {
  constexpr int G = 1 << LOG2G;
  int c = 0;
  static_for<LOG2G>([&](auto sc) {
    constexpr int step = decltype(sc)::v, off = G >> (1 + step);
    constexpr int live = (P >> step) > 1 ? (P >> step) : 1;
    if constexpr (live > 1) c += (gq & off) != 0 ? (live >> 1) : 0;
  });
  return c;
}

// acc + d * d in two roundings: the product on its own, then the sum.  Left to the compiler `acc += d * d` becomes one
// fma (as every such sum of head_bwd_pow2_kernel does), which is not the fold unetpp_head_mc promises.
__device__ __forceinline__ float mc_add_square(float acc, float d) {
#pragma clang fp contract(off)
  const float sq = d * d;
  return acc + sq;
}

// Monte-Carlo dropout at one head (unetpp_head_mc): head_fwd_stream_kernel<LOG2G, P, 1>'s layout, loop, loads and carried
// (image, position), with the samples as an inner loop over ONE read of x -- sample k redraws the keep flags from
// seed + kMcSeedStep * k and goes through the forward's own expressions (keep_bits / keep_one / keep_scale,
// head_pixel_logit, the __expf sigmoid), so s_k has the bits head_fwd_stream_kernel stores for that seed.  Two maps leave:
//   mean = (((s_0 + s_1) + ...) + s_{K-1}) / float(K)
//   var  = (((d_0 d_0 + d_1 d_1) + ...) + d_{K-1} d_{K-1}) / float(K - 1),   d_k = s_k - mean
// every product, sum and quotient rounded on its own (mc_add_square; nothing here is an fmaf but the dot product inside
// head_pixel_logit, which is spelled fmaf there).  The deviations need the mean, so the K samples of a pixel wait in LDS:
// a thread owns the column slab[k * kThreads + threadIdx.x], k < K (K * 1 KiB per workgroup, no bank conflict, no barrier:
// nobody else reads it), written in the sample loop and read back once.  Four pixels are loaded ahead as in the forward;
// their samples are drawn one pixel after the other, so one column serves all four.  No atomics; the result does not
// depend on the grid.
template <int LOG2G, int P>
__global__ __launch_bounds__(kThreads) void head_mc_kernel(const float* __restrict__ x, const float* __restrict__ weight,
                                                           const float* __restrict__ bias, unsigned pixels, unsigned HW,
                                                           int n_cls, float keep_scale, uint32_t thr16, uint64_t seed,
                                                           const uint64_t* __restrict__ seed_dev, int samples,
                                                           float* __restrict__ mean_out, float* __restrict__ var_out) {
  if (seed_dev != nullptr) seed += *seed_dev;
  extern __shared__ __attribute__((aligned(16))) float slab[];  // [samples][kThreads]
  constexpr int G = 1 << LOG2G;  // lanes (channel quads) per pixel
  const int gq = threadIdx.x & (G - 1);
  f32x4 wq[P];
#pragma unroll
  for (int k = 0; k < P; ++k)
    wq[k] = (k < n_cls) ? *reinterpret_cast<const f32x4*>(weight + k * 4 * G + 4 * gq) : f32x4{0.f, 0.f, 0.f, 0.f};
  constexpr unsigned ppb = kThreads >> LOG2G;
  constexpr int U = 4;
  constexpr int kDup = (G > P) ? G / P : 1;  // lanes that end with the same class total
  const unsigned span = gridDim.x * ppb, outer = U * span;
  const unsigned pl = threadIdx.x >> LOG2G;
  const unsigned span_n = span / HW, span_hw = span - span_n * HW;
  const int cls = head_lane_class<LOG2G, P>(gq);  // the class head_pixel_logit leaves with this lane
  const bool writer = cls < n_cls && (gq & (kDup - 1)) == 0;
  const float b = cls < n_cls ? bias[cls] : 0.f;
  const float count = static_cast<float>(samples), count1 = static_cast<float>(samples - 1);
  float* mine = slab + threadIdx.x;
  unsigned p0 = blockIdx.x * ppb + pl;
  unsigned n0 = p0 / HW, hw0 = p0 - n0 * HW;
  for (; p0 - pl < pixels; p0 += outer) {  // wave-uniform trip count
    f32x4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const unsigned p = p0 + u * span;
      v[u] = (p < pixels) ? *reinterpret_cast<const f32x4*>(x + ((p << (LOG2G + 2)) + 4 * gq)) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const unsigned p = p0 + u * span;
      float sum = 0.f;  // 0 + s_0 is s_0 (a sigmoid is never -0)
      uint64_t seed_k = seed;
      for (int k = 0; k < samples; ++k, seed_k += kMcSeedStep) {  // every lane of the wave: the logits are exchanged
        const uint64_t bits = keep_bits(seed_k, p, G, gq);
        f32x4 d;
#pragma unroll
        for (int q = 0; q < 4; ++q) d[q] = keep_one(bits, q, thr16) ? v[u][q] * keep_scale : 0.f;
        int c;
        const float logit = head_pixel_logit<LOG2G, P>(d, wq, gq, c);
        const float s = 1.0f / (1.0f + __expf(-(logit + b)));
        mine[k * kThreads] = s;
        sum += s;
      }
      const float mean = sum / count;
      float sq = 0.f;  // 0 + d_0 d_0 is d_0 d_0 (a square is never -0)
      for (int k = 0; k < samples; ++k) sq = mc_add_square(sq, mine[k * kThreads] - mean);
      const float var = sq / count1;
      unsigned n = n0 + u * span_n, hw = hw0 + u * span_hw;
#pragma unroll
      for (int c = 0; c < U - 1; ++c) {  // at most u carries
        const bool carry = c < u && hw >= HW;
        hw -= carry ? HW : 0u;
        n += carry ? 1u : 0u;
      }
      if (p < pixels && writer) {
        const long o = (static_cast<long>(n) * n_cls + cls) * HW + hw;
        mean_out[o] = mean;
        var_out[o] = var;
      }
    }
    n0 += U * span_n;
    hw0 += U * span_hw;
#pragma unroll
    for (int c = 0; c < U; ++c) {
      const bool carry = hw0 >= HW;
      hw0 -= carry ? HW : 0u;
      n0 += carry ? 1u : 0u;
    }
  }
}

// One head of a training step in ONE pass over x (unetpp_head_train): what head_fwd_stream_kernel, the gradient half of
// focal_bce_heads_kernel (caller.hip) and head_bwd_pow2_kernel do in three, with the same bits in the map, dx and every
// partial row.  Once the target is known everything the backward needs is in the forward's registers, so the map is
// written and never read back, d_out is never written, and x is read once.  head_bwd_pow2_kernel's tile walk, grid,
// partial rows and LDS plan; per 64-pixel tile
//   1. a thread's 16-byte pieces of x (lane = (pixel, channel quad), as both kernels have it): keep flags as the forward
//      takes them, x*keep*scale -> LDS for the weight gradient, the logits by head_pixel_logit (the forward's function,
//      lanes and order); the lane that ends up with a class adds the bias, stores the sigmoid, reads the target element
//      and forms d_out by focal_element (the mean over n_heads: scale = 1 / n_heads at the same place) and
//      dlogit = d_out * out * (1 - out) -> LDS
//   2. dx = keep*scale * (W^T dlogit) (+ 0, ReLU gate) from the pieces still in registers; the head is always the first
//      contribution to its node, so dx is never accumulated (the `+ 0.f` is head_bwd_pow2's `+ old` without an old
//      value: -0 becomes +0 there too)
//   3. the dW / db sums of head_bwd_pow2_kernel, same loops, same order
// A tile is a chain load -> logits -> loss -> barrier -> dx: with the target loaded after the sigmoid (a second memory
// latency per tile) and nothing in flight during steps 2 and 3 the pass took 171 us per head at 32 x 256 x 256 x 32, more
// than half again what its bytes cost.  The target is therefore loaded with x, and up to 32 channels the next tile's x
// and target are loaded before this tile's barrier: 118 us, head_bwd_pow2_kernel's own time.
// Where head_bwd_pow2_kernel's sums are written `s += a * b` the compiler contracts every one of them into an fma; this
// kernel says fmaf, because around its other code the same source came out as packed products and separate additions.
// No atomics: partial rows and unetpp_sum_partials' fixed-order finish.  PCLS <= G (the forward's reduce-scatter deals the
// classes to the lanes of a pixel), so a tile is ITEMS = G / 4 whole rounds of the workgroup.
template <int LOG2G, int DROP, int PCLS>
__global__ __launch_bounds__(kThreads, 4) void head_train_pow2_kernel(const float* __restrict__ x,
                                                                   const float* __restrict__ weight,
                                                                   const float* __restrict__ bias,
                                                                   const float* __restrict__ target, unsigned pixels,
                                                                   unsigned HW, int n_cls, float keep_scale, uint32_t thr16,
                                                                   uint64_t seed, const uint8_t* __restrict__ mask,
                                                                   const uint64_t* __restrict__ seed_dev, float gamma,
                                                                   float inv_rows, float inv_heads, float* __restrict__ out,
                                                                   float* __restrict__ dx, int gate_x,
                                                                   float* __restrict__ partial) {
  if (seed_dev != nullptr) seed += *seed_dev;  // graph-captured steps: the varying part of the seed lives in device memory
  extern __shared__ __attribute__((aligned(16))) float hsm[];
  constexpr int G = 1 << LOG2G, C = 4 * G, XS = C + 1;
  static_assert(G >= 4 && PCLS <= G, "a tile is whole rounds of the workgroup, and every class has a lane");
  constexpr int ITEMS = 64 * G / kThreads;   // 16-byte pieces of a 64-pixel tile per thread
  constexpr int PPR = kThreads >> LOG2G;     // pixels of one round
  // Up to 32 channels (two pieces per thread) the pieces of x stay in registers from step 1 to step 2 and the next tile's
  // are loaded a tile ahead; at 64 and 128 channels that does not fit 128 registers: step 1 loads two pieces at a time
  // and step 2 reads x again (from the cache) where the ReLU gate needs it
  constexpr bool kKeepX = ITEMS <= 2, kPrefetch = kKeepX;
  constexpr int kUnroll1 = kKeepX ? ITEMS : 2;
  constexpr int kDup = (G > PCLS) ? G / PCLS : 1;  // lanes that end with the same class total
  const int NW = n_cls * C;
  float* xs = hsm;
  float* dl = xs + 64 * XS;
  float* scratch = dl + 64 * kHeadMaxCls;
  const int tid = threadIdx.x;
  const int gq = tid & (G - 1);  // channel quad of every piece of this thread
  f32x4 wq[PCLS];
#pragma unroll
  for (int k = 0; k < PCLS; ++k)
    wq[k] = (k < n_cls) ? *reinterpret_cast<const f32x4*>(weight + k * C + 4 * gq) : f32x4{0.f, 0.f, 0.f, 0.f};
  constexpr int kMaxPairs = (PCLS * C + 127) / 128;  // (k, c) pairs per thread
  float wacc[kMaxPairs];
  const int pair0 = tid & 127, half = tid >> 7;
#pragma unroll
  for (int q = 0; q < kMaxPairs; ++q) wacc[q] = 0.f;
  float bacc = 0.f;
  const bool cube = gamma == 3.f, low = gamma < 1.f;
  // the class this lane ends up with in head_pixel_logit depends on its channel quad alone: the lane that stores a class
  // knows it, its bias and the target element before the logits exist, so the target is loaded WITH x, not after them
  const int my_cls = head_lane_class<LOG2G, PCLS>(gq);
  const bool owner = my_cls < n_cls && (gq & (kDup - 1)) == 0;
  const float my_bias = owner ? bias[my_cls] : 0.f;
  // one piece: x, the mask word, and for an owner the offset of its map element and the target there
  auto fetch = [&](unsigned p, f32x4& X, uint32_t& M, unsigned& O, float& T) {
    const bool valid = p < pixels;
    const unsigned off = (p << (LOG2G + 2)) + 4 * gq;
    X = valid ? *reinterpret_cast<const f32x4*>(x + off) : f32x4{0.f, 0.f, 0.f, 0.f};
    M = 0xffffffffu;
    if constexpr (DROP == 2) M = valid ? *reinterpret_cast<const uint32_t*>(mask + off) : 0xffffffffu;
    O = 0u;
    T = 0.f;
    if (owner && valid) {
      const unsigned n = p / HW, hw = p - n * HW;
      O = (n * n_cls + my_cls) * HW + hw;  // < pixels * 8 <= 2^31 * 8 / C: 32 bits
      T = target[O];
    }
  };
  constexpr int NK = kKeepX ? ITEMS : 1;
  f32x4 xv[NK], xn[kPrefetch ? NK : 1];     // the tile's pieces (kept for the ReLU gate of step 2) / the next tile's
  uint32_t mv[NK], mn[kPrefetch ? NK : 1];
  unsigned ov[NK], on[kPrefetch ? NK : 1];
  float tv[NK], tn[kPrefetch ? NK : 1];
  for (int i = tid; i < 64 * kHeadMaxCls; i += kThreads) dl[i] = 0.f;  // classes past n_cls are never written again
  const unsigned n_tiles = (pixels + 63) / 64;
  if constexpr (kPrefetch) {
    if (blockIdx.x < n_tiles) {
#pragma unroll
      for (int u = 0; u < NK; ++u) fetch(blockIdx.x * 64 + (tid >> LOG2G) + u * PPR, xn[u], mn[u], on[u], tn[u]);
    }
  }
  for (unsigned tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const unsigned p0 = tile * 64;
    if constexpr (kPrefetch) {  // this tile's loads were issued a tile ago; the next tile's go out now
#pragma unroll
      for (int u = 0; u < NK; ++u) xv[u] = xn[u], mv[u] = mn[u], ov[u] = on[u], tv[u] = tn[u];
      const unsigned next = tile + gridDim.x;
      if (next < n_tiles) {
#pragma unroll
        for (int u = 0; u < NK; ++u) fetch(next * 64 + (tid >> LOG2G) + u * PPR, xn[u], mn[u], on[u], tn[u]);
      }
    } else if constexpr (kKeepX) {
#pragma unroll
      for (int u = 0; u < NK; ++u) fetch(p0 + (tid >> LOG2G) + u * PPR, xv[u], mv[u], ov[u], tv[u]);
    }
    __syncthreads();
    unsigned kept = 0u;  // keep flags of the pieces, bit 4 * u + q
#pragma unroll kUnroll1
    for (int u = 0; u < ITEMS; ++u) {
      const int pl = (tid >> LOG2G) + u * PPR;
      const unsigned p = p0 + pl;
      const bool valid = p < pixels;  // (every lane stays: the logits are lane exchanges)
      f32x4 xu;
      uint32_t m4;
      unsigned o;
      float t;
      if constexpr (kKeepX)
        xu = xv[u], m4 = mv[u], o = ov[u], t = tv[u];
      else
        fetch(p, xu, m4, o, t);
      unsigned kb = 0xfu;
      if constexpr (DROP == 1) {
        const uint64_t bits = keep_bits(seed, p, G, gq);
        kb = 0u;
#pragma unroll
        for (int q = 0; q < 4; ++q) kb |= keep_one(bits, q, thr16) ? (1u << q) : 0u;
      } else if constexpr (DROP == 2) {
        kb = 0u;
#pragma unroll
        for (int q = 0; q < 4; ++q) kb |= ((m4 >> (8 * q)) & 0xffu) != 0 ? (1u << q) : 0u;
      }
      kept |= kb << (4 * u);
      f32x4 v = xu;  // the forward's operand: a dropped element is 0, whatever x holds
      float* xd = &xs[pl * XS + 4 * gq];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if constexpr (DROP != 0) {
          const bool keep = ((kb >> q) & 1u) != 0;
          v[q] = keep ? xu[q] * keep_scale : 0.f;
          xd[q] = xu[q] * (keep ? keep_scale : 0.f);  // the backward's x * keep * scale
        } else {
          xd[q] = xu[q] * 1.f;
        }
      }
      int cls;  // class this lane ends up with: my_cls
      const float logit = head_pixel_logit<LOG2G, PCLS>(v, wq, gq, cls);
      if (owner) {
        float dlv = 0.f;
        if (valid) {
          const float pr = 1.0f / (1.0f + __expf(-(logit + my_bias)));
          out[o] = pr;
          float g;
          if (low)
            focal_element<true>(pr, t, gamma, cube, inv_rows, inv_heads, g);
          else
            focal_element<false>(pr, t, gamma, cube, inv_rows, inv_heads, g);
          {
            // head_bwd_pow2 forms d_out * out * (1 - out) as a subtraction and two products; spelled out, so that no
            // contraction into fma(-out, d_out * out, d_out * out) can make this kernel's rounding another one
#pragma clang fp contract(off)
            const float om = 1.f - pr;
            dlv = (g * pr) * om;
          }
        }
        dl[pl * kHeadMaxCls + cls] = dlv;
      }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < ITEMS; ++u) {
      const int pl = (tid >> LOG2G) + u * PPR;
      const unsigned p = p0 + pl;
      if (p < pixels) {
        const unsigned off = (p << (LOG2G + 2)) + 4 * gq;
        f32x4 xg = {0.f, 0.f, 0.f, 0.f};
        if constexpr (kKeepX)
          xg = xv[u];
        else if (gate_x)
          xg = *reinterpret_cast<const f32x4*>(x + off);  // (64 and 128 channels: from the cache)
        f32x4 sacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < PCLS; ++k) {
          const float dk = dl[pl * kHeadMaxCls + k];
#pragma unroll
          for (int q = 0; q < 4; ++q) sacc[q] = fmaf(wq[k][q], dk, sacc[q]);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float ms = DROP == 0 ? 1.f : (((kept >> (4 * u + q)) & 1u) != 0 ? keep_scale : 0.f);
          float v = fmaf(sacc[q], ms, 0.f);
          if (gate_x) v = (xg[q] > 0.f) ? v : 0.f;
          sacc[q] = v;
        }
        *reinterpret_cast<f32x4*>(dx + off) = sacc;
      }
    }
#pragma unroll
    for (int q = 0; q < kMaxPairs; ++q) {
      if (pair0 + q * 128 < NW) {
        const int idx = pair0 + q * 128, k = idx >> (LOG2G + 2), c = idx & (C - 1);  // (decoded here: registers)
        float sum = 0.f;
#pragma unroll 4
        for (int pl = 32 * half; pl < 32 * half + 32; ++pl) sum = fmaf(dl[pl * kHeadMaxCls + k], xs[pl * XS + c], sum);
        wacc[q] += sum;
      }
    }
    if (tid < n_cls) {
      float sum = 0.f;
      for (int pl = 0; pl < 64; ++pl) sum += dl[pl * kHeadMaxCls + tid];
      bacc += sum;
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < kMaxPairs; ++q) {
    const int idx = pair0 + q * 128;
    if (idx < NW) scratch[half * NW + idx] = wacc[q];
  }
  __syncthreads();
  float* dst = partial + static_cast<long>(blockIdx.x) * (NW + n_cls);
  for (int i = tid; i < NW; i += kThreads) dst[i] = scratch[i] + scratch[NW + i];
  if (tid < n_cls) dst[NW + tid] = bacc;
}

// ------------------------------------------------------------------ bf16 storage
// ---- heads.  Forward: CG = C/8 lanes share a pixel (CG = 2^LOG2CG <= 16): every lane loads one octet, applies the
// dropout keep mask, multiplies it with the n_cls weight octets and the CG partial sums are folded across the lanes by
// DPP / ds_swizzle moves (xor_lane: the ds_bpermute shuffles of __shfl_xor made this kernel, like its fp32 twin,
// instruction bound at a third of the HBM rate).  DROP: 0 = none, 1 = counter hash, 2 = mask tensor -- separate
// instantiations keep the loop body straight-line.
// One class's logit (without the bias) of one pixel in the octet layout (lane = (pixel, channel octet), CG = 2^LOG2CG
// lanes per pixel): the lane's octet against the class's weight row in LDS, then the CG partial sums folded across the
// lanes in a fixed order; every lane of the pixel ends with the total.  Shared by head_fwd_bf16_kernel and
// heads_mean_bf16_kernel: both produce the same bits for the same operands.
template <int LOG2CG>
__device__ __forceinline__ float head_pixel_logit_bf16(const float (&f)[8], const float* wrow, int cg) {
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) s = fmaf(f[e], wrow[cg * 8 + e], s);
  static_for<LOG2CG>([&](auto mc) { s += xor_lane<(1 << decltype(mc)::v)>(s); });
  return s;
}

template <int LOG2CG, int DROP, int PCLS>  // PCLS = classes padded to 4, 6 or 8 (5 key-point maps: configs[4]): the class loops carry no n_cls branches
__global__ __launch_bounds__(kThreads) void head_fwd_bf16_kernel(const bf16_t* __restrict__ x, const float* __restrict__ weight,
                                                                 const float* __restrict__ bias, long pixels, int HW,
                                                                 int n_cls, float keep_scale, uint32_t thr16,
                                                                 uint64_t seed, const uint8_t* __restrict__ mask, const uint64_t* __restrict__ seed_dev,
                                                                 float* __restrict__ out) {
  if (seed_dev != nullptr) seed += *seed_dev;  // graph-captured steps: the varying part of the seed lives in device memory
  constexpr int CG = 1 << LOG2CG, C = 8 * CG;
  __shared__ float wsm[PCLS * C];  // zero rows past n_cls (the class weights in registers ran 1.2x slower, twice measured)
  for (int i = threadIdx.x; i < PCLS * C; i += kThreads) wsm[i] = i < n_cls * C ? weight[i] : 0.f;
  __syncthreads();
  constexpr int ppb = kThreads >> LOG2CG;  // pixels per workgroup pass
  const int cg = threadIdx.x & (CG - 1), pl = threadIdx.x >> LOG2CG;
  const unsigned npix = static_cast<unsigned>(pixels), uhw = static_cast<unsigned>(HW);  // < 2^31 (launcher)
  const unsigned passes = (npix + ppb - 1) / ppb;
  for (unsigned ps = blockIdx.x; ps < passes; ps += gridDim.x) {  // all lanes stay in the loop: lane exchanges below
    const unsigned p = ps * ppb + pl;
    const bool live = p < npix;
    float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (live) {
      unpack8(reinterpret_cast<const u32x4*>(x)[(static_cast<long>(p) << LOG2CG) + cg], f);
      if constexpr (DROP == 1) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          const uint64_t bits = keep_bits(seed, p, 2 * CG, 2 * cg + half);
#pragma unroll
          for (int q = 0; q < 4; ++q) f[4 * half + q] = keep_one(bits, q, thr16) ? f[4 * half + q] * keep_scale : 0.f;
        }
      } else if constexpr (DROP == 2) {
        const uint2 m8 = *reinterpret_cast<const uint2*>(mask + static_cast<long>(p) * C + cg * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const unsigned byte = ((e < 4 ? m8.x : m8.y) >> (8 * (e & 3))) & 0xffu;
          f[e] = byte != 0 ? f[e] * keep_scale : 0.f;
        }
      }
    }
    const unsigned n = p / uhw, hw = p - n * uhw;  // one 32-bit division per pixel
    float* obase = out + static_cast<long>(n) * n_cls * uhw + hw;
#pragma unroll
    for (int k = 0; k < PCLS; ++k) {
      const float s = head_pixel_logit_bf16<LOG2CG>(f, wsm + k * C, cg);  // every lane of the pixel holds the logit
      if (live && k < n_cls && (k & (CG - 1)) == cg)                // classes are dealt to the pixel's lanes round robin
        obase[static_cast<long>(k) * uhw] = 1.0f / (1.0f + __expf(-(s + bias[k])));
    }
  }
}

// Ensemble head (unetpp_heads_mean_fwd_bf16): head_fwd_bf16_kernel's layout and per-pixel logit without dropout, the
// heads as an inner loop -- every head's octet is loaded once (16 bytes), the sigmoids are added in head order and the
// mean is stored once.  LDS holds one zero-padded weight tile per head ([n_heads][PCLS * C], sized by the launcher).
template <int LOG2CG, int PCLS>
__global__ __launch_bounds__(kThreads) void heads_mean_bf16_kernel(const unetpp_heads_mean hd, long pixels, int HW, int n_cls,
                                                                   float* __restrict__ out) {
  constexpr int CG = 1 << LOG2CG, C = 8 * CG;
  extern __shared__ float hm_wsm[];
  const int n_heads = hd.n_heads;
  const float count = static_cast<float>(n_heads);
  for (int h = 0; h < n_heads; ++h) {
    const float* __restrict__ weight = hd.head[h].weight;
    for (int i = threadIdx.x; i < PCLS * C; i += kThreads) hm_wsm[h * PCLS * C + i] = i < n_cls * C ? weight[i] : 0.f;
  }
  __syncthreads();
  constexpr int ppb = kThreads >> LOG2CG;
  const int cg = threadIdx.x & (CG - 1), pl = threadIdx.x >> LOG2CG;
  const unsigned npix = static_cast<unsigned>(pixels), uhw = static_cast<unsigned>(HW);  // < 2^31 (launcher)
  const unsigned passes = (npix + ppb - 1) / ppb;
  for (unsigned ps = blockIdx.x; ps < passes; ps += gridDim.x) {  // all lanes stay in the loop: lane exchanges below
    const unsigned p = ps * ppb + pl;
    const bool live = p < npix;
    float sum[PCLS];
#pragma unroll
    for (int k = 0; k < PCLS; ++k) sum[k] = 0.f;  // 0 + s_1 is s_1: the sum is ((s_1 + s_2) + ...) in head order
    for (int h = 0; h < n_heads; ++h) {
      float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (live) unpack8(static_cast<const u32x4*>(hd.head[h].x)[(static_cast<long>(p) << LOG2CG) + cg], f);
      const float* __restrict__ bias = hd.head[h].bias;
#pragma unroll
      for (int k = 0; k < PCLS; ++k) {
        const float s = head_pixel_logit_bf16<LOG2CG>(f, hm_wsm + (h * PCLS + k) * C, cg);
        if (k < n_cls && (k & (CG - 1)) == cg) sum[k] += 1.0f / (1.0f + __expf(-(s + bias[k])));  // the lane that stores class k
      }
    }
    const unsigned n = p / uhw, hw = p - n * uhw;
    float* obase = out + static_cast<long>(n) * n_cls * uhw + hw;
#pragma unroll
    for (int k = 0; k < PCLS; ++k)
      if (live && k < n_cls && (k & (CG - 1)) == cg) obase[static_cast<long>(k) * uhw] = sum[k] / count;
  }
}

// Backward: 64-pixel tiles.  LDS: x*keep*scale fp32 [64][C+1], dlogit [64][8].  C = 8 * 2^LOG2CG: index arithmetic in
// shifts and 32 bits; a thread's octet position is the same for all its pieces, so its class weights stay in registers
// (the first version read 32 weights from LDS per octet); the (class, channel) pairs of the weight-gradient pass are
// decoded once; DROP (0 none, 1 counter hash, 2 mask tensor) keeps the piece loop free of per-element branches.
template <int LOG2CG, int DROP, int PCLS>  // PCLS = classes padded to 4, 6 or 8 (5 key-point maps: configs[4]): the class loops carry no n_cls branches
__global__ __launch_bounds__(kThreads) void head_bwd_bf16_kernel(const float* __restrict__ d_out, const float* __restrict__ outp,
                                                                 const bf16_t* __restrict__ x, const float* __restrict__ weight,
                                                                 unsigned pixels, unsigned HW, int n_cls, float keep_scale,
                                                                 uint32_t thr16, uint64_t seed, const uint8_t* __restrict__ mask, const uint64_t* __restrict__ seed_dev,
                                                                 bf16_t* __restrict__ dx, int accumulate, int gate_x,
                                                                 float* __restrict__ partial, unsigned active) {
  if (seed_dev != nullptr) seed += *seed_dev;  // graph-captured steps: the varying part of the seed lives in device memory
  // 256-pixel tiles (four items in flight per thread at 32 channels): dlogit = d_out * out * (1 - out) of the tile goes through LDS (the NCHW class planes are read
  // coalesced along the pixels), then every thread takes (pixel, channel octet) items: dx = keep * scale * (W^T dlogit)
  // (+ old dx, ReLU gate of x) and the weight gradient of ITS octet, dlogit_k * (x * keep * scale), summed in registers
  // over all its items of the launch.  (Until round 3 the weight gradient went through LDS per tile -- x * keep * scale
  // written back, a third barrier and a 64-step loop of two LDS reads per (class, channel) pair: most of the kernel.)
  // One reduction at the end: lanes that share an octet by xor-shuffles, the four waves through LDS, fixed order.
  extern __shared__ float hsm_bf[];  // (its own array: hsm of the fp32 kernels above is declared 16-byte aligned)
  constexpr int CG = 1 << LOG2CG, C = 8 * CG, TP = CG <= 8 ? kHeadTilePixels : 8 * kThreads / CG;  // <= 8 items per thread
  constexpr int ITEMS = (TP * CG + kThreads - 1) / kThreads;
  float* dl = hsm_bf;                  // [TP][8]
  float* red = dl + TP * kHeadMaxCls;  // [4 waves][PCLS * C + PCLS]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cg = tid & (CG - 1);
  const unsigned n_tiles = (pixels + TP - 1) / TP;
  // `active` workgroups walk the tiles (round 6).  A workgroup's fixed part -- 48 weight loads per thread, the shuffle and
  // LDS reduction of its 48 + 6 sums, a 1.3 KB row -- used to be paid per tile or two (one workgroup per tile up to 4096:
  // 2304 tiles at configs[4], 8192 at configs[3]); three workgroups per CU is what the registers allow to be resident.
  if (blockIdx.x >= n_tiles || blockIdx.x >= active) {
    // The grid and the partial rows are sized from 64-pixel tiles (unetpp_head_bwd_blocks, shared with the fp32 kernel);
    // blocks that own no tile of this kernel: a zero row (the caller sums every row) and out,
    // before the weight registers, the shuffles and the LDS reduction
    float* dst = partial + static_cast<long>(blockIdx.x) * (n_cls * C + n_cls);
    for (int i = tid; i < n_cls * C + n_cls; i += kThreads) dst[i] = 0.f;
    return;
  }
  float wq[PCLS][8], wacc[PCLS][8], bacc[PCLS];
#pragma unroll
  for (int k = 0; k < PCLS; ++k) {
    bacc[k] = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      wq[k][e] = (k < n_cls) ? weight[k * C + cg * 8 + e] : 0.f;
      wacc[k][e] = 0.f;
    }
  }
  for (int i = tid; i < TP * kHeadMaxCls; i += kThreads) dl[i] = 0.f;  // classes past n_cls are never written again
  for (unsigned tile = blockIdx.x; tile < n_tiles; tile += active) {
    const unsigned p0 = tile * TP;
    __syncthreads();
    for (int it = tid; it < TP * n_cls; it += kThreads) {  // dlogit = d_out * out * (1 - out)
      const int pl = it & (TP - 1), k = it / TP;
      const unsigned p = p0 + pl;
      float v = 0.f;
      if (p < pixels) {
        const unsigned n = p / HW, hw = p - n * HW;
        const long o = (static_cast<long>(n) * n_cls + k) * HW + hw;
        const float pr = outp[o];
        v = d_out[o] * pr * (1.f - pr);
      }
      dl[pl * kHeadMaxCls + k] = v;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < ITEMS; ++u) {
      const int it = tid + u * kThreads;
      if (ITEMS * kThreads != TP * CG && it >= TP * CG) break;
      const int pl = it >> LOG2CG;
      const unsigned p = p0 + pl;
      if (p >= pixels) continue;
      const long oct = (static_cast<long>(p) << LOG2CG) + cg;
      float raw[8], ks[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) ks[e] = 1.f;
      unpack8(reinterpret_cast<const u32x4*>(x)[oct], raw);
      if constexpr (DROP == 1) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          const uint64_t bits = keep_bits(seed, p, 2 * CG, 2 * cg + half);
#pragma unroll
          for (int q = 0; q < 4; ++q) ks[4 * half + q] = keep_one(bits, q, thr16) ? keep_scale : 0.f;
        }
      } else if constexpr (DROP == 2) {
        const uint2 m8 = *reinterpret_cast<const uint2*>(mask + oct * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) ks[e] = (((e < 4 ? m8.x : m8.y) >> (8 * (e & 3))) & 0xffu) != 0 ? keep_scale : 0.f;
      }
      float dk[PCLS];  // (rows past n_cls of dl are zero: written by the dlogit pass below n_cls only, cleared once)
#pragma unroll
      for (int k = 0; k < PCLS; ++k) dk[k] = dl[pl * kHeadMaxCls + k];
      float o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < PCLS; ++k) sum = fmaf(wq[k][e], dk[k], sum);
        o[e] = sum * ks[e];
      }
      if (accumulate) {
        float old[8];
        unpack8(reinterpret_cast<const u32x4*>(dx)[oct], old);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] += old[e];
      }
      if (gate_x) {
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (raw[e] > 0.f) ? o[e] : 0.f;
      }
      reinterpret_cast<u32x4*>(dx)[oct] = pack8(o);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float xd = raw[e] * ks[e];
#pragma unroll
        for (int k = 0; k < PCLS; ++k) wacc[k][e] = fmaf(dk[k], xd, wacc[k][e]);
      }
      if (cg == 0) {
#pragma unroll
        for (int k = 0; k < PCLS; ++k) bacc[k] += dk[k];
      }
    }
  }
  // ---- lanes of a wave that share an octet (lane bits >= LOG2CG), then the four waves: fixed order, reproducible ----
#pragma unroll
  for (int k = 0; k < PCLS; ++k) {
#pragma unroll
    for (int m = CG; m < 64; m <<= 1) bacc[k] += __shfl_xor(bacc[k], m);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float v = wacc[k][e];
#pragma unroll
      for (int m = CG; m < 64; m <<= 1) v += __shfl_xor(v, m);
      wacc[k][e] = v;
    }
  }
  __syncthreads();
  constexpr int ROW = PCLS * C + PCLS;
  if (lane < CG) {
#pragma unroll
    for (int k = 0; k < PCLS; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) red[wave * ROW + k * C + cg * 8 + e] = wacc[k][e];
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < PCLS; ++k) red[wave * ROW + PCLS * C + k] = bacc[k];
  }
  __syncthreads();
  const int NW = n_cls * C;
  float* dst = partial + static_cast<long>(blockIdx.x) * (NW + n_cls);
  for (int i = tid; i < NW; i += kThreads) dst[i] = (red[i] + red[ROW + i]) + (red[2 * ROW + i] + red[3 * ROW + i]);
  if (tid < n_cls)
    dst[NW + tid] = (red[PCLS * C + tid] + red[ROW + PCLS * C + tid]) + (red[2 * ROW + PCLS * C + tid] + red[3 * ROW + PCLS * C + tid]);
}

// ------------------------------------------------------------------ backward of the ensemble mean, one head per launch
// head_bwd_vec_kernel's 64-pixel tiles, grid and partial rows, without `out`: the mean's forward never wrote the head maps,
// so the tile of x that the weight gradient needs in LDS anyway is staged FIRST and the logits are recomputed from it.
//   1. x tile -> LDS as fp32 [64][C+1]            (VEC: 16-byte pieces -- fp32 quads / bf16 octets; else scalar loads)
//   2. lane = pixel, wave = class (and class + 4): z = bias + x . w over the LDS row (stride C+1: conflict-free; the weight
//      row is a broadcast read), s = 1 / (1 + exp(-z)), dl = (d_out * inv_heads) * (s * (1 - s)) -> LDS [64][8]
//      (s (1 - s) as one fma: three roundings in dl beside the one in inv_heads)
//   3. dx = W^T dl (+ old dx, ReLU gate of x) written back in the pieces of step 1
//   4. dW[k, c] += sum_p dl[p, k] xs[p, c]: all 256 threads, two pixel halves per (k, c); db likewise
// T = float or bf16_t (storage of x and dx).  64-bit element offsets.  LDS: xs | dl | W [8][C] | scratch [2][n_cls*C].
template <typename T, bool VEC>
__global__ __launch_bounds__(kThreads, 4) void heads_mean_bwd_kernel(const float* __restrict__ d_out, const T* __restrict__ x,
                                                                  const float* __restrict__ weight,
                                                                  const float* __restrict__ bias, long pixels, int HW, int C,
                                                                  int n_cls, float inv_heads, T* __restrict__ dx,
                                                                  int accumulate, int gate_x, float* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) float hmb[];
  constexpr int GW = sizeof(T) == 2 ? 8 : 4;  // elements of a 16-byte piece
  const int XS = C + 1, NW = n_cls * C, gn = C / GW;
  float* xs = hmb;
  float* dl = xs + 64 * XS;
  float* wsm = dl + 64 * kHeadMaxCls;
  float* scratch = wsm + kHeadMaxCls * C;
  const int tid = threadIdx.x;
  for (int i = tid; i < NW; i += kThreads) wsm[i] = weight[i];
  constexpr int kMaxPairs = (kHeadMaxCls * kHeadMaxC + 127) / 128;  // (k, c) pairs per thread
  float wacc[kMaxPairs];
#pragma unroll
  for (int q = 0; q < kMaxPairs; ++q) wacc[q] = 0.f;
  float bacc = 0.f;
  const int pair0 = tid & 127, half = tid >> 7;
  const long n_tiles = (pixels + 63) / 64;
  for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long p0 = tile * 64;
    __syncthreads();  // (the weights are in LDS; the previous tile's readers of xs and dl are done)
    if constexpr (VEC) {
      for (int it = tid; it < 64 * gn; it += kThreads) {
        const int pl = it / gn, g = it - pl * gn;
        const long p = p0 + pl;
        float f[GW];
#pragma unroll
        for (int e = 0; e < GW; ++e) f[e] = 0.f;
        if (p < pixels) {
          if constexpr (GW == 8) {
            unpack8(*reinterpret_cast<const u32x4*>(x + p * C + 8 * g), f);
          } else {
            const f32x4 v = *reinterpret_cast<const f32x4*>(x + p * C + 4 * g);
#pragma unroll
            for (int e = 0; e < 4; ++e) f[e] = v[e];
          }
        }
        float* xd = &xs[pl * XS + GW * g];
#pragma unroll
        for (int e = 0; e < GW; ++e) xd[e] = f[e];
      }
    } else {
      for (int it = tid; it < 64 * C; it += kThreads) {
        const int pl = it / C, c = it - pl * C;
        const long p = p0 + pl;
        xs[pl * XS + c] = (p < pixels) ? head_feature(x + p * C + c) : 0.f;
      }
    }
    __syncthreads();
    for (int it = tid; it < 64 * n_cls; it += kThreads) {
      const int pl = it & 63, k = it >> 6;
      const long p = p0 + pl;
      float v = 0.f;
      if (p < pixels) {
        float z = bias[k];
        const float* xr = &xs[pl * XS];
        const float* wr = &wsm[k * C];
        for (int c = 0; c < C; ++c) z = fmaf(xr[c], wr[c], z);
        const float s = 1.0f / (1.0f + expf(-z));
        const long n = p / HW, hw = p - n * HW;
        v = (d_out[(n * n_cls + k) * HW + hw] * inv_heads) * fmaf(-s, s, s);  // s (1 - s) = s - s^2, rounded once
      }
      dl[pl * kHeadMaxCls + k] = v;
    }
    __syncthreads();
    if constexpr (VEC) {
      for (int it = tid; it < 64 * gn; it += kThreads) {
        const int pl = it / gn, g = it - pl * gn;
        const long p = p0 + pl;
        if (p >= pixels) continue;
        float o[GW];
#pragma unroll
        for (int e = 0; e < GW; ++e) o[e] = 0.f;
#pragma unroll
        for (int k = 0; k < kHeadMaxCls; ++k) {
          if (k < n_cls) {
            const float dk = dl[pl * kHeadMaxCls + k];
#pragma unroll
            for (int e = 0; e < GW; ++e) o[e] = fmaf(wsm[k * C + GW * g + e], dk, o[e]);
          }
        }
        T* dst = dx + p * C + GW * g;
        if (accumulate) {
          if constexpr (GW == 8) {
            float old[8];
            unpack8(*reinterpret_cast<const u32x4*>(dst), old);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] += old[e];
          } else {
            const f32x4 old = *reinterpret_cast<const f32x4*>(dst);
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] += old[e];
          }
        }
        if (gate_x) {
          const float* xr = &xs[pl * XS + GW * g];
#pragma unroll
          for (int e = 0; e < GW; ++e) o[e] = (xr[e] > 0.f) ? o[e] : 0.f;
        }
        if constexpr (GW == 8) {
          *reinterpret_cast<u32x4*>(dst) = pack8(o);
        } else {
          *reinterpret_cast<f32x4*>(dst) = f32x4{o[0], o[1], o[2], o[3]};
        }
      }
    } else {
      for (int it = tid; it < 64 * C; it += kThreads) {
        const int pl = it / C, c = it - pl * C;
        const long p = p0 + pl;
        if (p >= pixels) continue;
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < kHeadMaxCls; ++k)
          if (k < n_cls) s = fmaf(wsm[k * C + c], dl[pl * kHeadMaxCls + k], s);
        if (accumulate) s += head_feature(dx + p * C + c);
        if (gate_x) s = (xs[pl * XS + c] > 0.f) ? s : 0.f;
        dx[p * C + c] = s;
      }
    }
#pragma unroll
    for (int q = 0; q < kMaxPairs; ++q) {
      const int idx = pair0 + q * 128;
      if (idx < NW) {
        const int k = idx / C, c = idx - k * C;
        float s = 0.f;
#pragma unroll 4
        for (int pl = 32 * half; pl < 32 * half + 32; ++pl) s += dl[pl * kHeadMaxCls + k] * xs[pl * XS + c];
        wacc[q] += s;
      }
    }
    if (tid < n_cls) {
      float s = 0.f;
      for (int pl = 0; pl < 64; ++pl) s += dl[pl * kHeadMaxCls + tid];
      bacc += s;
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < kMaxPairs; ++q) {
    const int idx = pair0 + q * 128;
    if (idx < NW) scratch[half * NW + idx] = wacc[q];
  }
  __syncthreads();
  float* dst = partial + static_cast<long>(blockIdx.x) * (NW + n_cls);
  for (int i = tid; i < NW; i += kThreads) dst[i] = scratch[i] + scratch[NW + i];
  if (tid < n_cls) dst[NW + tid] = bacc;
}


// ------------------------------------------------------------------ run-time triple -> instantiation
// f(std::integral_constant<int, V>{}) for the V of the list that equals v; false when none does
template <int... Vs, class F>
inline bool with_const(int v, F&& f) {
  return ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}
// f(L, D, PC) as integral constants for s's (log2g, drop, pcls).  Every launcher names, in an `if constexpr`, the
// coordinates its kernel is built for: nothing else is instantiated.
template <class F>
inline void with_head_instance(const HeadSel& s, F&& f) {
  with_const<0, 1, 2, 3, 4, 5>(s.log2g, [&](auto l) {
    with_const<0, 1, 2>(s.drop, [&](auto d) { with_const<4, 6, 8>(s.pcls, [&](auto pc) { f(l, d, pc); }); });
  });
}

inline unsigned low4(const void* p) { return static_cast<unsigned>(reinterpret_cast<uintptr_t>(p) & 15); }

HeadQuery head_query(HeadOp op, bool bf16, int N, int H, int W, int C, int n_cls, float p_drop, const void* x,
                     const void* weight, const void* dx, const void* mask) {
  HeadQuery q{};
  q.op = op, q.bf16 = bf16, q.N = N, q.H = H, q.W = W, q.C = C, q.n_cls = n_cls, q.p_drop = p_drop;
  q.has_mask = mask != nullptr;
  q.x_lo = low4(x), q.weight_lo = low4(weight), q.dx_lo = low4(dx), q.mask_lo = low4(mask);
  return q;
}

// the mean's query: false for a descriptor that cannot be read (head count, null pointers)
bool heads_mean_query(const unetpp_heads_mean* heads, bool bf16, int N, int H, int W, int C, int n_cls, HeadQuery& q) {
  if (!heads || heads->n_heads < 1 || heads->n_heads > UNETPP_MAX_HEADS) return false;
  q = head_query(HEADS_MEAN, bf16, N, H, W, C, n_cls, 0.f, nullptr, nullptr, nullptr, nullptr);
  q.n_heads = heads->n_heads;
  for (int h = 0; h < heads->n_heads; ++h) {
    const unetpp_head_src& s = heads->head[h];
    if (!s.x || !s.weight || !s.bias) return false;
    q.x_lo |= low4(s.x);
    q.weight_lo |= low4(s.weight);
  }
  return true;
}

// the query of the mean's backward: the forward's descriptor and the gradient descriptor must describe the same heads
bool heads_mean_bwd_query(const unetpp_heads_mean* heads, const unetpp_heads_mean_grad* grads, bool bf16, int N, int H, int W,
                          int C, int n_cls, HeadQuery& q) {
  if (!grads || !heads_mean_query(heads, bf16, N, H, W, C, n_cls, q) || grads->n_heads != heads->n_heads) return false;
  q.op = HEADS_MEAN_BWD;
  for (int h = 0; h < grads->n_heads; ++h) {
    const unetpp_head_grad& g = grads->head[h];
    if (!g.dx || !g.partial) return false;
    q.dx_lo |= low4(g.dx);
  }
  return true;
}

template <typename T>
int heads_mean_bwd_launch(const unetpp_heads_mean* heads, const unetpp_heads_mean_grad* grads, const float* d_out_nchw, int N,
                          int H, int W, int C, int n_cls, void* stream) {
  HeadQuery q;
  HeadSel s;
  if (!d_out_nchw || !heads_mean_bwd_query(heads, grads, sizeof(T) == 2, N, H, W, C, n_cls, q)) return UNETPP_EINVAL;
  const int rc = head_select(q, 0, s);
  if (rc != UNETPP_OK) return rc;
  const long pixels = static_cast<long>(N) * H * W;
  const float inv_heads = 1.0f / static_cast<float>(heads->n_heads);
  note_kernel(s.label);
  for (int h = 0; h < heads->n_heads; ++h) {  // one launch per head: every head's tile goes through the same LDS layout
    const unetpp_head_src& src = heads->head[h];
    const unetpp_head_grad& g = grads->head[h];
    if constexpr (sizeof(T) == 4) {  // (bf16 has the octet form only: head_select refuses the rest)
      if (s.form == HEAD_GENERIC) {
        hipLaunchKernelGGL((heads_mean_bwd_kernel<T, false>), dim3(s.grid), dim3(s.block), s.lds, ST(stream), d_out_nchw,
                           static_cast<const T*>(src.x), src.weight, src.bias, pixels, H * W, C, n_cls, inv_heads,
                           static_cast<T*>(g.dx), g.accumulate, g.gate_x, g.partial);
        continue;
      }
    }
      hipLaunchKernelGGL((heads_mean_bwd_kernel<T, true>), dim3(s.grid), dim3(s.block), s.lds, ST(stream), d_out_nchw,
                         static_cast<const T*>(src.x), src.weight, src.bias, pixels, H * W, C, n_cls, inv_heads,
                         static_cast<T*>(g.dx), g.accumulate, g.gate_x, g.partial);
  }
  return launch_status();
}

}  // namespace
}  // namespace unetpp

using namespace unetpp;

extern "C" int unetpp_head_fwd(const float* x, const float* weight, const float* bias, int32_t N, int32_t H, int32_t W,
                               int32_t C, int32_t n_cls, float p_drop, uint64_t seed, const uint8_t* mask, const uint64_t* seed_dev,
                               float* out_nchw, void* stream) {
  if (!x || !weight || !bias || !out_nchw) return UNETPP_EINVAL;
  HeadSel s;
  const int rc = head_select(head_query(HEAD_FWD, false, N, H, W, C, n_cls, p_drop, x, weight, nullptr, mask), 0, s);
  if (rc != UNETPP_OK) return rc;
  const long pixels = static_cast<long>(N) * H * W;
  const float keep_scale = 1.0f / (1.0f - p_drop);
  note_kernel(s.label);
  if (s.form == HEAD_STREAM)
    with_head_instance(s, [&](auto l, auto d, auto pc) {
      constexpr int L = decltype(l)::value, D = decltype(d)::value, PC = decltype(pc)::value;
      if constexpr (L >= 2 && PC != 6 && PC <= (1 << L))
        hipLaunchKernelGGL((head_fwd_stream_kernel<L, PC, D>), dim3(s.grid), dim3(s.block), 0, ST(stream), x, weight, bias,
                           static_cast<unsigned>(pixels), static_cast<unsigned>(H * W), n_cls, keep_scale,
                           keep_threshold(p_drop), seed, mask, seed_dev, out_nchw);
    });
  else if (s.form == HEAD_TILED)
    hipLaunchKernelGGL(head_fwd_tiled_kernel, dim3(s.grid), dim3(s.block), s.lds, ST(stream), x, weight, bias, pixels, H * W,
                       C, n_cls, keep_scale, keep_threshold(p_drop), seed, mask, seed_dev, s.drop != 0, out_nchw);
  else
    hipLaunchKernelGGL(head_fwd_kernel, dim3(s.grid), dim3(s.block), 0, ST(stream), x, weight, bias, pixels, H * W, C, n_cls,
                       keep_scale, keep_threshold(p_drop), seed, mask, seed_dev, s.drop != 0, out_nchw);
  return launch_status();
}

extern "C" int unetpp_head_fwd_bf16(const void* x, const float* weight, const float* bias, int32_t N, int32_t H, int32_t W,
                                    int32_t C, int32_t n_cls, float p_drop, uint64_t seed, const uint8_t* mask, const uint64_t* seed_dev,
                                    float* out_nchw, void* stream) {
  if (!x || !weight || !bias || !out_nchw) return UNETPP_EINVAL;
  HeadSel s;
  const int rc = head_select(head_query(HEAD_FWD, true, N, H, W, C, n_cls, p_drop, x, weight, nullptr, mask), 0, s);
  if (rc != UNETPP_OK) return rc;
  const long pixels = static_cast<long>(N) * H * W;
  note_kernel(s.label);
  with_head_instance(s, [&](auto l, auto d, auto pc) {
    constexpr int L = decltype(l)::value, D = decltype(d)::value, PC = decltype(pc)::value;
    if constexpr (L <= 4)
      hipLaunchKernelGGL((head_fwd_bf16_kernel<L, D, PC>), dim3(s.grid), dim3(s.block), 0, ST(stream),
                         static_cast<const bf16_t*>(x), weight, bias, pixels, H * W, n_cls, 1.0f / (1.0f - p_drop),
                         keep_threshold(p_drop), seed, mask, seed_dev, out_nchw);
  });
  return launch_status();
}

/* ---- ensemble head: mean of the first n_heads sigmoid heads in one pass (eval only) ---- */
extern "C" int unetpp_heads_mean_fwd(const unetpp_heads_mean* heads, int32_t N, int32_t H, int32_t W, int32_t C,
                                     int32_t n_cls, float* out_nchw, void* stream) {
  HeadQuery q;
  HeadSel s;
  if (!out_nchw || !heads_mean_query(heads, false, N, H, W, C, n_cls, q)) return UNETPP_EINVAL;
  const int rc = head_select(q, 0, s);
  if (rc != UNETPP_OK) return rc;
  const long pixels = static_cast<long>(N) * H * W;
  note_kernel(s.label);
  if (s.form == HEAD_STREAM)
    with_head_instance(s, [&](auto l, auto d, auto pc) {
      constexpr int L = decltype(l)::value, D = decltype(d)::value, PC = decltype(pc)::value;
      if constexpr (L >= 2 && D == 0 && PC != 6 && PC <= (1 << L))
        hipLaunchKernelGGL((heads_mean_stream_kernel<L, PC>), dim3(s.grid), dim3(s.block), 0, ST(stream), *heads,
                           static_cast<unsigned>(pixels), static_cast<unsigned>(H * W), n_cls, out_nchw);
    });
  else
    hipLaunchKernelGGL(heads_mean_general_kernel<float>, dim3(s.grid), dim3(s.block), 0, ST(stream), *heads, pixels, H * W, C,
                       n_cls, out_nchw);
  return launch_status();
}

extern "C" int unetpp_heads_mean_fwd_bf16(const unetpp_heads_mean* heads, int32_t N, int32_t H, int32_t W, int32_t C,
                                          int32_t n_cls, float* out_nchw, void* stream) {
  HeadQuery q;
  HeadSel s;
  if (!out_nchw || !heads_mean_query(heads, true, N, H, W, C, n_cls, q)) return UNETPP_EINVAL;
  const int rc = head_select(q, 0, s);
  if (rc != UNETPP_OK) return rc;
  const long pixels = static_cast<long>(N) * H * W;
  note_kernel(s.label);
  if (s.form == HEAD_OCTET)
    with_head_instance(s, [&](auto l, auto d, auto pc) {
      constexpr int L = decltype(l)::value, D = decltype(d)::value, PC = decltype(pc)::value;
      if constexpr (L <= 4 && D == 0)
        hipLaunchKernelGGL((heads_mean_bf16_kernel<L, PC>), dim3(s.grid), dim3(s.block), s.lds, ST(stream), *heads, pixels,
                           H * W, n_cls, out_nchw);
    });
  else
    hipLaunchKernelGGL(heads_mean_general_kernel<bf16_t>, dim3(s.grid), dim3(s.block), 0, ST(stream), *heads, pixels,
                       H * W, C, n_cls, out_nchw);
  return launch_status();
}

/* ---- backward of the ensemble head: one launch per head, the head maps recomputed from the staged features ---- */
extern "C" int unetpp_heads_mean_bwd(const unetpp_heads_mean* heads, const unetpp_heads_mean_grad* grads,
                                     const float* d_out_nchw, int32_t N, int32_t H, int32_t W, int32_t C, int32_t n_cls,
                                     void* stream) {
  return heads_mean_bwd_launch<float>(heads, grads, d_out_nchw, N, H, W, C, n_cls, stream);
}

extern "C" int unetpp_heads_mean_bwd_bf16(const unetpp_heads_mean* heads, const unetpp_heads_mean_grad* grads,
                                          const float* d_out_nchw, int32_t N, int32_t H, int32_t W, int32_t C,
                                          int32_t n_cls, void* stream) {
  return heads_mean_bwd_launch<bf16_t>(heads, grads, d_out_nchw, N, H, W, C, n_cls, stream);
}

extern "C" int64_t unetpp_head_bwd_blocks(int64_t pixels) {  // rows of `partial`; head_select sizes both backward grids alike
  if (pixels < 1) return 0;
  const long tiles = (pixels + 63) / 64;
  return tiles < 4096 ? tiles : 4096;
}

extern "C" int unetpp_head_bwd(const float* d_out_nchw, const float* out_nchw, const float* x, const float* weight,
                               int32_t N, int32_t H, int32_t W, int32_t C, int32_t n_cls, float p_drop, uint64_t seed,
                               const uint8_t* mask, const uint64_t* seed_dev, float* dx, int32_t accumulate, int32_t gate_x, float* partial,
                               void* stream) {
  if (!d_out_nchw || !out_nchw || !x || !weight || !dx || !partial) return UNETPP_EINVAL;
  HeadSel s;
  const int rc = head_select(head_query(HEAD_BWD, false, N, H, W, C, n_cls, p_drop, x, weight, dx, mask), 0, s);
  if (rc != UNETPP_OK) return rc;
  const long pixels = static_cast<long>(N) * H * W;
  const float keep_scale = 1.0f / (1.0f - p_drop);
  note_kernel(s.label);
  if (s.form == HEAD_POW2)
    with_head_instance(s, [&](auto l, auto d, auto pc) {
      constexpr int L = decltype(l)::value, D = decltype(d)::value, PC = decltype(pc)::value;
      if constexpr (L >= 1 && PC != 6)
        hipLaunchKernelGGL((head_bwd_pow2_kernel<L, D, PC>), dim3(s.grid), dim3(s.block), s.lds, ST(stream), d_out_nchw,
                           out_nchw, x, weight, static_cast<unsigned>(pixels), static_cast<unsigned>(H * W), n_cls,
                           keep_scale, keep_threshold(p_drop), seed, mask, seed_dev, dx, accumulate, gate_x, partial);
    });
  else if (s.form == HEAD_VEC)
    hipLaunchKernelGGL(head_bwd_vec_kernel, dim3(s.grid), dim3(s.block), s.lds, ST(stream), d_out_nchw, out_nchw, x, weight,
                       pixels, H * W, C, n_cls, keep_scale, keep_threshold(p_drop), seed, mask, seed_dev, s.drop != 0, dx,
                       accumulate, gate_x, partial);
  else
    hipLaunchKernelGGL(head_bwd_kernel, dim3(s.grid), dim3(s.block), 0, ST(stream), d_out_nchw, out_nchw, x, weight, pixels,
                       H * W, C, n_cls, keep_scale, keep_threshold(p_drop), seed, mask, seed_dev, s.drop != 0, dx,
                       accumulate, gate_x, partial);
  return launch_status();
}

/* ---- one head of a training step in one pass: forward, gradient of the mean focal loss over n_heads, backward ---- */
extern "C" int unetpp_head_train(const float* x, const float* weight, const float* bias, const float* target_nchw, int32_t N,
                                 int32_t H, int32_t W, int32_t C, int32_t n_cls, float p_drop, uint64_t seed,
                                 const uint8_t* mask, const uint64_t* seed_dev, int64_t rows, float gamma, int32_t n_heads,
                                 float* out_nchw, float* dx, int32_t gate_x, float* partial, void* stream) {
  if (!x || !weight || !bias || !target_nchw || !out_nchw || !dx || !partial || rows < 1) return UNETPP_EINVAL;
  HeadQuery q = head_query(HEAD_TRAIN, false, N, H, W, C, n_cls, p_drop, x, weight, dx, mask);
  q.n_heads = n_heads;
  HeadSel s;
  const int rc = head_select(q, 0, s);
  if (rc != UNETPP_OK) return rc;
  const long pixels = static_cast<long>(N) * H * W;
  const float keep_scale = 1.0f / (1.0f - p_drop);
  bool launched = false;
  with_head_instance(s, [&](auto l, auto d, auto pc) {
    constexpr int L = decltype(l)::value, D = decltype(d)::value, PC = decltype(pc)::value;
    if constexpr (L >= 2 && PC != 6 && PC <= (1 << L)) {
      hipLaunchKernelGGL((head_train_pow2_kernel<L, D, PC>), dim3(s.grid), dim3(s.block), s.lds, ST(stream), x, weight, bias,
                         target_nchw, static_cast<unsigned>(pixels), static_cast<unsigned>(H * W), n_cls, keep_scale,
                         keep_threshold(p_drop), seed, mask, seed_dev, gamma, 1.f / static_cast<float>(rows),
                         1.0f / static_cast<float>(n_heads), out_nchw, dx, gate_x, partial);
      launched = true;
    }
  });
  if (!launched) return UNETPP_EINVAL;  // (head_select accepts nothing without an instance)
  note_kernel(s.label);
  return launch_status();
}

/* ---- Monte-Carlo dropout at one head: mean and variance of `samples` dropout draws in one pass over x ---- */
extern "C" int unetpp_head_mc(const float* x, const float* weight, const float* bias, int32_t N, int32_t H, int32_t W,
                              int32_t C, int32_t n_cls, float p_drop, uint64_t seed, const uint64_t* seed_dev,
                              int32_t samples, float* mean_nchw, float* var_nchw, void* stream) {
  if (!x || !weight || !bias || !mean_nchw || !var_nchw) return UNETPP_EINVAL;
  HeadSel s;
  const int rc = head_mc_select(N, H, W, C, n_cls, p_drop, samples, low4(x), low4(weight), s);
  if (rc != UNETPP_OK) return rc;
  const long pixels = static_cast<long>(N) * H * W;
  const float keep_scale = 1.0f / (1.0f - p_drop);
  bool launched = false;
  with_const<2, 3, 4, 5>(s.log2g, [&](auto l) {
    with_const<4, 8>(s.pcls, [&](auto pc) {
      constexpr int L = decltype(l)::value, PC = decltype(pc)::value;
      if constexpr (PC <= (1 << L)) {
        hipLaunchKernelGGL((head_mc_kernel<L, PC>), dim3(s.grid), dim3(s.block), s.lds, ST(stream), x, weight, bias,
                           static_cast<unsigned>(pixels), static_cast<unsigned>(H * W), n_cls, keep_scale,
                           keep_threshold(p_drop), seed, seed_dev, samples, mean_nchw, var_nchw);
        launched = true;
      }
    });
  });
  if (!launched) return UNETPP_EINVAL;  // (head_mc_select accepts nothing without an instance)
  note_kernel(s.label);
  return launch_status();
}

extern "C" int unetpp_head_bwd_bf16(const float* d_out_nchw, const float* out_nchw, const void* x, const float* weight,
                                    int32_t N, int32_t H, int32_t W, int32_t C, int32_t n_cls, float p_drop, uint64_t seed,
                                    const uint8_t* mask, const uint64_t* seed_dev, void* dx, int32_t accumulate, int32_t gate_x, float* partial,
                                    void* stream) {
  if (!d_out_nchw || !out_nchw || !x || !weight || !dx || !partial) return UNETPP_EINVAL;
  HeadQuery q = head_query(HEAD_BWD, true, N, H, W, C, n_cls, p_drop, x, weight, dx, mask);
  q.wgs_per_cu = opt_value(OPT_HEAD_WGS_PER_CU, 4);
  HeadSel s;
  const int rc = head_select_with(q, [] { return device_cu_count(); }, s);
  if (rc != UNETPP_OK) return rc;
  note_kernel(s.label);
  with_head_instance(s, [&](auto l, auto d, auto pc) {
    constexpr int L = decltype(l)::value, D = decltype(d)::value, PC = decltype(pc)::value;
    if constexpr (L <= 4)
      hipLaunchKernelGGL((head_bwd_bf16_kernel<L, D, PC>), dim3(s.grid), dim3(s.block), s.lds, ST(stream), d_out_nchw,
                         out_nchw, static_cast<const bf16_t*>(x), weight, static_cast<unsigned>(static_cast<long>(N) * H * W),
                         static_cast<unsigned>(H * W), n_cls, 1.0f / (1.0f - p_drop), keep_threshold(p_drop), seed, mask,
                         seed_dev, static_cast<bf16_t*>(dx), accumulate, gate_x, partial, s.active);
  });
  return launch_status();
}
