// HBM-bound companions of the bf16 MFMA kernels (BASELINE configs[3]/[4]): every activation tensor is bf16 NHWC in
// HBM and is touched in 16-byte pieces = 8 channels of one pixel; the arithmetic, the BatchNorm sums and all
// parameter gradients are fp32.
//   unetpp_affine_relu_pool_bf16   BatchNorm apply + ReLU (+ 2x2 max-pool with argmax bytes) of a conv output
//   unetpp_bn_bwd_reduce_bf16      BatchNorm + ReLU backward, pass 1: per-workgroup (sum g, sum g*xhat) partials
//   unetpp_bn_bwd_apply_bf16       pass 2: dy = gamma*invstd*(g - dbeta/M - xhat*dgamma/M)
//                                  (both passes can route the gradient of the node's max-pooled copy to the window
//                                  argmax while they read d_act: no scatter pass, no read-modify-write)
//   unetpp_maxpool_bwd_bf16        max-pool gradient routed to the window argmax and added to d_act, optionally followed
//                                  by the ReLU mask of the node (is_batchnorm=False: no BatchNorm backward to route through)
//   unetpp_bilinear2x_fwd_bf16 / unetpp_bilinear2x_bwd_bf16   the is_deconv=False up path (align_corners=True), fp32
//                                  interpolation of bf16 values; backward in gather form, optional accumulate + ReLU mask
// (The bf16 heads sit beside their fp32 twins in heads.hip.)
#include "bf16_common.h"
#include "common.h"
#include "lds_asm.h"
#include "stream_select.h"

namespace unetpp {
namespace {

__device__ __forceinline__ void affine8(float (&f)[8], const float* scale, const float* shift, int c, int relu) {
  if (scale != nullptr) {
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = fmaf(f[e], scale[c + e], shift[c + e]);
  }
  if (relu) {
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = relu_keep_nan(f[e]);
  }
}

// thread = (pixel, channel octet)
__global__ __launch_bounds__(kThreads) void affine_relu_bf16_kernel(const bf16_t* __restrict__ y, const float* scale,
                                                                    const float* shift, int relu, long items, int CG,
                                                                    bf16_t* __restrict__ act) {
  for (long i = blockIdx.x * static_cast<long>(kThreads) + threadIdx.x; i < items;
       i += static_cast<long>(gridDim.x) * kThreads) {
    const int c = static_cast<int>(i % CG) * 8;
    float f[8];
    unpack8(reinterpret_cast<const u32x4*>(y)[i], f);
    affine8(f, scale, shift, c, relu);
    reinterpret_cast<u32x4*>(act)[i] = pack8(f);
  }
}

// thread = (2x2 window, channel octet): four 16-byte loads, four optional stores of the activation, one store of the
// pooled octet and 8 argmax bytes.  The winner is the first maximum in scan order of the ROUNDED (stored) values.
__global__ __launch_bounds__(kThreads) void affine_relu_pool_bf16_kernel(const bf16_t* __restrict__ y, const float* scale,
                                                                         const float* shift, int relu, int N, int H, int W,
                                                                         int CG, bf16_t* __restrict__ act,
                                                                         bf16_t* __restrict__ pooled,
                                                                         uint8_t* __restrict__ pool_idx) {
  const int Hp = H >> 1, Wp = W >> 1;
  const long items = static_cast<long>(N) * Hp * Wp * CG;
  for (long i = blockIdx.x * static_cast<long>(kThreads) + threadIdx.x; i < items;
       i += static_cast<long>(gridDim.x) * kThreads) {
    const unsigned iu = static_cast<unsigned>(i);  // items < 2^31 (launcher)
    const int cg = static_cast<int>(iu % static_cast<unsigned>(CG));
    unsigned r = iu / static_cast<unsigned>(CG);
    const int xp = static_cast<int>(r % static_cast<unsigned>(Wp));
    r /= static_cast<unsigned>(Wp);
    const int yp = static_cast<int>(r % static_cast<unsigned>(Hp));
    const long n = r / static_cast<unsigned>(Hp);
    const long base = ((n * H + 2 * yp) * W + 2 * xp) * CG + cg;  // in octets
    const long offs[4] = {base, base + CG, base + static_cast<long>(W) * CG, base + static_cast<long>(W) * CG + CG};
    float best[8];
    unsigned bi[8];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float f[8];
      unpack8(reinterpret_cast<const u32x4*>(y)[offs[q]], f);
      affine8(f, scale, shift, cg * 8, relu);
      const u32x4 packed = pack8(f);
      if (act != nullptr) reinterpret_cast<u32x4*>(act)[offs[q]] = packed;
      unpack8(packed, f);  // compare what is stored
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if (q == 0 || pool_takes(f[e], best[e])) {
          best[e] = f[e];
          bi[e] = q;
        }
      }
    }
    reinterpret_cast<u32x4*>(pooled)[i] = pack8(best);
    reinterpret_cast<u32x2*>(pool_idx)[i] = u32x2{bi[0] | (bi[1] << 8) | (bi[2] << 16) | (bi[3] << 24),
                                                  bi[4] | (bi[5] << 8) | (bi[6] << 16) | (bi[7] << 24)};
  }
}

// gradient of the activation at (pixel i, octet): d_act (+ the pooled gradient when this pixel won its window)
__device__ __forceinline__ void load_grad8(const bf16_t* d_act, const bf16_t* d_pooled, const uint8_t* pool_idx, long i,
                                           int CG, int H, int W, float (&g)[8]) {
  unpack8(reinterpret_cast<const u32x4*>(d_act)[i], g);
  if (d_pooled != nullptr) {  // 32-bit index arithmetic: items < 2^31 (launchers); CG is a power of two
    const unsigned iu = static_cast<unsigned>(i), ucg = static_cast<unsigned>(CG);
    const unsigned cg = iu & (ucg - 1u);
    unsigned r = iu / ucg;
    const unsigned x = r % static_cast<unsigned>(W);
    r /= static_cast<unsigned>(W);
    const unsigned y = r % static_cast<unsigned>(H);
    const unsigned n = r / static_cast<unsigned>(H);
    const unsigned wi = ((n * (static_cast<unsigned>(H) >> 1) + (y >> 1)) * (static_cast<unsigned>(W) >> 1) + (x >> 1)) * ucg + cg;
    const unsigned pos = (y & 1u) * 2u + (x & 1u);
    const u32x2 ib = reinterpret_cast<const u32x2*>(pool_idx)[wi];
    float dp[8];
    unpack8(reinterpret_cast<const u32x4*>(d_pooled)[wi], dp);
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (((ib[e >> 2] >> (8 * (e & 3))) & 0xffu) == pos) g[e] += dp[e];
  }
}

// The grid stride is a multiple of CG (a power of two <= 256), so a thread keeps one channel octet.
__global__ __launch_bounds__(kThreads) void bn_bwd_reduce_bf16_kernel(const bf16_t* __restrict__ d_act,
                                                                      const bf16_t* __restrict__ y, const float* scale,
                                                                      const float* shift, const float* mean,
                                                                      const float* invstd, const bf16_t* d_pooled,
                                                                      const uint8_t* pool_idx, long items, int CG, int H,
                                                                      int W, float* __restrict__ partial) {
  __shared__ float sm[kThreads][17];
  const long first = blockIdx.x * static_cast<long>(kThreads) + threadIdx.x;
  const int c = static_cast<int>(first % CG) * 8;
  float sc[8], sh[8], mu[8], is[8], s1[8], s2[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    sc[e] = scale[c + e];
    sh[e] = shift[c + e];
    mu[e] = mean[c + e];
    is[e] = invstd[c + e];
    s1[e] = 0.f;
    s2[e] = 0.f;
  }
  for (long i = first; i < items; i += static_cast<long>(gridDim.x) * kThreads) {
    float g[8], v[8];
    load_grad8(d_act, d_pooled, pool_idx, i, CG, H, W, g);
    unpack8(reinterpret_cast<const u32x4*>(y)[i], v);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float gg = (fmaf(v[e], sc[e], sh[e]) > 0.f) ? g[e] : 0.f;
      s1[e] += gg;
      s2[e] += gg * (v[e] - mu[e]) * is[e];
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    sm[threadIdx.x][2 * e] = s1[e];
    sm[threadIdx.x][2 * e + 1] = s2[e];
  }
  __syncthreads();
  const int C = CG * 8;
  for (int cc = threadIdx.x; cc < C; cc += kThreads) {  // kThreads % CG == 0: thread t holds octet t % CG
    const int cg = cc >> 3, e = cc & 7;
    float a = 0.f, b = 0.f;
    for (int t = cg; t < kThreads; t += CG) {  // fixed order
      a += sm[t][2 * e];
      b += sm[t][2 * e + 1];
    }
    partial[(static_cast<long>(blockIdx.x) * C + cc) * 2 + 0] = a;
    partial[(static_cast<long>(blockIdx.x) * C + cc) * 2 + 1] = b;
  }
}

__global__ __launch_bounds__(kThreads) void bn_bwd_apply_bf16_kernel(const bf16_t* __restrict__ d_act,
                                                                     const bf16_t* __restrict__ y, const float* scale,
                                                                     const float* shift, const float* mean,
                                                                     const float* invstd, const float* gamma,
                                                                     const float* dgamma, const float* dbeta,
                                                                     const bf16_t* d_pooled, const uint8_t* pool_idx,
                                                                     float inv_count, long items, int CG, int H, int W,
                                                                     bf16_t* __restrict__ dy) {
  for (long i = blockIdx.x * static_cast<long>(kThreads) + threadIdx.x; i < items;
       i += static_cast<long>(gridDim.x) * kThreads) {
    const int c = static_cast<int>(static_cast<unsigned>(i) & static_cast<unsigned>(CG - 1)) * 8;  // CG is a power of two
    float g[8], v[8], out[8];
    load_grad8(d_act, d_pooled, pool_idx, i, CG, H, W, g);
    unpack8(reinterpret_cast<const u32x4*>(y)[i], v);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float gg = (fmaf(v[e], scale[c + e], shift[c + e]) > 0.f) ? g[e] : 0.f;
      const float xhat = (v[e] - mean[c + e]) * invstd[c + e];
      out[e] = gamma[c + e] * invstd[c + e] * (gg - dbeta[c + e] * inv_count - xhat * dgamma[c + e] * inv_count);
    }
    reinterpret_cast<u32x4*>(dy)[i] = pack8(out);  // may alias d_act: the item was read by this thread above
  }
}

// BatchNorm backward of a FROZEN layer (running statistics): one pass -- gg = (fma(y, scale, shift) > 0) ? g : 0,
// dy = bf16(gg * scale) -- with the fp32 (sum gg, sum gg * xhat) rows as a by-product (SUMS).  dy may alias d_act.
template <bool SUMS>
__global__ __launch_bounds__(kThreads) void bn_frozen_bwd_bf16_kernel(const bf16_t* d_act, const bf16_t* __restrict__ y,
                                                                      const float* scale, const float* shift,
                                                                      const float* mean, const float* invstd,
                                                                      const bf16_t* d_pooled, const uint8_t* pool_idx,
                                                                      long items, int CG, int H, int W, bf16_t* dy,
                                                                      float* __restrict__ partial) {
  __shared__ float sm[SUMS ? kThreads : 1][17];
  const long first = blockIdx.x * static_cast<long>(kThreads) + threadIdx.x;
  const int c = static_cast<int>(first % CG) * 8;  // the grid stride is a multiple of CG (a power of two <= 256)
  float sc[8], sh[8], mu[8], is[8], s1[8], s2[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    sc[e] = scale[c + e];
    sh[e] = shift[c + e];
    mu[e] = SUMS ? mean[c + e] : 0.f;
    is[e] = SUMS ? invstd[c + e] : 0.f;
    s1[e] = 0.f;
    s2[e] = 0.f;
  }
  for (long i = first; i < items; i += static_cast<long>(gridDim.x) * kThreads) {
    float g[8], v[8], out[8];
    load_grad8(d_act, d_pooled, pool_idx, i, CG, H, W, g);
    unpack8(reinterpret_cast<const u32x4*>(y)[i], v);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float gg = (fmaf(v[e], sc[e], sh[e]) > 0.f) ? g[e] : 0.f;
      if constexpr (SUMS) {
        s1[e] += gg;
        s2[e] += gg * (v[e] - mu[e]) * is[e];
      }
      out[e] = gg * sc[e];
    }
    reinterpret_cast<u32x4*>(dy)[i] = pack8(out);  // may alias d_act: the item was read by this thread above
  }
  if constexpr (SUMS) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      sm[threadIdx.x][2 * e] = s1[e];
      sm[threadIdx.x][2 * e + 1] = s2[e];
    }
    __syncthreads();
    const int C = CG * 8;
    for (int cc = threadIdx.x; cc < C; cc += kThreads) {  // kThreads % CG == 0: thread t holds octet t % CG
      const int cg = cc >> 3, e = cc & 7;
      float a = 0.f, b = 0.f;
      for (int t = cg; t < kThreads; t += CG) {  // fixed order
        a += sm[t][2 * e];
        b += sm[t][2 * e + 1];
      }
      partial[(static_cast<long>(blockIdx.x) * C + cc) * 2 + 0] = a;
      partial[(static_cast<long>(blockIdx.x) * C + cc) * 2 + 1] = b;
    }
  }
}


// ---- max-pool backward without a BatchNorm to route through (is_batchnorm=False): thread = (pixel, octet) ----
__global__ __launch_bounds__(kThreads) void maxpool_bwd_bf16_kernel(const bf16_t* __restrict__ d_pooled,
                                                                    const uint8_t* __restrict__ pool_idx, int N, int H, int W,
                                                                    int CG, bf16_t* __restrict__ d_act,
                                                                    const bf16_t* __restrict__ gate) {
  const long items = static_cast<long>(N) * H * W * CG;
  const unsigned ucg = static_cast<unsigned>(CG);
  for (long i = blockIdx.x * static_cast<long>(kThreads) + threadIdx.x; i < items;
       i += static_cast<long>(gridDim.x) * kThreads) {
    const unsigned iu = static_cast<unsigned>(i);  // items < 2^31 (launcher)
    const unsigned cg = iu % ucg;
    unsigned r = iu / ucg;
    const unsigned x = r % static_cast<unsigned>(W);
    r /= static_cast<unsigned>(W);
    const unsigned y = r % static_cast<unsigned>(H);
    const unsigned n = r / static_cast<unsigned>(H);
    const unsigned wi = ((n * (static_cast<unsigned>(H) >> 1) + (y >> 1)) * (static_cast<unsigned>(W) >> 1) + (x >> 1)) * ucg + cg;
    const unsigned pos = (y & 1u) * 2u + (x & 1u);
    const u32x2 ib = reinterpret_cast<const u32x2*>(pool_idx)[wi];
    float g[8], dp[8];
    unpack8(reinterpret_cast<const u32x4*>(d_act)[i], g);
    unpack8(reinterpret_cast<const u32x4*>(d_pooled)[wi], dp);
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (((ib[e >> 2] >> (8 * (e & 3))) & 0xffu) == pos) g[e] += dp[e];
    if (gate != nullptr) {
      float gt[8];
      unpack8(reinterpret_cast<const u32x4*>(gate)[i], gt);
#pragma unroll
      for (int e = 0; e < 8; ++e) g[e] = (gt[e] > 0.f) ? g[e] : 0.f;
    }
    reinterpret_cast<u32x4*>(d_act)[i] = pack8(g);
  }
}

// ---- bilinear x2, align_corners=True (nn.UpsamplingBilinear2d, models/unet.py:190) on bf16 NHWC ----
__device__ __forceinline__ void bilinear_src_bf(int dst, int in_size, float rscale, int& i0, int& i1, float& l1) {
  const float s = rscale * static_cast<float>(dst);
  i0 = static_cast<int>(s);
  if (i0 > in_size - 1) i0 = in_size - 1;
  i1 = i0 + ((i0 < in_size - 1) ? 1 : 0);
  l1 = s - static_cast<float>(i0);
}

// thread = (output pixel, octet): four 16-byte loads, the fp32 expression of the fp32 kernel, one rounding
__global__ __launch_bounds__(kThreads) void bilinear2x_fwd_bf16_kernel(const bf16_t* __restrict__ x, int N, int H, int W,
                                                                       int CG, bf16_t* __restrict__ y) {
  const int Ho = 2 * H, Wo = 2 * W;
  const float ry = (Ho > 1) ? static_cast<float>(H - 1) / static_cast<float>(Ho - 1) : 0.f;
  const float rx = (Wo > 1) ? static_cast<float>(W - 1) / static_cast<float>(Wo - 1) : 0.f;
  const long items = static_cast<long>(N) * Ho * Wo * CG;
  for (long i = blockIdx.x * static_cast<long>(kThreads) + threadIdx.x; i < items;
       i += static_cast<long>(gridDim.x) * kThreads) {
    const int cg = static_cast<int>(i % CG);
    long r = i / CG;
    const int xo = static_cast<int>(r % Wo);
    r /= Wo;
    const int yo = static_cast<int>(r % Ho);
    const long n = r / Ho;
    int y0, y1, x0, x1;
    float ly, lx;
    bilinear_src_bf(yo, H, ry, y0, y1, ly);
    bilinear_src_bf(xo, W, rx, x0, x1, lx);
    const u32x4* b = reinterpret_cast<const u32x4*>(x) + n * H * W * CG + cg;
    float v00[8], v01[8], v10[8], v11[8], o[8];
    unpack8(b[(static_cast<long>(y0) * W + x0) * CG], v00);
    unpack8(b[(static_cast<long>(y0) * W + x1) * CG], v01);
    unpack8(b[(static_cast<long>(y1) * W + x0) * CG], v10);
    unpack8(b[(static_cast<long>(y1) * W + x1) * CG], v11);
#pragma unroll
    for (int e = 0; e < 8; ++e)
      o[e] = (1.f - ly) * ((1.f - lx) * v00[e] + lx * v01[e]) + ly * ((1.f - lx) * v10[e] + lx * v11[e]);
    reinterpret_cast<u32x4*>(y)[i] = pack8(o);
  }
}

// gather form of the transposed stencil (fixed summation order, no atomics): thread = (source pixel, octet)
__global__ __launch_bounds__(kThreads) void bilinear2x_bwd_bf16_kernel(const bf16_t* __restrict__ dy, int N, int H, int W,
                                                                       int CG, bf16_t* __restrict__ dx, int accumulate,
                                                                       const bf16_t* __restrict__ gate) {
  const int Ho = 2 * H, Wo = 2 * W;
  const float ry = (Ho > 1) ? static_cast<float>(H - 1) / static_cast<float>(Ho - 1) : 0.f;
  const float rx = (Wo > 1) ? static_cast<float>(W - 1) / static_cast<float>(Wo - 1) : 0.f;
  const long items = static_cast<long>(N) * H * W * CG;
  for (long i = blockIdx.x * static_cast<long>(kThreads) + threadIdx.x; i < items;
       i += static_cast<long>(gridDim.x) * kThreads) {
    const int cg = static_cast<int>(i % CG);
    long r = i / CG;
    const int xs = static_cast<int>(r % W);
    r /= W;
    const int ys = static_cast<int>(r % H);
    const long n = r / H;
    const int ylo = max(0, 2 * ys - 3), yhi = min(Ho - 1, 2 * ys + 3);
    const int xlo = max(0, 2 * xs - 3), xhi = min(Wo - 1, 2 * xs + 3);
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int yo = ylo; yo <= yhi; ++yo) {
      int y0, y1;
      float ly;
      bilinear_src_bf(yo, H, ry, y0, y1, ly);
      float wy = 0.f;
      if (y0 == ys) wy += 1.f - ly;
      if (y1 == ys) wy += ly;
      if (wy == 0.f) continue;
      for (int xo = xlo; xo <= xhi; ++xo) {
        int x0, x1;
        float lx;
        bilinear_src_bf(xo, W, rx, x0, x1, lx);
        float wx = 0.f;
        if (x0 == xs) wx += 1.f - lx;
        if (x1 == xs) wx += lx;
        if (wx != 0.f) {
          float v[8];
          unpack8(reinterpret_cast<const u32x4*>(dy)[((n * Ho + yo) * Wo + xo) * CG + cg], v);
#pragma unroll
          for (int e = 0; e < 8; ++e) s[e] += wy * wx * v[e];
        }
      }
    }
    if (accumulate) {
      float old[8];
      unpack8(reinterpret_cast<const u32x4*>(dx)[i], old);
#pragma unroll
      for (int e = 0; e < 8; ++e) s[e] += old[e];
    }
    if (gate != nullptr) {
      float gt[8];
      unpack8(reinterpret_cast<const u32x4*>(gate)[i], gt);
#pragma unroll
      for (int e = 0; e < 8; ++e) s[e] = (gt[e] > 0.f) ? s[e] : 0.f;
    }
    reinterpret_cast<u32x4*>(dx)[i] = pack8(s);
  }
}

}  // namespace
}  // namespace unetpp

using namespace unetpp;

// ---- the streaming launchers: NULL checks here, every other decision in stream_select.h ----
static_assert(kStreamThreads == kThreads, "stream_select sizes its grids for kThreads threads per workgroup");

extern "C" int unetpp_affine_relu_pool_bf16(const void* y, const float* scale, const float* shift, int32_t relu, int32_t N,
                                            int32_t H, int32_t W, int32_t C, void* act, void* pooled, uint8_t* pool_idx,
                                            void* stream) {
  if (!y) return UNETPP_EINVAL;
  StreamQuery q = stream_query(STREAM_AFFINE, true, N, H, W, C);
  q.has_scale = scale != nullptr, q.has_shift = shift != nullptr, q.has_act = act != nullptr;
  q.has_pooled = pooled != nullptr, q.has_idx = pool_idx != nullptr;
  q.in_lo = stream_lo4(y), q.out_lo = stream_lo4(act), q.pooled_lo = stream_lo4(pooled), q.idx_lo = stream_lo4(pool_idx);
  StreamSel s;
  if (stream_select(q, s) != UNETPP_OK) return UNETPP_EINVAL;
  note_kernel(s.label);
  if (pooled == nullptr)
    hipLaunchKernelGGL(affine_relu_bf16_kernel, dim3(s.grid), dim3(s.block), 0, ST(stream), static_cast<const bf16_t*>(y),
                       scale, shift, relu, s.items, s.cg, static_cast<bf16_t*>(act));
  else
    hipLaunchKernelGGL(affine_relu_pool_bf16_kernel, dim3(s.grid), dim3(s.block), 0, ST(stream),
                       static_cast<const bf16_t*>(y), scale, shift, relu, N, H, W, s.cg, static_cast<bf16_t*>(act),
                       static_cast<bf16_t*>(pooled), pool_idx);
  return launch_status();
}

extern "C" int64_t unetpp_bn_bwd_blocks_bf16(int64_t pixels, int32_t C) { return stream_partial_rows(true, false, pixels, C); }
extern "C" int64_t unetpp_bn_frozen_bwd_blocks_bf16(int64_t pixels, int32_t C) { return stream_partial_rows(true, true, pixels, C); }

extern "C" int unetpp_bn_bwd_reduce_bf16(const void* d_act, const void* y, const float* scale, const float* shift,
                                         const float* mean, const float* invstd, const void* d_pooled,
                                         const uint8_t* pool_idx, int32_t N, int32_t H, int32_t W, int32_t C, float* partial,
                                         void* stream) {
  if (!d_act || !y || !scale || !shift || !mean || !invstd || !partial) return UNETPP_EINVAL;
  const StreamQuery q = stream_bn_query(STREAM_BN_REDUCE, true, N, H, W, C, d_act, y, nullptr, scale, shift, mean, invstd,
                                        nullptr, nullptr, nullptr, d_pooled, pool_idx, partial);
  StreamSel s;
  if (stream_select(q, s) != UNETPP_OK) return UNETPP_EINVAL;
  note_kernel(s.label);
  hipLaunchKernelGGL(bn_bwd_reduce_bf16_kernel, dim3(s.grid), dim3(s.block), 0, ST(stream),
                     static_cast<const bf16_t*>(d_act), static_cast<const bf16_t*>(y), scale, shift, mean, invstd,
                     static_cast<const bf16_t*>(d_pooled), pool_idx, s.items, s.cg, H, W, partial);
  return launch_status();
}

extern "C" int unetpp_bn_bwd_apply_bf16(const void* d_act, const void* y, const float* scale, const float* shift,
                                        const float* mean, const float* invstd, const float* gamma, const float* dgamma,
                                        const float* dbeta, const void* d_pooled, const uint8_t* pool_idx, int32_t N,
                                        int32_t H, int32_t W, int32_t C, void* dy, void* stream) {
  if (!d_act || !y || !scale || !shift || !mean || !invstd || !gamma || !dgamma || !dbeta || !dy) return UNETPP_EINVAL;
  const StreamQuery q = stream_bn_query(STREAM_BN_APPLY, true, N, H, W, C, d_act, y, dy, scale, shift, mean, invstd, gamma,
                                        dgamma, dbeta, d_pooled, pool_idx, nullptr);
  StreamSel s;
  if (stream_select(q, s) != UNETPP_OK) return UNETPP_EINVAL;
  const long pixels = static_cast<long>(N) * H * W;
  note_kernel(s.label);
  hipLaunchKernelGGL(bn_bwd_apply_bf16_kernel, dim3(s.grid), dim3(s.block), 0, ST(stream),
                     static_cast<const bf16_t*>(d_act), static_cast<const bf16_t*>(y), scale, shift, mean, invstd, gamma,
                     dgamma, dbeta, static_cast<const bf16_t*>(d_pooled), pool_idx, 1.0f / static_cast<float>(pixels),
                     s.items, s.cg, H, W, static_cast<bf16_t*>(dy));
  return launch_status();
}

extern "C" int unetpp_bn_frozen_bwd_bf16(const void* d_act, const void* y, const float* scale, const float* shift,
                                         const float* mean, const float* invstd, const void* d_pooled,
                                         const uint8_t* pool_idx, int32_t N, int32_t H, int32_t W, int32_t C, void* dy,
                                         float* partial, void* stream) {
  if (!d_act || !y || !scale || !shift || !dy) return UNETPP_EINVAL;
  const StreamQuery q = stream_bn_query(STREAM_BN_FROZEN, true, N, H, W, C, d_act, y, dy, scale, shift, mean, invstd,
                                        nullptr, nullptr, nullptr, d_pooled, pool_idx, partial);
  StreamSel s;
  if (stream_select(q, s) != UNETPP_OK) return UNETPP_EINVAL;
  note_kernel(s.label);
#define UNETPP_FROZEN_BF16(SUMS)                                                                                       \
  hipLaunchKernelGGL(bn_frozen_bwd_bf16_kernel<SUMS>, dim3(s.grid), dim3(s.block), 0, ST(stream),                      \
                     static_cast<const bf16_t*>(d_act), static_cast<const bf16_t*>(y), scale, shift, mean, invstd,     \
                     static_cast<const bf16_t*>(d_pooled), pool_idx, s.items, s.cg, H, W, static_cast<bf16_t*>(dy),    \
                     partial)
  if (partial != nullptr)
    UNETPP_FROZEN_BF16(true);
  else
    UNETPP_FROZEN_BF16(false);
#undef UNETPP_FROZEN_BF16
  return launch_status();
}

extern "C" int unetpp_maxpool_bwd_bf16(const void* d_pooled, const uint8_t* pool_idx, int32_t N, int32_t H, int32_t W,
                                       int32_t C, void* d_act, const void* gate, void* stream) {
  if (!d_pooled || !pool_idx || !d_act) return UNETPP_EINVAL;
  StreamQuery q = stream_query(STREAM_POOL_BWD, true, N, H, W, C);
  q.has_gate = gate != nullptr;
  q.pooled_lo = stream_lo4(d_pooled), q.idx_lo = stream_lo4(pool_idx), q.out_lo = stream_lo4(d_act), q.gate_lo = stream_lo4(gate);
  StreamSel s;
  if (stream_select(q, s) != UNETPP_OK) return UNETPP_EINVAL;
  note_kernel(s.label);
  hipLaunchKernelGGL(maxpool_bwd_bf16_kernel, dim3(s.grid), dim3(s.block), 0, ST(stream),
                     static_cast<const bf16_t*>(d_pooled), pool_idx, N, H, W, s.cg, static_cast<bf16_t*>(d_act),
                     static_cast<const bf16_t*>(gate));
  return launch_status();
}

extern "C" int unetpp_bilinear2x_fwd_bf16(const void* x, int32_t N, int32_t H, int32_t W, int32_t C, void* y, void* stream) {
  if (!x || !y || N < 1 || H < 1 || W < 1 || C < 8 || (C & 7) || !aligned16(x) || !aligned16(y)) return UNETPP_EINVAL;
  const long items = static_cast<long>(N) * 4 * H * W * (C >> 3);
  note_kernel("bilinear2x_fwd_bf16");
  hipLaunchKernelGGL(bilinear2x_fwd_bf16_kernel, dim3(grid_for(items)), dim3(kThreads), 0, ST(stream),
                     static_cast<const bf16_t*>(x), N, H, W, C >> 3, static_cast<bf16_t*>(y));
  return launch_status();
}

extern "C" int unetpp_bilinear2x_bwd_bf16(const void* dy, int32_t N, int32_t H, int32_t W, int32_t C, void* dx,
                                          int32_t accumulate, const void* gate, void* stream) {
  if (!dy || !dx || N < 1 || H < 1 || W < 1 || C < 8 || (C & 7) || !aligned16(dy) || !aligned16(dx) || (gate && !aligned16(gate))) return UNETPP_EINVAL;
  const long items = static_cast<long>(N) * H * W * (C >> 3);
  note_kernel("bilinear2x_bwd_bf16");
  hipLaunchKernelGGL(bilinear2x_bwd_bf16_kernel, dim3(grid_for(items)), dim3(kThreads), 0, ST(stream),
                     static_cast<const bf16_t*>(dy), N, H, W, C >> 3, static_cast<bf16_t*>(dx), accumulate,
                     static_cast<const bf16_t*>(gate));
  return launch_status();
}
