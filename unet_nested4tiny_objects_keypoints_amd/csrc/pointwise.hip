// HBM-bound companions of the MFMA kernels: BatchNorm statistics / apply / backward (training and frozen), fused
// affine+ReLU+2x2 max-pool and its backward, the sum over partial rows (unetpp_sum_partials), bilinear x2
// (align_corners), and the NCHW<->NHWC converters used at the network edge.  All NHWC fp32; 16-byte vector
// accesses whenever the channel count is a multiple of 4, scalar fallback otherwise.  (The heads: heads.hip.)
#include "common.h"
#include "lds_asm.h"
#include "stream_select.h"

namespace unetpp {
namespace {

template <int VEC>
struct Pack;
template <>
struct Pack<4> {
  using T = f32x4;
};
template <>
struct Pack<1> {
  using T = float;
};
template <int VEC>
__device__ __forceinline__ float& lane_of(typename Pack<VEC>::T& v, int i) {
  if constexpr (VEC == 4)
    return reinterpret_cast<float*>(&v)[i];
  else
    return v;
}
template <int VEC>
__device__ __forceinline__ float lane_of(const typename Pack<VEC>::T& v, int i) {
  if constexpr (VEC == 4)
    return v[i];
  else
    return v;
}

// ------------------------------------------------------------------ BatchNorm statistics
// partial [n_blocks][C][2] -> per-channel totals in double; one workgroup (kFinThreads or fewer threads) per channel:
// 8-byte loads, eight rows in flight per thread, wave shuffles, then the waves' totals in wave order.
constexpr int kFinThreads = 1024;
__device__ __forceinline__ void reduce_pair_over_blocks(const float* partial, long n_blocks, int C, int c,
                                                         double& s1, double& s2) {
  __shared__ double red[2][kFinThreads / 64];
  double a = 0.0, b = 0.0;
  const float2* p = reinterpret_cast<const float2*>(partial) + c;
  const long step = blockDim.x;
  long i = threadIdx.x;
  for (; i + 7 * step < n_blocks; i += 8 * step) {
    float2 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = p[(i + u * step) * C];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      a += static_cast<double>(v[u].x);
      b += static_cast<double>(v[u].y);
    }
  }
  for (; i < n_blocks; i += step) {
    const float2 v = p[i * C];
    a += static_cast<double>(v.x);
    b += static_cast<double>(v.y);
  }
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) {
    a += __shfl_xor(a, m);
    b += __shfl_xor(b, m);
  }
  const int wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[0][wave] = a;
    red[1][wave] = b;
  }
  __syncthreads();
  a = 0.0;
  b = 0.0;
  for (int w = 0; w < n_waves; ++w) {
    a += red[0][w];
    b += red[1][w];
  }
  s1 = a;
  s2 = b;
}

__global__ __launch_bounds__(kFinThreads) void bn_finalize_kernel(const float* partial, long n_blocks, int C, long count,
                                                               const float* gamma, const float* beta, float eps,
                                                               float momentum, float* running_mean, float* running_var,
                                                               float* mean, float* invstd, float* scale, float* shift) {
  const int c = blockIdx.x;
  double s1, s2;
  reduce_pair_over_blocks(partial, n_blocks, C, c, s1, s2);
  if (threadIdx.x == 0) {
    const double m = s1 / static_cast<double>(count);
    double var = s2 / static_cast<double>(count) - m * m;
    if (var < 0.0) var = 0.0;
    const double is = 1.0 / sqrt(var + static_cast<double>(eps));
    const double sc = static_cast<double>(gamma[c]) * is;
    mean[c] = static_cast<float>(m);
    invstd[c] = static_cast<float>(is);
    scale[c] = static_cast<float>(sc);
    shift[c] = static_cast<float>(static_cast<double>(beta[c]) - m * sc);
    if (running_mean != nullptr) {
      const double unbiased = count > 1 ? var * static_cast<double>(count) / static_cast<double>(count - 1) : var;
      running_mean[c] = static_cast<float>((1.0 - momentum) * running_mean[c] + momentum * m);
      running_var[c] = static_cast<float>((1.0 - momentum) * running_var[c] + momentum * unbiased);
    }
  }
}

// mean_out / invstd_out (both or neither): what the frozen BatchNorm backward needs besides the coefficients -- a snapshot
// of the running mean and 1/sqrt(running_var + eps).  One kernel for both entry points: scale and shift have the same bits.
__global__ void bn_eval_coeffs_kernel(const float* gamma, const float* beta, const float* rm, const float* rv, float eps,
                                      int C, float* scale, float* shift, float* mean_out, float* invstd_out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float is = 1.0f / sqrtf(rv[c] + eps);
  const float sc = gamma[c] * is;
  scale[c] = sc;
  shift[c] = beta[c] - rm[c] * sc;
  if (mean_out != nullptr) {
    mean_out[c] = rm[c];
    invstd_out[c] = is;
  }
}

__global__ __launch_bounds__(kFinThreads) void bn_bwd_finalize_kernel(const float* partial, long n_blocks, int C,
                                                                   float* dgamma, float* dbeta) {
  const int c = blockIdx.x;
  double s1, s2;
  reduce_pair_over_blocks(partial, n_blocks, C, c, s1, s2);
  if (threadIdx.x == 0) {
    dbeta[c] = static_cast<float>(s1);
    dgamma[c] = static_cast<float>(s2);
  }
}

// ------------------------------------------------------------------ affine + ReLU (+ 2x2 max-pool)
template <int VEC>
__global__ __launch_bounds__(kThreads) void affine_relu_kernel(const float* __restrict__ y, const float* __restrict__ scale,
                                                               const float* __restrict__ shift, int relu, long items,
                                                               int CG, float* __restrict__ act) {
  using P = typename Pack<VEC>::T;
  for (long i = blockIdx.x * static_cast<long>(kThreads) + threadIdx.x; i < items;
       i += static_cast<long>(gridDim.x) * kThreads) {
    const int c = static_cast<int>(i % CG) * VEC;
    P v = reinterpret_cast<const P*>(y)[i];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      float t = lane_of<VEC>(v, k);
      if (scale != nullptr) t = fmaf(t, scale[c + k], shift[c + k]);
      if (relu) t = relu_keep_nan(t);
      lane_of<VEC>(v, k) = t;
    }
    reinterpret_cast<P*>(act)[i] = v;
  }
}

template <int VEC>
__global__ __launch_bounds__(kThreads) void affine_relu_pool_kernel(const float* __restrict__ y,
                                                                    const float* __restrict__ scale,
                                                                    const float* __restrict__ shift, int relu, int N,
                                                                    int H, int W, int CG, float* __restrict__ act,
                                                                    float* __restrict__ pooled,
                                                                    uint8_t* __restrict__ pool_idx) {
  using P = typename Pack<VEC>::T;
  const int Ho = H >> 1, Wo = W >> 1;
  const long items = static_cast<long>(N) * Ho * Wo * CG;
  for (long i = blockIdx.x * static_cast<long>(kThreads) + threadIdx.x; i < items;
       i += static_cast<long>(gridDim.x) * kThreads) {
    const int cg = static_cast<int>(i % CG);
    long r = i / CG;
    const int xo = static_cast<int>(r % Wo);
    r /= Wo;
    const int yo = static_cast<int>(r % Ho);
    const int n = static_cast<int>(r / Ho);
    const int c = cg * VEC;
    float best[VEC];
    uint8_t bi[VEC];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const long pix = (static_cast<long>(n) * H + (2 * yo + (q >> 1))) * W + (2 * xo + (q & 1));
      P v = reinterpret_cast<const P*>(y)[pix * CG + cg];
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        float t = lane_of<VEC>(v, k);
        if (scale != nullptr) t = fmaf(t, scale[c + k], shift[c + k]);
        if (relu) t = relu_keep_nan(t);
        lane_of<VEC>(v, k) = t;
        if (q == 0 || pool_takes(t, best[k])) {  // first maximum wins, scan order (0,0),(0,1),(1,0),(1,1)
          best[k] = t;
          bi[k] = static_cast<uint8_t>(q);
        }
      }
      if (act != nullptr) reinterpret_cast<P*>(act)[pix * CG + cg] = v;
    }
    P out;
#pragma unroll
    for (int k = 0; k < VEC; ++k) lane_of<VEC>(out, k) = best[k];
    reinterpret_cast<P*>(pooled)[i] = out;
    if (pool_idx != nullptr) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) pool_idx[i * VEC + k] = bi[k];
    }
  }
}

template <int VEC>
__global__ __launch_bounds__(kThreads) void maxpool_bwd_kernel(const float* __restrict__ d_pooled,
                                                               const uint8_t* __restrict__ pool_idx, int N, int H, int W,
                                                               int CG, float* __restrict__ d_act) {
  const int Ho = H >> 1, Wo = W >> 1;
  const long items = static_cast<long>(N) * Ho * Wo * CG;
  for (long i = blockIdx.x * static_cast<long>(kThreads) + threadIdx.x; i < items;
       i += static_cast<long>(gridDim.x) * kThreads) {
    const int cg = static_cast<int>(i % CG);
    long r = i / CG;
    const int xo = static_cast<int>(r % Wo);
    r /= Wo;
    const int yo = static_cast<int>(r % Ho);
    const int n = static_cast<int>(r / Ho);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const int q = pool_idx[i * VEC + k];
      const long pix = (static_cast<long>(n) * H + (2 * yo + (q >> 1))) * W + (2 * xo + (q & 1));
      d_act[(pix * CG + cg) * VEC + k] += d_pooled[i * VEC + k];
    }
  }
}

// Row-structured forms of the two pool kernels for 4-aligned channels and tensors below 2^31 elements: a workgroup
// walks whole rows of windows (row = n * Ho + yo), a thread the (window, channel quad) items j = xo * CG + cg of the
// row, so the index arithmetic is 32-bit and division free (the item's two input rows sit at 2j - cg and
// 2j - cg + CG quads from the row starts) and the four argmax bytes of a quad leave as one dword.
// Streaming (non-temporal) accesses for the two full-resolution tensors of the pool pass (y is not read again before
// the backward pass, act not before the decoder): 114 -> 98 us on the X_0,0 shape.  -DUNETPP_POOL_NO_NT turns them off.
#ifndef UNETPP_POOL_NO_NT
#define UNETPP_POOL_LOAD(p) __builtin_nontemporal_load(p)
#define UNETPP_POOL_STORE(p, v) __builtin_nontemporal_store(v, p)
#else
#define UNETPP_POOL_LOAD(p) (*(p))
#define UNETPP_POOL_STORE(p, v) (*(p) = (v))
#endif
__global__ __launch_bounds__(kThreads) void affine_relu_pool_rows_kernel(
    const f32x4* __restrict__ y, const f32x4* __restrict__ scale, const f32x4* __restrict__ shift, int relu,
    unsigned rows, unsigned Wo, unsigned CG, f32x4* __restrict__ act, f32x4* __restrict__ pooled,
    uint32_t* __restrict__ pool_idx) {
  const unsigned row_items = Wo * CG;  // quads per pooled row; an input row holds 2 * row_items quads
  for (unsigned row = blockIdx.x; row < rows; row += gridDim.x) {
    const unsigned in0 = row * 4u * row_items;  // input row 2 * row (rows of one image are consecutive: H = 2 Ho)
    for (unsigned j = threadIdx.x; j < row_items; j += kThreads) {
      const unsigned cg = j % CG;
      const unsigned a = in0 + 2u * j - cg;
      const unsigned off[4] = {a, a + CG, a + 2u * row_items, a + 2u * row_items + CG};
      f32x4 v[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = UNETPP_POOL_LOAD(y + off[q]);
      f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
      if (scale != nullptr) {
        sc = scale[cg];
        sh = shift[cg];
      }
      f32x4 best;
      uint32_t bi = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float t = fmaf(v[q][k], sc[k], sh[k]);
          if (relu) t = relu_keep_nan(t);
          v[q][k] = t;
          if (q == 0) {
            best[k] = t;
          } else if (pool_takes(t, best[k])) {  // first maximum wins, scan order (0,0),(0,1),(1,0),(1,1)
            best[k] = t;
            bi = (bi & ~(0xffu << (8 * k))) | (static_cast<uint32_t>(q) << (8 * k));
          }
        }
        if (act != nullptr) UNETPP_POOL_STORE(act + off[q], v[q]);
      }
      pooled[row * row_items + j] = best;
      if (pool_idx != nullptr) pool_idx[row * row_items + j] = bi;
    }
  }
}

__global__ __launch_bounds__(kThreads) void maxpool_bwd_rows_kernel(const f32x4* __restrict__ d_pooled,
                                                                    const uint32_t* __restrict__ pool_idx, unsigned rows,
                                                                    unsigned Wo, unsigned CG, f32x4* __restrict__ d_act) {
  const unsigned row_items = Wo * CG;
  for (unsigned row = blockIdx.x; row < rows; row += gridDim.x) {
    const unsigned in0 = row * 4u * row_items;
    for (unsigned j = threadIdx.x; j < row_items; j += kThreads) {
      const unsigned cg = j % CG;
      const unsigned a = in0 + 2u * j - cg;
      const unsigned off[4] = {a, a + CG, a + 2u * row_items, a + 2u * row_items + CG};
      const uint32_t bi = pool_idx[row * row_items + j];
      const f32x4 d = d_pooled[row * row_items + j];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        bool any = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) any = any || ((bi >> (8 * k)) & 0xffu) == static_cast<uint32_t>(q);
        if (any) {  // untouched quads are neither read nor written
          f32x4 g = d_act[off[q]];
#pragma unroll
          for (int k = 0; k < 4; ++k) g[k] += (((bi >> (8 * k)) & 0xffu) == static_cast<uint32_t>(q)) ? d[k] : 0.f;
          d_act[off[q]] = g;
        }
      }
    }
  }
}

// ------------------------------------------------------------------ BatchNorm backward
// Grid stride is a multiple of CG, so a thread keeps one channel group for its whole loop.
template <int VEC>
__global__ __launch_bounds__(kThreads) void bn_bwd_reduce_kernel(const float* __restrict__ d_act,
                                                                 const float* __restrict__ y,
                                                                 const float* __restrict__ scale,
                                                                 const float* __restrict__ shift,
                                                                 const float* __restrict__ mean,
                                                                 const float* __restrict__ invstd, long items, int CG,
                                                                 float* __restrict__ partial) {
  using P = typename Pack<VEC>::T;
  __shared__ float sm[kThreads][VEC * 2];
  const long first = blockIdx.x * static_cast<long>(kThreads) + threadIdx.x;
  const int c = static_cast<int>(first % CG) * VEC;
  float sc[VEC], sh[VEC], mu[VEC], is[VEC], s1[VEC], s2[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    sc[k] = scale[c + k];
    sh[k] = shift[c + k];
    mu[k] = mean[c + k];
    is[k] = invstd[c + k];
    s1[k] = 0.f;
    s2[k] = 0.f;
  }
  for (long i = first; i < items; i += static_cast<long>(gridDim.x) * kThreads) {
    const P g = reinterpret_cast<const P*>(d_act)[i];
    const P v = reinterpret_cast<const P*>(y)[i];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const float yy = lane_of<VEC>(v, k);
      const float gg = (fmaf(yy, sc[k], sh[k]) > 0.f) ? lane_of<VEC>(g, k) : 0.f;
      s1[k] += gg;
      s2[k] += gg * (yy - mu[k]) * is[k];
    }
  }
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    sm[threadIdx.x][2 * k] = s1[k];
    sm[threadIdx.x][2 * k + 1] = s2[k];
  }
  __syncthreads();
  const int C = CG * VEC;
  const int base = static_cast<int>((blockIdx.x * static_cast<long>(kThreads)) % CG);
  for (int cc = threadIdx.x; cc < C; cc += kThreads) {
    const int cg = cc / VEC, k = cc % VEC;
    float a = 0.f, b = 0.f;
    for (int t = (cg - base + CG) % CG; t < kThreads; t += CG) {
      a += sm[t][2 * k];
      b += sm[t][2 * k + 1];
    }
    partial[(static_cast<long>(blockIdx.x) * C + cc) * 2 + 0] = a;
    partial[(static_cast<long>(blockIdx.x) * C + cc) * 2 + 1] = b;
  }
}

template <int VEC>
__global__ __launch_bounds__(kThreads) void bn_bwd_apply_kernel(const float* __restrict__ d_act, const float* __restrict__ y,
                                                                const float* __restrict__ scale,
                                                                const float* __restrict__ shift,
                                                                const float* __restrict__ mean,
                                                                const float* __restrict__ invstd,
                                                                const float* __restrict__ gamma,
                                                                const float* __restrict__ dgamma,
                                                                const float* __restrict__ dbeta, float inv_count,
                                                                long items, int CG, float* __restrict__ dy) {
  using P = typename Pack<VEC>::T;
  for (long i = blockIdx.x * static_cast<long>(kThreads) + threadIdx.x; i < items;
       i += static_cast<long>(gridDim.x) * kThreads) {
    const int c = static_cast<int>(i % CG) * VEC;
    const P g = reinterpret_cast<const P*>(d_act)[i];
    const P v = reinterpret_cast<const P*>(y)[i];
    P out;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const float yy = lane_of<VEC>(v, k);
      const float gg = (fmaf(yy, scale[c + k], shift[c + k]) > 0.f) ? lane_of<VEC>(g, k) : 0.f;
      const float xhat = (yy - mean[c + k]) * invstd[c + k];
      lane_of<VEC>(out, k) =
          gamma[c + k] * invstd[c + k] * (gg - dbeta[c + k] * inv_count - xhat * dgamma[c + k] * inv_count);
    }
    reinterpret_cast<P*>(dy)[i] = out;
  }
}

// ---- BatchNorm backward of an encoder node whose output was also max-pooled: the pooled consumer's gradient is routed
// to its argmax WHILE d_act is read (in both passes), which saves maxpool_bwd's read-modify-write pass over d_act.
// Row structured like the pool kernels: a workgroup walks image rows, a thread the (pixel, channel quad) items of a row;
// needs 4-aligned channels with a power-of-two quad count <= 256 (a thread keeps its quad), even H and W, tensors
// below 2^31 elements.  The global row index r = n * H + y has y's parity, and r >> 1 is the pooled row.
__device__ __forceinline__ f32x4 routed_grad(const f32x4* __restrict__ d_act, const f32x4* __restrict__ d_pooled,
                                             const uint32_t* __restrict__ pool_idx, unsigned row, unsigned x,
                                             unsigned cg, unsigned log2CG, unsigned row_items) {
  f32x4 g = d_act[row * row_items + (x << log2CG) + cg];
  const unsigned pitem = (row >> 1) * (row_items >> 1) + ((x >> 1) << log2CG) + cg;
  const uint32_t bi = pool_idx[pitem];
  const f32x4 dp = d_pooled[pitem];
  const uint32_t q = ((row & 1u) << 1) | (x & 1u);
#pragma unroll
  for (int k = 0; k < 4; ++k) g[k] += (((bi >> (8 * k)) & 0xffu) == q) ? dp[k] : 0.f;
  return g;
}

__global__ __launch_bounds__(kThreads) void bn_bwd_reduce_pool_kernel(
    const f32x4* __restrict__ d_act, const f32x4* __restrict__ y, const f32x4* __restrict__ scale,
    const f32x4* __restrict__ shift, const f32x4* __restrict__ mean, const f32x4* __restrict__ invstd,
    const f32x4* __restrict__ d_pooled, const uint32_t* __restrict__ pool_idx, unsigned rows, unsigned W,
    unsigned log2CG, float* __restrict__ partial) {
  __shared__ float sm[kThreads][8];
  const unsigned CG = 1u << log2CG, cg = threadIdx.x & (CG - 1), row_items = W << log2CG;
  const f32x4 sc = scale[cg], sh = shift[cg], mu = mean[cg], is = invstd[cg];
  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
  for (unsigned row = blockIdx.x; row < rows; row += gridDim.x) {
    for (unsigned j = threadIdx.x; j < row_items; j += kThreads) {
      const f32x4 g = routed_grad(d_act, d_pooled, pool_idx, row, j >> log2CG, cg, log2CG, row_items);
      const f32x4 v = y[row * row_items + j];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float gg = (fmaf(v[k], sc[k], sh[k]) > 0.f) ? g[k] : 0.f;
        s1[k] += gg;
        s2[k] += gg * (v[k] - mu[k]) * is[k];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    sm[threadIdx.x][2 * k] = s1[k];
    sm[threadIdx.x][2 * k + 1] = s2[k];
  }
  __syncthreads();
  const unsigned C = CG * 4;
  for (unsigned cc = threadIdx.x; cc < C; cc += kThreads) {
    const unsigned g4 = cc >> 2, k = cc & 3;
    float a = 0.f, b = 0.f;
    for (unsigned t = g4; t < kThreads; t += CG) {
      a += sm[t][2 * k];
      b += sm[t][2 * k + 1];
    }
    partial[(static_cast<long>(blockIdx.x) * C + cc) * 2 + 0] = a;
    partial[(static_cast<long>(blockIdx.x) * C + cc) * 2 + 1] = b;
  }
}

__global__ __launch_bounds__(kThreads) void bn_bwd_apply_pool_kernel(
    const f32x4* __restrict__ d_act, const f32x4* __restrict__ y, const f32x4* __restrict__ scale,
    const f32x4* __restrict__ shift, const f32x4* __restrict__ mean, const f32x4* __restrict__ invstd,
    const f32x4* __restrict__ gamma, const f32x4* __restrict__ dgamma, const f32x4* __restrict__ dbeta,
    const f32x4* __restrict__ d_pooled, const uint32_t* __restrict__ pool_idx, float inv_count, unsigned rows, unsigned W,
    unsigned log2CG, f32x4* __restrict__ dy) {
  const unsigned CG = 1u << log2CG, cg = threadIdx.x & (CG - 1), row_items = W << log2CG;
  const f32x4 sc = scale[cg], sh = shift[cg], mu = mean[cg], is = invstd[cg], ga = gamma[cg], dg = dgamma[cg],
              db = dbeta[cg];
  for (unsigned row = blockIdx.x; row < rows; row += gridDim.x) {
    for (unsigned j = threadIdx.x; j < row_items; j += kThreads) {
      const f32x4 g = routed_grad(d_act, d_pooled, pool_idx, row, j >> log2CG, cg, log2CG, row_items);
      const f32x4 v = y[row * row_items + j];
      f32x4 out;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float gg = (fmaf(v[k], sc[k], sh[k]) > 0.f) ? g[k] : 0.f;
        const float xhat = (v[k] - mu[k]) * is[k];
        out[k] = ga[k] * is[k] * (gg - db[k] * inv_count - xhat * dg[k] * inv_count);
      }
      dy[row * row_items + j] = out;  // may alias d_act: the item was read by this thread above
    }
  }
}

// ---- BatchNorm backward of a FROZEN layer (normalised with its running statistics): dy does not depend on the channel
// sums, so one streaming pass does everything -- gg = (fma(y, scale, shift) > 0) ? g : 0, dy = gg * scale -- and the
// (sum gg, sum gg * xhat) rows for dgamma / dbeta are a by-product (SUMS; without it no LDS, no partial rows).
// Grid stride is a multiple of CG, so a thread keeps one channel group and its coefficients in registers.
// dy may alias d_act (neither is __restrict__): an item is read and written by the same thread.
// the workgroup's row of the partial buffer: thread t holds channel group (base + t) % CG; fixed order, no atomics
template <int VEC>
__device__ __forceinline__ void frozen_block_sums(float (&sm)[kThreads][VEC * 2], const float (&s1)[VEC],
                                                  const float (&s2)[VEC], int CG, int base, float* __restrict__ partial) {
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    sm[threadIdx.x][2 * k] = s1[k];
    sm[threadIdx.x][2 * k + 1] = s2[k];
  }
  __syncthreads();
  const int C = CG * VEC;
  for (int cc = threadIdx.x; cc < C; cc += kThreads) {
    const int cg = cc / VEC, k = cc % VEC;
    float a = 0.f, b = 0.f;
    for (int t = (cg - base + CG) % CG; t < kThreads; t += CG) {
      a += sm[t][2 * k];
      b += sm[t][2 * k + 1];
    }
    partial[(static_cast<long>(blockIdx.x) * C + cc) * 2 + 0] = a;
    partial[(static_cast<long>(blockIdx.x) * C + cc) * 2 + 1] = b;
  }
}

template <int VEC, bool SUMS>
__global__ __launch_bounds__(kThreads) void bn_frozen_bwd_kernel(const float* d_act, const float* __restrict__ y,
                                                                 const float* __restrict__ scale,
                                                                 const float* __restrict__ shift,
                                                                 const float* __restrict__ mean,
                                                                 const float* __restrict__ invstd, long items, int CG,
                                                                 float* dy, float* __restrict__ partial) {
  using P = typename Pack<VEC>::T;
  __shared__ float sm[SUMS ? kThreads : 1][VEC * 2];
  const long first = blockIdx.x * static_cast<long>(kThreads) + threadIdx.x;
  const int c = static_cast<int>(first % CG) * VEC;
  float sc[VEC], sh[VEC], mu[VEC], is[VEC], s1[VEC], s2[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    sc[k] = scale[c + k];
    sh[k] = shift[c + k];
    mu[k] = SUMS ? mean[c + k] : 0.f;
    is[k] = SUMS ? invstd[c + k] : 0.f;
    s1[k] = 0.f;
    s2[k] = 0.f;
  }
  for (long i = first; i < items; i += static_cast<long>(gridDim.x) * kThreads) {
    const P g = reinterpret_cast<const P*>(d_act)[i];
    const P v = reinterpret_cast<const P*>(y)[i];
    P out;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const float yy = lane_of<VEC>(v, k);
      const float gg = (fmaf(yy, sc[k], sh[k]) > 0.f) ? lane_of<VEC>(g, k) : 0.f;
      if constexpr (SUMS) {
        s1[k] += gg;
        s2[k] += gg * (yy - mu[k]) * is[k];
      }
      lane_of<VEC>(out, k) = gg * sc[k];
    }
    reinterpret_cast<P*>(dy)[i] = out;
  }
  if constexpr (SUMS) {
    const int base = static_cast<int>((blockIdx.x * static_cast<long>(kThreads)) % CG);
    frozen_block_sums<VEC>(sm, s1, s2, CG, base, partial);
  }
}

// the pooled consumer's gradient routed to its argmax while d_act is read (routed_grad); row structured, conditions of
// stream_bn_pool_ok.  thread t holds quad t & (CG - 1) for all its items
template <bool SUMS>
__global__ __launch_bounds__(kThreads) void bn_frozen_bwd_pool_kernel(
    const f32x4* d_act, const f32x4* __restrict__ y, const f32x4* __restrict__ scale, const f32x4* __restrict__ shift,
    const f32x4* __restrict__ mean, const f32x4* __restrict__ invstd, const f32x4* __restrict__ d_pooled,
    const uint32_t* __restrict__ pool_idx, unsigned rows, unsigned W, unsigned log2CG, f32x4* dy,
    float* __restrict__ partial) {
  __shared__ float sm[SUMS ? kThreads : 1][8];
  const unsigned CG = 1u << log2CG, cg = threadIdx.x & (CG - 1), row_items = W << log2CG;
  const f32x4 sc = scale[cg], sh = shift[cg];
  f32x4 mu = {0.f, 0.f, 0.f, 0.f}, is = {0.f, 0.f, 0.f, 0.f};
  if constexpr (SUMS) {
    mu = mean[cg];
    is = invstd[cg];
  }
  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
  for (unsigned row = blockIdx.x; row < rows; row += gridDim.x) {
    for (unsigned j = threadIdx.x; j < row_items; j += kThreads) {
      const f32x4 g = routed_grad(d_act, d_pooled, pool_idx, row, j >> log2CG, cg, log2CG, row_items);
      const f32x4 v = y[row * row_items + j];
      f32x4 out;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float gg = (fmaf(v[k], sc[k], sh[k]) > 0.f) ? g[k] : 0.f;
        if constexpr (SUMS) {
          s1[k] += gg;
          s2[k] += gg * (v[k] - mu[k]) * is[k];
        }
        out[k] = gg * sc[k];
      }
      dy[row * row_items + j] = out;  // may alias d_act: the item was read by this thread above
    }
  }
  if constexpr (SUMS)
    frozen_block_sums<4>(sm, s1, s2, static_cast<int>(CG), 0, partial);
}


__global__ void sum_partials_kernel(const float* __restrict__ partial, long n_blocks, long len, float* __restrict__ out) {
  // 16 outputs x 64 row groups per workgroup (1024 threads): a thread adds n_blocks / 64 rows (4 loads in flight);
  // the groups are combined through LDS in fixed order.  fp64 sums: thousands of same-sign partials.
  __shared__ double part[64][16];
  const int e = threadIdx.x & 15, g = threadIdx.x >> 4;
  const long i = blockIdx.x * 16L + e;
  double s = 0.0;
  if (i < len) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    long b = g;
    for (; b + 192 < n_blocks; b += 256) {
      s0 += static_cast<double>(partial[b * len + i]);
      s1 += static_cast<double>(partial[(b + 64) * len + i]);
      s2 += static_cast<double>(partial[(b + 128) * len + i]);
      s3 += static_cast<double>(partial[(b + 192) * len + i]);
    }
    for (; b < n_blocks; b += 64) s0 += static_cast<double>(partial[b * len + i]);
    s = (s0 + s1) + (s2 + s3);
  }
  part[g][e] = s;
  __syncthreads();
  if (g == 0 && i < len) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < 64; ++k) t += part[k][e];
    out[i] = static_cast<float>(t);
  }
}

// ------------------------------------------------------------------ bilinear x2, align_corners = True
__device__ __forceinline__ void bilinear_src(int dst, int in_size, float rscale, int& i0, int& i1, float& l1) {
  const float s = rscale * static_cast<float>(dst);
  i0 = static_cast<int>(s);
  if (i0 > in_size - 1) i0 = in_size - 1;
  i1 = i0 + ((i0 < in_size - 1) ? 1 : 0);
  l1 = s - static_cast<float>(i0);
}

__global__ __launch_bounds__(kThreads) void bilinear2x_fwd_kernel(const float* __restrict__ x, int N, int H, int W, int C,
                                                                  float* __restrict__ y) {
  const int Ho = 2 * H, Wo = 2 * W;
  const float ry = (Ho > 1) ? static_cast<float>(H - 1) / static_cast<float>(Ho - 1) : 0.f;
  const float rx = (Wo > 1) ? static_cast<float>(W - 1) / static_cast<float>(Wo - 1) : 0.f;
  const long items = static_cast<long>(N) * Ho * Wo * C;
  for (long i = blockIdx.x * static_cast<long>(kThreads) + threadIdx.x; i < items;
       i += static_cast<long>(gridDim.x) * kThreads) {
    const int c = static_cast<int>(i % C);
    long r = i / C;
    const int xo = static_cast<int>(r % Wo);
    r /= Wo;
    const int yo = static_cast<int>(r % Ho);
    const int n = static_cast<int>(r / Ho);
    int y0, y1, x0, x1;
    float ly, lx;
    bilinear_src(yo, H, ry, y0, y1, ly);
    bilinear_src(xo, W, rx, x0, x1, lx);
    const float* b = x + static_cast<long>(n) * H * W * C + c;
    const float v00 = b[(static_cast<long>(y0) * W + x0) * C], v01 = b[(static_cast<long>(y0) * W + x1) * C];
    const float v10 = b[(static_cast<long>(y1) * W + x0) * C], v11 = b[(static_cast<long>(y1) * W + x1) * C];
    y[i] = (1.f - ly) * ((1.f - lx) * v00 + lx * v01) + ly * ((1.f - lx) * v10 + lx * v11);
  }
}

// gather form of the transposed stencil: every source pixel visits the <= 5x5 destination pixels that can
// reference it and recomputes their weights, so the sum has a fixed order (no atomics).
__global__ __launch_bounds__(kThreads) void bilinear2x_bwd_kernel(const float* __restrict__ dy, int N, int H, int W, int C,
                                                                  float* __restrict__ dx, int accumulate) {
  const int Ho = 2 * H, Wo = 2 * W;
  const float ry = (Ho > 1) ? static_cast<float>(H - 1) / static_cast<float>(Ho - 1) : 0.f;
  const float rx = (Wo > 1) ? static_cast<float>(W - 1) / static_cast<float>(Wo - 1) : 0.f;
  const long items = static_cast<long>(N) * H * W * C;
  for (long i = blockIdx.x * static_cast<long>(kThreads) + threadIdx.x; i < items;
       i += static_cast<long>(gridDim.x) * kThreads) {
    const int c = static_cast<int>(i % C);
    long r = i / C;
    const int xs = static_cast<int>(r % W);
    r /= W;
    const int ys = static_cast<int>(r % H);
    const int n = static_cast<int>(r / H);
    const int ylo = max(0, 2 * ys - 3), yhi = min(Ho - 1, 2 * ys + 3);
    const int xlo = max(0, 2 * xs - 3), xhi = min(Wo - 1, 2 * xs + 3);
    float s = 0.f;
    for (int yo = ylo; yo <= yhi; ++yo) {
      int y0, y1;
      float ly;
      bilinear_src(yo, H, ry, y0, y1, ly);
      float wy = 0.f;
      if (y0 == ys) wy += 1.f - ly;
      if (y1 == ys) wy += ly;
      if (wy == 0.f) continue;
      for (int xo = xlo; xo <= xhi; ++xo) {
        int x0, x1;
        float lx;
        bilinear_src(xo, W, rx, x0, x1, lx);
        float wx = 0.f;
        if (x0 == xs) wx += 1.f - lx;
        if (x1 == xs) wx += lx;
        if (wx != 0.f) s += wy * wx * dy[((static_cast<long>(n) * Ho + yo) * Wo + xo) * C + c];
      }
    }
    dx[i] = accumulate ? dx[i] + s : s;
  }
}

// ------------------------------------------------------------------ layout converters
__global__ __launch_bounds__(kThreads) void nchw_to_nhwc_kernel(const float* __restrict__ src, int N, int C, long HW,
                                                                float* __restrict__ dst) {
  const long items = static_cast<long>(N) * C * HW;
  for (long i = blockIdx.x * static_cast<long>(kThreads) + threadIdx.x; i < items;
       i += static_cast<long>(gridDim.x) * kThreads) {
    const int c = static_cast<int>(i % C);
    const long r = i / C;
    const long hw = r % HW, n = r / HW;
    dst[i] = src[(n * C + c) * HW + hw];
  }
}
__global__ __launch_bounds__(kThreads) void nhwc_to_nchw_kernel(const float* __restrict__ src, int N, int C, long HW,
                                                                float* __restrict__ dst) {
  const long items = static_cast<long>(N) * C * HW;
  for (long i = blockIdx.x * static_cast<long>(kThreads) + threadIdx.x; i < items;
       i += static_cast<long>(gridDim.x) * kThreads) {
    const long hw = i % HW;
    const long r = i / HW;
    const int c = static_cast<int>(r % C);
    const long n = r / C;
    dst[i] = src[(n * HW + hw) * C + c];
  }
}

inline unsigned fin_threads(long n_blocks) {  // workgroup size of the per-channel reductions over partial rows
  return n_blocks >= 4096 ? 1024u : n_blocks >= 1024 ? 512u : 256u;
}
inline const char* fin_label(long n_blocks, const char* l256, const char* l512, const char* l1024) {  // name of that form
  const unsigned t = fin_threads(n_blocks);
  return t == 1024u ? l1024 : t == 512u ? l512 : l256;
}

}  // namespace
}  // namespace unetpp

using namespace unetpp;

extern "C" int unetpp_bn_finalize(const float* partial, int64_t n_blocks, int32_t C, int64_t count, const float* gamma,
                                  const float* beta, float eps, float momentum, float* running_mean,
                                  float* running_var, float* mean, float* invstd, float* scale, float* shift,
                                  void* stream) {
  if (!partial || n_blocks < 1 || C < 1 || count < 1 || !gamma || !beta || !mean || !invstd || !scale || !shift)
    return UNETPP_EINVAL;
  if ((running_mean == nullptr) != (running_var == nullptr)) return UNETPP_EINVAL;
  if ((reinterpret_cast<uintptr_t>(partial) & 7) != 0) return UNETPP_EINVAL;  // rows are read as (sum, sum of squares) pairs
  note_kernel(fin_label(n_blocks, "bn_finalize/256", "bn_finalize/512", "bn_finalize/1024"));
  hipLaunchKernelGGL(bn_finalize_kernel, dim3(C), dim3(fin_threads(n_blocks)), 0, ST(stream), partial, n_blocks, C,
                     count, gamma, beta, eps, momentum, running_mean, running_var, mean, invstd, scale, shift);
  return launch_status();
}

extern "C" int unetpp_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean,
                                     const float* running_var, float eps, int32_t C, float* scale, float* shift,
                                     void* stream) {
  if (!gamma || !beta || !running_mean || !running_var || C < 1 || !scale || !shift) return UNETPP_EINVAL;
  note_kernel("bn_eval_coeffs");
  hipLaunchKernelGGL(bn_eval_coeffs_kernel, dim3((C + 63) / 64), dim3(64), 0, ST(stream), gamma, beta, running_mean,
                     running_var, eps, C, scale, shift, static_cast<float*>(nullptr), static_cast<float*>(nullptr));
  return launch_status();
}

extern "C" int unetpp_bn_eval_coeffs_stats(const float* gamma, const float* beta, const float* running_mean,
                                           const float* running_var, float eps, int32_t C, float* scale, float* shift,
                                           float* mean, float* invstd, void* stream) {
  if (!gamma || !beta || !running_mean || !running_var || C < 1 || !scale || !shift || !mean || !invstd)
    return UNETPP_EINVAL;
  note_kernel("bn_eval_coeffs/stats");
  hipLaunchKernelGGL(bn_eval_coeffs_kernel, dim3((C + 63) / 64), dim3(64), 0, ST(stream), gamma, beta, running_mean,
                     running_var, eps, C, scale, shift, mean, invstd);
  return launch_status();
}

// ---- the streaming launchers: NULL checks here, every other decision in stream_select.h ----
namespace {
static_assert(kStreamThreads == kThreads, "stream_select sizes its grids for kThreads threads per workgroup");

inline unsigned ilog2(unsigned v) {
  unsigned l = 0;
  while ((1u << l) < v) ++l;
  return l;
}

// Unused rows of a partial-sum workspace are zeroed by a KERNEL, not by hipMemsetAsync.  History: round 4 saw non-finite
// BatchNorm gradients from the second replay of a captured training step and blamed the ordering of memset NODES; round 5
// read the captured graph back (tools/probes/graph_topology.py): memset nodes sit in the chain like any kernel node and
// the symptom did not reproduce once warm-up and capture shared one stream.  The kernel stays -- it
// costs the same and keeps the captured step a chain of kernel nodes only; unetpp_debug_set("MEMSET_NODES", 1) switches
// to the memset for that probe.
__global__ __launch_bounds__(kThreads) void zero_rows_kernel(float* __restrict__ p, long n) {
  for (long i = blockIdx.x * static_cast<long>(kThreads) + threadIdx.x; i < n; i += static_cast<long>(gridDim.x) * kThreads)
    p[i] = 0.f;
}
inline void zero_rows(float* p, long n, hipStream_t st) {
  if (opt_value(OPT_MEMSET_NODES, 0) == 1) {   // tools/probes/graph_topology.py only: what a memset NODE does to a captured step
    (void)hipMemsetAsync(p, 0, static_cast<size_t>(n) * sizeof(float), st);
    return;
  }
  const long want = (n + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(zero_rows_kernel, dim3(static_cast<unsigned>(want < 1024 ? want : 1024)), dim3(kThreads), 0, st, p, n);
}
// the partial buffer [buf_rows][C][2] always has stream_partial_rows() rows; those beyond this launch's grid are zeroed
inline void zero_unwritten_rows(float* partial, const StreamSel& s, int C, hipStream_t st) {
  if (s.rows < s.buf_rows) zero_rows(partial + s.rows * C * 2, (s.buf_rows - s.rows) * C * 2, st);
}
}  // namespace

extern "C" int unetpp_affine_relu_pool(const float* y, const float* scale, const float* shift, int32_t relu, int32_t N,
                                       int32_t H, int32_t W, int32_t C, float* act, float* pooled, uint8_t* pool_idx,
                                       void* stream) {
  if (!y) return UNETPP_EINVAL;
  StreamQuery q = stream_query(STREAM_AFFINE, false, N, H, W, C);
  q.has_scale = scale != nullptr, q.has_shift = shift != nullptr, q.has_act = act != nullptr;
  q.has_pooled = pooled != nullptr, q.has_idx = pool_idx != nullptr;
  q.in_lo = stream_lo4(y), q.out_lo = stream_lo4(act), q.pooled_lo = stream_lo4(pooled), q.idx_lo = stream_lo4(pool_idx);
  q.coef_lo = stream_lo4(scale, shift);
  StreamSel s;
  if (stream_select(q, s) != UNETPP_OK) return UNETPP_EINVAL;
  if (s.two_pass) {
    // odd H or W (models/unet.py:40-46): the apply pass over the whole tensor, then the window kernel on the activation
    // (its index arithmetic uses H, W as strides and H/2, W/2 as the window grid; the winners are those of the
    // transformed values either way)
    const int rc = unetpp_affine_relu_pool(y, scale, shift, relu, N, H, W, C, act, nullptr, nullptr, stream);
    if (rc != UNETPP_OK) return rc;
    y = act;
    act = nullptr;
    scale = shift = nullptr;
    relu = 0;
  }
  const dim3 grid(s.grid), block(s.block);
  note_kernel(s.label);
  if (pooled == nullptr) {
    if (s.form == STREAM_VEC)
      hipLaunchKernelGGL(affine_relu_kernel<4>, grid, block, 0, ST(stream), y, scale, shift, relu, s.items, s.cg, act);
    else
      hipLaunchKernelGGL(affine_relu_kernel<1>, grid, block, 0, ST(stream), y, scale, shift, relu, s.items, s.cg, act);
  } else if (s.form == STREAM_ROWS) {
    hipLaunchKernelGGL(affine_relu_pool_rows_kernel, grid, block, 0, ST(stream), reinterpret_cast<const f32x4*>(y),
                       reinterpret_cast<const f32x4*>(scale), reinterpret_cast<const f32x4*>(shift), relu,
                       static_cast<unsigned>(s.items), static_cast<unsigned>(W / 2), static_cast<unsigned>(s.cg),
                       reinterpret_cast<f32x4*>(act), reinterpret_cast<f32x4*>(pooled),
                       reinterpret_cast<uint32_t*>(pool_idx));
  } else if (s.form == STREAM_VEC) {
    hipLaunchKernelGGL(affine_relu_pool_kernel<4>, grid, block, 0, ST(stream), y, scale, shift, relu, N, H, W, s.cg, act,
                       pooled, pool_idx);
  } else {
    hipLaunchKernelGGL(affine_relu_pool_kernel<1>, grid, block, 0, ST(stream), y, scale, shift, relu, N, H, W, s.cg, act,
                       pooled, pool_idx);
  }
  return launch_status();
}

extern "C" int unetpp_maxpool_bwd(const float* d_pooled, const uint8_t* pool_idx, int32_t N, int32_t H, int32_t W,
                                  int32_t C, float* d_act, void* stream) {
  if (!d_pooled || !pool_idx || !d_act) return UNETPP_EINVAL;
  StreamQuery q = stream_query(STREAM_POOL_BWD, false, N, H, W, C);
  q.pooled_lo = stream_lo4(d_pooled), q.idx_lo = stream_lo4(pool_idx), q.out_lo = stream_lo4(d_act);
  StreamSel s;
  if (stream_select(q, s) != UNETPP_OK) return UNETPP_EINVAL;
  const dim3 grid(s.grid), block(s.block);
  note_kernel(s.label);
  if (s.form == STREAM_ROWS)
    hipLaunchKernelGGL(maxpool_bwd_rows_kernel, grid, block, 0, ST(stream), reinterpret_cast<const f32x4*>(d_pooled),
                       reinterpret_cast<const uint32_t*>(pool_idx), static_cast<unsigned>(s.items),
                       static_cast<unsigned>(W / 2), static_cast<unsigned>(s.cg), reinterpret_cast<f32x4*>(d_act));
  else if (s.form == STREAM_VEC)
    hipLaunchKernelGGL(maxpool_bwd_kernel<4>, grid, block, 0, ST(stream), d_pooled, pool_idx, N, H, W, s.cg, d_act);
  else
    hipLaunchKernelGGL(maxpool_bwd_kernel<1>, grid, block, 0, ST(stream), d_pooled, pool_idx, N, H, W, s.cg, d_act);
  return launch_status();
}

extern "C" int64_t unetpp_bn_bwd_blocks(int64_t pixels, int32_t C) { return stream_partial_rows(false, false, pixels, C); }
extern "C" int64_t unetpp_bn_frozen_bwd_blocks(int64_t pixels, int32_t C) { return stream_partial_rows(false, true, pixels, C); }
extern "C" int unetpp_bn_bwd_pool_ok(int32_t N, int32_t H, int32_t W, int32_t C) { return stream_bn_pool_ok(N, H, W, C) ? 1 : 0; }

extern "C" int unetpp_bn_bwd_plan(const unetpp_bn_bwd_query* b, unetpp_bn_bwd_sizes* out) {
  if (!b || !out || (b->d_pooled == nullptr) != (b->pool_idx == nullptr)) return UNETPP_EINVAL;
  BnBwdQuery q{};
  q.frozen = b->frozen != 0, q.bf16 = b->bf16 != 0, q.sums = b->want_sums != 0, q.pool = b->d_pooled != nullptr;
  q.N = b->N, q.H = b->H, q.W = b->W, q.C = b->C;
  q.in_lo = stream_lo4(b->d_act, b->y), q.out_lo = stream_lo4(b->dy), q.pooled_lo = stream_lo4(b->d_pooled);
  q.idx_lo = stream_lo4(b->pool_idx), q.coef_lo = stream_lo4(b->scale, b->shift), q.stat_lo = stream_lo4(b->mean, b->invstd);
  q.gamma_lo = stream_lo4(b->gamma, b->dgamma, b->dbeta);
  BnBwdPlan p;
  const int rc = bn_bwd_plan(q, p);
  *out = unetpp_bn_bwd_sizes{p.route, 0, p.partial_rows, p.partial_floats};
  return rc;
}

extern "C" int unetpp_bn_bwd_reduce(const float* d_act, const float* y, const float* scale, const float* shift,
                                    const float* mean, const float* invstd, int64_t pixels, int32_t C, float* partial,
                                    void* stream) {
  if (!d_act || !y || !scale || !shift || !mean || !invstd || !partial) return UNETPP_EINVAL;
  const StreamQuery q = stream_bn_query(STREAM_BN_REDUCE, false, pixels, 1, 1, C, d_act, y, nullptr, scale, shift, mean,
                                        invstd, nullptr, nullptr, nullptr, nullptr, nullptr, partial);
  StreamSel s;
  if (stream_select(q, s) != UNETPP_OK) return UNETPP_EINVAL;
  zero_unwritten_rows(partial, s, C, ST(stream));
  note_kernel(s.label);
  if (s.form == STREAM_VEC)
    hipLaunchKernelGGL(bn_bwd_reduce_kernel<4>, dim3(s.grid), dim3(s.block), 0, ST(stream), d_act, y, scale, shift, mean,
                       invstd, s.items, s.cg, partial);
  else
    hipLaunchKernelGGL(bn_bwd_reduce_kernel<1>, dim3(s.grid), dim3(s.block), 0, ST(stream), d_act, y, scale, shift, mean,
                       invstd, s.items, s.cg, partial);
  return launch_status();
}

extern "C" int unetpp_bn_bwd_finalize(const float* partial, int64_t n_blocks, int32_t C, float* dgamma, float* dbeta,
                                      void* stream) {
  if (!partial || n_blocks < 1 || C < 1 || !dgamma || !dbeta) return UNETPP_EINVAL;
  if ((reinterpret_cast<uintptr_t>(partial) & 7) != 0) return UNETPP_EINVAL;
  note_kernel(fin_label(n_blocks, "bn_bwd_finalize/256", "bn_bwd_finalize/512", "bn_bwd_finalize/1024"));
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(C), dim3(fin_threads(n_blocks)), 0, ST(stream), partial, n_blocks, C,
                     dgamma, dbeta);
  return launch_status();
}

extern "C" int unetpp_bn_bwd_apply(const float* d_act, const float* y, const float* scale, const float* shift,
                                   const float* mean, const float* invstd, const float* gamma, const float* dgamma,
                                   const float* dbeta, int64_t pixels, int32_t C, float* dy, void* stream) {
  if (!d_act || !y || !scale || !shift || !mean || !invstd || !gamma || !dgamma || !dbeta || !dy) return UNETPP_EINVAL;
  const StreamQuery q = stream_bn_query(STREAM_BN_APPLY, false, pixels, 1, 1, C, d_act, y, dy, scale, shift, mean, invstd,
                                        gamma, dgamma, dbeta, nullptr, nullptr, nullptr);
  StreamSel s;
  if (stream_select(q, s) != UNETPP_OK) return UNETPP_EINVAL;
  const float inv_count = 1.0f / static_cast<float>(pixels);
  note_kernel(s.label);
  if (s.form == STREAM_VEC)
    hipLaunchKernelGGL(bn_bwd_apply_kernel<4>, dim3(s.grid), dim3(s.block), 0, ST(stream), d_act, y, scale, shift, mean,
                       invstd, gamma, dgamma, dbeta, inv_count, s.items, s.cg, dy);
  else
    hipLaunchKernelGGL(bn_bwd_apply_kernel<1>, dim3(s.grid), dim3(s.block), 0, ST(stream), d_act, y, scale, shift, mean,
                       invstd, gamma, dgamma, dbeta, inv_count, s.items, s.cg, dy);
  return launch_status();
}

extern "C" int unetpp_bn_bwd_reduce_pool(const float* d_act, const float* y, const float* scale, const float* shift,
                                         const float* mean, const float* invstd, const float* d_pooled,
                                         const uint8_t* pool_idx, int32_t N, int32_t H, int32_t W, int32_t C,
                                         float* partial, void* stream) {
  if (!d_act || !y || !scale || !shift || !mean || !invstd || !d_pooled || !pool_idx || !partial) return UNETPP_EINVAL;
  const StreamQuery q = stream_bn_query(STREAM_BN_REDUCE, false, N, H, W, C, d_act, y, nullptr, scale, shift, mean, invstd,
                                        nullptr, nullptr, nullptr, d_pooled, pool_idx, partial);
  StreamSel s;
  if (stream_select(q, s) != UNETPP_OK) return UNETPP_EINVAL;
  zero_unwritten_rows(partial, s, C, ST(stream));
  note_kernel(s.label);
  hipLaunchKernelGGL(bn_bwd_reduce_pool_kernel, dim3(s.grid), dim3(s.block), 0, ST(stream),
                     reinterpret_cast<const f32x4*>(d_act), reinterpret_cast<const f32x4*>(y),
                     reinterpret_cast<const f32x4*>(scale), reinterpret_cast<const f32x4*>(shift),
                     reinterpret_cast<const f32x4*>(mean), reinterpret_cast<const f32x4*>(invstd),
                     reinterpret_cast<const f32x4*>(d_pooled), reinterpret_cast<const uint32_t*>(pool_idx),
                     static_cast<unsigned>(s.items), static_cast<unsigned>(W), ilog2(static_cast<unsigned>(s.cg)),
                     partial);
  return launch_status();
}

extern "C" int unetpp_bn_bwd_apply_pool(const float* d_act, const float* y, const float* scale, const float* shift,
                                        const float* mean, const float* invstd, const float* gamma, const float* dgamma,
                                        const float* dbeta, const float* d_pooled, const uint8_t* pool_idx, int32_t N,
                                        int32_t H, int32_t W, int32_t C, float* dy, void* stream) {
  if (!d_act || !y || !scale || !shift || !mean || !invstd || !gamma || !dgamma || !dbeta || !d_pooled || !pool_idx || !dy)
    return UNETPP_EINVAL;
  const StreamQuery q = stream_bn_query(STREAM_BN_APPLY, false, N, H, W, C, d_act, y, dy, scale, shift, mean, invstd, gamma,
                                        dgamma, dbeta, d_pooled, pool_idx, nullptr);
  StreamSel s;
  if (stream_select(q, s) != UNETPP_OK) return UNETPP_EINVAL;
  const float inv_count = 1.0f / static_cast<float>(s.items * W);
  note_kernel(s.label);
  hipLaunchKernelGGL(bn_bwd_apply_pool_kernel, dim3(s.grid), dim3(s.block), 0, ST(stream),
                     reinterpret_cast<const f32x4*>(d_act), reinterpret_cast<const f32x4*>(y),
                     reinterpret_cast<const f32x4*>(scale), reinterpret_cast<const f32x4*>(shift),
                     reinterpret_cast<const f32x4*>(mean), reinterpret_cast<const f32x4*>(invstd),
                     reinterpret_cast<const f32x4*>(gamma), reinterpret_cast<const f32x4*>(dgamma),
                     reinterpret_cast<const f32x4*>(dbeta), reinterpret_cast<const f32x4*>(d_pooled),
                     reinterpret_cast<const uint32_t*>(pool_idx), inv_count, static_cast<unsigned>(s.items),
                     static_cast<unsigned>(W), ilog2(static_cast<unsigned>(s.cg)), reinterpret_cast<f32x4*>(dy));
  return launch_status();
}

extern "C" int unetpp_bn_frozen_bwd(const float* d_act, const float* y, const float* scale, const float* shift,
                                    const float* mean, const float* invstd, const float* d_pooled,
                                    const uint8_t* pool_idx, int32_t N, int32_t H, int32_t W, int32_t C, float* dy,
                                    float* partial, void* stream) {
  if (!d_act || !y || !scale || !shift || !dy) return UNETPP_EINVAL;
  const StreamQuery q = stream_bn_query(STREAM_BN_FROZEN, false, N, H, W, C, d_act, y, dy, scale, shift, mean, invstd,
                                        nullptr, nullptr, nullptr, d_pooled, pool_idx, partial);
  StreamSel s;
  if (stream_select(q, s) != UNETPP_OK) return UNETPP_EINVAL;
  zero_unwritten_rows(partial, s, C, ST(stream));
  note_kernel(s.label);
  if (s.form == STREAM_ROWS) {
#define UNETPP_FROZEN_POOL(SUMS)                                                                                       \
  hipLaunchKernelGGL(bn_frozen_bwd_pool_kernel<SUMS>, dim3(s.grid), dim3(s.block), 0, ST(stream),                      \
                     reinterpret_cast<const f32x4*>(d_act), reinterpret_cast<const f32x4*>(y),                         \
                     reinterpret_cast<const f32x4*>(scale), reinterpret_cast<const f32x4*>(shift),                     \
                     reinterpret_cast<const f32x4*>(mean), reinterpret_cast<const f32x4*>(invstd),                     \
                     reinterpret_cast<const f32x4*>(d_pooled), reinterpret_cast<const uint32_t*>(pool_idx),            \
                     static_cast<unsigned>(s.items), static_cast<unsigned>(W), ilog2(static_cast<unsigned>(s.cg)),     \
                     reinterpret_cast<f32x4*>(dy), partial)
    if (partial != nullptr)
      UNETPP_FROZEN_POOL(true);
    else
      UNETPP_FROZEN_POOL(false);
#undef UNETPP_FROZEN_POOL
    return launch_status();
  }
#define UNETPP_FROZEN(VEC, SUMS)                                                                                       \
  hipLaunchKernelGGL((bn_frozen_bwd_kernel<VEC, SUMS>), dim3(s.grid), dim3(s.block), 0, ST(stream), d_act, y, scale,    \
                     shift, mean, invstd, s.items, s.cg, dy, partial)
  if (s.form == STREAM_VEC) {
    if (partial != nullptr)
      UNETPP_FROZEN(4, true);
    else
      UNETPP_FROZEN(4, false);
  } else {
    if (partial != nullptr)
      UNETPP_FROZEN(1, true);
    else
      UNETPP_FROZEN(1, false);
  }
#undef UNETPP_FROZEN
  return launch_status();
}

extern "C" int unetpp_sum_partials(const float* partial, int64_t n_blocks, int64_t len, float* out, void* stream) {
  if (!partial || !out || n_blocks < 1 || len < 1) return UNETPP_EINVAL;
  // (one form, and no note_kernel: this launch finishes a head's backward, whose label the caller reads afterwards)
  hipLaunchKernelGGL(sum_partials_kernel, dim3(static_cast<unsigned>((len + 15) / 16)), dim3(1024), 0, ST(stream),
                     partial, n_blocks, len, out);
  return launch_status();
}

extern "C" int unetpp_bilinear2x_fwd(const float* x, int32_t N, int32_t H, int32_t W, int32_t C, float* y, void* stream) {
  if (!x || !y || N < 1 || H < 1 || W < 1 || C < 1) return UNETPP_EINVAL;
  const long items = static_cast<long>(N) * 4 * H * W * C;
  note_kernel("bilinear2x_fwd");
  hipLaunchKernelGGL(bilinear2x_fwd_kernel, dim3(grid_for(items)), dim3(kThreads), 0, ST(stream), x, N, H, W, C, y);
  return launch_status();
}

extern "C" int unetpp_bilinear2x_bwd(const float* dy, int32_t N, int32_t H, int32_t W, int32_t C, float* dx,
                                     int32_t accumulate, void* stream) {
  if (!dy || !dx || N < 1 || H < 1 || W < 1 || C < 1) return UNETPP_EINVAL;
  const long items = static_cast<long>(N) * H * W * C;
  note_kernel("bilinear2x_bwd");
  hipLaunchKernelGGL(bilinear2x_bwd_kernel, dim3(grid_for(items)), dim3(kThreads), 0, ST(stream), dy, N, H, W, C, dx, accumulate);
  return launch_status();
}

extern "C" int unetpp_nchw_to_nhwc(const float* src, int32_t N, int32_t C, int32_t H, int32_t W, float* dst, void* stream) {
  if (!src || !dst || N < 1 || C < 1 || H < 1 || W < 1) return UNETPP_EINVAL;
  const long items = static_cast<long>(N) * C * H * W;
  note_kernel("nchw_to_nhwc");
  hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3(grid_for(items)), dim3(kThreads), 0, ST(stream), src, N, C,
                     static_cast<long>(H) * W, dst);
  return launch_status();
}

extern "C" int unetpp_nhwc_to_nchw(const float* src, int32_t N, int32_t C, int32_t H, int32_t W, float* dst, void* stream) {
  if (!src || !dst || N < 1 || C < 1 || H < 1 || W < 1) return UNETPP_EINVAL;
  const long items = static_cast<long>(N) * C * H * W;
  note_kernel("nhwc_to_nchw");
  hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3(grid_for(items)), dim3(kThreads), 0, ST(stream), src, N, C,
                     static_cast<long>(H) * W, dst);
  return launch_status();
}

extern "C" int unetpp_abi_version(void) { return UNETPP_ABI_VERSION; }
extern "C" const char* unetpp_build_arch(void) { return "gfx950"; }
