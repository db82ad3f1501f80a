// Caller-side kernels of the training step: the loss and the target synthesis the reference runs on
// the CPU each step (trainer/trainer.py:122-135; both carry a "put on GPU" TODO there).
//   * FocalLoss_BCE_2d (tools/losses/focal_loss.py:255-301), forward and gradient in one pass over (pred, target):
//       e = 1 - |p - t| + 1e-20,  L = sum -(1 - e)^gamma log e / rows,  dL/dp = [u^gamma / e - gamma u^(gamma-1) log e] sign(p - t) / rows
//     (u = 1 - e; abs'(0) = 0 as in autograd).  Geometry, partial sums and the fixed-order finish: loss_heads.h.
//   * create_heatmap (tools/misc/helper.py:87-172): Gaussian-of-distance maps exp(-0.5 sqrt(dx^2 + dy^2) / R) of the
//     key points, channels 1 and 3 divided by their per-image maximum.  Each map is evaluated in fp64; the sums of channels 1 and 3
//     are float32 running sums and the quotient is float32, as in the reference's numpy code.
#include "common.h"
#include "focal_element.h"
#include "loss_heads.h"

namespace unetpp {
namespace {

// The elements of one thread (2 x float4 at `base`): the gradient (times `scale`: 1 for a single head, 1 / heads under
// the trainer's mean over heads -- a second float32 product, as autograd forms it) and the thread's part of the loss sum.
// t[2][4]: the thread's targets, read once for all heads.  The element arithmetic (and kLow) is focal_element.h.
// kIgnore: an element whose target is negative (t < 0.0f: -0.0 and a NaN are not) is ignored -- its gradient is +0.0 and
// its term is not added, whatever pred holds; every other element runs the element arithmetic unchanged.  The term is
// left out by the condition of the addition, not by a select on the term: `sum += le` is contracted with the product
// inside focal_element, and a select between the two would make the sums of the two instantiations differ in the last
// bit on a target without a negative element.
template <bool kLow, bool kIgnore = false>
__device__ __forceinline__ float focal_thread(const float* __restrict__ pred, float* __restrict__ grad,
                                              const float (&t)[kLossVecs][4], long base, long n, float gamma,
                                              float inv_rows, float scale) {
  const bool cube = gamma == 3.f;
  float sum = 0.f;
#pragma unroll
  for (int h = 0; h < kLossVecs; ++h) {
    const long i = base + 4 * h;
    if (i >= n) break;
    float p[4], g[4];
    const bool vec = (i + 4 <= n);
    if (vec) {
      const f32x4 pv = *reinterpret_cast<const f32x4*>(pred + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) p[e] = pv[e];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) p[e] = (i + e < n) ? pred[i + e] : 0.f;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float le = focal_element<kLow>(p[e], t[h][e], gamma, cube, inv_rows, scale, g[e]);
      bool take = i + e < n;
      if constexpr (kIgnore) {
        if (t[h][e] < 0.f) take = false, g[e] = 0.f;
      }
      if (take) sum += le;
    }
    if (grad != nullptr) {
      if (vec) {
        *reinterpret_cast<f32x4*>(grad + i) = f32x4{g[0], g[1], g[2], g[3]};
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (i + e < n) grad[i + e] = g[e];
      }
    }
  }
  return sum;
}

template <bool kLow>
__global__ __launch_bounds__(kLossThreads) void focal_bce_kernel(const float* __restrict__ pred,
                                                                const float* __restrict__ target, long n, float gamma,
                                                                float inv_rows, float* __restrict__ grad,
                                                                float* __restrict__ partial) {
  __shared__ float red[kLossThreads / 64];
  const long base = (blockIdx.x * static_cast<long>(kLossThreads) + threadIdx.x) * kLossPerThread;
  float t[kLossVecs][4];
  load_thread(target, base, n, t);
  float sum = focal_thread<kLow>(pred, grad, t, base, n, gamma, inv_rows, 1.f);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = ((red[0] + red[1]) + (red[2] + red[3])) * inv_rows;
}

// All deep-supervision heads against one target: the target is read once, partial[h * gridDim.x + block] as
// focal_bce_kernel writes partial[block] for head h (same per-thread order, same wave and block sums).
template <bool kLow, bool kIgnore = false>
__global__ __launch_bounds__(kLossThreads) void focal_bce_heads_kernel(const unetpp_focal_heads hd,
                                                                      const float* __restrict__ target, long n, float gamma,
                                                                      float inv_rows, float scale,
                                                                      float* __restrict__ partial) {
  __shared__ float red[UNETPP_MAX_HEADS][kLossThreads / 64];
  const long base = (blockIdx.x * static_cast<long>(kLossThreads) + threadIdx.x) * kLossPerThread;
  float t[kLossVecs][4];
  load_thread(target, base, n, t);
  for (int h = 0; h < hd.n_heads; ++h) {
    float sum = focal_thread<kLow, kIgnore>(hd.pred[h], hd.grad[h], t, base, n, gamma, inv_rows, scale);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
    if ((threadIdx.x & 63) == 0) red[h][threadIdx.x >> 6] = sum;
  }
  __syncthreads();
  if (static_cast<int>(threadIdx.x) < hd.n_heads) {
    const float* r = red[threadIdx.x];
    partial[static_cast<long>(threadIdx.x) * gridDim.x + blockIdx.x] = ((r[0] + r[1]) + (r[2] + r[3])) * inv_rows;
  }
}

// one block: loss = the sum of the per-block partials
__global__ __launch_bounds__(kFinishThreads) void focal_bce_finish_kernel(const float* __restrict__ partial, long n_blocks,
                                                                          float* __restrict__ loss) {
  __shared__ float red[kFinishThreads];
  const float s = finish_sum(partial, n_blocks, red);
  if (threadIdx.x == 0) loss[0] = s;
}

// one block: every head's loss as focal_bce_finish_kernel sums it, then the mean over heads
__global__ __launch_bounds__(kFinishThreads) void loss_heads_finish_kernel(const float* __restrict__ partial, long n_blocks,
                                                                           int n_heads, float inv_heads,
                                                                           float* __restrict__ loss) {
  __shared__ float red[kFinishThreads];
  finish_heads(n_heads, inv_heads, loss, [&](int h) { return finish_sum(partial + h * n_blocks, n_blocks, red); });
}

// grid (blocks per image, N): unnormalised maps of the 4 channels + per-block maxima of channels 1 and 3
__global__ __launch_bounds__(256) void heatmap_kernel(const float* __restrict__ points, int P, int H, int W, double radius,
                                                      float* __restrict__ out, float* __restrict__ scratch,
                                                      float* __restrict__ blockmax) {
  __shared__ float red[2][4];
  const int n = blockIdx.y;
  const long hw = static_cast<long>(H) * W;
  const long i = blockIdx.x * 256L + threadIdx.x;
  const float* pts = points + static_cast<long>(n) * P * 2;
  double c0 = 0.0, c2 = 0.0;
  float c1 = 0.f, c3 = 0.f;  // channels 1 and 3: float32 running sums, rounded after every addition (the reference
                             // does `float32_array += float64_map`)
  if (i < hw) {
    const double y = static_cast<double>(i / W), x = static_cast<double>(i % W);
    for (int p = 0; p < P; ++p) {
      const double dx = x - static_cast<double>(pts[2 * p]), dy = y - static_cast<double>(pts[2 * p + 1]);
      const double v = exp(-0.5 * sqrt(dx * dx + dy * dy) / radius);
      if (p == 0) c0 = v;
      else if (p < 4) c1 = static_cast<float>(static_cast<double>(c1) + v);
      else if (p == 4) c2 = v;
      else c3 = static_cast<float>(static_cast<double>(c3) + v);
    }
    float* o = out + static_cast<long>(n) * 4 * hw + i;
    o[0] = static_cast<float>(c0);
    o[2 * hw] = static_cast<float>(c2);
    float* s = scratch + static_cast<long>(n) * 2 * hw + i;
    s[0] = c1;
    s[hw] = c3;
  }
  float m1 = c1, m3 = c3;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    m1 = fmaxf(m1, __shfl_xor(m1, off));
    m3 = fmaxf(m3, __shfl_xor(m3, off));
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = m1;
    red[1][threadIdx.x >> 6] = m3;
  }
  __syncthreads();
  if (threadIdx.x < 2)
    blockmax[(static_cast<long>(n) * 2 + threadIdx.x) * gridDim.x + blockIdx.x] =
        fmaxf(fmaxf(red[threadIdx.x][0], red[threadIdx.x][1]), fmaxf(red[threadIdx.x][2], red[threadIdx.x][3]));
}

__global__ __launch_bounds__(256) void heatmap_norm_kernel(int H, int W, float* __restrict__ out,
                                                           const float* __restrict__ scratch,
                                                           const float* __restrict__ blockmax) {
  __shared__ float red[2][256];
  const int n = blockIdx.y;
  const long hw = static_cast<long>(H) * W;
  float m1 = 0.f, m3 = 0.f;
  for (unsigned b = threadIdx.x; b < gridDim.x; b += 256) {
    m1 = fmaxf(m1, blockmax[(static_cast<long>(n) * 2 + 0) * gridDim.x + b]);
    m3 = fmaxf(m3, blockmax[(static_cast<long>(n) * 2 + 1) * gridDim.x + b]);
  }
  red[0][threadIdx.x] = m1;
  red[1][threadIdx.x] = m3;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if (static_cast<int>(threadIdx.x) < s) {
      red[0][threadIdx.x] = fmaxf(red[0][threadIdx.x], red[0][threadIdx.x + s]);
      red[1][threadIdx.x] = fmaxf(red[1][threadIdx.x], red[1][threadIdx.x + s]);
    }
    __syncthreads();
  }
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i >= hw) return;
  const float* s = scratch + static_cast<long>(n) * 2 * hw + i;
  float* o = out + static_cast<long>(n) * 4 * hw + i;
  o[hw] = s[0] / red[0][0];  // float32 sum / float32 maximum, as the reference's array arithmetic
  o[3 * hw] = s[hw] / red[1][0];
}

}  // namespace

void launch_loss_heads_finish(const float* partial, long n_blocks, int n_heads, float inv_heads, float* loss, hipStream_t st) {
  hipLaunchKernelGGL(loss_heads_finish_kernel, dim3(1), dim3(kFinishThreads), 0, st, partial, n_blocks, n_heads, inv_heads, loss);
}

}  // namespace unetpp

using namespace unetpp;

extern "C" int64_t unetpp_focal_bce_blocks(int64_t n) { return loss_blocks(n); }

extern "C" int unetpp_focal_bce(const float* pred, const float* target, int64_t n, int64_t rows, float gamma, float* grad,
                                float* partial, float* loss, void* stream) {
  if (pred == nullptr || target == nullptr || partial == nullptr || loss == nullptr || n < 1 || rows < 1) return UNETPP_EINVAL;
  if (((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(target) | reinterpret_cast<uintptr_t>(grad)) & 15) != 0)
    return UNETPP_EINVAL;
  const int64_t blocks = loss_blocks(n);
  if (blocks > 0x7fffffffLL) return UNETPP_EINVAL;
  hipLaunchKernelGGL(gamma < 1.f ? focal_bce_kernel<true> : focal_bce_kernel<false>, dim3(static_cast<unsigned>(blocks)),
                     dim3(kLossThreads), 0, static_cast<hipStream_t>(stream), pred, target, static_cast<long>(n), gamma,
                     1.f / static_cast<float>(rows), grad, partial);
  hipLaunchKernelGGL(focal_bce_finish_kernel, dim3(1), dim3(kFinishThreads), 0, static_cast<hipStream_t>(stream), partial,
                     static_cast<long>(blocks), loss);
  return launch_status();
}

namespace {

template <bool kIgnore>
int focal_bce_heads_launch(const unetpp_focal_heads* heads, const float* target, int64_t n, int64_t rows, float gamma,
                           float* partial, float* loss, void* stream) {
  unetpp_focal_heads hd;
  if (loss_heads_checked(heads, target, hd) != UNETPP_OK) return UNETPP_EINVAL;
  if (partial == nullptr || loss == nullptr || n < 1 || rows < 1) return UNETPP_EINVAL;
  const int64_t blocks = loss_blocks(n);
  if (blocks > 0x7fffffffLL) return UNETPP_EINVAL;
  const float inv_heads = 1.0f / static_cast<float>(hd.n_heads);
  const auto kernel = gamma < 1.f ? focal_bce_heads_kernel<true, kIgnore> : focal_bce_heads_kernel<false, kIgnore>;
  hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(blocks)), dim3(kLossThreads), 0, static_cast<hipStream_t>(stream), hd, target,
                     static_cast<long>(n), gamma, 1.f / static_cast<float>(rows), inv_heads, partial);
  launch_loss_heads_finish(partial, static_cast<long>(blocks), hd.n_heads, inv_heads, loss, static_cast<hipStream_t>(stream));
  return launch_status();
}

}  // namespace

extern "C" int unetpp_focal_bce_heads(const unetpp_focal_heads* heads, const float* target, int64_t n, int64_t rows,
                                      float gamma, float* partial, float* loss, void* stream) {
  return focal_bce_heads_launch<false>(heads, target, n, rows, gamma, partial, loss, stream);
}

extern "C" int unetpp_focal_bce_heads_ignore(const unetpp_focal_heads* heads, const float* target, int64_t n, int64_t rows,
                                             float gamma, float* partial, float* loss, void* stream) {
  return focal_bce_heads_launch<true>(heads, target, n, rows, gamma, partial, loss, stream);
}

extern "C" int64_t unetpp_heatmap_workspace_bytes(int32_t N, int32_t H, int32_t W) {
  if (N < 1 || H < 1 || W < 1) return 0;
  const int64_t hw = static_cast<int64_t>(H) * W, blocks = (hw + 255) / 256;
  return (static_cast<int64_t>(N) * 2 * hw + static_cast<int64_t>(N) * 2 * blocks) * 4;
}

extern "C" int unetpp_create_heatmap(const float* points, int32_t N, int32_t P, int32_t H, int32_t W, float radius,
                                     float* out_nchw, void* workspace, void* stream) {
  if (points == nullptr || out_nchw == nullptr || workspace == nullptr) return UNETPP_EINVAL;
  if (N < 1 || N > 65535 || P < 6 || H < 1 || W < 1 || !(radius > 0.f)) return UNETPP_EINVAL;
  const long hw = static_cast<long>(H) * W;
  const unsigned blocks = static_cast<unsigned>((hw + 255) / 256);
  float* scratch = static_cast<float*>(workspace);
  float* blockmax = scratch + static_cast<long>(N) * 2 * hw;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(heatmap_kernel, dim3(blocks, N), dim3(256), 0, st, points, P, H, W, static_cast<double>(radius),
                     out_nchw, scratch, blockmax);
  hipLaunchKernelGGL(heatmap_norm_kernel, dim3(blocks, N), dim3(256), 0, st, H, W, out_nchw, scratch, blockmax);
  return launch_status();
}
