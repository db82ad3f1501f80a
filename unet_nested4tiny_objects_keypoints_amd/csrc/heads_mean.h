// The general form of the ensemble head (unetpp_heads_mean_fwd / unetpp_heads_mean_fwd_bf16): one kernel body for both
// storage types of the features.
#pragma once
#include "bf16_common.h"
#include "common.h"
#include "head_select.h"

namespace unetpp {

__device__ __forceinline__ float head_feature(const float* p) { return *p; }
__device__ __forceinline__ float head_feature(const bf16_t* p) { return bf_to_f(*p); }

// Any channel count (scalar loads), 64-bit offsets; thread = pixel, the weights through uniform loads.  T = float or
// bf16_t, the storage type of every feature tensor of the descriptor.
template <typename T>
__global__ __launch_bounds__(kThreads) void heads_mean_general_kernel(const unetpp_heads_mean hd, long pixels, int HW, int C,
                                                                      int n_cls, float* __restrict__ out) {
  const int n_heads = hd.n_heads;
  const float count = static_cast<float>(n_heads);
  for (long p = blockIdx.x * static_cast<long>(kThreads) + threadIdx.x; p < pixels;
       p += static_cast<long>(gridDim.x) * kThreads) {
    float sum[kHeadMaxCls];
#pragma unroll
    for (int k = 0; k < kHeadMaxCls; ++k) sum[k] = 0.f;  // 0 + s_1 is s_1: the sum is ((s_1 + s_2) + ...) in head order
    for (int h = 0; h < n_heads; ++h) {
      const T* __restrict__ xp = static_cast<const T*>(hd.head[h].x) + p * C;
      const float* __restrict__ weight = hd.head[h].weight;
      const float* __restrict__ bias = hd.head[h].bias;
      float acc[kHeadMaxCls];
#pragma unroll
      for (int k = 0; k < kHeadMaxCls; ++k) acc[k] = (k < n_cls) ? bias[k] : 0.f;
      for (int c = 0; c < C; ++c) {
        const float v = head_feature(xp + c);
#pragma unroll
        for (int k = 0; k < kHeadMaxCls; ++k)
          if (k < n_cls) acc[k] = fmaf(v, weight[k * C + c], acc[k]);
      }
#pragma unroll
      for (int k = 0; k < kHeadMaxCls; ++k)
        if (k < n_cls) sum[k] += 1.0f / (1.0f + expf(-acc[k]));
    }
    const long n = p / HW, hw = p - n * HW;
#pragma unroll
    for (int k = 0; k < kHeadMaxCls; ++k)
      if (k < n_cls) out[(n * n_cls + k) * HW + hw] = sum[k] / count;
  }
}

}  // namespace unetpp
