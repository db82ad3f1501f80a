// What the fused losses over the deep-supervision heads share (caller.hip: FocalLoss_BCE_2d; topk_loss.hip: its top-k
// form; pr_focal.hip: the penalty-reduced focal loss; distill.hip: self-distillation).  A head loss supplies its element
// rule, its own argument checks and, where a head's value is more than the sum of its partials, its per-head combine.
//   geometry    one workgroup of kLossThreads threads per kLossThreads * kLossPerThread elements, a thread's elements
//               consecutive (2 x float4 per tensor); loss_blocks(n) workgroups, the number unetpp_focal_bce_blocks reports.
//   access      16-byte loads and stores wherever four elements remain, scalar ones on the last one to three (load4,
//               load_thread, store4): every tensor of a call is 16-byte aligned, which loss_heads_checked enforces.
//               The main kernels carry exact-bit contracts that were tested on their instruction listings as they are,
//               and a helper in place of the same statements written out changes a listing (a dead tail load goes, a
//               null test moves): focal_thread (caller.hip) keeps its pred load and its store written out and
//               pr_focal_kernel its store, see profiles/loss_refactor/device_code.txt.  A new loss takes the helpers.
//   partials    a thread's terms in index order -> 6 wave shuffles -> (w0 + w1) + (w2 + w3) -> partial[h * blocks + block].
//   finish      one workgroup of kFinishThreads: a head's partials summed in a fixed order (finish_sum: 1024 strided sums,
//               then a 10-level LDS tree), then the trainer's mean over heads in ITS order (finish_heads):
//               avg = 0; avg = avg + loss_h (h = 0, 1, ...); avg = 1.0 * avg / heads -- float32 tensor arithmetic, the
//               division by a Python scalar being a product with float32(1 / heads).  No atomics: the same bits on every
//               run, and bit for bit what the loop over single-head calls computes.
#pragma once
#include "common.h"

namespace unetpp {

constexpr int kLossThreads = 256;
constexpr int kLossPerThread = 8;  // elements per thread: 2 x float4
constexpr int kLossVecs = kLossPerThread / 4;
constexpr int kFinishThreads = 1024;

// workgroups of a main pass over n elements; 0 for n < 1
inline int64_t loss_blocks(int64_t n) {
  return n < 1 ? 0 : (n - 1) / (static_cast<int64_t>(kLossThreads) * kLossPerThread) + 1;
}

// What every launcher asks of its heads: 1 .. UNETPP_MAX_HEADS of them, no null pred, and target, every pred and every
// grad (null: not wanted) on a 16-byte boundary.  UNETPP_OK: hd is *heads with the unused slots cleared.
inline int loss_heads_checked(const unetpp_focal_heads* heads, const float* target, unetpp_focal_heads& hd) {
  if (heads == nullptr || target == nullptr) return UNETPP_EINVAL;
  if (heads->n_heads < 1 || heads->n_heads > UNETPP_MAX_HEADS) return UNETPP_EINVAL;
  uintptr_t bits = reinterpret_cast<uintptr_t>(target);
  for (int h = 0; h < heads->n_heads; ++h) {
    if (heads->pred[h] == nullptr) return UNETPP_EINVAL;
    bits |= reinterpret_cast<uintptr_t>(heads->pred[h]) | reinterpret_cast<uintptr_t>(heads->grad[h]);
  }
  if ((bits & 15) != 0) return UNETPP_EINVAL;
  hd = *heads;
  for (int h = hd.n_heads; h < UNETPP_MAX_HEADS; ++h) hd.pred[h] = nullptr, hd.grad[h] = nullptr;
  return UNETPP_OK;
}

// caller.hip: loss[1 + h] = the sum of partial[h * n_blocks ..] (finish_sum), loss[0] = their mean (finish_heads); one
// kernel for every loss whose head value is that sum
void launch_loss_heads_finish(const float* partial, long n_blocks, int n_heads, float inv_heads, float* loss, hipStream_t st);

// elements i .. i + 3 of src[0 .. n); `pad` where the index is past the end
__device__ __forceinline__ void load4(const float* __restrict__ src, long i, long n, float pad, float (&v)[4]) {
  if (i + 4 <= n) {
    const f32x4 q = *reinterpret_cast<const f32x4*>(src + i);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = q[e];
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (i + e < n) ? src[i + e] : pad;
  }
}

// A thread's kLossPerThread elements at `base`, 0 past the end.  Not a loop over load4: written out in the loop, the
// main kernels of caller.hip and distill.hip keep the instruction listings their exact-bit contracts were tested on.
__device__ __forceinline__ void load_thread(const float* __restrict__ src, long base, long n, float (&v)[kLossVecs][4]) {
#pragma unroll
  for (int h = 0; h < kLossVecs; ++h) {
    const long i = base + 4 * h;
    if (i + 4 <= n) {
      const f32x4 q = *reinterpret_cast<const f32x4*>(src + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[h][e] = q[e];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[h][e] = (i + e < n) ? src[i + e] : 0.f;
    }
  }
}

// the matching store; a null grad (the gradient is not wanted) stores nothing
__device__ __forceinline__ void store4(float* __restrict__ grad, long i, long n, const float (&g)[4]) {
  if (grad == nullptr) return;
  if (i + 4 <= n) {
    *reinterpret_cast<f32x4*>(grad + i) = f32x4{g[0], g[1], g[2], g[3]};
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (i + e < n) grad[i + e] = g[e];
  }
}

// the sum of n_blocks partials in the fixed order, valid in thread 0; red: kFinishThreads floats of LDS
__device__ __forceinline__ float finish_sum(const float* __restrict__ partial, long n_blocks, float* red) {
  float s = 0.f;
  for (long i = threadIdx.x; i < n_blocks; i += kFinishThreads) s += partial[i];
  __syncthreads();  // (the previous sum's red[0] has been read)
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = kFinishThreads / 2; w >= 1; w >>= 1) {
    if (static_cast<int>(threadIdx.x) < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  return red[0];
}

// loss[1 + h] = head_loss(h) (called by the whole workgroup, valid in thread 0), loss[0] = the mean over heads
template <typename HeadLoss>
__device__ __forceinline__ void finish_heads(int n_heads, float inv_heads, float* __restrict__ loss, HeadLoss head_loss) {
  // (no contraction: the mean is the sum of the values written to loss[1 + h], whatever product head_loss ends with)
#pragma clang fp contract(off)
  float avg = 0.f;
  for (int h = 0; h < n_heads; ++h) {
    const float v = head_loss(h);
    if (threadIdx.x == 0) {
      loss[1 + h] = v;
      avg = avg + v;
    }
  }
  if (threadIdx.x == 0) loss[0] = (1.0f * avg) * inv_heads;
}

}  // namespace unetpp
