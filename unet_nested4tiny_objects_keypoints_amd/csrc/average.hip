// Weight averaging: the reference trainer's `model_save == "average"` strategy (trainer/trainer.py:243-252, left
// unimplemented there) as ONE multi-tensor streaming launch per update.  Every floating state-dict entry of the model
// is a segment {avg, src} (two streams) of a device table; the table, the persistent grid, the chunk walk and the
// arrival counter of capturable launches are multi_tensor.h's and are described there.
//
// Per element, n = the number of updates made before this one:
//   mean / ema   n == 0 or segment.copy:  avg = src                       (bit for bit)
//                otherwise:               d = src - avg;  avg = avg + w*d  (three operations, each rounded once)
//                w = float(1 / (n + 1))  (mean),  float(1 - decay)  (ema), formed in double and rounded once
//   swap         avg <-> src, both streams written, copy segments included
// Implicit contraction is off: w*d and the add are two roundings on every path, so the vector and the scalar path give
// the same bits.  No floating-point atomics, no cross-workgroup order: every element's result depends on that element
// alone.  Capturable launches read n (float32) and decay (double) from the device, and the last workgroup to arrive
// advances n -- as optim_kernel advances its step counters.
#include "common.h"
#include "multi_tensor.h"

#pragma clang fp contract(off)

namespace unetpp {
namespace {

template <int KIND>
__device__ __forceinline__ void apply(float& a, float& s, float w, bool copy) {
  if (KIND == UNETPP_AVG_SWAP) {
    const float t = a;
    a = s;
    s = t;
  } else if (copy) {
    a = s;
  } else {
    const float d = s - a;
    const float wd = w * d;
    a = a + wd;
  }
}

template <int KIND>
__global__ void __launch_bounds__(kMtThreads) avg_kernel(const unetpp_avg_segment* __restrict__ segs,
                                                         const int32_t* __restrict__ chunk_seg, int64_t n_chunks,
                                                         float w_host, int32_t first_host, float* count_dev,
                                                         const double* __restrict__ hyper_dev, int32_t* done) {
  constexpr bool kSwap = KIND == UNETPP_AVG_SWAP;
  float w = w_host;
  bool first = first_host != 0;
  float n_before = 0.f;
  if (!kSwap && count_dev != nullptr) {   // capturable: the count and the decay live on the device
    n_before = *count_dev;
    first = n_before == 0.f;
    w = KIND == UNETPP_AVG_MEAN ? static_cast<float>(1.0 / (static_cast<double>(n_before) + 1.0))
                                : static_cast<float>(1.0 - hyper_dev[0]);
  }
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const unetpp_avg_segment sg = segs[chunk_seg[c]];
    const bool copy = first || sg.copy != 0;
    float* __restrict__ A = sg.avg;
    float* __restrict__ S = sg.src;
    walk_chunk(
        chunk_span(sg.numel, sg.chunk_begin, c), sg.vec != 0,
        [&](int64_t i) __attribute__((always_inline)) {
          f32x4 a = *reinterpret_cast<const f32x4*>(A + i);
          f32x4 s = *reinterpret_cast<const f32x4*>(S + i);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float ae = a[e], se = s[e];
            apply<KIND>(ae, se, w, copy);
            a[e] = ae, s[e] = se;
          }
          *reinterpret_cast<f32x4*>(A + i) = a;
          if (kSwap) *reinterpret_cast<f32x4*>(S + i) = s;
        },
        [&](int64_t i) __attribute__((always_inline)) {
          float ae = A[i], se = S[i];
          apply<KIND>(ae, se, w, copy);
          A[i] = ae;
          if (kSwap) S[i] = se;
        });
  }
  if (kSwap || done == nullptr) return;
  // capturable: the device count advances once every workgroup has read it
  if (!last_workgroup(done)) return;
  if (threadIdx.x == 0) {
    *count_dev = n_before + 1.f;
    *done = 0;
  }
}

template <int KIND>
void launch(const unetpp_avg_segment* segs, const int32_t* chunk_seg, int64_t n_chunks, float w, int32_t first,
            float* count_dev, const double* hyper_dev, int32_t* done, hipStream_t st) {
  hipLaunchKernelGGL((avg_kernel<KIND>), dim3(persistent_grid(n_chunks)), dim3(kMtThreads), 0, st, segs, chunk_seg,
                     n_chunks, w, first, count_dev, hyper_dev, done);
}

}  // namespace
}  // namespace unetpp

using namespace unetpp;

extern "C" int unetpp_avg_update(int32_t kind, int32_t flags, const unetpp_avg_segment* segments, int32_t n_segments,
                                 const int32_t* chunk_segment, int64_t n_chunks, int64_t count, double decay,
                                 float* count_dev, const double* hyper_dev, int32_t* done, void* stream) {
  if (!table_args_ok(segments, n_segments, chunk_segment, n_chunks)) return UNETPP_EINVAL;
  if (kind < UNETPP_AVG_MEAN || kind > UNETPP_AVG_SWAP) return UNETPP_EINVAL;
  if ((flags & ~UNETPP_AVG_CAPTURABLE) != 0) return UNETPP_EINVAL;
  const bool capturable = (flags & UNETPP_AVG_CAPTURABLE) != 0;
  if (kind == UNETPP_AVG_SWAP) {   // a swap has no count: nothing of either mode may be passed
    if (capturable || count_dev != nullptr || hyper_dev != nullptr || done != nullptr) return UNETPP_EINVAL;
  } else if (capturable) {
    if (count_dev == nullptr || done == nullptr) return UNETPP_EINVAL;
    if (kind == UNETPP_AVG_EMA && hyper_dev == nullptr) return UNETPP_EINVAL;
  } else {
    if (count_dev != nullptr || hyper_dev != nullptr || done != nullptr || count < 0) return UNETPP_EINVAL;
    if (kind == UNETPP_AVG_EMA && !(decay >= 0.0 && decay < 1.0)) return UNETPP_EINVAL;
  }
  const hipStream_t st = static_cast<hipStream_t>(stream);
  float w = 0.f;
  int32_t first = 0;
  if (!capturable && kind != UNETPP_AVG_SWAP) {
    first = count == 0;
    w = kind == UNETPP_AVG_MEAN ? static_cast<float>(1.0 / (static_cast<double>(count) + 1.0))
                                : static_cast<float>(1.0 - decay);
  }
  switch (kind) {
    case UNETPP_AVG_MEAN: launch<UNETPP_AVG_MEAN>(segments, chunk_segment, n_chunks, w, first, count_dev, hyper_dev, done, st); note_kernel("avg_mean"); break;
    case UNETPP_AVG_EMA: launch<UNETPP_AVG_EMA>(segments, chunk_segment, n_chunks, w, first, count_dev, hyper_dev, done, st); note_kernel("avg_ema"); break;
    default: launch<UNETPP_AVG_SWAP>(segments, chunk_segment, n_chunks, 0.f, 0, nullptr, nullptr, nullptr, st); note_kernel("avg_swap"); break;
  }
  return launch_status();
}
