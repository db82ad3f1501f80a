// Validation matcher: the reference's unfinished HeatmapPattern.match_distmin (tools/misc/heatmap.py:57-79) and the
// landmark loss its validation loop meant to compute with nn.MSELoss (trainer/trainer.py:220-221), for every head of a
// batch in ONE launch.
//
// Matching, per (head, image, map c): the labels are pattern[c] (positions i = 0..L-1 of the map's index list), the
// predictions the map's first `found` extracted points (j = 0..P-1, peak order).  Distance: dx = px - tx, dy = py - ty in
// float32, d = (double)dx*dx + (double)dy*dy in float64 (both products are exact; contraction is off all the same).
// Greedy global minimum: min(L, P) times, among the labels not yet assigned and the predictions not yet used, the pair
// with the lexicographically smallest (d, i, j) is assigned.  The scan below walks (i, j) in lexicographic order and
// replaces the best pair only on a strictly smaller d, which is exactly that rule.
//
// Landmark loss of a head: sum of d over its matched labels / (2 * count), i.e. MSELoss (mean) over the matched
// coordinates; 0 / 0 = NaN when nothing matched, as MSELoss of two empty tensors.  Summation order, fixed: thread t of
// the head's workgroup adds, in float64 starting from 0.0, the terms of maps t, t + 256, t + 512, ... (map m = n * C + c),
// each map's terms in the order the greedy rule assigns them; then the 256 partials are summed by the tree
// p[t] += p[t + s] for s = 128, 64, ..., 1; the quotient is formed in float64 and rounded once to float32.
// No floating-point atomics: the result depends on the inputs alone.
#include "common.h"

#pragma clang fp contract(off)

namespace unetpp {
namespace {

constexpr int kMatchThreads = 256;

__device__ __forceinline__ double match_dist(float px, float py, float tx, float ty) {
  const float dx = px - tx;
  const float dy = py - ty;
  return static_cast<double>(dx) * static_cast<double>(dx) + static_cast<double>(dy) * static_cast<double>(dy);
}

__global__ void __launch_bounds__(kMatchThreads) match_kernel(const float* __restrict__ points,
                                                              const int32_t* __restrict__ found, int32_t N, int32_t C,
                                                              int32_t K, const float* __restrict__ labels, int32_t S,
                                                              const int32_t* __restrict__ map_points,
                                                              const int32_t* __restrict__ map_begin,
                                                              float* __restrict__ matched, uint8_t* __restrict__ mask,
                                                              float* __restrict__ loss, int32_t* __restrict__ count) {
  __shared__ double part_sum[kMatchThreads];
  __shared__ int32_t part_count[kMatchThreads];
  const int h = blockIdx.x;
  const int t = threadIdx.x;
  const int64_t ns = int64_t(N) * S;
  float* __restrict__ mh = matched + int64_t(h) * ns * 2;
  uint8_t* __restrict__ kh = mask + int64_t(h) * ns;
  // labels that no map matches (or that no map holds) read (-1, -1) / 0; the matches overwrite after the barrier
  for (int64_t e = t; e < ns; e += kMatchThreads) {
    mh[2 * e] = -1.f;
    mh[2 * e + 1] = -1.f;
    kh[e] = 0;
  }
  __syncthreads();

  double sum = 0.0;
  int32_t cnt = 0;
  const int maps = N * C;
  for (int m = t; m < maps; m += kMatchThreads) {
    const int n = m / C;
    const int c = m - n * C;
    const int b = map_begin[c];
    const int L = min(max(map_begin[c + 1] - b, 0), UNETPP_MATCH_MAX);
    const int64_t g = int64_t(h) * maps + m;
    const int P = min(max(found[g], 0), min(K, UNETPP_MATCH_MAX));
    const float* __restrict__ pp = points + g * K * 2;
    const float* __restrict__ lab = labels + int64_t(n) * S * 2;
    uint64_t lab_used = 0, pred_used = 0;
    const int rounds = min(L, P);
    for (int r = 0; r < rounds; ++r) {
      double best = 0.0;
      int bi = -1, bj = -1;
      for (int i = 0; i < L; ++i) {
        const int s = map_points[b + i];
        if (((lab_used >> i) & 1u) || s < 0 || s >= S) continue;   // the host rejects such indices; never read them
        const float tx = lab[2 * s], ty = lab[2 * s + 1];
        for (int j = 0; j < P; ++j) {
          if ((pred_used >> j) & 1u) continue;
          const double d = match_dist(pp[2 * j], pp[2 * j + 1], tx, ty);
          if (bi < 0 || d < best) {
            best = d;
            bi = i;
            bj = j;
          }
        }
      }
      if (bi < 0) break;
      lab_used |= uint64_t(1) << bi;
      pred_used |= uint64_t(1) << bj;
      const int64_t e = int64_t(n) * S + map_points[b + bi];
      mh[2 * e] = pp[2 * bj];
      mh[2 * e + 1] = pp[2 * bj + 1];
      kh[e] = 1;
      sum += best;
      ++cnt;
    }
  }

  part_sum[t] = sum;
  part_count[t] = cnt;
  __syncthreads();
  for (int s = kMatchThreads / 2; s > 0; s >>= 1) {
    if (t < s) {
      part_sum[t] += part_sum[t + s];
      part_count[t] += part_count[t + s];
    }
    __syncthreads();
  }
  if (t == 0) {
    const int32_t total = part_count[0];
    loss[h] = static_cast<float>(part_sum[0] / (2.0 * static_cast<double>(total)));
    count[h] = total;
  }
}

}  // namespace
}  // namespace unetpp

using namespace unetpp;

extern "C" int unetpp_match_points(const float* points, const int32_t* found, int32_t heads, int32_t N, int32_t C,
                                   int32_t K, const float* labels, int32_t S, const int32_t* map_points,
                                   const int32_t* map_begin, float* matched, uint8_t* mask, float* loss,
                                   int32_t* count, void* stream) {
  if (points == nullptr || found == nullptr || labels == nullptr || map_points == nullptr || map_begin == nullptr ||
      matched == nullptr || mask == nullptr || loss == nullptr || count == nullptr)
    return UNETPP_EINVAL;
  if (heads <= 0 || N <= 0 || C <= 0 || S <= 0 || K <= 0 || K > UNETPP_MATCH_MAX) return UNETPP_EINVAL;
  if (int64_t(heads) * N * C > INT32_MAX || int64_t(N) * S > INT32_MAX) return UNETPP_EINVAL;
  hipLaunchKernelGGL(match_kernel, dim3(static_cast<unsigned>(heads)), dim3(kMatchThreads), 0,
                     static_cast<hipStream_t>(stream), points, found, N, C, K, labels, S, map_points, map_begin, matched,
                     mask, loss, count);
  note_kernel("match_points");
  return launch_status();
}
