// Detection for scene maps: local-maximum peaks of float32 heat maps as a compact list in raster order
// (unetpp_peaks_detect), and the scoring of such lists against labelled points (unetpp_detect_match).  DESIGN.md 5i.
//
// Peak rule.  Pixel p of a map is a peak when v_p >= threshold and no other pixel q of the (2r+1)^2 window around p,
// clipped to the map, beats it: q beats p when v_q > v_p, or v_q == v_p and q comes earlier in raster order.  Plain
// comparisons: a NaN is never a peak and never beats anything.  A plateau has one peak, its first pixel.
// Position: integer peak + per-axis parabola offset.  With a, b, c the float32 values at x-1, x, x+1 converted to
// float64: den = (a - 2*b) + c; den < 0: off = (0.5 * (a - c)) / den, then off < -0.5 -> -0.5, off > 0.5 -> 0.5;
// otherwise (den >= 0, den NaN, or a neighbour outside the map) off = 0.  x_out = float32(double(x) + off), one rounding.
//
// Three launches, no host read-back, no atomics of any kind:
//   mark   one bit per pixel.  A workgroup owns 2048 consecutive raster pixels of one map (8 groups of 256; a wave
//          takes a group per iteration, a lane 4 consecutive pixels of it, one 16-byte load where aligned).  Only a
//          pixel that reaches the threshold takes the window test, so a sparse map is read once.  Bits are stored as
//          the ballots themselves: word 4*g + j of the workgroup holds, at bit `lane`, pixel 256*g + 4*lane + j.
//          The workgroup's count goes to block_count[map][workgroup].
//   scan   one workgroup per map turns block_count into exclusive offsets (in place), writes count[map] and fills
//          the rows k >= min(count, cap) of xy / score with -1 / -inf.
//   store  the grid of `mark` again: a workgroup whose offset is already >= cap leaves; the others turn set bits into
//          ranks (offset + popcount of the ballot bits that precede the pixel in raster order), refine and store.
// Ranks come from counts alone, so the list is in raster order whatever the grid, and two runs give the same bits.
// Every raster index and every offset into the maps is 64-bit.
//
// Matcher.  One workgroup per group g = (frame s, class c).  Predictions are served in `order`; each takes the nearest
// label of its group that no earlier prediction took, d = (double)dx*dx + (double)dy*dy of the float32 differences (as
// validate.hip), if d <= (double)tolerance * tolerance; ties go to the lowest label index.  Thread t looks at labels
// t, t + 256, ...; label l is initialised, read and written (label_pred) by thread l mod 256 alone, so the "spent" state
// needs no ordering between threads.  (d, l) arg-min by wave shuffles, then over the 4 waves through LDS (two buffers:
// one barrier per prediction).  Integer bookkeeping only.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace unetpp {
namespace {

constexpr int kDetThreads = 256;
constexpr int kDetWaves = kDetThreads / 64;
constexpr int kDetGroupPixels = 256;                                   // 64 lanes x 4 pixels
constexpr int kDetGroups = 8;                                          // per workgroup: two per wave
constexpr int kDetBlockPixels = kDetGroups * kDetGroupPixels;          // 2048
constexpr int kDetBlockWords = kDetGroups * 4;                         // 32 ballot words of 64 bits
constexpr int kDetMaxRadius = 8;
constexpr int kDetMaxSide = 1 << 24;
constexpr int kDetMaxMaps = 65535;

__device__ __forceinline__ bool is_peak(const float* __restrict__ map, int H, int W, int r, int y, int x, float v) {
  const int y0 = max(y - r, 0), y1 = min(y + r, H - 1);
  const int x0 = max(x - r, 0), x1 = min(x + r, W - 1);
  for (int yy = y0; yy <= y1; ++yy) {
    const float* __restrict__ row = map + int64_t(yy) * W;
    for (int xx = x0; xx <= x1; ++xx) {
      const float q = row[xx];
      const bool earlier = yy < y || (yy == y && xx < x);
      if (q > v || (q == v && earlier)) return false;   // (the pixel itself: q == v and not earlier)
    }
  }
  return true;
}

// the 4 pixels of a lane: raster index i0 .. i0 + 3 of the map; pixels past the map's end read NaN (never a peak)
__device__ __forceinline__ f32x4 load_quad(const float* __restrict__ map, int64_t i0, int64_t HW) {
  const float nan = __builtin_nanf("");
  f32x4 v = {nan, nan, nan, nan};
  const float* p = map + i0;
  if (i0 + 3 < HW && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
    v = *reinterpret_cast<const f32x4*>(p);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (i0 + j < HW) v[j] = p[j];
  }
  return v;
}

__global__ void __launch_bounds__(kDetThreads) peaks_mark_kernel(const float* __restrict__ maps, int H, int W, int64_t HW,
                                                                 float thr, int r, int blocks_per_map,
                                                                 uint64_t* __restrict__ bits,
                                                                 int32_t* __restrict__ block_count) {
  __shared__ int32_t wave_count[kDetWaves];
  const int m = blockIdx.y;
  const int64_t blk = blockIdx.x;
  const float* __restrict__ map = maps + int64_t(m) * HW;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t* __restrict__ words = bits + (int64_t(m) * blocks_per_map + blk) * kDetBlockWords;

  f32x4 v[2];
  int64_t i0[2];
#pragma unroll
  for (int it = 0; it < 2; ++it) {   // both loads in flight before the first use
    i0[it] = blk * kDetBlockPixels + int64_t(wave + kDetWaves * it) * kDetGroupPixels + 4 * lane;
    v[it] = load_quad(map, i0[it], HW);
  }
  int32_t cnt = 0;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int g = wave + kDetWaves * it;
    bool f[4] = {false, false, false, false};
    if (v[it][0] >= thr || v[it][1] >= thr || v[it][2] >= thr || v[it][3] >= thr) {   // rare on a sparse map
      const int64_t y0 = i0[it] / W;
      const int x0 = static_cast<int>(i0[it] - y0 * W);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (v[it][j] >= thr) {
          int x = x0 + j, y = static_cast<int>(y0);
          while (x >= W) {   // the quad may run over the end of a row (more than once when W < 4)
            x -= W;
            ++y;
          }
          f[j] = is_peak(map, H, W, r, y, x, v[it][j]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint64_t b = __ballot(f[j]);
      cnt += __popcll(b);
      if (lane == j) words[4 * g + j] = b;
    }
  }
  if (lane == 0) wave_count[wave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t total = 0;
#pragma unroll
    for (int w = 0; w < kDetWaves; ++w) total += wave_count[w];
    block_count[int64_t(m) * blocks_per_map + blk] = total;
  }
}

__device__ __forceinline__ int32_t wave_inclusive_scan(int32_t c, int lane) {
  int32_t inc = c;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int32_t n = __shfl_up(inc, off, 64);
    if (lane >= off) inc += n;
  }
  return inc;
}

__global__ void __launch_bounds__(kDetThreads) peaks_scan_kernel(int32_t* __restrict__ block_count, int blocks_per_map,
                                                                 int cap, float* __restrict__ xy,
                                                                 float* __restrict__ score, int32_t* __restrict__ count) {
  __shared__ int32_t wave_total[kDetWaves];
  const int m = blockIdx.x;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int32_t* __restrict__ bc = block_count + int64_t(m) * blocks_per_map;
  int64_t carry = 0;   // peaks of the workgroups before `base`; offsets saturate at INT32_MAX (only ranks < cap are used)
  for (int64_t base = 0; base < blocks_per_map; base += kDetThreads) {
    const int64_t i = base + t;
    const int32_t c = i < blocks_per_map ? bc[i] : 0;
    const int32_t inc = wave_inclusive_scan(c, lane);   // at most 64 * 2048
    if (lane == 63) wave_total[wave] = inc;
    __syncthreads();
    int32_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kDetWaves; ++w) {
      if (w < wave) before += wave_total[w];
      total += wave_total[w];
    }
    const int64_t excl = carry + before + (inc - c);
    if (i < blocks_per_map) bc[i] = static_cast<int32_t>(excl < INT32_MAX ? excl : INT32_MAX);
    carry += total;
    __syncthreads();   // wave_total is rewritten by the next round
  }
  if (t == 0) count[m] = static_cast<int32_t>(carry < INT32_MAX ? carry : INT32_MAX);
  const int64_t kept = carry < cap ? carry : cap;
  for (int64_t k = kept + t; k < cap; k += kDetThreads) {
    const int64_t e = int64_t(m) * cap + k;
    xy[2 * e] = -1.f;
    xy[2 * e + 1] = -1.f;
    score[e] = -INFINITY;
  }
}

// parabola offset of one axis from the float32 neighbours, in float64 (the operation order of the header comment)
__device__ __forceinline__ double parabola_offset(float fa, float fb, float fc) {
  const double a = fa, b = fb, c = fc;
  const double den = (a - (2.0 * b)) + c;
  double off = 0.0;
  if (den < 0.0) {
    off = (0.5 * (a - c)) / den;
    if (off < -0.5) off = -0.5;
    if (off > 0.5) off = 0.5;
  }
  return off;
}

__global__ void __launch_bounds__(kDetThreads) peaks_store_kernel(const float* __restrict__ maps, int H, int W, int64_t HW,
                                                                  int refine, int cap, int blocks_per_map,
                                                                  const uint64_t* __restrict__ bits,
                                                                  const int32_t* __restrict__ block_offset,
                                                                  float* __restrict__ xy, float* __restrict__ score) {
  const int m = blockIdx.y;
  const int64_t blk = blockIdx.x;
  const int32_t first = block_offset[int64_t(m) * blocks_per_map + blk];
  if (first >= cap) return;   // the whole workgroup lies past the capacity
  const float* __restrict__ map = maps + int64_t(m) * HW;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t* __restrict__ words = bits + (int64_t(m) * blocks_per_map + blk) * kDetBlockWords;
  const uint64_t word = lane < kDetBlockWords ? words[lane] : 0;
  const int32_t inc = wave_inclusive_scan(__popcll(word), lane);   // every wave scans the workgroup's 32 words itself
  if (__shfl(inc, 63, 64) == 0) return;
  const uint64_t below = (uint64_t(1) << lane) - 1;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int g = wave + kDetWaves * it;
    const int32_t before = __shfl(inc, g == 0 ? 0 : 4 * g - 1, 64);
    uint64_t b[4];
    int32_t rank = g == 0 ? 0 : before;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      b[j] = __shfl(word, 4 * g + j, 64);
      rank += __popcll(b[j] & below);   // pixels of earlier lanes precede this lane's four
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (((b[j] >> lane) & 1) == 0) continue;
      const int64_t k = int64_t(first) + rank;
      ++rank;
      if (k >= cap) continue;
      const int64_t i = blk * kDetBlockPixels + int64_t(g) * kDetGroupPixels + 4 * lane + j;
      const int64_t y = i / W;
      const int x = static_cast<int>(i - y * W);
      const float v = map[i];
      double ox = 0.0, oy = 0.0;
      if (refine) {
        if (x > 0 && x < W - 1) ox = parabola_offset(map[i - 1], v, map[i + 1]);
        if (y > 0 && y < H - 1) oy = parabola_offset(map[i - W], v, map[i + W]);
      }
      const int64_t e = int64_t(m) * cap + k;
      xy[2 * e] = static_cast<float>(static_cast<double>(x) + ox);
      xy[2 * e + 1] = static_cast<float>(static_cast<double>(y) + oy);
      score[e] = v;
    }
  }
}

constexpr int kNoLabel = INT32_MAX;

// (d, l) of `o` replaces (best, bl) when it is a candidate and lexicographically smaller
__device__ __forceinline__ void take_smaller(double& best, int32_t& bl, double od, int32_t ol) {
  if (ol != kNoLabel && (bl == kNoLabel || od < best || (od == best && ol < bl))) {
    best = od;
    bl = ol;
  }
}

__global__ void __launch_bounds__(kDetThreads) detect_match_kernel(
    const float* __restrict__ xy, const int32_t* __restrict__ n_pred, const int32_t* __restrict__ order, int C, int cap,
    const float* __restrict__ labels, const int32_t* __restrict__ label_class, int L, double tol2,
    int32_t* __restrict__ pred_label, int32_t* label_pred, int32_t* __restrict__ stats) {
  __shared__ double red_d[2][kDetWaves];
  __shared__ int32_t red_l[2][kDetWaves];
  __shared__ int32_t red_n[kDetWaves];
  const int64_t g = blockIdx.x;
  const int s = static_cast<int>(g / C), c = static_cast<int>(g - int64_t(s) * C);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const float* __restrict__ lab = labels + int64_t(s) * L * 2;
  const int32_t* __restrict__ cls = label_class + int64_t(s) * L;
  int32_t* lp = label_pred + int64_t(s) * L;   // label l: thread l mod 256 of its class's workgroup alone touches it
  int32_t* __restrict__ pl = pred_label + g * cap;
  const float* __restrict__ pxy = xy + g * cap * 2;
  const int32_t* __restrict__ ord = order + g * cap;

  int32_t mine = 0;
  for (int l = t; l < L; l += kDetThreads) {
    const int32_t k = cls[l];
    if (k == c) {
      lp[l] = -1;
      ++mine;
    } else if (c == 0 && (k < 0 || k >= C)) {   // labels of no group: padding
      lp[l] = -1;
    }
  }
  for (int k = t; k < cap; k += kDetThreads) pl[k] = -1;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off, 64);
  if (lane == 0) red_n[wave] = mine;
  __syncthreads();
  int32_t n_labels = 0;
#pragma unroll
  for (int w = 0; w < kDetWaves; ++w) n_labels += red_n[w];

  const int32_t np = min(max(n_pred[g], 0), cap);
  int32_t tp = 0, served = 0;
  int par = 0;
  for (int kk = 0; kk < np; ++kk) {
    const int32_t p = ord[kk];           // the same value in every thread
    if (p < 0 || p >= cap) continue;     // a slot that does not exist is not served (the Python layer never passes one)
    ++served;
    const float px = pxy[2 * int64_t(p)], py = pxy[2 * int64_t(p) + 1];
    double best = 0.0;
    int32_t bl = kNoLabel;
    for (int l = t; l < L; l += kDetThreads) {
      if (cls[l] != c || lp[l] >= 0) continue;
      const float dx = px - lab[2 * int64_t(l)];
      const float dy = py - lab[2 * int64_t(l) + 1];
      const double d = static_cast<double>(dx) * static_cast<double>(dx) + static_cast<double>(dy) * static_cast<double>(dy);
      if (d <= tol2 && (bl == kNoLabel || d < best)) {   // l ascends: an equal d keeps the lower index
        best = d;
        bl = l;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double od = __shfl_xor(best, off, 64);
      const int32_t ol = __shfl_xor(bl, off, 64);
      take_smaller(best, bl, od, ol);
    }
    if (lane == 0) {
      red_d[par][wave] = best;
      red_l[par][wave] = bl;
    }
    __syncthreads();
    best = red_d[par][0];
    bl = red_l[par][0];
#pragma unroll
    for (int w = 1; w < kDetWaves; ++w) take_smaller(best, bl, red_d[par][w], red_l[par][w]);
    par ^= 1;
    if (bl != kNoLabel) {
      ++tp;
      if ((bl & (kDetThreads - 1)) == t) {
        lp[bl] = p;
        pl[p] = bl;
      }
    }
  }
  if (t == 0) {
    stats[3 * g] = tp;
    stats[3 * g + 1] = served - tp;
    stats[3 * g + 2] = n_labels - tp;
  }
}

inline int64_t peaks_blocks_per_map(int64_t H, int64_t W) { return (H * W + kDetBlockPixels - 1) / kDetBlockPixels; }

inline bool peaks_shape_ok(int32_t M, int32_t H, int32_t W) {
  if (M <= 0 || H <= 0 || W <= 0 || M > kDetMaxMaps || H >= kDetMaxSide || W >= kDetMaxSide) return false;
  return peaks_blocks_per_map(H, W) <= INT32_MAX;   // grid.x
}

}  // namespace
}  // namespace unetpp

using namespace unetpp;

extern "C" int64_t unetpp_peaks_workspace_bytes(int32_t M, int32_t H, int32_t W) {
  if (!peaks_shape_ok(M, H, W)) return 0;
  return int64_t(M) * peaks_blocks_per_map(H, W) * (kDetBlockWords * 8 + 4);
}

extern "C" int unetpp_peaks_detect(const float* maps, int32_t M, int32_t H, int32_t W, float threshold, int32_t radius,
                                   int32_t refine, int32_t cap, float* xy, float* score, int32_t* count,
                                   void* workspace, void* stream) {
  if (maps == nullptr || xy == nullptr || score == nullptr || count == nullptr || workspace == nullptr)
    return UNETPP_EINVAL;
  if (!peaks_shape_ok(M, H, W) || cap <= 0 || radius < 1 || radius > kDetMaxRadius) return UNETPP_EINVAL;
  if (threshold != threshold) return UNETPP_EINVAL;
  if ((reinterpret_cast<uintptr_t>(workspace) & 7) != 0) return UNETPP_EINVAL;
  const int64_t HW = int64_t(H) * W;
  const int bpm = static_cast<int>(peaks_blocks_per_map(H, W));
  uint64_t* bits = static_cast<uint64_t*>(workspace);
  int32_t* block_count = reinterpret_cast<int32_t*>(bits + int64_t(M) * bpm * kDetBlockWords);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(static_cast<unsigned>(bpm), static_cast<unsigned>(M));
  hipLaunchKernelGGL(peaks_mark_kernel, grid, dim3(kDetThreads), 0, st, maps, H, W, HW, threshold, radius, bpm, bits,
                     block_count);
  hipLaunchKernelGGL(peaks_scan_kernel, dim3(static_cast<unsigned>(M)), dim3(kDetThreads), 0, st, block_count, bpm, cap,
                     xy, score, count);
  hipLaunchKernelGGL(peaks_store_kernel, grid, dim3(kDetThreads), 0, st, maps, H, W, HW, refine != 0 ? 1 : 0, cap, bpm,
                     bits, block_count, xy, score);
  note_kernel("peaks_detect");
  return launch_status();
}

extern "C" int unetpp_detect_match(const float* xy, const int32_t* n_pred, const int32_t* order, int32_t S, int32_t C,
                                   int32_t cap, const float* labels, const int32_t* label_class, int32_t L,
                                   float tolerance, int32_t* pred_label, int32_t* label_pred, int32_t* stats,
                                   void* stream) {
  if (xy == nullptr || n_pred == nullptr || order == nullptr || labels == nullptr || label_class == nullptr ||
      pred_label == nullptr || label_pred == nullptr || stats == nullptr)
    return UNETPP_EINVAL;
  if (S <= 0 || C <= 0 || cap <= 0 || L <= 0) return UNETPP_EINVAL;
  if (!(tolerance >= 0.f)) return UNETPP_EINVAL;   // negative or NaN
  if (int64_t(S) * C > INT32_MAX) return UNETPP_EINVAL;
  const double tol2 = static_cast<double>(tolerance) * static_cast<double>(tolerance);
  hipLaunchKernelGGL(detect_match_kernel, dim3(static_cast<unsigned>(S * C)), dim3(kDetThreads), 0,
                     static_cast<hipStream_t>(stream), xy, n_pred, order, C, cap, labels, label_class, L, tol2, pred_label,
                     label_pred, stats);
  note_kernel("detect_match");
  return launch_status();
}
