// Ignore masks of partially labelled scenes: packed bit planes of a frame, built from a raster
// (mask_pack_kernel) or from polygon rings (mask_polygons_kernel), and looked up per window pixel by the per-step kernel
// (target_ignore_mask_kernel), the companion of crops.hip's target_ignore_kernel.
//
// Layout: bits int32 [S, P, H, Wd], Wd = ceil(W / 32).  Bit (x & 31) of word (x >> 5) of row y is pixel (x, y); the
// unused high bits of a row's last word are zero.
//
// mask_pack_kernel: a wave owns 64 consecutive x of one row: one element per lane, one ballot, two words.  The low word
// is stored by lane 0 and the high word by lane 32 as two 32-bit stores, so a row of an odd word count that starts off
// an 8-byte boundary needs nothing special; a lane past W votes 0, so tail bits are zero; every word has one writer.
//
// mask_polygons_kernel: a unit is (frame, plane, tile of 16 rows x 64 pixels = one word pair per row); thread (wave,
// lane) owns pixels x = x_lo + lane, y = y_lo + 4 wave + j, j = 0..3.  The rule per ring (even-odd, float64, every
// operation rounded on its own):
//   for every used edge, the closing one included, with the endpoints ordered so that y0 <= y1 (an edge with y0 == y1
//   straddles nothing):  straddles iff y0 <= py < y1;  d = (x1 - x0) * (py - y0) - (px - x0) * (y1 - y0);  toggles iff
//   d > 0.  Inside iff the number of toggles is odd.  A plane's rings are walked in list order: an inside pixel is set
//   by a plain ring and cleared by a clearing ring.
// Per unit the workgroup takes the frame's G rings 256 at a time: thread t scans ring t's used vertices for its float
// bounding box, the survivors (right plane, 3..V vertices, every used vertex finite, box meets the tile) are compacted
// IN LIST ORDER into an LDS list with wave ballots and popcounts, and each survivor's edges then pass through LDS
// kEdgeChunk at a time, ordered by y, as the float32 vertices themselves.  A thread carries 4 parity bits of the current
// ring and 4 running bits; at the end each row's word pair is one ballot.
// Culling never changes a bit: a ring is dropped for a tile only when no pixel of the tile can be inside it --
//   rows:   a toggling edge has y0 <= py < y1, so ymin <= py < ymax: dropped when y_hi < ymin or !(y_lo < ymax);
//   right:  for px >= xmax every straddling edge has d <= 0 (rounding is monotone): dropped when !(x_lo < xmax);
//   left:   for px <= xmin - 1 every straddling edge has d > 0, and a closed ring has an even number of straddling
//           edges at any py: dropped when x_hi + 1 <= xmin -- only for rings whose x lie within +-2^24, where the
//           margin of one pixel dwarfs every rounding of the expression.
// The bounds are minima and maxima of the same float32 values; a ring with a NaN or an infinity is padding.
// No atomics; every word of the output has exactly one writer and is written whether a ring touches it or not; the
// same bits on any grid.
//
// target_ignore_mask_kernel: the unit and thread shape of target_ignore_kernel -- (sample, 64 x 16 tile), 4 consecutive
// x of one row per thread, all classes.  The source position is window.h's map_inverse, as in that kernel; a position
// is in the frame iff 0 <= xs <= Ws - 1 and 0 <= ys <= Hs - 1 (a NaN is outside), its pixel is the nearest one,
// clamped.  Under the exact augmentation family the 4 pixels of a thread lie in one row or one column of the frame: a
// thread keeps the last word it loaded per plane walk, so neighbours in a row share a load.  Stores of -1.0f only,
// nothing of target is read: idempotent stores of one constant, the same bits on any grid.
#include "window.h"

#pragma clang fp contract(off)

namespace unetpp {
namespace {

constexpr int kRingChunk = 256;     // rings examined at a time: one per thread
constexpr int kEdgeChunk = 256;     // edges of a ring held in LDS at a time: one per thread
constexpr int64_t kMaxElems = 2147483647;   // elements / words one launch indexes

// ---------------------------------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ bool nonzero(T v) {
  return !(v == T(0));   // a NaN is nonzero, -0.0 is zero
}

template <typename T>
__global__ void __launch_bounds__(kThreads256) mask_pack_kernel(const T* __restrict__ mask, int W, int Wd, int chunks,
                                                                int32_t* __restrict__ bits, int64_t units) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6), stride = int64_t(gridDim.x) * 4;
  for (int64_t unit = wave0; unit < units; unit += stride) {   // (uniform over a wave)
    const int64_t row = unit / chunks;
    const int chunk = static_cast<int>(unit % chunks);
    const int x = chunk * 64 + lane;
    bool set = false;
    if (x < W) set = nonzero(mask[row * W + x]);
    const uint64_t vote = __ballot(set);
    const int word = 2 * chunk + (lane >> 5);
    if ((lane & 31) == 0 && word < Wd)
      bits[row * Wd + word] = static_cast<int32_t>(static_cast<uint32_t>(lane == 0 ? vote : vote >> 32));
  }
}

// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads256) mask_polygons_kernel(
    const float* __restrict__ vertices, const int32_t* __restrict__ counts, const int32_t* __restrict__ poly_plane,
    const int32_t* __restrict__ poly_clear, int G, int V, int P, int H, int W, int Wd, int32_t* __restrict__ bits,
    int tiles_x, int tiles_y, int64_t units) {
  __shared__ float edge[kEdgeChunk][4];   // x0, y0, x1, y1 with y0 <= y1
  __shared__ int ring_list[kRingChunk];
  __shared__ int wave_cnt[4];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t below = (uint64_t(1) << lane) - 1;
  const float lim = static_cast<float>(kMaxSide);

  for (int64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
    const int tx = static_cast<int>(unit % tiles_x);
    int64_t r = unit / tiles_x;
    const int ty = static_cast<int>(r % tiles_y);
    r /= tiles_y;
    const int plane = static_cast<int>(r % P);
    const int64_t s = r / P;
    const int x_lo = tx * kTileW, y_lo = ty * kTileH;
    const int x_hi = (x_lo + kTileW < W ? x_lo + kTileW : W) - 1;
    const int y_hi = (y_lo + kTileH < H ? y_lo + kTileH : H) - 1;
    const float fx_lo = static_cast<float>(x_lo), fy_lo = static_cast<float>(y_lo);   // exact: sides <= 2^24
    const float fx_next = static_cast<float>(x_hi + 1), fy_hi = static_cast<float>(y_hi);
    const int px = x_lo + lane, py0 = y_lo + wave * 4;
    const double pxd = static_cast<double>(px);

    unsigned bit = 0;   // bit j: pixel (px, py0 + j) as the rings so far leave it

    for (int base = 0; base < G; base += kRingChunk) {
      // which rings of this chunk can touch the tile
      const int g = base + tid;
      bool keep = false;
      if (g < G) {
        const int64_t ring = s * G + g;
        const int n = counts[ring];
        if (poly_plane[ring] == plane && n >= 3 && n <= V) {
          const float* v = vertices + ring * V * 2;
          float xmin = v[0], xmax = v[0], ymin = v[1], ymax = v[1];
          bool finite = true;
          for (int i = 0; i < n; ++i) {
            const float x = v[2 * i], y = v[2 * i + 1];
            finite = finite && fabsf(x) <= 3.402823466e38f && fabsf(y) <= 3.402823466e38f;   // (false for a NaN)
            xmin = x < xmin ? x : xmin;
            xmax = x > xmax ? x : xmax;
            ymin = y < ymin ? y : ymin;
            ymax = y > ymax ? y : ymax;
          }
          const bool modest = xmin >= -lim && xmax <= lim;
          keep = finite && fy_hi >= ymin && fy_lo < ymax && fx_lo < xmax && !(modest && fx_next <= xmin);
        }
      }
      const uint64_t vote = __ballot(keep);
      __syncthreads();   // (the previous chunk's list and counts have been read)
      if (lane == 0) wave_cnt[wave] = __popcll(vote);
      __syncthreads();
      int before = 0, total = 0;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const int cnt = wave_cnt[w];
        before += w < wave ? cnt : 0;
        total += cnt;
      }
      if (keep) ring_list[before + __popcll(vote & below)] = g;   // (list order kept; < 256: one ring per thread)
      __syncthreads();

      for (int i = 0; i < total; ++i) {   // (uniform over the workgroup)
        const int64_t ring = s * G + ring_list[i];
        const int n = counts[ring];
        const bool clear = poly_clear[ring] != 0;
        const float* v = vertices + ring * V * 2;
        unsigned parity = 0;   // bit j: toggles of pixel (px, py0 + j) by this ring so far, mod 2
        for (int e0 = 0; e0 < n; e0 += kEdgeChunk) {
          const int cnt = n - e0 < kEdgeChunk ? n - e0 : kEdgeChunk;
          __syncthreads();   // (the previous chunk of edges has been read)
          if (tid < cnt) {
            const int a = e0 + tid, b = a + 1 < n ? a + 1 : 0;   // (b = 0: the closing edge)
            const float xa = v[2 * a], ya = v[2 * a + 1], xb = v[2 * b], yb = v[2 * b + 1];
            const bool swap = ya > yb;
            edge[tid][0] = swap ? xb : xa;
            edge[tid][1] = swap ? yb : ya;
            edge[tid][2] = swap ? xa : xb;
            edge[tid][3] = swap ? ya : yb;
          }
          __syncthreads();
          for (int e = 0; e < cnt; ++e) {   // (LDS broadcast reads)
            const double x0 = static_cast<double>(edge[e][0]), y0 = static_cast<double>(edge[e][1]);
            const double x1 = static_cast<double>(edge[e][2]), y1 = static_cast<double>(edge[e][3]);
            if (y0 == y1) continue;   // (uniform)
            const double dx = x1 - x0, dy = y1 - y0;
            const double right = (pxd - x0) * dy;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const double pyd = static_cast<double>(py0 + j);
              const double d = dx * (pyd - y0) - right;
              parity ^= (y0 <= pyd && pyd < y1 && d > 0.0) ? (1u << j) : 0u;
            }
          }
        }
        bit = clear ? (bit & ~parity) : (bit | parity);
      }
    }

    // one ballot per row: the word pair of (row, tile)
    const int64_t plane_row0 = (s * P + plane) * H;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int py = py0 + j;
      const uint64_t vote = __ballot(px <= x_hi && ((bit >> j) & 1u) != 0);
      const int word = 2 * tx + (lane >> 5);
      if ((lane & 31) == 0 && word < Wd && py <= y_hi)
        bits[(plane_row0 + py) * Wd + word] = static_cast<int32_t>(static_cast<uint32_t>(lane == 0 ? vote : vote >> 32));
    }
    __syncthreads();   // the list and the wave slots are the next unit's
  }
}

// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads256) target_ignore_mask_kernel(
    const int32_t* __restrict__ bits, const int32_t* __restrict__ plane_class, int64_t M, int P, int Hs, int Ws, int Wd,
    const int64_t* __restrict__ index, const float* __restrict__ params, int C, int Ho, int Wo, int outside,
    float* __restrict__ target, int tiles_x, int tiles_y, int64_t units) {
  const int tid = threadIdx.x;
  const float x_max = static_cast<float>(Ws - 1), y_max = static_cast<float>(Hs - 1);   // exact: sides <= 2^24

  for (int64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
    const int tx = static_cast<int>(unit % tiles_x);
    const int64_t r = unit / tiles_x;
    const int ty = static_cast<int>(r % tiles_y);
    const int n = static_cast<int>(r / tiles_y);
    const int x_lo = tx * kTileW, y_lo = ty * kTileH;
    const int x_hi = (x_lo + kTileW < Wo ? x_lo + kTileW : Wo) - 1;
    const int y_hi = (y_lo + kTileH < Ho ? y_lo + kTileH : Ho) - 1;
    const int px = x_lo + (tid & 15) * 4, py = y_lo + (tid >> 4);
    if (!(py <= y_hi && px <= x_hi)) continue;   // (no barrier in this kernel)

    const int64_t idx = index[n];
    const bool live = idx >= 0 && idx < M;   // (uniform over the workgroup)
    const float* Pm = params + int64_t(n) * UNETPP_WARP_PARAMS;
    const float yf = static_cast<float>(py);
    int64_t at[4];        // word offset of the pixel inside a plane, -1: not in the frame
    unsigned shift[4];
    unsigned every = 0;   // bit p: pixel px + p is ignored for every class
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      float xs, ys;
      map_inverse(Pm, static_cast<float>(px + p), yf, xs, ys);
      const bool in = live && 0.f <= xs && xs <= x_max && 0.f <= ys && ys <= y_max;
      every |= (outside != 0 && !in) ? (1u << p) : 0u;
      at[p] = -1;
      shift[p] = 0;
      if (in) {
        int xi = static_cast<int>(floorf(xs + 0.5f)), yi = static_cast<int>(floorf(ys + 0.5f));
        xi = xi < 0 ? 0 : xi > Ws - 1 ? Ws - 1 : xi;
        yi = yi < 0 ? 0 : yi > Hs - 1 ? Hs - 1 : yi;
        at[p] = int64_t(yi) * Wd + (xi >> 5);
        shift[p] = static_cast<unsigned>(xi & 31);
      }
    }

    const int n_planes = live ? P : 0;
    for (int c0 = 0; c0 < C; c0 += kClassGroup) {
      uint32_t cls_bits[4] = {0u, 0u, 0u, 0u};   // bit k of [p]: pixel px + p is ignored for class c0 + k
      for (int pl = 0; pl < n_planes; ++pl) {
        const int k = plane_class[pl];
        const bool all = k == -1;
        const bool here = k >= c0 && k < c0 + kClassGroup && k < C;
        if ((!all || c0 > 0) && !here) continue;   // (uniform; an every-class plane is walked once, in group 0)
        const uint32_t cbit = here ? (1u << (k - c0)) : 0u;
        const int32_t* plane = bits + (idx * P + pl) * int64_t(Hs) * Wd;
        int64_t last = -1;
        uint32_t word = 0;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          if (at[p] < 0) continue;
          if (at[p] != last) {
            last = at[p];
            word = static_cast<uint32_t>(__ldg(plane + last));
          }
          if ((word >> shift[p]) & 1u) {
            cls_bits[p] |= cbit;
            if (all) every |= 1u << p;
          }
        }
      }
      const int c_end = c0 + kClassGroup < C ? c0 + kClassGroup : C;
      for (int c = c0; c < c_end; ++c) {
        unsigned m = every;
#pragma unroll
        for (int p = 0; p < 4; ++p) m |= ((cls_bits[p] >> (c - c0)) & 1u) << p;
        if (m == 0) continue;
        float* dst = target + ((int64_t(n) * C + c) * Ho + py) * Wo + px;
        if (m == 15u && px + 3 <= x_hi && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
          *reinterpret_cast<f32x4*>(dst) = f32x4{-1.f, -1.f, -1.f, -1.f};
        } else {
#pragma unroll
          for (int p = 0; p < 4; ++p)
            if (((m >> p) & 1u) && px + p <= x_hi) dst[p] = -1.f;
        }
      }
    }
  }
}

}  // namespace
}  // namespace unetpp

using namespace unetpp;

extern "C" int unetpp_mask_pack(const void* mask, int32_t kind, int64_t rows, int32_t W, int32_t* bits, void* stream) {
  if (mask == nullptr || bits == nullptr) return UNETPP_EINVAL;
  if (rows <= 0 || W <= 0 || W > kMaxSide) return UNETPP_EINVAL;
  if (kind != UNETPP_MASK_U8 && kind != UNETPP_MASK_F32) return UNETPP_EINVAL;
  if (rows > kMaxElems / W) return UNETPP_EINVAL;
  const int Wd = (W + 31) / 32, chunks = (W + 63) / 64;
  const int64_t units = rows * chunks;   // one per wave
  const unsigned grid = capped_grid((units + 3) / 4);
  if (kind == UNETPP_MASK_U8) {
    hipLaunchKernelGGL(mask_pack_kernel<uint8_t>, dim3(grid), dim3(kThreads256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint8_t*>(mask), W, Wd, chunks, bits, units);
  } else {
    hipLaunchKernelGGL(mask_pack_kernel<float>, dim3(grid), dim3(kThreads256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const float*>(mask), W, Wd, chunks, bits, units);
  }
  note_kernel("mask_pack");
  return launch_status();
}

extern "C" int unetpp_mask_polygons(const float* vertices, const int32_t* counts, const int32_t* poly_plane,
                                    const int32_t* poly_clear, int32_t S, int32_t G, int32_t V, int32_t P, int32_t H,
                                    int32_t W, int32_t* bits, void* stream) {
  if (bits == nullptr) return UNETPP_EINVAL;
  if (S <= 0 || G < 0 || V < 0 || P <= 0 || H <= 0 || W <= 0 || H > kMaxSide || W > kMaxSide) return UNETPP_EINVAL;
  if (G > 0 && (counts == nullptr || poly_plane == nullptr || poly_clear == nullptr)) return UNETPP_EINVAL;
  if (G > 0 && V > 0 && vertices == nullptr) return UNETPP_EINVAL;
  const int Wd = (W + 31) / 32;
  if (int64_t(S) * P > kMaxElems / H || int64_t(S) * P * H > kMaxElems / Wd) return UNETPP_EINVAL;
  if (G > 0 && V > 0 && int64_t(S) * G > kMaxElems / (2 * int64_t(V))) return UNETPP_EINVAL;
  const int tiles_x = (W + kTileW - 1) / kTileW, tiles_y = (H + kTileH - 1) / kTileH;
  const int64_t units = int64_t(S) * P * tiles_y * tiles_x;
  hipLaunchKernelGGL(mask_polygons_kernel, dim3(capped_grid(units)), dim3(kThreads256), 0,
                     static_cast<hipStream_t>(stream), vertices, counts, poly_plane, poly_clear, G, V, P, H, W, Wd, bits,
                     tiles_x, tiles_y, units);
  note_kernel("mask_polygons");
  return launch_status();
}

extern "C" int unetpp_target_ignore_mask(const int32_t* bits, const int32_t* plane_class, int64_t M, int32_t P,
                                         int32_t Hs, int32_t Ws, const int64_t* index, int32_t N, const float* params,
                                         int32_t C, int32_t Ho, int32_t Wo, int32_t outside, float* target,
                                         void* stream) {
  if (index == nullptr || params == nullptr || target == nullptr) return UNETPP_EINVAL;
  if (M <= 0 || P < 0 || N <= 0 || C <= 0 || Ho <= 0 || Wo <= 0 || Hs <= 0 || Ws <= 0) return UNETPP_EINVAL;
  if (P > 0 && (bits == nullptr || plane_class == nullptr)) return UNETPP_EINVAL;
  if (C > kMaxClasses || Ho > kMaxSide || Wo > kMaxSide || Hs > kMaxSide || Ws > kMaxSide) return UNETPP_EINVAL;
  const int Wd = (Ws + 31) / 32;
  if (P > 0 && int64_t(Hs) * Wd > kMaxElems / P) return UNETPP_EINVAL;   // words of one frame
  if (P == 0 && outside == 0) return UNETPP_OK;   // nothing to mark
  const int tiles_x = (Wo + kTileW - 1) / kTileW, tiles_y = (Ho + kTileH - 1) / kTileH;
  const int64_t units = int64_t(N) * tiles_y * tiles_x;
  hipLaunchKernelGGL(target_ignore_mask_kernel, dim3(capped_grid(units)), dim3(kThreads256), 0,
                     static_cast<hipStream_t>(stream), bits, plane_class, M, P, Hs, Ws, Wd, index, params, C, Ho, Wo,
                     outside, target, tiles_x, tiles_y, units);
  note_kernel("target_ignore_mask");
  return launch_status();
}
