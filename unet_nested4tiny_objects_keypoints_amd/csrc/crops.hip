// Training on large scenes: where the windows of a batch are (crops_draw_kernel), the target maps of those windows
// from the frames' variable-length label lists (points_target_kernel) and their ignored elements
// (target_ignore_kernel).  The warp between the draw and the targets is loader.hip's.  What these kernels share with
// loader.hip, paste.hip and mask.hip -- the parameter row and its draw, the two window maps, the label rule, the
// nearest-label value -- is window.h's; the tile decode is typed out in each tile kernel (DESIGN.md 5g says why).
//
// points_target_kernel: out[n, c, y, x] = nearest_value(m), m = the least dx*dx + dy*dy (float64) over the valid labels
// of class c of frame index[n], each at its position under map_forward (so it is the labels_out the warp reports);
// exactly 0 where the class has no valid label.  The maximum of exp(-k d) over points is exp(-k d_min): an exact
// nearest-label search with one sqrt and one exp per pixel, no cutoff radius and no normalisation pass.
//
// A workgroup of 256 threads owns a 64 x 16 pixel tile (one thread: 4 consecutive x of one row) and kClasses classes of
// it -- all of them for C <= 4, so the label list is read by one workgroup per tile; a wider C takes ceil(C / 4) class
// groups.  It sweeps the frame's L labels twice, the second time out of the cache:
//   sweep 1  per class, U = the least over the labels of up_l, the GREATEST squared distance from label l to the
//            tile's rectangle of pixel centres (a min over the workgroup: the same value in any order);
//   sweep 2  label l is kept iff lo_l <= U, lo_l = its LEAST squared distance to that rectangle.  Kept labels are
//            compacted into a per-class candidate list in LDS with wave ballots and popcounts.
// lo_l and up_l are formed from the same rounded float64 differences as a pixel's distance, and rounding is monotone, so
// lo_l <= d(p, l) <= up_l for every pixel p of the tile: a dropped label is strictly farther from every pixel than the
// label that set U, and can be neither the nearest nor tied with it.  Coincident labels all survive.  The candidate
// list has a fixed size, 256 per class: the labels are taken 256 at a time, and the survivors of such a chunk are folded
// into the running minima of the workgroup's pixels before the next chunk reuses the list (a round).  A minimum is exact
// and commutative, so rounds, the order inside a list and the grid change nothing: the same bits on every run.  No
// atomics; implicit contraction is off; offsets into out and label numbers are 64-bit; interior stores are 16 bytes
// wide where the address allows, scalar on ragged edges.
//
// target_ignore_kernel: writes -1.0f into the elements of such a target whose source position lies in an ignore
// rectangle of the frame or outside the frame; stores only, described at the kernel.
//
// crops_draw_kernel: one thread per sample; uniforms 9..12 choose between an object window (a row of the centre table
// plus jitter) and a uniform one, and augment_row writes the row about that window's centre.
#include "window.h"

#pragma clang fp contract(off)

namespace unetpp {
namespace {

constexpr int kClasses = 4;         // classes a workgroup serves at once
constexpr int kCand = 256;          // candidates per class held in LDS: what one chunk of labels can add

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double o = __shfl_xor(v, off, 64);
    v = o < v ? o : v;
  }
  return v;
}

// label l of the frame under the sample's forward map (P: its parameter row); false: not a label (sentinel)
__device__ __forceinline__ bool label_at(const float* __restrict__ lab, const float* __restrict__ P, int64_t l,
                                         float& xo, float& yo) {
  const float x = lab[2 * l], y = lab[2 * l + 1];
  map_forward(P, x, y, xo, yo);
  return label_valid(x, y);
}

// least / greatest squared distance along one axis from position p to the pixel centres a..b (a <= b)
__device__ __forceinline__ void axis_bounds(float p, int a, int b, double& lo2, double& up2) {
  const double pd = static_cast<double>(p);
  const double da = static_cast<double>(a) - pd, db = static_cast<double>(b) - pd;
  const double qa = da * da, qb = db * db;
  up2 = qa > qb ? qa : qb;
  lo2 = pd < static_cast<double>(a) ? qa : pd > static_cast<double>(b) ? qb : 0.0;
}

__global__ void __launch_bounds__(kThreads256) points_target_kernel(
    const float* __restrict__ labels, const int32_t* __restrict__ label_class, int64_t M, int L,
    const int64_t* __restrict__ index, int N, const float* __restrict__ params, int C, int Ho, int Wo, double radius,
    float* __restrict__ out, int tiles_x, int tiles_y, int groups, int64_t units) {
  __shared__ float cand[kClasses][kCand][2];
  __shared__ double wave_up[4][kClasses];
  __shared__ int wave_cnt[4][kClasses];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t below = (uint64_t(1) << lane) - 1;
  const double inf = __builtin_huge_val();

  for (int64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
    const int tx = static_cast<int>(unit % tiles_x);
    int64_t r = unit / tiles_x;
    const int ty = static_cast<int>(r % tiles_y);
    r /= tiles_y;
    const int g = static_cast<int>(r % groups);
    const int n = static_cast<int>(r / groups);
    const int c0 = g * kClasses;
    const int x_lo = tx * kTileW, y_lo = ty * kTileH;
    const int x_hi = (x_lo + kTileW < Wo ? x_lo + kTileW : Wo) - 1;
    const int y_hi = (y_lo + kTileH < Ho ? y_lo + kTileH : Ho) - 1;
    const int px = x_lo + (tid & 15) * 4, py = y_lo + (tid >> 4);

    double m[kClasses][4];
    bool has[kClasses];
#pragma unroll
    for (int k = 0; k < kClasses; ++k) {
      has[k] = false;
#pragma unroll
      for (int p = 0; p < 4; ++p) m[k][p] = inf;
    }

    const int64_t idx = index[n];
    if (idx >= 0 && idx < M) {   // (uniform over the workgroup)
      const float* lab = labels + idx * L * 2;
      const int32_t* cls = label_class + idx * L;
      const float* P = params + int64_t(n) * UNETPP_WARP_PARAMS;

      // sweep 1: U[k] = min over the labels of class c0 + k of up_l
      double U[kClasses];
#pragma unroll
      for (int k = 0; k < kClasses; ++k) U[k] = inf;
      for (int64_t l = tid; l < L; l += kThreads256) {
        const int c = cls[l];
        float xo, yo;
        if (c < c0 || c >= c0 + kClasses || c >= C || !label_at(lab, P, l, xo, yo)) continue;
        const int k = c - c0;
        double lx, ux, ly, uy;
        axis_bounds(xo, x_lo, x_hi, lx, ux);
        axis_bounds(yo, y_lo, y_hi, ly, uy);
        const double up = ux + uy;
#pragma unroll
        for (int j = 0; j < kClasses; ++j) U[j] = (j == k && up < U[j]) ? up : U[j];
      }
#pragma unroll
      for (int k = 0; k < kClasses; ++k) {
        const double w = wave_min(U[k]);
        if (lane == 0) wave_up[wave][k] = w;
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < kClasses; ++k) {
        double u = wave_up[0][k];
#pragma unroll
        for (int w = 1; w < 4; ++w) u = wave_up[w][k] < u ? wave_up[w][k] : u;
        U[k] = u;
      }

      // sweep 2: chunks of 256 labels; the survivors of a chunk are compacted into the lists and folded into the
      // running minima of the pixels before the next chunk overwrites them (a round)
      for (int64_t base = 0; base < L; base += kThreads256) {
        const int64_t l = base + tid;
        int k = -1;
        float xo = 0.f, yo = 0.f;
        if (l < L) {
          const int c = cls[l];
          if (c >= c0 && c < c0 + kClasses && c < C && label_at(lab, P, l, xo, yo)) {
            const int kk = c - c0;
            double lx, ux, ly, uy;
            axis_bounds(xo, x_lo, x_hi, lx, ux);
            axis_bounds(yo, y_lo, y_hi, ly, uy);
            const double lo = lx + ly;
#pragma unroll
            for (int j = 0; j < kClasses; ++j)
              if (j == kk && lo <= U[j]) k = kk;
          }
        }
        uint64_t mask[kClasses];
#pragma unroll
        for (int j = 0; j < kClasses; ++j) {
          mask[j] = __ballot(k == j);
          if (lane == 0) wave_cnt[wave][j] = __popcll(mask[j]);
        }
        __syncthreads();   // (also: every thread has left the previous chunk's fold, the lists are free)
        int count[kClasses];
#pragma unroll
        for (int j = 0; j < kClasses; ++j) {
          int before = 0, total = 0;
#pragma unroll
          for (int w = 0; w < 4; ++w) {
            const int cnt = wave_cnt[w][j];
            before += w < wave ? cnt : 0;
            total += cnt;
          }
          if (k == j) {
            const int slot = before + __popcll(mask[j] & below);   // < 256: at most one label per thread
            cand[j][slot][0] = xo;
            cand[j][slot][1] = yo;
          }
          count[j] = total;
          has[j] = has[j] || total > 0;
        }
        __syncthreads();   // (the wave counts are free for the next chunk)
        // (the fold below and the store at the end are spelled out here and again in paste_target_kernel: behind a
        // function this kernel takes 131 vector registers, past the 128 at which a SIMD holds one wave fewer)
        const double yd = static_cast<double>(py);
#pragma unroll
        for (int j = 0; j < kClasses; ++j) {
          for (int i = 0; i < count[j]; ++i) {
            const double cx = static_cast<double>(cand[j][i][0]), cy = static_cast<double>(cand[j][i][1]);
            const double dy = yd - cy;
            const double dy2 = dy * dy;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
              const double dx = static_cast<double>(px + p) - cx;
              const double d = dx * dx + dy2;
              m[j][p] = d < m[j][p] ? d : m[j][p];
            }
          }
        }
      }
    }

    if (py <= y_hi && px <= x_hi) {
#pragma unroll
      for (int k = 0; k < kClasses; ++k) {
        if (c0 + k >= C) continue;
        f32x4 v;
#pragma unroll
        for (int p = 0; p < 4; ++p) v[p] = has[k] ? nearest_value(m[k][p], radius) : 0.f;
        float* dst = out + ((int64_t(n) * C + (c0 + k)) * Ho + py) * Wo + px;
        if (px + 3 <= x_hi && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
          *reinterpret_cast<f32x4*>(dst) = v;
        } else {
#pragma unroll
          for (int p = 0; p < 4; ++p)
            if (px + p <= x_hi) dst[p] = v[p];
        }
      }
    }
    __syncthreads();   // the lists and the wave slots are the next unit's
  }
}

// target_ignore_kernel: marks the ignored elements of a target that points_target_kernel (or anything else) wrote.
// A unit is (sample, 64 x 16 tile), a thread 4 consecutive x of one row, all classes.  The source position of a window
// pixel is window.h's map_inverse, the function the warp samples by; the frame test and the stores of -1 are this
// kernel's own, as they are target_ignore_mask_kernel's in mask.hip.  The tests are plain float32
// comparisons, so a NaN position or a NaN / reversed rectangle (padding) is never inside a rectangle and always
// outside the frame.  The frame's R rectangles pass through LDS kRectChunk at a time; per pixel a thread keeps one bit
// per class of the current group of 32 classes (one group for C <= 32) and one for "every class".  The kernel only
// stores -1.0f where it ignores and reads nothing of target: idempotent stores of one constant, no atomics, the same
// bits on any grid.
constexpr int kRectChunk = 256;

__global__ void __launch_bounds__(kThreads256) target_ignore_kernel(
    const float* __restrict__ rects, const int32_t* __restrict__ rect_class, int64_t M, int R,
    const int64_t* __restrict__ index, const float* __restrict__ params, int C, int Ho, int Wo, int Hs, int Ws, int outside,
    float* __restrict__ target, int tiles_x, int tiles_y, int64_t units) {
  __shared__ float rc[kRectChunk][4];
  __shared__ int32_t rcls[kRectChunk];
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
    const bool mine = py <= y_hi && px <= x_hi;

    const int64_t idx = index[n];
    const bool live = idx >= 0 && idx < M;   // (uniform over the workgroup)
    const float* P = params + int64_t(n) * UNETPP_WARP_PARAMS;
    const float yf = static_cast<float>(py);
    float xs[4], ys[4];
    unsigned every = 0;   // bit p: pixel px + p is ignored for every class
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const float xf = static_cast<float>(px + p);
      float x, y;
      map_inverse(P, xf, yf, x, y);
      xs[p] = x, ys[p] = y;
      const bool in = live && 0.f <= xs[p] && xs[p] <= x_max && 0.f <= ys[p] && ys[p] <= y_max;
      every |= (outside != 0 && !in) ? (1u << p) : 0u;
    }

    const int n_rect = live ? R : 0;
    for (int c0 = 0; c0 < C; c0 += kClassGroup) {
      uint32_t cls_bits[4] = {0u, 0u, 0u, 0u};   // bit k of [p]: pixel px + p is ignored for class c0 + k
      for (int base = 0; base < n_rect; base += kRectChunk) {
        __syncthreads();   // (the previous chunk, group or unit has been read)
        const int cnt = n_rect - base < kRectChunk ? n_rect - base : kRectChunk;
        if (tid < cnt) {
          const int64_t row = idx * R + base + tid;
#pragma unroll
          for (int j = 0; j < 4; ++j) rc[tid][j] = rects[row * 4 + j];
          rcls[tid] = rect_class[row];
        }
        __syncthreads();
        for (int i = 0; i < cnt; ++i) {
          const float x0 = rc[i][0], y0 = rc[i][1], x1 = rc[i][2], y1 = rc[i][3];
          const int k = rcls[i];
          const bool all = k == -1;
          const bool here = k >= c0 && k < c0 + kClassGroup && k < C;
          if (!all && !here) continue;   // (uniform: an LDS broadcast)
          const uint32_t bit = here ? (1u << (k - c0)) : 0u;
#pragma unroll
          for (int p = 0; p < 4; ++p) {
            const bool in = x0 <= xs[p] && xs[p] <= x1 && y0 <= ys[p] && ys[p] <= y1;
            if (in) {
              cls_bits[p] |= bit;
              if (all) every |= 1u << p;
            }
          }
        }
      }
      if (mine) {
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
}

// window origin along one axis from its centre pixel: inside the frame, or a centred pad of a frame below the window
__device__ __forceinline__ int window_origin(double centre, int src, int win) {
  if (src < win) return -((win - src) / 2);
  const double o = centre - static_cast<double>(win / 2), hi = static_cast<double>(src - win);
  return static_cast<int>(!(o >= 0.0) ? 0.0 : o > hi ? hi : o);
}

__global__ void __launch_bounds__(kThreads256) crops_draw_kernel(
    float* __restrict__ params, int64_t* __restrict__ index, int32_t* __restrict__ origin, int N, uint64_t seed, int M,
    int Hs, int Ws, int Ho, int Wo, const int32_t* __restrict__ centre_frame, const float* __restrict__ centre_xy, int V,
    float p_object, float jitter_x, float jitter_y, unetpp_augment a) {
  const int n = blockIdx.x * kThreads256 + threadIdx.x;
  if (n >= N) return;
  // which window: a row of the centre table with jitter, or any pixel of any frame
  const bool object = V > 0 && static_cast<float>(sample_uniform(seed, n, 9)) < p_object;
  const double u10 = sample_uniform(seed, n, 10), u11 = sample_uniform(seed, n, 11), u12 = sample_uniform(seed, n, 12);
  int frame;
  double cx, cy;
  if (object) {
    const int j = static_cast<int>(pick(u10, V));
    frame = centre_frame[j];
    cx = floor(static_cast<double>(centre_xy[2 * int64_t(j)]) + 0.5);
    cy = floor(static_cast<double>(centre_xy[2 * int64_t(j) + 1]) + 0.5);
    cx += floor((2.0 * u11 - 1.0) * static_cast<double>(jitter_x) + 0.5);
    cy += floor((2.0 * u12 - 1.0) * static_cast<double>(jitter_y) + 0.5);
  } else {
    frame = static_cast<int>(pick(u10, M));
    cx = pick(u11, Ws);
    cy = pick(u12, Hs);
  }
  const int ox = window_origin(cx, Ws, Wo), oy = window_origin(cy, Hs, Ho);
  index[n] = frame >= 0 && frame < M ? frame : -1;
  origin[2 * int64_t(n)] = ox;
  origin[2 * int64_t(n) + 1] = oy;

  // the source centre: the window's centre in the frame
  const double cox = 0.5 * (Wo - 1), coy = 0.5 * (Ho - 1);
  augment_row(params + int64_t(n) * UNETPP_WARP_PARAMS, seed, n, a, static_cast<double>(ox) + cox,
              static_cast<double>(oy) + coy, cox, coy);
}

}  // namespace
}  // namespace unetpp

using namespace unetpp;

extern "C" int unetpp_points_target(const float* labels, const int32_t* label_class, int64_t M, int32_t L,
                                    const int64_t* index, int32_t N, const float* params, int32_t C, int32_t Ho,
                                    int32_t Wo, float radius, float* out, void* stream) {
  if (labels == nullptr || label_class == nullptr || index == nullptr || params == nullptr || out == nullptr)
    return UNETPP_EINVAL;
  if (M <= 0 || L <= 0 || N <= 0 || C <= 0 || Ho <= 0 || Wo <= 0) return UNETPP_EINVAL;
  if (C > kMaxClasses || Ho > kMaxSide || Wo > kMaxSide) return UNETPP_EINVAL;
  if (!(radius > 0.f)) return UNETPP_EINVAL;   // (a NaN too)
  const int tiles_x = (Wo + kTileW - 1) / kTileW, tiles_y = (Ho + kTileH - 1) / kTileH;
  const int groups = (C + kClasses - 1) / kClasses;
  const int64_t units = int64_t(N) * groups * tiles_y * tiles_x;
  hipLaunchKernelGGL(points_target_kernel, dim3(capped_grid(units)), dim3(kThreads256), 0,
                     static_cast<hipStream_t>(stream), labels, label_class, M, L, index, N, params, C, Ho, Wo,
                     static_cast<double>(radius), out, tiles_x, tiles_y, groups, units);
  note_kernel("points_target");
  return launch_status();
}

extern "C" int unetpp_target_ignore(const float* rects, const int32_t* rect_class, int64_t M, int32_t R,
                                    const int64_t* index, int32_t N, const float* params, int32_t C, int32_t Ho,
                                    int32_t Wo, int32_t Hs, int32_t Ws, int32_t outside, float* target, void* stream) {
  if (index == nullptr || params == nullptr || target == nullptr) return UNETPP_EINVAL;
  if (M <= 0 || R < 0 || N <= 0 || C <= 0 || Ho <= 0 || Wo <= 0 || Hs <= 0 || Ws <= 0) return UNETPP_EINVAL;
  if (R > 0 && (rects == nullptr || rect_class == nullptr)) return UNETPP_EINVAL;
  if (C > kMaxClasses || Ho > kMaxSide || Wo > kMaxSide || Hs > kMaxSide || Ws > kMaxSide) return UNETPP_EINVAL;
  if (R == 0 && outside == 0) return UNETPP_OK;   // nothing to mark
  const int tiles_x = (Wo + kTileW - 1) / kTileW, tiles_y = (Ho + kTileH - 1) / kTileH;
  const int64_t units = int64_t(N) * tiles_y * tiles_x;
  hipLaunchKernelGGL(target_ignore_kernel, dim3(capped_grid(units)), dim3(kThreads256), 0,
                     static_cast<hipStream_t>(stream), rects, rect_class, M, R, index, params, C, Ho, Wo, Hs, Ws,
                     outside, target, tiles_x, tiles_y, units);
  note_kernel("target_ignore");
  return launch_status();
}

extern "C" int unetpp_crops_draw(float* params, int64_t* index, int32_t* origin, int32_t N, uint64_t seed, int32_t M,
                                 int32_t Hs, int32_t Ws, int32_t Ho, int32_t Wo, const int32_t* centre_frame,
                                 const float* centre_xy, int32_t V, float p_object, float jitter_x, float jitter_y,
                                 const unetpp_augment* augment, void* stream) {
  if (params == nullptr || index == nullptr || origin == nullptr || augment == nullptr) return UNETPP_EINVAL;
  if (N <= 0 || M <= 0 || Hs <= 0 || Ws <= 0 || Ho <= 0 || Wo <= 0 || V < 0) return UNETPP_EINVAL;
  if (Hs > kMaxSide || Ws > kMaxSide || Ho > kMaxSide || Wo > kMaxSide) return UNETPP_EINVAL;
  if (V > 0 && (centre_frame == nullptr || centre_xy == nullptr)) return UNETPP_EINVAL;
  if (!(p_object >= 0.f) || !(jitter_x >= 0.f) || !(jitter_y >= 0.f)) return UNETPP_EINVAL;   // (a NaN too)
  if (!(augment->scale_lo > 0.f) || !(augment->scale_hi > 0.f)) return UNETPP_EINVAL;
  if (augment->max_tx != 0.f || augment->max_ty != 0.f) return UNETPP_EINVAL;   // a window's place is its origin
  if (augment->rot90 != 0 && Ho != Wo) return UNETPP_EINVAL;
  const unsigned grid = static_cast<unsigned>((N + kThreads256 - 1) / kThreads256);
  hipLaunchKernelGGL(crops_draw_kernel, dim3(grid), dim3(kThreads256), 0, static_cast<hipStream_t>(stream), params,
                     index, origin, N, seed, M, Hs, Ws, Ho, Wo, centre_frame, centre_xy, V, p_object, jitter_x, jitter_y,
                     *augment);
  note_kernel("crops_draw");
  return launch_status();
}
