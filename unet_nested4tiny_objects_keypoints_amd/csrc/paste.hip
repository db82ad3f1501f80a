// Copy-paste augmentation of tiny objects for scene training (crops.py: ObjectPaste): where the patches of
// a batch go (paste_draw_kernel), the pixels (paste_apply_kernel) and the pasted labels' share of the target maps
// (paste_target_kernel).  They run between the launches of crops.hip and loader.hip: draw, warp, PASTE DRAW, PASTE
// APPLY, targets, PASTE TARGET, ignore.
//
// A patch is the (2R+1) x (2R+1) whole pixels about the rounded centre of a row of the source table, under one of the
// eight flips and quarter turns (a code), blended into the window by a radial weight table the host made.  Code c:
// q = c & 3 quarter turns, then a flip in x when c & 4 -- T_c = D Q^q with Q^q = [[qc, -qs], [qs, qc]] as whole numbers,
// the matrices of window.h's augment_row.  A source offset (i, j) from the source centre lands at T_c (i, j) from the
// destination centre, so destination offset (i, j) reads source offset T_c^-1 (i, j) = Q^-q D (i, j); the label's
// sub-pixel offset goes through T_c like the pixels.
//
// paste_draw_kernel: one workgroup per window.  Threads k < K draw slot k's five uniforms and test its source row;
// every thread then walks the frame's labels once and marks, in a 64-bit mask, the slots a label is too close to; the
// masks are OR-ed over the workgroup through one LDS flag per slot; thread 0 accepts the slots in order against the
// earlier accepted ones.  Accepted patches of a window are pairwise disjoint, so the other two kernels need no order
// among them.
//
// paste_apply_kernel: a unit is (window, slot), its threads stride over (channel, row, column) of the patch.  Every row
// is checked again against the table, the frame, the window and the code range before an address is formed.
//
// paste_target_kernel: the tiles and thread layout of target_ignore_kernel; the K rows of a window pass through LDS
// once per unit; per class that has a live slot, the least squared distance (float64, the fold of
// points_target_kernel) and its nearest_value, one sqrt and one exp per pixel, stored only where it exceeds a target
// that is not negative.
//
// The label positions, the frame store, the pixel's normalisation, the draws and the grid are window.h's, shared with
// loader.hip, crops.hip and mask.hip.
//
// No atomics; implicit contraction is off; every offset into a store, the inputs or the target is 64-bit; a unit's
// result does not depend on which workgroup computes it: the same bits on any grid.
#include "window.h"

#pragma clang fp contract(off)

namespace unetpp {
namespace {

constexpr int kSlots = UNETPP_PASTE_MAX_SLOTS;

// uniform j (0..7) of slot k of window n
__device__ __forceinline__ double slot_uniform(uint64_t seed, int n, int k, int j) {
  return uniform24(seed, (static_cast<uint64_t>(n) * kSlots + k) * 8 + j + 1);
}

// (qc, qs, dx) of a code: Q^q = [[qc, -qs], [qs, qc]], dx = -1 with the flip in x
__device__ __forceinline__ void code_parts(int code, int& qc, int& qs, int& dx) {
  const int q = code & 3;
  qc = q == 0 ? 1 : q == 2 ? -1 : 0;
  qs = q == 1 ? 1 : q == 3 ? -1 : 0;
  dx = (code & 4) != 0 ? -1 : 1;
}

// row t of the source table: its frame and rounded centre; false when the row cannot be pasted (frame or class out of
// range, a coordinate that is not finite, a patch that is not inside the frame).  The comparisons are on doubles, so a
// NaN or an infinity fails them before anything is converted to an integer.
__device__ __forceinline__ bool source_row(const int32_t* __restrict__ src_frame, const float* __restrict__ src_xy,
                                           const int32_t* __restrict__ src_class, int64_t t, int64_t M, int C, int Hs,
                                           int Ws, int R, int& frame, int& cx, int& cy, int& cls) {
  frame = src_frame[t];
  cls = src_class[t];
  const double fx = floor(static_cast<double>(src_xy[2 * t]) + 0.5);
  const double fy = floor(static_cast<double>(src_xy[2 * t + 1]) + 0.5);
  const bool ok = frame >= 0 && frame < M && cls >= 0 && cls < C && fx >= static_cast<double>(R) &&
                  fx <= static_cast<double>(Ws - 1 - R) && fy >= static_cast<double>(R) &&
                  fy <= static_cast<double>(Hs - 1 - R);
  cx = ok ? static_cast<int>(fx) : 0;
  cy = ok ? static_cast<int>(fy) : 0;
  return ok;
}

__global__ void __launch_bounds__(kThreads256) paste_draw_kernel(
    int32_t* __restrict__ src, int32_t* __restrict__ dst, int32_t* __restrict__ code, float* __restrict__ xy,
    int32_t* __restrict__ cls, int N, int K, uint64_t seed, const int32_t* __restrict__ src_frame,
    const float* __restrict__ src_xy, const int32_t* __restrict__ src_class, int T, const float* __restrict__ labels,
    const int32_t* __restrict__ label_class, int64_t M, int L, const int64_t* __restrict__ index,
    const float* __restrict__ params, int C, int Hs, int Ws, int Ho, int Wo, float p, int R, double clearance2,
    int dihedral) {
  __shared__ int s_px[kSlots], s_py[kSlots], s_row[kSlots], s_ok[kSlots], s_near[kSlots];
  const int tid = threadIdx.x;

  for (int n = blockIdx.x; n < N; n += gridDim.x) {
    const int64_t idx = index[n];
    const bool live = idx >= 0 && idx < M;   // (uniform over the workgroup)
    int my_code = 0;
    if (tid < K) {
      const double u0 = slot_uniform(seed, n, tid, 0), u1 = slot_uniform(seed, n, tid, 1);
      const double u2 = slot_uniform(seed, n, tid, 2), u3 = slot_uniform(seed, n, tid, 3);
      const double u4 = slot_uniform(seed, n, tid, 4);
      const int t = static_cast<int>(pick(u1, T));
      my_code = dihedral != 0 ? static_cast<int>(8.0 * u2) : 0;
      int frame, cx, cy, c;
      const bool row_ok = source_row(src_frame, src_xy, src_class, t, M, C, Hs, Ws, R, frame, cx, cy, c);
      s_px[tid] = R + static_cast<int>(pick(u3, Wo - 2 * R));
      s_py[tid] = R + static_cast<int>(pick(u4, Ho - 2 * R));
      s_row[tid] = t;
      s_ok[tid] = (static_cast<float>(u0) < p && live && row_ok) ? 1 : 0;
      s_near[tid] = 0;
    }
    __syncthreads();

    // one walk over the frame's labels: bit k of near = a label lies within the clearance of slot k's centre
    uint64_t near = 0;
    if (live) {
      const float* lab = labels + idx * L * 2;
      const int32_t* lc = label_class + idx * L;
      const float* P = params + int64_t(n) * UNETPP_WARP_PARAMS;
      for (int64_t l = tid; l < L; l += kThreads256) {
        const float x = lab[2 * l], y = lab[2 * l + 1];
        if (lc[l] < 0 || x < 0.f || y < 0.f) continue;   // (!label_valid(x, y) spelled out: 2 scalar spills fewer)
        float xo, yo;
        map_forward(P, x, y, xo, yo);
        for (int k = 0; k < K; ++k) {
          if (s_ok[k] == 0) continue;   // (uniform: an LDS broadcast)
          const double dx = static_cast<double>(xo) - static_cast<double>(s_px[k]);
          const double dy = static_cast<double>(yo) - static_cast<double>(s_py[k]);
          if (dx * dx + dy * dy < clearance2) near |= uint64_t(1) << k;
        }
      }
    }
    for (int k = 0; k < K; ++k)   // the OR over the workgroup: stores of one value, whoever makes them
      if ((near >> k) & 1u) s_near[k] = 1;
    __syncthreads();

    if (tid == 0) {   // slots in order: accepted patches keep a Chebyshev distance above 2R from one another
      for (int k = 0; k < K; ++k) {
        bool ok = s_ok[k] != 0 && s_near[k] == 0;
        for (int e = 0; ok && e < k; ++e) {
          if (s_ok[e] == 0) continue;
          const int ax = s_px[k] - s_px[e], ay = s_py[k] - s_py[e];
          const int cheb = max(ax < 0 ? -ax : ax, ay < 0 ? -ay : ay);
          ok = cheb > 2 * R;
        }
        s_ok[k] = ok ? 1 : 0;
      }
    }
    __syncthreads();

    if (tid < K) {
      const int64_t o = int64_t(n) * K + tid;
      const bool ok = s_ok[tid] != 0;
      const int64_t t = s_row[tid];
      float lx = -1.f, ly = -1.f;
      if (ok) {   // the label: dst + T_code (src_xy - floor(src_xy + 0.5)); the differences are exact
        int qc, qs, dx;
        code_parts(my_code, qc, qs, dx);
        const double sx = static_cast<double>(src_xy[2 * t]), sy = static_cast<double>(src_xy[2 * t + 1]);
        const double ox = sx - floor(sx + 0.5), oy = sy - floor(sy + 0.5);
        const double tx = static_cast<double>(dx) * (static_cast<double>(qc) * ox - static_cast<double>(qs) * oy);
        const double ty = static_cast<double>(qs) * ox + static_cast<double>(qc) * oy;
        lx = static_cast<float>(static_cast<double>(s_px[tid]) + tx);
        ly = static_cast<float>(static_cast<double>(s_py[tid]) + ty);
      }
      src[o] = ok ? static_cast<int32_t>(t) : -1;
      dst[2 * o] = s_px[tid];
      dst[2 * o + 1] = s_py[tid];
      code[o] = my_code;
      xy[2 * o] = lx;
      xy[2 * o + 1] = ly;
      cls[o] = ok ? src_class[t] : -1;
    }
    __syncthreads();   // the slots are the next window's
  }
}

template <bool U8>
__global__ void __launch_bounds__(kThreads256) paste_apply_kernel(
    float* __restrict__ inputs, int N, int K, int Cin, int Ho, int Wo, const int32_t* __restrict__ src,
    const int32_t* __restrict__ dst, const int32_t* __restrict__ code, const int32_t* __restrict__ src_frame,
    const float* __restrict__ src_xy, const int32_t* __restrict__ src_class, int T, const void* __restrict__ store,
    int64_t M, int Hs, int Ws, int C, const float* __restrict__ params, const float* __restrict__ mul,
    const float* __restrict__ add, const float* __restrict__ alpha, int R, int64_t units) {
  const int side = 2 * R + 1;
  const int per = side * side * Cin;
  // element strides of the store: to the next pixel in x, the next row, the next channel
  const int64_t sx = U8 ? Cin : 1;
  const int64_t sy = int64_t(Ws) * sx;
  const int64_t sc = U8 ? 1 : int64_t(Hs) * Ws;
  const int64_t sample = int64_t(Hs) * Ws * Cin;

  for (int64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {   // everything below is uniform over the unit
    const int n = static_cast<int>(unit / K);
    const int64_t t = src[unit];
    const int px = dst[2 * unit], py = dst[2 * unit + 1], cd = code[unit];
    if (t < 0 || t >= T || cd < 0 || cd > 7) continue;
    if (px < R || px > Wo - 1 - R || py < R || py > Ho - 1 - R) continue;
    int frame, cx, cy, cls;
    if (!source_row(src_frame, src_xy, src_class, t, M, C, Hs, Ws, R, frame, cx, cy, cls)) continue;
    int qc, qs, dx;
    code_parts(cd, qc, qs, dx);
    const float* P = params + int64_t(n) * UNETPP_WARP_PARAMS;
    const float gain = P[12], bias = P[13];
    const int64_t base = int64_t(frame) * sample + int64_t(cy) * sy + int64_t(cx) * sx;

    for (int e = threadIdx.x; e < per; e += kThreads256) {
      const int i = e % side - R;
      const int r = e / side;
      const int j = r % side - R;
      const int c = r / side;
      const float a = alpha[(j + R) * side + (i + R)];
      // the source offset of destination offset (i, j): Q^-q D (i, j)
      const int fi = dx * i;
      const int si = qc * fi + qs * j, sj = qc * j - qs * fi;
      const float v = load_src<U8>(store, base + int64_t(sj) * sy + int64_t(si) * sx + c * sc);
      const float pv = window_value(v, mul[c], add[c], gain, bias);
      float* out = inputs + ((int64_t(n) * Cin + c) * Ho + (py + j)) * Wo + (px + i);
      const float d = *out;
      *out = a == 1.f ? pv : a == 0.f ? d : d + a * (pv - d);
    }
  }
}

constexpr int kQuad = 4;

__global__ void __launch_bounds__(kThreads256) paste_target_kernel(
    float* __restrict__ target, int N, int K, int C, int Ho, int Wo, const float* __restrict__ xy,
    const int32_t* __restrict__ cls, double radius, int tiles_x, int tiles_y, int64_t units) {
  __shared__ float s_x[kSlots], s_y[kSlots];
  __shared__ int s_cls[kSlots], s_first[kSlots];
  const int tid = threadIdx.x;

  for (int64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
    const int tx = static_cast<int>(unit % tiles_x);
    const int64_t r = unit / tiles_x;
    const int ty = static_cast<int>(r % tiles_y);
    const int n = static_cast<int>(r / tiles_y);
    const int x_lo = tx * kTileW, y_lo = ty * kTileH;
    const int x_hi = (x_lo + kTileW < Wo ? x_lo + kTileW : Wo) - 1;
    const int y_hi = (y_lo + kTileH < Ho ? y_lo + kTileH : Ho) - 1;
    const int px = x_lo + (tid & 15) * kQuad, py = y_lo + (tid >> 4);
    const bool mine = py <= y_hi && px <= x_hi;

    __syncthreads();   // (the previous unit has read its rows)
    int is_live = 0;
    if (tid < K) {
      const int64_t o = int64_t(n) * K + tid;
      const int c = cls[o];
      is_live = (c >= 0 && c < C) ? 1 : 0;
      s_x[tid] = xy[2 * o];
      s_y[tid] = xy[2 * o + 1];
      s_cls[tid] = is_live ? c : -1;
    }
    if (__syncthreads_or(is_live) == 0) continue;   // no live slot: nothing of this window is touched (uniform)
    if (tid < K) {   // the first slot of every class that has one
      int first = s_cls[tid] >= 0 ? 1 : 0;
      for (int e = 0; e < tid; ++e) first = s_cls[e] == s_cls[tid] ? 0 : first;
      s_first[tid] = first;
    }
    __syncthreads();

    const double yd = static_cast<double>(py);
    for (int k = 0; k < K; ++k) {
      if (s_first[k] == 0) continue;   // (uniform: an LDS broadcast)
      const int c = s_cls[k];
      double m[kQuad];
#pragma unroll
      for (int p = 0; p < kQuad; ++p) m[p] = __builtin_huge_val();
      for (int e = k; e < K; ++e) {
        if (s_cls[e] != c) continue;
        const double cx = static_cast<double>(s_x[e]), cy = static_cast<double>(s_y[e]);
        const double dy = yd - cy;
        const double dy2 = dy * dy;
#pragma unroll
        for (int p = 0; p < kQuad; ++p) {
          const double dx = static_cast<double>(px + p) - cx;
          const double d = dx * dx + dy2;
          m[p] = d < m[p] ? d : m[p];
        }
      }
      if (!mine) continue;
      float* row = target + ((int64_t(n) * C + c) * Ho + py) * Wo + px;
      const bool vec = px + 3 <= x_hi && (reinterpret_cast<uintptr_t>(row) & 15) == 0;
      f32x4 t = {0.f, 0.f, 0.f, 0.f};
      if (vec) {
        t = *reinterpret_cast<const f32x4*>(row);
      } else {
#pragma unroll
        for (int p = 0; p < kQuad; ++p)
          if (px + p <= x_hi) t[p] = row[p];
      }
      unsigned change = 0;
#pragma unroll
      for (int p = 0; p < kQuad; ++p) {
        const float v = nearest_value(m[p], radius);
        if (v > t[p] && !(t[p] < 0.f) && px + p <= x_hi) {
          t[p] = v;
          change |= 1u << p;
        }
      }
      if (change == 0) continue;
      if (vec) {
        *reinterpret_cast<f32x4*>(row) = t;   // the unchanged lanes carry the bits just read
      } else {
#pragma unroll
        for (int p = 0; p < kQuad; ++p)
          if ((change >> p) & 1u) row[p] = t[p];
      }
    }
  }
}

}  // namespace
}  // namespace unetpp

using namespace unetpp;

extern "C" int unetpp_paste_draw(int32_t* src, int32_t* dst, int32_t* code, float* xy, int32_t* cls, int32_t N,
                                 int32_t K, uint64_t seed, const int32_t* src_frame, const float* src_xy,
                                 const int32_t* src_class, int32_t T, const float* labels, const int32_t* label_class,
                                 int64_t M, int32_t L, const int64_t* index, const float* params, int32_t C, int32_t Hs,
                                 int32_t Ws, int32_t Ho, int32_t Wo, float p, int32_t R, float clearance,
                                 int32_t dihedral, void* stream) {
  if (src == nullptr || dst == nullptr || code == nullptr || xy == nullptr || cls == nullptr) return UNETPP_EINVAL;
  if (src_frame == nullptr || src_xy == nullptr || src_class == nullptr || labels == nullptr || label_class == nullptr ||
      index == nullptr || params == nullptr)
    return UNETPP_EINVAL;
  if (N <= 0 || K <= 0 || K > kSlots || T <= 0 || M <= 0 || L <= 0 || C <= 0 || C > kMaxClasses) return UNETPP_EINVAL;
  if (Hs <= 0 || Ws <= 0 || Hs > kMaxSide || Ws > kMaxSide || Ho > kMaxSide || Wo > kMaxSide) return UNETPP_EINVAL;
  if (R < 0 || R > UNETPP_PASTE_MAX_RADIUS || Ho < 2 * R + 1 || Wo < 2 * R + 1) return UNETPP_EINVAL;
  if (!(p >= 0.f) || !(clearance >= 0.f)) return UNETPP_EINVAL;   // (a NaN too)
  const double cl = static_cast<double>(clearance);
  hipLaunchKernelGGL(paste_draw_kernel, dim3(capped_grid(N)), dim3(kThreads256), 0, static_cast<hipStream_t>(stream),
                     src, dst, code, xy, cls, N, K, seed, src_frame, src_xy, src_class, T, labels, label_class, M, L,
                     index, params, C, Hs, Ws, Ho, Wo, p, R, cl * cl, dihedral);
  note_kernel("paste_draw");
  return launch_status();
}

extern "C" int unetpp_paste_apply(float* inputs, int32_t N, int32_t K, int32_t Cin, int32_t Ho, int32_t Wo,
                                  const int32_t* src, const int32_t* dst, const int32_t* code, const int32_t* src_frame,
                                  const float* src_xy, const int32_t* src_class, int32_t T, const void* store,
                                  int32_t store_type, int64_t M, int32_t Hs, int32_t Ws, int32_t C, const float* params,
                                  const float* mul, const float* add, const float* alpha, int32_t R, void* stream) {
  if (inputs == nullptr || src == nullptr || dst == nullptr || code == nullptr || src_frame == nullptr ||
      src_xy == nullptr || src_class == nullptr || store == nullptr || params == nullptr || mul == nullptr ||
      add == nullptr || alpha == nullptr)
    return UNETPP_EINVAL;
  if (N <= 0 || K <= 0 || K > kSlots || T <= 0 || M <= 0 || C <= 0 || C > kMaxClasses) return UNETPP_EINVAL;
  if (Cin <= 0 || Cin > UNETPP_WARP_MAX_C || Hs <= 0 || Ws <= 0 || Ho <= 0 || Wo <= 0) return UNETPP_EINVAL;
  if (Hs > kMaxSide || Ws > kMaxSide || Ho > kMaxSide || Wo > kMaxSide) return UNETPP_EINVAL;
  if (R < 0 || R > UNETPP_PASTE_MAX_RADIUS) return UNETPP_EINVAL;
  if (store_type != UNETPP_STORE_U8 && store_type != UNETPP_STORE_F32) return UNETPP_EINVAL;
  const int64_t units = int64_t(N) * K;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (store_type == UNETPP_STORE_U8) {
    hipLaunchKernelGGL(paste_apply_kernel<true>, dim3(capped_grid(units)), dim3(kThreads256), 0, st, inputs, N, K, Cin,
                       Ho, Wo, src, dst, code, src_frame, src_xy, src_class, T, store, M, Hs, Ws, C, params, mul, add,
                       alpha, R, units);
    note_kernel("paste_apply_u8");
  } else {
    hipLaunchKernelGGL(paste_apply_kernel<false>, dim3(capped_grid(units)), dim3(kThreads256), 0, st, inputs, N, K, Cin,
                       Ho, Wo, src, dst, code, src_frame, src_xy, src_class, T, store, M, Hs, Ws, C, params, mul, add,
                       alpha, R, units);
    note_kernel("paste_apply_f32");
  }
  return launch_status();
}

extern "C" int unetpp_paste_target(float* target, int32_t N, int32_t K, int32_t C, int32_t Ho, int32_t Wo,
                                   const float* xy, const int32_t* cls, float radius, void* stream) {
  if (target == nullptr || xy == nullptr || cls == nullptr) return UNETPP_EINVAL;
  if (N <= 0 || K <= 0 || K > kSlots || C <= 0 || C > kMaxClasses || Ho <= 0 || Wo <= 0) return UNETPP_EINVAL;
  if (Ho > kMaxSide || Wo > kMaxSide) return UNETPP_EINVAL;
  if (!(radius > 0.f)) return UNETPP_EINVAL;   // (a NaN too)
  const int tiles_x = (Wo + kTileW - 1) / kTileW, tiles_y = (Ho + kTileH - 1) / kTileH;
  const int64_t units = int64_t(N) * tiles_y * tiles_x;
  hipLaunchKernelGGL(paste_target_kernel, dim3(capped_grid(units)), dim3(kThreads256), 0,
                     static_cast<hipStream_t>(stream), target, N, K, C, Ho, Wo, xy, cls, static_cast<double>(radius),
                     tiles_x, tiles_y, units);
  note_kernel("paste_target");
  return launch_status();
}
