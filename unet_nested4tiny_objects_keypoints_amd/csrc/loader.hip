// Device-resident input pipeline: the decoded data set stays in HBM (uint8 [M, Hs, Ws, C] or float32 [M, C, Hs, Ws]) and
// ONE launch produces a training batch from it -- gather by a device index, affine warp (bilinear, constant fill),
// per-channel normalisation, contrast / brightness, NCHW fp32 out -- and carries the key-point labels through the same
// transform.  A second, tiny launch draws the per-sample transforms from a 64-bit seed.  The parameter row and its draw,
// the two maps, the label rule, the frame store's layout and the pixel's normalisation are window.h's: crops.hip,
// paste.hip and mask.hip place their labels, ignore marks and pasted pixels by the same definitions.
//
// warp_kernel: one thread produces 4 consecutive xo of one output row and loops over the channels; one 16-byte store per
// channel plane where the address is 16-byte aligned and the 4 pixels are inside the row, scalar stores otherwise (the row
// tail, a misaligned row).  Source pixels are plain global loads: under a rotation the gather is irregular and is left
// to L2.  There is one code path, and no special case for whole-pixel maps: their weights are exactly 0 and 1 and
// fill * 0 = 0, so the output is the source pixel bit for bit.  Implicit contraction is off: every operation is rounded
// once, on the vector and on the scalar path alike.  No atomics, no LDS; every store offset is 64-bit.
// A neighbour outside the frame contributes `fill`; its address is never formed into a load.  A position so far outside
// that its floor does not fit the frame's index range (or a NaN) is an all-fill pixel.
#include "window.h"

#pragma clang fp contract(off)

namespace unetpp {
namespace {

template <bool U8>
__global__ void __launch_bounds__(kThreads256) warp_kernel(
    const void* __restrict__ store, int64_t M, int Hs, int Ws, int C, const int64_t* __restrict__ index, int N,
    const float* __restrict__ params, const float* __restrict__ mul, const float* __restrict__ add, float fill,
    float* __restrict__ out, int Ho, int Wo, const float* __restrict__ labels, int S, float* __restrict__ labels_out,
    uint8_t* __restrict__ inside) {
  const int64_t n_threads = int64_t(gridDim.x) * kThreads256;
  const int64_t tid = int64_t(blockIdx.x) * kThreads256 + threadIdx.x;

  if (labels != nullptr) {   // one label per thread: forward map, frame test, sentinel
    const int64_t n_labels = int64_t(N) * S;
    for (int64_t i = tid; i < n_labels; i += n_threads) {
      const int n = static_cast<int>(i / S);
      const int64_t s = i - int64_t(n) * S;
      const int64_t idx = index[n];
      float xo = -1.f, yo = -1.f;
      uint8_t in = 0;
      if (idx >= 0 && idx < M) {
        const float* L = labels + (idx * S + s) * 2;
        const float x = L[0], y = L[1];
        if (label_valid(x, y)) {
          map_forward(params + int64_t(n) * UNETPP_WARP_PARAMS, x, y, xo, yo);
          in = xo >= 0.f && xo <= static_cast<float>(Wo - 1) && yo >= 0.f && yo <= static_cast<float>(Ho - 1);
        }
      }
      labels_out[i * 2] = xo;
      labels_out[i * 2 + 1] = yo;
      inside[i] = in;
    }
  }

  const int quads_x = (Wo + 3) >> 2;
  const int64_t n_quads = int64_t(N) * Ho * quads_x;
  // element strides of the store: to the next pixel in x, the next row, the next channel
  const int64_t sx = U8 ? C : 1;
  const int64_t sy = int64_t(Ws) * sx;
  const int64_t sc = U8 ? 1 : int64_t(Hs) * Ws;
  const int64_t sample = int64_t(Hs) * Ws * C;
  for (int64_t t = tid; t < n_quads; t += n_threads) {
    const int xo0 = static_cast<int>(t % quads_x) * 4;
    const int64_t row = t / quads_x;
    const int yo = static_cast<int>(row % Ho);
    const int n = static_cast<int>(row / Ho);
    const float* P = params + int64_t(n) * UNETPP_WARP_PARAMS;
    const float inv[6] = {P[0], P[1], P[2], P[3], P[4], P[5]}, gain = P[12], bias = P[13];   // read once per quad
    const int64_t idx = index[n];
    const bool live = idx >= 0 && idx < M;
    const int64_t base = live ? idx * sample : 0;

    float w[4][4];
    bool ok[4][4];
    int64_t off[4];   // of neighbour (x0, y0), channel 0; meaningful wherever a neighbour is inside the frame
    const float yf = static_cast<float>(yo);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      float xs, ys;
      map_inverse(inv, static_cast<float>(xo0 + p), yf, xs, ys);
      const float x0f = floorf(xs), y0f = floorf(ys);
      const bool in_reach = x0f >= -2.f && x0f <= static_cast<float>(Ws) && y0f >= -2.f && y0f <= static_cast<float>(Hs);
      const int x0 = in_reach ? static_cast<int>(x0f) : -2;
      const int y0 = in_reach ? static_cast<int>(y0f) : -2;
      const float fx = in_reach ? xs - x0f : 0.f;
      const float fy = in_reach ? ys - y0f : 0.f;
      const float gx = 1.f - fx, gy = 1.f - fy;
      w[p][0] = gx * gy, w[p][1] = fx * gy, w[p][2] = gx * fy, w[p][3] = fx * fy;
      const bool vx0 = x0 >= 0 && x0 < Ws, vx1 = x0 + 1 >= 0 && x0 + 1 < Ws;
      const bool vy0 = live && y0 >= 0 && y0 < Hs, vy1 = live && y0 + 1 >= 0 && y0 + 1 < Hs;
      ok[p][0] = vx0 && vy0, ok[p][1] = vx1 && vy0, ok[p][2] = vx0 && vy1, ok[p][3] = vx1 && vy1;
      off[p] = base + int64_t(y0) * sy + int64_t(x0) * sx;
    }

    const bool row_full = xo0 + 4 <= Wo;
    for (int c = 0; c < C; ++c) {
      const float mc = mul[c], ac = add[c];
      f32x4 r;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int64_t o = off[p] + c * sc;
        float v00 = fill, v01 = fill, v10 = fill, v11 = fill;
        if (ok[p][0]) v00 = load_src<U8>(store, o);
        if (ok[p][1]) v01 = load_src<U8>(store, o + sx);
        if (ok[p][2]) v10 = load_src<U8>(store, o + sy);
        if (ok[p][3]) v11 = load_src<U8>(store, o + sy + sx);
        const float v = (w[p][0] * v00 + w[p][1] * v01) + (w[p][2] * v10 + w[p][3] * v11);
        r[p] = window_value(v, mc, ac, gain, bias);
      }
      float* dst = out + ((int64_t(n) * C + c) * Ho + yo) * Wo + xo0;
      if (row_full && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        *reinterpret_cast<f32x4*>(dst) = r;
      } else {
#pragma unroll
        for (int p = 0; p < 4; ++p)
          if (xo0 + p < Wo) dst[p] = r[p];
      }
    }
  }
}

__global__ void __launch_bounds__(kThreads256) draw_kernel(float* __restrict__ params, int N, uint64_t seed, int Hs,
                                                           int Ws, int Ho, int Wo, unetpp_augment a) {
  const int n = blockIdx.x * kThreads256 + threadIdx.x;
  if (n >= N) return;
  // the source centre: the frame's, moved by a whole number of pixels (uniforms 5 and 6)
  const double tx = floor((2.0 * sample_uniform(seed, n, 5) - 1.0) * static_cast<double>(a.max_tx) + 0.5);
  const double ty = floor((2.0 * sample_uniform(seed, n, 6) - 1.0) * static_cast<double>(a.max_ty) + 0.5);
  const double csx = 0.5 * (Ws - 1), csy = 0.5 * (Hs - 1);
  augment_row(params + int64_t(n) * UNETPP_WARP_PARAMS, seed, n, a, csx + tx, csy + ty, 0.5 * (Wo - 1), 0.5 * (Ho - 1));
}

}  // namespace
}  // namespace unetpp

using namespace unetpp;

extern "C" int unetpp_warp_batch(const void* store, int32_t store_type, int64_t M, int32_t Hs, int32_t Ws, int32_t C,
                                 const int64_t* index, int32_t N, const float* params, const float* mul,
                                 const float* add, float fill, float* out, int32_t Ho, int32_t Wo, const float* labels,
                                 int32_t S, float* labels_out, uint8_t* inside, void* stream) {
  if (store == nullptr || index == nullptr || params == nullptr || mul == nullptr || add == nullptr || out == nullptr)
    return UNETPP_EINVAL;
  if (M <= 0 || Hs <= 0 || Ws <= 0 || C <= 0 || N <= 0 || Ho <= 0 || Wo <= 0) return UNETPP_EINVAL;
  if (C > UNETPP_WARP_MAX_C || Hs > kMaxSide || Ws > kMaxSide || Ho > kMaxSide || Wo > kMaxSide) return UNETPP_EINVAL;
  if (store_type != UNETPP_STORE_U8 && store_type != UNETPP_STORE_F32) return UNETPP_EINVAL;
  if (labels != nullptr) {
    if (S <= 0 || labels_out == nullptr || inside == nullptr) return UNETPP_EINVAL;
  } else if (S != 0 || labels_out != nullptr || inside != nullptr) {
    return UNETPP_EINVAL;
  }
  const int64_t n_quads = int64_t(N) * Ho * ((Wo + 3) >> 2);
  const int64_t n_labels = int64_t(N) * S;
  const int64_t work = n_quads > n_labels ? n_quads : n_labels;
  const int64_t blocks = (work + kThreads256 - 1) / kThreads256;
  const unsigned grid = capped_grid(blocks);   // the rest of the work is grid-strided
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (store_type == UNETPP_STORE_U8) {
    hipLaunchKernelGGL(warp_kernel<true>, dim3(grid), dim3(kThreads256), 0, st, store, M, Hs, Ws, C, index, N, params,
                       mul, add, fill, out, Ho, Wo, labels, S, labels_out, inside);
    note_kernel("warp_u8");
  } else {
    hipLaunchKernelGGL(warp_kernel<false>, dim3(grid), dim3(kThreads256), 0, st, store, M, Hs, Ws, C, index, N, params,
                       mul, add, fill, out, Ho, Wo, labels, S, labels_out, inside);
    note_kernel("warp_f32");
  }
  return launch_status();
}

extern "C" int unetpp_augment_draw(float* params, int32_t N, uint64_t seed, int32_t Hs, int32_t Ws, int32_t Ho,
                                   int32_t Wo, const unetpp_augment* augment, void* stream) {
  if (params == nullptr || augment == nullptr) return UNETPP_EINVAL;
  if (N <= 0 || Hs <= 0 || Ws <= 0 || Ho <= 0 || Wo <= 0) return UNETPP_EINVAL;
  if (!(augment->scale_lo > 0.f) || !(augment->scale_hi > 0.f)) return UNETPP_EINVAL;
  const unsigned grid = static_cast<unsigned>((N + kThreads256 - 1) / kThreads256);
  hipLaunchKernelGGL(draw_kernel, dim3(grid), dim3(kThreads256), 0, static_cast<hipStream_t>(stream), params, N, seed,
                     Hs, Ws, Ho, Wo, *augment);
  note_kernel("augment_draw");
  return launch_status();
}
