// What the scene-training data kernels share (loader.hip, crops.hip, paste.hip, mask.hip): the window of a sample is a
// 16-float parameter row drawn from a 64-bit seed, and the position of a pixel, a label or an ignore mark in it and the
// value of a pixel go through the definitions below, so the kernels agree to the bit -- the label position a target map
// uses is the labels_out the warp reports, an ignore test uses the warp's own source position, a pasted pixel the
// warp's own normalisation.  The tile decode, the quad stores and the float64 minimum fold stay in the kernels: as
// calls they change the kernels' code.
// Implicit contraction is off here and in every file that includes this: each operation is rounded once.
#pragma once
#include "common.h"
#include "dropout.h"

#pragma clang fp contract(off)

namespace unetpp {

constexpr int kThreads256 = 256;
constexpr int kMaxSide = 1 << 24;         // pixel indices are exact in fp32 up to here
constexpr int kTileW = 64, kTileH = 16;   // a tile: 16 quads x 16 rows = 256 threads
constexpr int kMaxClasses = 65535;
constexpr int kClassGroup = 32;           // classes an ignore kernel keeps one bit each for at a time

// grid of a persistent launch: one workgroup per unit up to 8 per CU, the rest of the units are grid-strided
inline unsigned capped_grid(int64_t units) {
  const int cus = device_cu_count();
  const int64_t cap = int64_t(cus > 0 ? cus : 256) * 8;
  return static_cast<unsigned>(units < cap ? units : cap);
}

// ---- draws ----------------------------------------------------------------------------------------------------------
// uniform number `ctr` (>= 1) of a seed, in [0, 1): 24 bits, exact in fp32
__device__ __forceinline__ double uniform24(uint64_t seed, uint64_t ctr) {
  const uint64_t bits = mix64(seed + 0x9E3779B97F4A7C15ULL * ctr);
  return static_cast<double>(static_cast<float>(bits >> 40) * 0x1p-24f);
}
// uniform k (0..15) of sample n
__device__ __forceinline__ double sample_uniform(uint64_t seed, int n, int k) {
  return uniform24(seed, static_cast<uint64_t>(n) * 16 + k + 1);
}

// floor(u * count) limited to count - 1, as a double
__device__ __forceinline__ double pick(double u, int count) {
  const double v = floor(u * static_cast<double>(count));
  return v < static_cast<double>(count - 1) ? v : static_cast<double>(count - 1);
}

// ---- the parameter row ----------------------------------------------------------------------------------------------
// Row P[0..15] of sample n from its uniforms 0..4, 7, 8: flip, quarter turn, angle, scale, gain, bias about the source
// centre (sx, sy) and the window centre (cox, coy).  P[0..5]: the inverse map (window -> source, what the warp samples
// by), P[6..11]: the forward map (source -> window, what carries the labels), P[12], P[13]: gain and bias.
__device__ __forceinline__ void augment_row(float* P, uint64_t seed, int n, const unetpp_augment& a,
                                            double sx, double sy, double cox, double coy) {
  const double dx = static_cast<float>(sample_uniform(seed, n, 0)) < a.p_flip_h ? -1.0 : 1.0;
  const double dy = static_cast<float>(sample_uniform(seed, n, 1)) < a.p_flip_v ? -1.0 : 1.0;
  const int q = a.rot90 != 0 ? static_cast<int>(4.0 * sample_uniform(seed, n, 2)) : 0;
  const double theta = (2.0 * sample_uniform(seed, n, 3) - 1.0) * static_cast<double>(a.max_deg) * (M_PI / 180.0);
  const double ln_lo = log(static_cast<double>(a.scale_lo)), ln_hi = log(static_cast<double>(a.scale_hi));
  const double s = exp(ln_lo + sample_uniform(seed, n, 4) * (ln_hi - ln_lo));
  const double lo = a.gain_lo, hi = a.gain_hi;
  const double gain = lo + sample_uniform(seed, n, 7) * (hi - lo);
  const double bias = (2.0 * sample_uniform(seed, n, 8) - 1.0) * static_cast<double>(a.max_bias);

  // R(theta) Q^q with Q^q as whole numbers: Q^q = [[qc, -qs], [qs, qc]], (qc, qs) = (1, 0), (0, 1), (-1, 0), (0, -1)
  const double qc = q == 0 ? 1.0 : q == 2 ? -1.0 : 0.0;
  const double qs = q == 1 ? 1.0 : q == 3 ? -1.0 : 0.0;
  const double ct = cos(theta), st = sin(theta);
  const double r00 = ct * qc - st * qs, r01 = -ct * qs - st * qc;   // R Q^q, again a rotation [[r00, r01], [-r01, r00]]
  const double r10 = -r01, r11 = r00;
  // forward A = s D (R Q^q); inverse B = (1/s) (R Q^q)^T D; both about the two centres
  const double a00 = s * dx * r00, a01 = s * dx * r01, a10 = s * dy * r10, a11 = s * dy * r11;
  const double is = 1.0 / s;
  const double b00 = is * r00 * dx, b01 = is * r10 * dy, b10 = is * r01 * dx, b11 = is * r11 * dy;
  P[0] = static_cast<float>(b00);
  P[1] = static_cast<float>(b01);
  P[2] = static_cast<float>(sx - b00 * cox - b01 * coy);
  P[3] = static_cast<float>(b10);
  P[4] = static_cast<float>(b11);
  P[5] = static_cast<float>(sy - b10 * cox - b11 * coy);
  P[6] = static_cast<float>(a00);
  P[7] = static_cast<float>(a01);
  P[8] = static_cast<float>(cox - a00 * sx - a01 * sy);
  P[9] = static_cast<float>(a10);
  P[10] = static_cast<float>(a11);
  P[11] = static_cast<float>(coy - a10 * sx - a11 * sy);
  P[12] = static_cast<float>(gain);
  P[13] = static_cast<float>(bias);
  P[14] = 0.f;
  P[15] = 0.f;
}

// ---- window maps (P: a sample's parameter row) ----------------------------------------------------------------------
// source position of window pixel (xf, yf)
__device__ __forceinline__ void map_inverse(const float* P, float xf, float yf, float& xs, float& ys) {
  xs = (P[0] * xf + P[1] * yf) + P[2];
  ys = (P[3] * xf + P[4] * yf) + P[5];
}
// window position of source point (x, y)
__device__ __forceinline__ void map_forward(const float* P, float x, float y, float& xo, float& yo) {
  xo = (P[6] * x + P[7] * y) + P[8];
  yo = (P[9] * x + P[10] * y) + P[11];
}
// a row of a label table is a label unless a coordinate is negative (the sentinel); a NaN is a label
__device__ __forceinline__ bool label_valid(float x, float y) { return !(x < 0.f) && !(y < 0.f); }

// ---- the frame store: uint8 [M, Hs, Ws, C] or float32 [M, C, Hs, Ws] -----------------------------------------------
template <bool U8>
__device__ __forceinline__ float load_src(const void* __restrict__ store, int64_t off) {
  if (U8) return static_cast<float>(static_cast<const uint8_t*>(store)[off]);
  return static_cast<const float*>(store)[off];
}

// a sampled store value as the window holds it: the channel's normalisation, then the sample's contrast and brightness
__device__ __forceinline__ float window_value(float v, float mul, float add, float gain, float bias) {
  return gain * (v * mul + add) + bias;
}

// ---- nearest-label value --------------------------------------------------------------------------------------------
// the map's value at least squared distance m: the maximum of exp(-0.5 d / radius) over labels is that of the nearest
// (the float64 fold that finds m is spelled out in points_target_kernel and in paste_target_kernel: crops.hip says why)
__device__ __forceinline__ float nearest_value(double m, double radius) {
  return static_cast<float>(exp(-0.5 * sqrt(m) / radius));
}

}  // namespace unetpp
