// Scene inference: the launch that puts a chunk of tile maps back into the frame maps (unetpp_scene_stitch).  A frame
// is cut into overlapping tiles, each tile -- and, for test-time augmentation, up to 8 dihedral variants of it -- runs
// through the eval forward, and every tile OWNS a rectangle of the frame that is far enough from its cut edges for the
// head to be exact there.  This kernel writes, for every owned pixel, the mean of the variants read at
// the inverse-transformed position:  out = (((v_0 + v_1) + ...) + v_{K-1}) / float(K), the expression and the true
// division of heads_mean.h; K = 1 is a copy.
//
// Grid (blocks of rows x quads, class, tile in chunk), sized by the largest owned rectangle of the chunk; a thread owns
// 4 consecutive x on a 4-aligned FRAME column, so with W a multiple of 4 every interior store is one 16-byte store and
// only a rectangle's ragged first / last quad takes the scalar path (owned rectangles start at multiples of 2^(depth-1),
// 2 for a depth-2 network).  Same bits on both paths: nothing here but loads, K - 1 additions and one division, each
// rounded once (implicit contraction off).  Variants without a transpose read 4 consecutive floats (one 16-byte load
// where aligned, reversed for a flip in x); transposing variants read with a stride of Tw floats.  The maps have
// n_classes channels against the forward's 32 and more: the strided reads are left to L2.  No atomics, no LDS; every
// offset into `out` is 64-bit.  Nothing outside a tile's owned rectangle is read or written.
//
// The second launch of this file, unetpp_scene_screen, reduces rectangles of a frame map to one flag and one maximum
// each: the device-side decision of cascaded scene inference (described at its kernel below).
#include "common.h"

#pragma clang fp contract(off)

namespace unetpp {
namespace {

constexpr int kStitchThreads = 256;
constexpr int kStitchMaxGridYZ = 65535;

struct SceneVariants {
  int32_t code[UNETPP_SCENE_MAX_VARIANTS];
};

__global__ void __launch_bounds__(kStitchThreads) scene_stitch_kernel(
    const float* __restrict__ tiles, const unetpp_scene_rect* __restrict__ rects, SceneVariants var, int K, int C, int Th,
    int Tw, float* __restrict__ out, int S, int H, int W, int quads) {
  const int t = blockIdx.z, c = blockIdx.y;
  const unetpp_scene_rect r = rects[t];
  if (r.frame < 0) return;   // a padding tile
  // the host checked its copy of the table; a device row that disagrees is skipped, never followed
  if (r.frame >= S || r.oy < 0 || r.ox < 0 || r.oy > H - Th || r.ox > W - Tw) return;
  if (r.y_lo < r.oy || r.y_hi > r.oy + Th || r.x_lo < r.ox || r.x_hi > r.ox + Tw) return;

  const int64_t idx = int64_t(blockIdx.x) * kStitchThreads + threadIdx.x;
  const int64_t row = idx / quads;
  const int q = static_cast<int>(idx - row * quads);
  if (row >= r.y_hi - r.y_lo) return;
  const int y = r.y_lo + static_cast<int>(row);
  const int x0 = (r.x_lo & ~3) + 4 * q;   // a 4-aligned frame column
  if (x0 >= r.x_hi) return;
  const int lo = x0 > r.x_lo ? x0 : r.x_lo;
  const int hi = x0 + 4 < r.x_hi ? x0 + 4 : r.x_hi;
  const bool full = hi - lo == 4;
  const int ty = y - r.oy, tx0 = x0 - r.ox;   // tile coordinates (tx0 may be negative in a ragged first quad)

  const int64_t plane = int64_t(Th) * Tw;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < K; ++k) {
    const int code = var.code[k];
    const float* __restrict__ src = tiles + ((int64_t(t) * K + k) * C + c) * plane;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    const bool fx = (code & UNETPP_SCENE_FLIP_X) != 0, fy = (code & UNETPP_SCENE_FLIP_Y) != 0;
    if ((code & UNETPP_SCENE_TRANSPOSE) == 0) {
      const int a = fy ? Th - 1 - ty : ty;
      // the quad's 4 pixels are consecutive in the variant's row: ascending from tx0, or descending from Tw-1-tx0
      const float* p4 = src + int64_t(a) * Tw + (fx ? Tw - 4 - tx0 : tx0);
      if (full && (reinterpret_cast<uintptr_t>(p4) & 15) == 0) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(p4);
        if (fx) {
          v[0] = w[3], v[1] = w[2], v[2] = w[1], v[3] = w[0];
        } else {
          v = w;
        }
      } else {
#pragma unroll
        for (int p = 0; p < 4; ++p)
          if (x0 + p >= lo && x0 + p < hi) v[p] = p4[fx ? 3 - p : p];
      }
    } else {   // (a, b) = (x, y): Th == Tw here
      const int b = fx ? Tw - 1 - ty : ty;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        if (x0 + p >= lo && x0 + p < hi) {
          const int a = fy ? Th - 1 - (tx0 + p) : tx0 + p;
          v[p] = src[int64_t(a) * Tw + b];
        }
      }
    }
    if (k == 0) {
      acc = v;
    } else {
#pragma unroll
      for (int p = 0; p < 4; ++p) acc[p] = acc[p] + v[p];
    }
  }
  if (K > 1) {
    const float count = static_cast<float>(K);
#pragma unroll
    for (int p = 0; p < 4; ++p) acc[p] = acc[p] / count;
  }

  float* dst = out + ((int64_t(r.frame) * C + c) * H + y) * W + x0;
  if (full && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
    *reinterpret_cast<f32x4*>(dst) = acc;
  } else {
#pragma unroll
    for (int p = 0; p < 4; ++p)
      if (x0 + p >= lo && x0 + p < hi) dst[p] = acc[p];
  }
}

// ---- unetpp_scene_screen: which rectangles of a frame map hold anything (cascaded scene inference) -------
// One workgroup per rectangle, one launch, one writer per rectangle: over all classes and all pixels of the rectangle,
// active = any(!(v < threshold)) -- so a value equal to the threshold and a NaN both activate -- and score = fmax of the
// values (a NaN is ignored; -inf when there is nothing else).  Both are order-independent, so the result is a pure
// function of the rectangle's values: the same bits whatever the grid.  The four waves of a workgroup take rows of the
// rectangle in turn, four rows in flight per wave; the lanes take quads of 4 floats cut at 16-byte boundaries of MEMORY
// (a row starts wherever ((frame * C + c) * H + y) * W + x_lo puts it), so every whole quad is one aligned 16-byte load
// whatever W is and only a row's ragged first and last quad are read float by float.  Nothing outside a rectangle is
// read.  Reduction by shuffles within a wave and through 2 x 4 words of LDS across waves; no atomics, no partial buffers;
// every offset into the maps is 64-bit.
constexpr int kScreenThreads = 256;
constexpr int kScreenWaves = kScreenThreads / 64;
constexpr int kScreenRowsInFlight = 4;

__device__ __forceinline__ bool screen_row_ok(const unetpp_scene_rect& r, int S, int H, int W) {
  return r.frame < S && r.y_lo >= 0 && r.y_lo < r.y_hi && r.y_hi <= H && r.x_lo >= 0 && r.x_lo < r.x_hi && r.x_hi <= W;
}

__global__ void __launch_bounds__(kScreenThreads) scene_screen_kernel(
    const float* __restrict__ maps, const unetpp_scene_rect* __restrict__ rects, int S, int C, int H, int W,
    float threshold, int32_t* __restrict__ active, float* __restrict__ score) {
  __shared__ float wave_max[kScreenWaves];
  __shared__ int wave_any[kScreenWaves];
  const int t = blockIdx.x;
  const unetpp_scene_rect r = rects[t];
  const float ninf = -__builtin_inff();
  // a padding row, or a device row that disagrees with the frame (the host checked its copy): reported empty, never followed
  if (r.frame < 0 || !screen_row_ok(r, S, H, W)) {
    if (threadIdx.x == 0) active[t] = 0, score[t] = ninf;
    return;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rows = r.y_hi - r.y_lo, w = r.x_hi - r.x_lo;
  const int quads = (w + 6) >> 2;   // of the row that starts 3 floats past a 16-byte boundary

  float best = ninf;
  bool any = false;
  for (int c = 0; c < C; ++c) {
    const float* __restrict__ plane = maps + (int64_t(r.frame) * C + c) * H * W;
    for (int row0 = wave; row0 < rows; row0 += kScreenWaves * kScreenRowsInFlight) {
      for (int q = lane; q < quads; q += 64) {
        f32x4 v[kScreenRowsInFlight];
#pragma unroll
        for (int u = 0; u < kScreenRowsInFlight; ++u) {
          v[u] = f32x4{ninf, ninf, ninf, ninf};   // -inf changes neither result (a live rectangle is never empty)
          const int row = row0 + u * kScreenWaves;
          if (row < rows) {
            const float* p = plane + int64_t(r.y_lo + row) * W + r.x_lo;
            const int a = static_cast<int>((reinterpret_cast<uintptr_t>(p) >> 2) & 3);   // floats past the boundary
            const int rel = 4 * q - a;   // the quad's first float, relative to x_lo
            const int lo = rel > 0 ? rel : 0, hi = rel + 4 < w ? rel + 4 : w;
            if (hi - lo == 4) {
              v[u] = *reinterpret_cast<const f32x4*>(p + rel);
            } else {
#pragma unroll
              for (int k = 0; k < 4; ++k)
                if (rel + k >= lo && rel + k < hi) v[u][k] = p[rel + k];
            }
          }
        }
#pragma unroll
        for (int u = 0; u < kScreenRowsInFlight; ++u) {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            any = any || !(v[u][k] < threshold);
            best = fmaxf(best, v[u][k]);
          }
        }
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) best = fmaxf(best, __shfl_xor(best, off, 64));
  const bool any_wave = __any(any) != 0;
  if (lane == 0) wave_max[wave] = best, wave_any[wave] = any_wave;
  __syncthreads();
  if (threadIdx.x == 0) {
    float m = wave_max[0];
    int f = wave_any[0];
#pragma unroll
    for (int i = 1; i < kScreenWaves; ++i) m = fmaxf(m, wave_max[i]), f |= wave_any[i];
    active[t] = f;
    score[t] = m;
  }
}

}  // namespace
}  // namespace unetpp

using namespace unetpp;

extern "C" int unetpp_scene_stitch(const float* tiles, int32_t n_tiles, int32_t K, int32_t C, int32_t Th, int32_t Tw,
                                   const int32_t* variants, const unetpp_scene_rect* rects,
                                   const unetpp_scene_rect* rects_dev, float* out, int32_t S, int32_t H, int32_t W,
                                   void* stream) {
  if (tiles == nullptr || variants == nullptr || rects == nullptr || rects_dev == nullptr || out == nullptr)
    return UNETPP_EINVAL;
  if (n_tiles <= 0 || C <= 0 || Th <= 0 || Tw <= 0 || S <= 0 || H <= 0 || W <= 0) return UNETPP_EINVAL;
  if (K < 1 || K > UNETPP_SCENE_MAX_VARIANTS) return UNETPP_EINVAL;
  if (n_tiles > kStitchMaxGridYZ || C > kStitchMaxGridYZ || Th > H || Tw > W) return UNETPP_EINVAL;
  SceneVariants var = {};
  for (int k = 0; k < K; ++k) {
    const int32_t code = variants[k];
    if (code < 0 || code > (UNETPP_SCENE_FLIP_X | UNETPP_SCENE_FLIP_Y | UNETPP_SCENE_TRANSPOSE)) return UNETPP_EINVAL;
    if ((code & UNETPP_SCENE_TRANSPOSE) != 0 && Th != Tw) return UNETPP_EINVAL;
    var.code[k] = code;
  }
  int rows = 0, quads = 0;   // of the largest owned rectangle
  for (int t = 0; t < n_tiles; ++t) {
    const unetpp_scene_rect& r = rects[t];
    if (r.frame < 0) continue;
    if (r.frame >= S || r.oy < 0 || r.ox < 0 || r.oy > H - Th || r.ox > W - Tw) return UNETPP_EINVAL;
    if (r.y_lo < r.oy || r.y_hi > r.oy + Th || r.x_lo < r.ox || r.x_hi > r.ox + Tw) return UNETPP_EINVAL;
    if (r.y_lo >= r.y_hi || r.x_lo >= r.x_hi) return UNETPP_EINVAL;
    const int h = r.y_hi - r.y_lo, q = ((r.x_hi + 3) >> 2) - (r.x_lo >> 2);
    rows = h > rows ? h : rows;
    quads = q > quads ? q : quads;
  }
  if (rows == 0) return UNETPP_OK;   // nothing but padding tiles
  const int64_t blocks = (int64_t(rows) * quads + kStitchThreads - 1) / kStitchThreads;
  if (blocks > 0x7fffffff) return UNETPP_EINVAL;
  hipLaunchKernelGGL(scene_stitch_kernel, dim3(static_cast<unsigned>(blocks), C, n_tiles), dim3(kStitchThreads), 0,
                     static_cast<hipStream_t>(stream), tiles, rects_dev, var, K, C, Th, Tw, out, S, H, W, quads);
  note_kernel("scene_stitch");
  return launch_status();
}

extern "C" int unetpp_scene_screen(const float* maps, int32_t S, int32_t C, int32_t H, int32_t W,
                                   const unetpp_scene_rect* rects, const unetpp_scene_rect* rects_dev, int32_t n_rects,
                                   float threshold, int32_t* active, float* score, void* stream) {
  if (maps == nullptr || rects == nullptr || rects_dev == nullptr || active == nullptr || score == nullptr)
    return UNETPP_EINVAL;
  if (n_rects <= 0 || S <= 0 || C <= 0 || H <= 0 || W <= 0) return UNETPP_EINVAL;
  if (threshold != threshold) return UNETPP_EINVAL;
  bool live = false;
  for (int t = 0; t < n_rects; ++t) {
    const unetpp_scene_rect& r = rects[t];
    if (r.frame < 0) continue;
    if (r.frame >= S || r.y_lo < 0 || r.y_hi > H || r.x_lo < 0 || r.x_hi > W) return UNETPP_EINVAL;
    if (r.y_lo >= r.y_hi || r.x_lo >= r.x_hi) return UNETPP_EINVAL;
    live = true;
  }
  if (!live) return UNETPP_OK;   // nothing but padding rows
  hipLaunchKernelGGL(scene_screen_kernel, dim3(static_cast<unsigned>(n_rects)), dim3(kScreenThreads), 0,
                     static_cast<hipStream_t>(stream), maps, rects_dev, S, C, H, W, threshold, active, score);
  note_kernel("scene_screen");
  return launch_status();
}
