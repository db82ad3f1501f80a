// Weight images of the fast GEMM kernels, built straight from the torch-layout parameters.
//
// A fast kernel reads its B operand as an LDS image per (column tile, K chunk): the direct kernels
// (gemm_fast.hip) [tap][g 2][col 32][half' 2][4] over 16-channel chunks, the Winograd kernel (gemm_wino.hip)
// [s 2][xi / 2][g 4][col 16][xi % 2][nh 2] of U = G g G^T over 8-channel chunks (16 bytes per lane (g, col) and pair of
// transform positions).  The element of the GEMM weight that lands in an image slot is W[tap][k][n]; `unetpp_weight_src` says where that element sits in memory:
//     src[tap' * s_t + (k % k_inner) * s_k + (k / k_inner) * s_ko + (n % n_inner) * s_n + (n / n_inner) * s_no],
// tap' = flip ? taps - 1 - tap : tap, which covers the packed [taps][K][N] operand as well as nn.Conv2d
// ([co,ci,3,3]: forward and 180-degree-rotated input-gradient form) and nn.ConvTranspose2d ([ci,co,2,2]: forward
// with N = 4 phases x co, input gradient with K = 4 phases x co) parameters -- no intermediate re-layout launch.
// There is ONE packer body (pack_image): it derives the layout from a job's taps and flags by the rule the selection uses
// (image_layout, gemm_units.h) and walks whole image rows.  unetpp_gemm_pack_weight_images runs it over a table of jobs in
// device memory -- the images of many launches (a whole forward or backward pass) in ONE launch;
// unetpp_gemm_pack_weight_image[_from] runs it on one job passed by value as the kernel argument.
#include "bf16_common.h"
#include "common.h"
#include "gemm_units.h"

namespace unetpp {
namespace {

// image kinds (gemm_units.h): kKindFast, kKindWino, kKindBf16 = gemm_bf16.hip, [tap][g 2][col 32][h 2][8 bf16], 32-channel chunks

struct PackGeom {  // a job's layout and channel structure, decoded once per workgroup
  ImageLayout l;
  int taps;
  int n_in, n_out;
  int in_len[UNETPP_MAX_VIEWS], out_len[UNETPP_MAX_VIEWS];
  int n_chunks, n_tiles;
  int rows;  // image rows of l.row_slots slots each (< 2^31: an image of 2^31 rows would be 4 TB)
};

__device__ __forceinline__ float wsrc_at(const unetpp_weight_src& w, int taps, int tap, int k, int n) {
  const int tt = w.flip ? taps - 1 - tap : tap;
  const int ki = w.k_inner > 0 ? k % w.k_inner : k, ko = w.k_inner > 0 ? k / w.k_inner : 0;
  const int ni = w.n_inner > 0 ? n % w.n_inner : n, no = w.n_inner > 0 ? n / w.n_inner : 0;
  return w.src[tt * w.s_t + ki * w.s_k + ko * w.s_ko + ni * w.s_n + no * w.s_no];
}

// (tile, chunk) of an image row -> input view / first GEMM row of the chunk, output view / first GEMM column of the tile
struct RowOrigin {
  int k0, k_room;  // GEMM row of the chunk's channel 0; channels left in its view from there
  int n0, n_room;  // GEMM column of the tile's column 0; columns left in its view from there
};
__device__ __forceinline__ RowOrigin row_origin(const PackGeom& g, int nt, int chunk) {
  int kbase = 0, v = 0;
  for (; v < g.n_in - 1; ++v) {
    const int ch = g.l.chunks(g.in_len[v]);
    if (chunk < ch) break;
    chunk -= ch;
    kbase += g.in_len[v];
  }
  int col_base = 0, ov = 0;
  for (; ov < g.n_out - 1; ++ov) {
    const int tv = g.l.tiles(g.out_len[ov]);
    if (nt < tv) break;
    nt -= tv;
    col_base += g.out_len[ov];
  }
  RowOrigin o;
  o.k0 = kbase + (chunk << g.l.log2_kc);
  o.k_room = g.in_len[v] - (chunk << g.l.log2_kc);
  o.n0 = col_base + (nt << g.l.log2_ncol);
  o.n_room = g.out_len[ov] - (nt << g.l.log2_ncol);
  return o;
}

// The packer walks whole image rows: row = (tile, chunk[, tap]) is decoded once per workgroup iteration
// (uniform: scalar unit), a thread only splits its slot's bit fields.  (Decoding per element cost ~80 instructions
// per 4 bytes written: 175 us per launch for the 73 MB of bf16 images of the depth-5 network.)
__device__ __forceinline__ void fill_image_row(const PackGeom& g, const unetpp_weight_src& w, int row, float* __restrict__ img) {
  const int tid = threadIdx.x;
  if (g.l.kind == kKindWino) {  // row = (tile, chunk): 256 (channel, column) pairs x 16 transform elements
    const RowOrigin o = row_origin(g, row / g.n_chunks, row % g.n_chunks);
    const int t = tid;  // nh | col << 1 | gq << 5 | s << 7
    const int kk = 2 * ((t >> 5) & 3) + ((t >> 7) & 1), cl = 16 * (t & 1) + ((t >> 1) & 15);
    // slot of (xi, lane = gq | col, nh): nh | (xi & 1) << 1 | lane << 2 | (xi >> 1) << 8 | s << 11
    float* dst = img + row * 4096L + (t & 1) + (((t >> 1) & 63) << 2) + (static_cast<long>(t >> 7) << 11);
    auto slot = [](int xi) { return ((xi & 1) << 1) + ((xi >> 1) << 8); };
    if (kk >= o.k_room || cl >= o.n_room) {
#pragma unroll
      for (int xi = 0; xi < 16; ++xi) dst[slot(xi)] = 0.f;
      return;
    }
    const int k = o.k0 + kk, n = o.n0 + cl;
    float tr[4][3];  // G g: row ra of G down the filter rows, per filter column
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float w0 = wsrc_at(w, 9, 0 * 3 + c, k, n), w1 = wsrc_at(w, 9, 1 * 3 + c, k, n), w2 = wsrc_at(w, 9, 2 * 3 + c, k, n);
      tr[0][c] = w0;
      tr[1][c] = 0.5f * (w0 + w1 + w2);
      tr[2][c] = 0.5f * (w0 - w1 + w2);
      tr[3][c] = w2;
    }
#pragma unroll
    for (int ra = 0; ra < 4; ++ra) {
      dst[slot(4 * ra + 0)] = tr[ra][0];
      dst[slot(4 * ra + 1)] = 0.5f * (tr[ra][0] + tr[ra][1] + tr[ra][2]);
      dst[slot(4 * ra + 2)] = 0.5f * (tr[ra][0] - tr[ra][1] + tr[ra][2]);
      dst[slot(4 * ra + 3)] = tr[ra][2];
    }
    return;
  }
  // direct kernels: row = (tile, chunk, tap), 512 four-byte slots
  const int tap = row % g.taps, rc = row / g.taps;
  const RowOrigin o = row_origin(g, rc / g.n_chunks, rc % g.n_chunks);
  float* dst = img + row * 512L;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int e = tid + q * 256;
    if (g.l.kind == kKindBf16) {  // slot = two bf16: elements 2e, 2e+1 of [g 2][col 32][h 2][8]
      const int i0 = 2 * e;
      const int kk = 16 * ((i0 >> 9) & 1) + 8 * ((i0 >> 3) & 1) + (i0 & 7), cl = (i0 >> 4) & 31;
      float a = 0.f, b = 0.f;
      if (cl < o.n_room) {
        if (kk < o.k_room) a = wsrc_at(w, g.taps, tap, o.k0 + kk, o.n0 + cl);
        if (kk + 1 < o.k_room) b = wsrc_at(w, g.taps, tap, o.k0 + kk + 1, o.n0 + cl);
      }
      dst[e] = __uint_as_float(pack_bf2(a, b));
    } else {  // [g 2][col 32][half' 2][4], half' = half ^ ((col>>3)&1)
      const int j = (e >> 3) & 31;
      const int kk = 8 * ((e >> 8) & 1) + 4 * (((e >> 2) & 1) ^ ((j >> 3) & 1)) + (e & 3);
      dst[e] = (kk < o.k_room && j < o.n_room) ? wsrc_at(w, g.taps, tap, o.k0 + kk, o.n0 + j) : 0.f;
    }
  }
}

// bf16 3x3 images, nine rows at a time: the 32 x 32 x 9 source block of a (tile, chunk) goes through LDS, read in the
// order it lies in memory (the taps of a (channel, column) pair are adjacent, then whichever of channel / column has
// the smaller stride) -- fill_image_row reads it as 4-byte pieces 36 bytes apart, nine times over (once per tap) --
// and leaves as 16-byte stores.
__device__ __forceinline__ void fill_bf16_3x3_block(const PackGeom& g, const unetpp_weight_src& w, int rc,
                                                     float* __restrict__ img, float* lds /* [9][32][33] */) {
  const int tid = threadIdx.x;
  const RowOrigin o = row_origin(g, rc / g.n_chunks, rc % g.n_chunks);
  const bool k_inner_most = w.s_k < w.s_n;  // forward layout [co][ci][3][3]: channel k = ci runs faster than column n = co
  __syncthreads();  // the previous block's readers are done
  // 16-byte reads where the nine taps of 32 consecutive inner indices form one aligned 1152-byte run (plain conv
  // parameters: tap stride 1, inner stride 9, 16-byte aligned block origin), 4-byte reads otherwise
  const long inner_stride = k_inner_most ? w.s_k : w.s_n, outer_stride = k_inner_most ? w.s_n : w.s_k;
  const int inner_room = k_inner_most ? o.k_room : o.n_room, outer_room = k_inner_most ? o.n_room : o.k_room;
  const long origin = static_cast<long>(o.k0) * w.s_k + static_cast<long>(o.n0) * w.s_n;
  const bool wide = w.s_t == 1 && inner_stride == 9 && w.k_inner <= 0 && w.n_inner <= 0 && inner_room >= 32 &&
                    ((reinterpret_cast<uintptr_t>(w.src + origin) | static_cast<uintptr_t>(outer_stride * 4)) & 15) == 0;
  if (wide) {
#pragma unroll 3
    for (int q = tid; q < 32 * 72; q += 256) {  // 72 float4 per outer index
      const int oo = q / 72, r4 = q - oo * 72;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (oo < outer_room) v = *reinterpret_cast<const f32x4*>(w.src + origin + oo * outer_stride + 4 * r4);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int f = 4 * r4 + c, m = f / 9;
        const int tap_m = f - 9 * m, tap = w.flip ? 8 - tap_m : tap_m;
        const int kk = k_inner_most ? m : oo, cl = k_inner_most ? oo : m;
        lds[(tap * 32 + kk) * 33 + cl] = v[c];
      }
    }
  } else {
#pragma unroll 6
    for (int idx = tid; idx < 9 * 32 * 32; idx += 256) {
      const int tap = idx % 9, m = (idx / 9) & 31, oo = idx / (9 * 32);
      const int kk = k_inner_most ? m : oo, cl = k_inner_most ? oo : m;
      lds[(tap * 32 + kk) * 33 + cl] = (kk < o.k_room && cl < o.n_room) ? wsrc_at(w, 9, tap, o.k0 + kk, o.n0 + cl) : 0.f;
    }
  }
  __syncthreads();
  // one 16-byte store per thread and round: four slots = the eight channels 16 gq + 8 hs .. + 7 of one column
  f32x4* dst4 = reinterpret_cast<f32x4*>(img + rc * (9 * 512L));
#pragma unroll 3
  for (int s4 = tid; s4 < 9 * 128; s4 += 256) {
    const int tap = s4 >> 7, e4 = s4 & 127;  // slots 4 e4 .. 4 e4 + 3 of the tap's row
    const int cl = (e4 >> 1) & 31, kk0 = 16 * ((e4 >> 6) & 1) + 8 * (e4 & 1);
    f32x4 out;
#pragma unroll
    for (int c = 0; c < 4; ++c)
      out[c] = __uint_as_float(pack_bf2(lds[(tap * 32 + kk0 + 2 * c) * 33 + cl], lds[(tap * 32 + kk0 + 2 * c + 1) * 33 + cl]));
    dst4[s4] = out;
  }
}

// One job: the geometry follows from its taps, flags and channel lists alone; the workgroups of gridDim.x share its rows.
__device__ __forceinline__ void pack_image(const unetpp_pack_job& j) {
  __shared__ PackGeom g;
  if (threadIdx.x == 0) {
    g.l = image_layout(j.taps, j.flags);
    g.taps = j.taps;
    g.n_in = j.n_in;
    g.n_out = j.n_out;
    int n_chunks = 0, n_tiles = 0;
    for (int i = 0; i < UNETPP_MAX_VIEWS; ++i) {
      g.in_len[i] = j.in_len[i];
      g.out_len[i] = j.out_len[i];
      if (i < j.n_in) n_chunks += g.l.chunks(j.in_len[i]);
      if (i < j.n_out) n_tiles += g.l.tiles(j.out_len[i]);
    }
    g.n_chunks = n_chunks;
    g.n_tiles = n_tiles;
    g.rows = n_tiles * n_chunks * g.l.unit_rows;
  }
  __syncthreads();
  const int rows = g.rows;
  if (g.l.kind == kKindBf16 && g.taps == 9) {
    __shared__ float stage[9 * 32 * 33];
    for (int rc = blockIdx.x; rc < rows / 9; rc += gridDim.x) fill_bf16_3x3_block(g, j.src, rc, j.image, stage);
    return;
  }
  for (int row = blockIdx.x; row < rows; row += gridDim.x) fill_image_row(g, j.src, row, j.image);
}

__global__ void pack_image_jobs_kernel(const unetpp_pack_job* __restrict__ jobs) { pack_image(jobs[blockIdx.y]); }  // blockIdx.y = job
__global__ void pack_image_job_kernel(const unetpp_pack_job j) { pack_image(j); }

// workgroups per job: ~8 slots per thread for an image of this size, 256 at most
unsigned pack_grid_x(long image_floats) {
  const long bx = (image_floats + 256L * 8 - 1) / (256L * 8);
  return static_cast<unsigned>(bx > 256 ? 256 : bx);
}

}  // namespace
}  // namespace unetpp

using namespace unetpp;

extern "C" int64_t unetpp_gemm_weight_image_floats(const unetpp_gemm_desc* d) {
  GemmSel s;
  return gemm_image_of(d, s) ? s.image_floats : 0;
}

extern "C" int unetpp_gemm_pack_weight_image_from(const unetpp_gemm_desc* d, const unetpp_weight_src* src, float* image,
                                                  void* stream) {
  GemmSel s;
  if (src == nullptr || src->src == nullptr || image == nullptr || !gemm_image_of(d, s)) return UNETPP_EINVAL;
  unetpp_pack_job j = {};  // what PackPlan records for this launch
  j.src = *src;
  j.image = image;
  j.taps = d->taps;
  j.flags = d->flags;
  j.n_in = d->n_in;
  j.n_out = d->n_out;
  for (int i = 0; i < d->n_in; ++i) j.in_len[i] = d->in[i].c_len;
  for (int i = 0; i < d->n_out; ++i) j.out_len[i] = d->out[i].c_len;
  hipLaunchKernelGGL(pack_image_job_kernel, dim3(pack_grid_x(s.image_floats)), dim3(256), 0, static_cast<hipStream_t>(stream), j);
  return launch_status();
}

extern "C" int unetpp_gemm_pack_weight_image(const unetpp_gemm_desc* d, float* image, void* stream) {
  if (d == nullptr || d->weight == nullptr) return UNETPP_EINVAL;
  long K = 0, N = 0;
  for (int i = 0; i < d->n_in && i < UNETPP_MAX_VIEWS; ++i) K += d->in[i].c_len;
  for (int i = 0; i < d->n_out && i < UNETPP_MAX_VIEWS; ++i) N += d->out[i].c_len;
  unetpp_weight_src w = {};  // the packed [taps][K][Ncols] operand
  w.src = d->weight;
  w.s_t = K * N;
  w.s_k = N;
  w.s_n = 1;
  return unetpp_gemm_pack_weight_image_from(d, &w, image, stream);
}

extern "C" int unetpp_gemm_pack_weight_images(const unetpp_pack_job* jobs_device, int32_t n_jobs, int64_t max_image_floats,
                                              void* stream) {
  if (jobs_device == nullptr || n_jobs < 1 || n_jobs > 65535 || max_image_floats < 1) return UNETPP_EINVAL;
  hipLaunchKernelGGL(pack_image_jobs_kernel, dim3(pack_grid_x(max_image_floats), static_cast<unsigned>(n_jobs)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), jobs_device);
  return launch_status();
}
