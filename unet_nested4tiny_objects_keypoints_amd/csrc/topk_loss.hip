// Top-k focal loss: per (head, row = one (n, c) map of P pixels) only the k_eff = min(k, P) pixels with the largest
// |pred - target| enter FocalLoss_BCE_2d; their gradient is focal_element's, every other pixel's is +0.0.
//   key     the bits of fabsf(fl32(p - t)) as uint32: numeric order for non-negative floats, a NaN above everything;
//   select  the k_eff largest keys; among the elements whose key equals the k-th largest, the lowest indices;
//   kth     that k-th largest |d| (exact), per head and row.
// One workgroup per (head, row) does the whole job, nothing crosses workgroups, so the result is the same on any grid:
//   3 digit passes (bits 30..20, 19..10, 9..0 of the key; bit 31 is clear), most significant first: a 32-bit LDS
//     histogram of the digit over the elements that match the prefix found so far, a suffix scan of it, the bin that
//     holds the k-th largest.  After the last pass tau (the key of the k-th largest), `above` (keys > tau) and
//     need = k_eff - above (ties to take) are known exactly.  Keys are recomputed from pred / target (no buffer is
//     needed, so validation runs without grad) -- but when the first pass leaves at most 2048 elements in its bin, as
//     on any row that is not flat, the second pass also copies their keys into LDS (in any order: only the multiset
//     counts) and the third pass reads that list instead of the row: three passes over global memory, not four.
//     A wave whose lanes all hit one bin -- a saturated background row -- adds its count with ONE atomic: the
//     leader's bin is broadcast and its matches are balloted.  A thread issues the loads of four strides before it
//     works on the first: four waves per workgroup do not hide a memory latency per stride otherwise.
//   emit pass: an element is selected iff key > tau, or key == tau and its index-ordered rank among the ties < need.
//     The rank is ballots and popcounts inside a wave, wave counts through LDS, and a running count carried over the
//     workgroup's strides.  Loss: thread (in index order) -> 6 wave shuffles -> (w0 + w1) + (w2 + w3) -> times 1 / denom.
// Rows start at r * P floats and are 16-byte aligned only when that is a multiple of 4: the workgroup walks the row in
// 4-element chunks of the ALIGNED index space (the row's first and last chunk may be partial and take scalar accesses).
// kIgnore (unetpp_topk_focal_heads_ignore): an element whose target is negative has key 0 and is never emitted, so it
// ranks last, takes a tie's rank when tau is 0, and adds +0.0 to the loss and the gradient selected or not; k >= P then
// runs unetpp_focal_bce_heads_ignore.  The plain instantiation is the code it was.
// The row partials take the finish of loss_heads.h (launch_loss_heads_finish, over rows instead of blocks).  k >= P is
// FocalLoss_BCE_2d itself: value and gradient come from unetpp_focal_bce_heads (same bits), this file's kernel then
// only finds kth (the smallest |d| of the row).
#include "common.h"
#include "focal_element.h"
#include "loss_heads.h"

namespace unetpp {
namespace {

constexpr int kTopkThreads = 256;
constexpr int kTopkWaves = kTopkThreads / 64;
constexpr int kTopkBins = 2048;   // the first digit has 11 bits, the other two 10
constexpr int kTopkPasses = 3;
constexpr int kTopkAhead = 4;     // strides whose loads a thread issues before it works on the first of them
constexpr int kTopkCand = 2048;   // keys of the first pass's bin the second pass lists in LDS for the third

// kIgnore: an element whose target is negative (t < 0.0f) has key 0 -- it ranks last, and selected or not it
// contributes +0.0 to the loss and the gradient
template <bool kIgnore = false>
__device__ __forceinline__ uint32_t topk_key(float p, float t) {
  if constexpr (kIgnore) {
    if (t < 0.f) return 0u;
  }
  return __float_as_uint(fabsf(p - t));
}

// Elements 4c .. 4c+3 of the aligned index space of a row (a = the row's pointer rounded down to 16 bytes); an element
// j belongs to the row iff lo <= j < hi.  -> bit e set iff 4c + e does; elements outside are not touched.
__device__ __forceinline__ unsigned topk_load4(const float* __restrict__ a, long c, long lo, long hi, float (&v)[4]) {
  const long j = 4 * c;
  if (j >= lo && j + 4 <= hi) {
    const f32x4 q = *reinterpret_cast<const f32x4*>(a + j);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = q[e];
    return 15u;
  }
  unsigned m = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const bool in = (j + e >= lo) && (j + e < hi);
    v[e] = in ? a[j + e] : 0.f;
    m |= in ? (1u << e) : 0u;
  }
  return m;
}

// grid (rows, heads).  k: k_eff, 1 <= k <= P.  emit false: kth only.
template <bool kLow, bool kIgnore = false>
__global__ __launch_bounds__(kTopkThreads) void topk_focal_kernel(const unetpp_focal_heads hd,
                                                                  const float* __restrict__ target, long P, uint32_t k,
                                                                  float gamma, float inv_denom, float scale, int emit,
                                                                  float* __restrict__ partial, float* __restrict__ kth) {
  __shared__ uint32_t hist[kTopkBins];
  __shared__ uint32_t wave_tot[kTopkWaves];
  __shared__ uint32_t tie_cnt[2][kTopkWaves];
  __shared__ uint32_t found[3];   // the bin, the count of the bins above it, the bin's own count
  __shared__ uint32_t cand[kTopkCand];
  __shared__ uint32_t cand_n;
  __shared__ float red[kTopkWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long r = blockIdx.x, rows = gridDim.x;
  const int h = blockIdx.y;
  const long base = r * P;                  // 64-bit: rows * P may pass 2^31
  const long lo = base & 3, hi = lo + P;    // the row inside its aligned index space
  const float* __restrict__ pa = hd.pred[h] + (base - lo);
  const float* __restrict__ ta = target + (base - lo);
  const long chunks = (hi + 3) >> 2;
  const long iters = (chunks + kTopkThreads - 1) / kTopkThreads;

  // ---- select: tau, above, need
  const uint64_t below = (uint64_t(1) << lane) - 1;
  uint32_t prefix = 0, prefix_mask = 0, kr = k, above = 0;
  uint32_t live = static_cast<uint32_t>(P), listed = 0;   // elements that match the prefix; of them in cand (0: none)
#pragma unroll 1
  for (int pass = 0; pass < kTopkPasses; ++pass) {
    const int shift = (pass == 0) ? 20 : (pass == 1 ? 10 : 0);
    const int bins = (pass == 0) ? 2048 : 1024;
    const bool collect = (pass == 1) && live <= static_cast<uint32_t>(kTopkCand);   // (workgroup-uniform)
    for (int b = tid; b < kTopkBins; b += kTopkThreads) hist[b] = 0;
    if (tid == 0) cand_n = 0;
    __syncthreads();
    if (pass == 2 && listed != 0) {
      // every key that matches the first two digits is in cand: no global read
      for (uint32_t i = tid; i < listed; i += kTopkThreads) {
        const uint32_t key = cand[i];
        if ((key & prefix_mask) == prefix) atomicAdd(&hist[key & static_cast<uint32_t>(bins - 1)], 1u);
      }
    } else {
#pragma unroll 1
      for (long it0 = 0; it0 < iters; it0 += kTopkAhead) {
        // (a workgroup has 4 waves and a chip holds few workgroups per CU at 128 rows: without loads in flight ahead
        // of the work the row is read at one memory latency per stride)
        float pp[kTopkAhead][4], tt[kTopkAhead][4];
        unsigned vv[kTopkAhead];
#pragma unroll
        for (int a = 0; a < kTopkAhead; ++a) {   // (a stride past the row's end loads nothing)
          const long c = (it0 + a) * kTopkThreads + tid;
          vv[a] = topk_load4(pa, c, lo, hi, pp[a]);
          topk_load4(ta, c, lo, hi, tt[a]);
        }
#pragma unroll
        for (int ae = 0; ae < 4 * kTopkAhead; ++ae) {
          const int e = ae & 3;
          const unsigned valid = vv[ae >> 2];
          const uint32_t key = topk_key<kIgnore>(pp[ae >> 2][e], tt[ae >> 2][e]);
          const bool act = ((valid >> e) & 1u) && ((key & prefix_mask) == prefix);
          const uint32_t bin = (key >> shift) & static_cast<uint32_t>(bins - 1);
          const uint64_t am = __ballot(act);
          if (am != 0) {   // (wave-uniform)
            const int leader = __ffsll(static_cast<unsigned long long>(am)) - 1;
            const uint32_t lb = __shfl(bin, leader, 64);
            const uint64_t same = __ballot(act && bin == lb);
            if (lane == leader) atomicAdd(&hist[lb], static_cast<uint32_t>(__popcll(same)));
            if (act && bin != lb) atomicAdd(&hist[bin], 1u);
            if (collect) {   // one slot range per wave; the matching elements number exactly `live` <= kTopkCand
              uint32_t slot = 0;
              if (lane == leader) slot = atomicAdd(&cand_n, static_cast<uint32_t>(__popcll(am)));
              slot = __shfl(slot, leader, 64) + static_cast<uint32_t>(__popcll(am & below));
              if (act && slot < static_cast<uint32_t>(kTopkCand)) cand[slot] = key;
            }
          }
        }
      }
    }
    if (collect) listed = live;
    __syncthreads();
    // bins in descending order: thread `tid` owns rb = tid * per .. + per - 1, rb = bins - 1 - bin
    const int per = bins / kTopkThreads;   // 8 or 4
    uint32_t cnt[8], own = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      cnt[i] = (i < per) ? hist[bins - 1 - (tid * per + i)] : 0u;
      own += cnt[i];
    }
    uint32_t inc = own;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t up = __shfl_up(inc, off, 64);
      if (lane >= off) inc += up;
    }
    if (lane == 63) wave_tot[wave] = inc;
    __syncthreads();
    uint32_t excl = inc - own;
    for (int w = 0; w < wave; ++w) excl += wave_tot[w];
    if (excl < kr && kr <= excl + own) {   // exactly one thread: the counts of the matching elements sum to >= kr
      uint32_t run = excl;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (i < per) {
          if (run < kr && kr <= run + cnt[i]) {
            found[0] = static_cast<uint32_t>(bins - 1 - (tid * per + i));
            found[1] = run;
            found[2] = cnt[i];
          }
          run += cnt[i];
        }
      }
    }
    __syncthreads();
    prefix |= found[0] << shift;
    prefix_mask |= static_cast<uint32_t>(bins - 1) << shift;
    above += found[1];
    kr -= found[1];
    live = found[2];
    // (the next pass's zeroing of hist comes after this barrier; found is written again only two barriers later)
  }
  const uint32_t tau = prefix, need = kr;   // need >= 1 ties are taken, in index order
  if (tid == 0) kth[static_cast<long>(h) * rows + r] = __uint_as_float(tau);
  if (!emit) return;

  // ---- emit
  float* __restrict__ ga = (hd.grad[h] != nullptr) ? hd.grad[h] + (base - lo) : nullptr;
  const bool cube = gamma == 3.f;
  uint32_t taken = 0;   // ties of the earlier strides
  float sum = 0.f;
#pragma unroll 1
  for (long it0 = 0; it0 < iters; it0 += kTopkAhead) {
    float pp[kTopkAhead][4], tt[kTopkAhead][4];
    unsigned vv[kTopkAhead];
#pragma unroll
    for (int a = 0; a < kTopkAhead; ++a) {
      const long c = (it0 + a) * kTopkThreads + tid;
      vv[a] = topk_load4(pa, c, lo, hi, pp[a]);
      topk_load4(ta, c, lo, hi, tt[a]);
    }
#pragma unroll
    for (int a = 0; a < kTopkAhead; ++a) {   // the strides in index order (one past the row's end is all invalid)
      const long it = it0 + a;
      const long c = it * kTopkThreads + tid;
      const float(&p)[4] = pp[a];
      const float(&t)[4] = tt[a];
      const unsigned valid = vv[a];
      float g[4];
      bool tie[4], big[4];
      uint32_t before = 0, mine = 0;   // ties in the lower lanes of this wave, ties of this thread
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const uint32_t key = topk_key<kIgnore>(p[e], t[e]);
        const bool v = (valid >> e) & 1u;
        big[e] = v && key > tau;
        tie[e] = v && key == tau;
        const uint64_t b = __ballot(tie[e]);
        before += __popcll(b & below);
        mine += tie[e] ? 1u : 0u;
      }
      // (lane 63's before + mine is the wave's count)
      if (lane == 63) tie_cnt[it & 1][wave] = before + mine;
      __syncthreads();   // (two buffers: a wave that runs ahead writes the other one)
      uint32_t rank = taken + before, total = 0;
#pragma unroll
      for (int w = 0; w < kTopkWaves; ++w) {
        const uint32_t n = tie_cnt[it & 1][w];
        rank += (w < wave) ? n : 0u;
        total += n;
      }
      taken += total;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        bool sel = big[e] || (tie[e] && rank < need);
        if constexpr (kIgnore) sel = sel && !(t[e] < 0.f);   // (a selected ignored element still takes its rank)
        rank += tie[e] ? 1u : 0u;
        g[e] = 0.f;
        if (sel) {
          sum += focal_element<kLow>(p[e], t[e], gamma, cube, inv_denom, scale, g[e]);
          // a selected exact hit (fewer than k elements of the row differ from the target): focal_element's zero
          // carries a minus sign; every zero this kernel writes is +0.0
          if (topk_key(p[e], t[e]) == 0u) g[e] = 0.f;
        }
      }
      if (ga != nullptr) {
        if (valid == 15u) {
          *reinterpret_cast<f32x4*>(ga + 4 * c) = f32x4{g[0], g[1], g[2], g[3]};
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if ((valid >> e) & 1u) ga[4 * c + e] = g[e];
        }
      }
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
  if (lane == 0) red[wave] = sum;
  __syncthreads();
  if (tid == 0) partial[static_cast<long>(h) * rows + r] = ((red[0] + red[1]) + (red[2] + red[3])) * inv_denom;
}

constexpr int64_t kTopkMaxP = 0x7fffffffLL;      // P < 2^31: 32-bit counts, the aligned index space in a long
constexpr int64_t kTopkMaxRows = 0x7fffffffLL;   // gridDim.x

}  // namespace
}  // namespace unetpp

using namespace unetpp;

extern "C" int64_t unetpp_topk_focal_workspace_bytes(int32_t n_heads, int64_t rows, int64_t P) {
  if (n_heads < 1 || n_heads > UNETPP_MAX_HEADS || rows < 1 || rows > kTopkMaxRows || P < 1 || P > kTopkMaxP) return 0;
  if (rows > INT64_MAX / P) return 0;
  const int64_t blocks = loss_blocks(rows * P);   // k >= P runs unetpp_focal_bce_heads on this workspace
  return static_cast<int64_t>(n_heads) * (rows > blocks ? rows : blocks) * 4;
}

namespace {

template <bool kIgnore>
int topk_focal_heads_launch(const unetpp_focal_heads* heads, const float* target, int64_t rows, int64_t P, int64_t k,
                            int64_t denom, float gamma, void* workspace, float* kth, float* loss, void* stream) {
  unetpp_focal_heads hd;
  if (loss_heads_checked(heads, target, hd) != UNETPP_OK) return UNETPP_EINVAL;
  if (workspace == nullptr || kth == nullptr || loss == nullptr) return UNETPP_EINVAL;
  if (rows < 1 || rows > kTopkMaxRows || P < 1 || P > kTopkMaxP || k < 1 || denom < 1) return UNETPP_EINVAL;
  if (rows > INT64_MAX / P) return UNETPP_EINVAL;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const bool all = k >= P;
  if (all) {
    const int status = (kIgnore ? unetpp_focal_bce_heads_ignore : unetpp_focal_bce_heads)(
        &hd, target, rows * P, denom, gamma, static_cast<float*>(workspace), loss, stream);
    if (status != UNETPP_OK) return status;
  }
  const float inv_heads = 1.0f / static_cast<float>(hd.n_heads);
  const dim3 grid(static_cast<unsigned>(rows), static_cast<unsigned>(hd.n_heads));
  const auto kernel = gamma < 1.f ? topk_focal_kernel<true, kIgnore> : topk_focal_kernel<false, kIgnore>;
  hipLaunchKernelGGL(kernel, grid, dim3(kTopkThreads), 0, st, hd,
                     target, static_cast<long>(P), static_cast<uint32_t>(all ? P : k), gamma,
                     1.f / static_cast<float>(denom), inv_heads, all ? 0 : 1, static_cast<float*>(workspace), kth);
  if (!all)
    launch_loss_heads_finish(static_cast<const float*>(workspace), static_cast<long>(rows), hd.n_heads, inv_heads, loss, st);
  return launch_status();
}

}  // namespace

extern "C" int unetpp_topk_focal_heads(const unetpp_focal_heads* heads, const float* target, int64_t rows, int64_t P,
                                       int64_t k, int64_t denom, float gamma, void* workspace, float* kth, float* loss,
                                       void* stream) {
  return topk_focal_heads_launch<false>(heads, target, rows, P, k, denom, gamma, workspace, kth, loss, stream);
}

extern "C" int unetpp_topk_focal_heads_ignore(const unetpp_focal_heads* heads, const float* target, int64_t rows, int64_t P,
                                              int64_t k, int64_t denom, float gamma, void* workspace, float* kth,
                                              float* loss, void* stream) {
  return topk_focal_heads_launch<true>(heads, target, rows, P, k, denom, gamma, workspace, kth, loss, stream);
}
