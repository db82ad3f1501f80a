// Monte-Carlo dropout at one head (unetpp_head_mc, heads.hip): what the launcher accepts, and what follows from that.
// The kernel is head_fwd_stream_kernel's layout with the samples as an inner loop, so it takes exactly the fp32 calls for
// which head_select answers HEAD_STREAM to a HEAD_FWD query with hashed dropout and no mask -- that question is asked of
// head_select itself, its queries and answers stay as they are -- plus 0 < p_drop < 1 and 2 <= samples <=
// UNETPP_MC_MAX_SAMPLES.  Host only (no HIP header), as head_select.h.
#pragma once
#include "head_select.h"

namespace unetpp {

// sample k of a call draws its keep flags from seed + kMcSeedStep * k (mod 2^64)
constexpr uint64_t kMcSeedStep = 0xD6E8FEB86659FD93ULL;

// "head_mc<3,4>" and the like for every (log2g, pcls): a constant table, as kHeadLabels
struct HeadMcLabels {
  char s[6][2][16];  // [log2g][pcls / 4 - 1]
};
constexpr HeadMcLabels make_head_mc_labels() {
  const char* pattern = "head_mc<L,P>";
  HeadMcLabels t{};
  for (int l = 0; l < 6; ++l)
    for (int p = 0; p < 2; ++p)
      for (int n = 0; pattern[n] != 0; ++n) {
        const char c = pattern[n];
        t.s[l][p][n] = static_cast<char>(c == 'L' ? '0' + l : c == 'P' ? '4' + 4 * p : c);
      }
  return t;
}
inline constexpr HeadMcLabels kHeadMcLabels = make_head_mc_labels();

// UNETPP_OK with s filled (log2g, pcls, the forward's grid and workgroup, the sample slab as dynamic LDS, the label), or
// UNETPP_EINVAL.  x_lo / weight_lo: the low four address bits of x and weight.
inline int head_mc_select(int N, int H, int W, int C, int n_cls, float p_drop, int samples, unsigned x_lo,
                          unsigned weight_lo, HeadSel& s) {
  s = HeadSel{};
  if (!(p_drop > 0.f && p_drop < 1.f) || samples < 2 || samples > UNETPP_MC_MAX_SAMPLES) return UNETPP_EINVAL;
  HeadQuery q{};
  q.op = HEAD_FWD, q.bf16 = false, q.N = N, q.H = H, q.W = W, q.C = C, q.n_cls = n_cls, q.p_drop = p_drop;
  q.has_mask = false;
  q.x_lo = x_lo, q.weight_lo = weight_lo;
  const int rc = head_select(q, 0, s);
  if (rc != UNETPP_OK) return rc;
  if (s.form != HEAD_STREAM || s.drop != 1) return UNETPP_EINVAL;
  s.lds = static_cast<size_t>(samples) * kHeadThreads * sizeof(float);  // one column of `samples` floats per thread
  s.label = kHeadMcLabels.s[s.log2g][s.pcls / 4 - 1];
  return UNETPP_OK;
}

}  // namespace unetpp
