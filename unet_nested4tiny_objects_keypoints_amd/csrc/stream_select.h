// The streaming kernels between the GEMMs -- BatchNorm apply and pool, pool backward, BatchNorm backward in training and
// frozen mode, fp32 and bf16 storage: stream_select decides ONCE, from the arguments of a launcher, which kernel of
// pointwise.hip / pointwise_bf16.hip takes the call and everything that follows from that -- every refusal, the form,
// grid, workgroup, the item and channel-group counts, the rows of the partial buffer and the label.  The twelve
// launchers check their pointers for NULL, fill a StreamQuery and launch what the StreamSel says; bn_bwd_plan asks the
// same selection which route a whole backward takes (unetpp_bn_bwd_plan).  Host only (no HIP header):
// tests/test_stream_select.py compiles it with a plain C++17 compiler.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "unetpp_hip.h"

namespace unetpp {

constexpr int kStreamThreads = 256;   // kThreads (pointwise.hip asserts it)
constexpr long kStreamLimit = 0x7fffffffL;  // 32-bit element offsets (fp32 row forms) and item counts (bf16)
constexpr long kStreamGridCap = 2048 * 8;   // grid_for: one item per thread up to here, then a grid stride
constexpr long kStreamRowCap = 16384;       // the row-structured kernels: one image row (pair) per workgroup up to here
constexpr long kStreamSumCap = 2048;        // the reducing kernels: rows of the partial buffer

enum StreamOp {
  STREAM_AFFINE,     // unetpp_affine_relu_pool[_bf16]: affine + ReLU (+ 2x2 max-pool)
  STREAM_POOL_BWD,   // unetpp_maxpool_bwd[_bf16]
  STREAM_BN_REDUCE,  // unetpp_bn_bwd_reduce, _reduce_pool, _reduce_bf16
  STREAM_BN_APPLY,   // unetpp_bn_bwd_apply, _apply_pool, _apply_bf16
  STREAM_BN_FROZEN,  // unetpp_bn_frozen_bwd[_bf16]
};
enum StreamForm {
  STREAM_SCALAR,  // fp32, any C: item = element
  STREAM_VEC,     // fp32, C % 4 == 0 and 16-byte activations: item = channel quad
  STREAM_ROWS,    // fp32 pool forms: workgroup = image row (pair), 32-bit offsets, four winners per index word
  STREAM_OCTET,   // bf16: item = channel octet
};

struct StreamQuery {
  StreamOp op;
  bool bf16;
  long N;  // the launchers that take a pixel count pass it here, with H = W = 1
  int H, W, C;
  // which optional arguments were given (every other pointer is the launcher's own NULL check)
  bool has_scale, has_shift, has_act, has_pooled;  // STREAM_AFFINE
  bool has_idx, has_dpooled;  // index bytes (STREAM_AFFINE: optional output); the pool gradient pair is d_pooled + index
  bool has_stats, has_partial;  // STREAM_BN_FROZEN: mean and invstd both given; sums wanted
  bool has_gate;                // STREAM_POOL_BWD bf16
  // low four address bits per pointer role, OR-ed over the pointers of a role; 0 for a pointer that was not given
  unsigned in_lo;      // activations read: y, d_act
  unsigned out_lo;     // activations written: act, dy; d_act of the pool backward
  unsigned pooled_lo;  // pooled / d_pooled
  unsigned idx_lo;     // index bytes
  unsigned coef_lo;    // scale | shift
  unsigned stat_lo;    // mean | invstd
  unsigned gamma_lo;   // gamma | dgamma | dbeta
  unsigned gate_lo;
};

// the low four address bits of a pointer role (NULL counts as aligned)
inline unsigned stream_lo4(const void* a, const void* b = nullptr, const void* c = nullptr) {
  return static_cast<unsigned>((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15);
}
inline StreamQuery stream_query(StreamOp op, bool bf16, long N, int H, int W, int C) {
  StreamQuery q{};
  q.op = op, q.bf16 = bf16, q.N = N, q.H = H, q.W = W, q.C = C;
  return q;
}
// the query of a BatchNorm backward pass from its pointers; NULL for what the pass does not take
inline StreamQuery stream_bn_query(StreamOp op, bool bf16, long N, int H, int W, int C, const void* d_act, const void* y,
                                   const void* dy, const void* scale, const void* shift, const void* mean,
                                   const void* invstd, const void* gamma, const void* dgamma, const void* dbeta,
                                   const void* d_pooled, const void* pool_idx, const void* partial) {
  StreamQuery q = stream_query(op, bf16, N, H, W, C);
  q.has_dpooled = d_pooled != nullptr, q.has_idx = pool_idx != nullptr;
  q.has_stats = mean != nullptr && invstd != nullptr, q.has_partial = partial != nullptr;
  q.in_lo = stream_lo4(d_act, y), q.out_lo = stream_lo4(dy), q.pooled_lo = stream_lo4(d_pooled), q.idx_lo = stream_lo4(pool_idx);
  q.coef_lo = stream_lo4(scale, shift), q.stat_lo = stream_lo4(mean, invstd), q.gamma_lo = stream_lo4(gamma, dgamma, dbeta);
  return q;
}

struct StreamSel {
  StreamForm form;
  bool two_pass;  // STREAM_AFFINE with a pool on odd H or W and act wanted: the answer is the window pass over act; the
                  // launcher asks again without the pool for the apply pass that comes first
  unsigned grid, block;
  long items;  // what the kernel loops over: items of the form, image rows for STREAM_ROWS
  int cg;      // channel groups per pixel: C, C / 4 or C / 8
  long buf_rows, rows;  // reducing forms: rows of the partial buffer, rows this grid writes (the launcher zeroes the rest)
  const char* label;
};

inline bool stream_a16(unsigned lo) { return (lo & 15) == 0; }
inline bool stream_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
inline unsigned stream_grid_for(long items) {
  const long b = (items + kStreamThreads - 1) / kStreamThreads;
  return static_cast<unsigned>(b < 1 ? 1 : b > kStreamGridCap ? kStreamGridCap : b);
}

// bf16 BatchNorm backward: C = 8 * CG, CG a power of two <= 256 (a thread keeps its octet across a grid stride)
inline bool stream_octets_ok(int C) { return C >= 8 && (C & 7) == 0 && stream_pow2(C >> 3) && (C >> 3) <= 256; }
// the row-structured pool kernels: 32-bit element offsets, rows long enough to occupy a workgroup
inline bool stream_rows_form_ok(long N, int H, int W, int C) {
  return N * H * W * C < kStreamLimit && static_cast<long>(W / 2) * (C / 4) >= 64;
}
// eligibility of the pool-routing BatchNorm backward, training and frozen (unetpp_bn_bwd_pool_ok)
inline bool stream_bn_pool_ok(long N, int H, int W, int C) {
  if (N < 1 || H < 2 || W < 2 || C < 4 || (H & 1) || (W & 1) || (C & 3)) return false;
  return stream_pow2(C >> 2) && (C >> 2) <= kStreamThreads && N * H * W * C < kStreamLimit;
}
// workgroups of a reducing fp32 form: `per` items each up to kStreamSumCap, and a multiple of the channel-group count
// so that the grid stride keeps every thread on one channel group
inline long stream_sum_blocks(long pixels, int cg, long per) {
  long want = (pixels * cg + per - 1) / per;
  want = want > kStreamSumCap ? kStreamSumCap : want < 1 ? 1 : want;
  return (want + cg - 1) / cg * cg;
}
// Rows of the partial buffer of a BatchNorm backward (the four unetpp_*_blocks exports): the training reduce gives a
// thread 16 items (bf16: 4), the frozen pass one.  fp32: the upper bound over the vector, scalar and pool-routing forms,
// so one workspace serves whichever is launched.  0 for a shape that has no kernel.
inline long stream_partial_rows(bool bf16, bool frozen, long pixels, int C) {
  if (pixels < 1 || C < 1 || (bf16 && !stream_octets_ok(C))) return 0;
  if (bf16) {
    const long per = (frozen ? 1L : 4L) * kStreamThreads, b = (pixels * (C >> 3) + per - 1) / per;
    return b > kStreamSumCap ? kStreamSumCap : b < 1 ? 1 : b;
  }
  const long per = (frozen ? 1L : 16L) * kStreamThreads;
  const long a = (C % 4 == 0) ? stream_sum_blocks(pixels, C / 4, per) : 0, b = stream_sum_blocks(pixels, C, per);
  return a > b ? a : b;
}

// UNETPP_OK or UNETPP_EINVAL
inline int stream_select(const StreamQuery& q, StreamSel& s) {
  s = StreamSel{};
  s.block = kStreamThreads;
  if (q.N < 1 || q.H < 1 || q.W < 1 || q.C < 1) return UNETPP_EINVAL;
  const long pixels = q.N * q.H * q.W, img_rows = q.N * q.H;
  const long windows = q.N * (q.H / 2) * (q.W / 2);  // odd H / W: the last row / column is in no window (floor)
  const bool odd = ((q.H | q.W) & 1) != 0, quads = q.C % 4 == 0;
  const bool in16 = stream_a16(q.in_lo), out16 = stream_a16(q.out_lo), pooled16 = stream_a16(q.pooled_lo);
  const bool coef16 = stream_a16(q.coef_lo), stat16 = stream_a16(q.stat_lo), idx4 = (q.idx_lo & 3) == 0;
  const bool pool = q.has_dpooled, sums = q.op == STREAM_BN_REDUCE || (q.op == STREAM_BN_FROZEN && q.has_partial);
  const bool frozen = q.op == STREAM_BN_FROZEN;
  // the item forms: scalar / quads / octets, one item per thread up to the grid cap
  const auto per_item = [&](StreamForm form, long n_pixels, const char* label) {
    s.form = form;
    s.cg = form == STREAM_OCTET ? q.C >> 3 : form == STREAM_VEC ? q.C / 4 : q.C;
    s.items = n_pixels * s.cg;
    s.grid = stream_grid_for(s.items);
    s.label = label;
    return UNETPP_OK;
  };
  // the row forms: a workgroup per image row (STREAM_AFFINE / STREAM_POOL_BWD: per window row) up to `cap`
  const auto per_row = [&](long rows, long cap, const char* label) {
    s.form = STREAM_ROWS;
    s.cg = q.C >> 2;
    s.items = rows;
    s.grid = static_cast<unsigned>(rows < cap ? rows : cap);
    s.label = label;
    return UNETPP_OK;
  };
  // the reducing forms: the grid is the rows it writes
  const auto summing = [&](long rows) {
    s.buf_rows = stream_partial_rows(q.bf16, frozen, pixels, q.C);
    s.rows = rows < s.buf_rows ? rows : s.buf_rows;
    s.grid = static_cast<unsigned>(s.rows);
  };

  if (q.op == STREAM_AFFINE) {
    if (q.has_scale != q.has_shift || (!q.has_act && !q.has_pooled)) return UNETPP_EINVAL;
    if (q.bf16) {
      if (q.C < 8 || (q.C & 7) || !in16 || !out16) return UNETPP_EINVAL;
      if (!q.has_pooled) return per_item(STREAM_OCTET, pixels, "affine_relu_bf16");
      if (odd || !q.has_idx || !pooled16 || (q.idx_lo & 7) || windows * (q.C >> 3) >= kStreamLimit) return UNETPP_EINVAL;
      return per_item(STREAM_OCTET, windows, "affine_relu_pool_bf16");
    }
    const bool vec = quads && in16 && out16 && pooled16;
    if (!q.has_pooled) return vec ? per_item(STREAM_VEC, pixels, "affine_relu<4>") : per_item(STREAM_SCALAR, pixels, "affine_relu<1>");
    if (q.H < 2 || q.W < 2) return UNETPP_EINVAL;  // (pool_idx may be absent: forward-only callers need no winners)
    if (odd) {
      // nn.MaxPool2d(2) floors: the last odd row / column is in no window, but the activation is wanted for ALL pixels --
      // an apply pass over the whole tensor first, then the window kernel on the activation
      s.two_pass = q.has_act;
      const bool v4 = quads && (q.has_act ? out16 : in16) && pooled16;
      return v4 ? per_item(STREAM_VEC, windows, "affine_relu_pool<4>") : per_item(STREAM_SCALAR, windows, "affine_relu_pool<1>");
    }
    if (vec && stream_rows_form_ok(q.N, q.H, q.W, q.C) && coef16 && idx4) return per_row(q.N * (q.H / 2), kStreamRowCap, "affine_relu_pool_rows");
    return vec ? per_item(STREAM_VEC, windows, "affine_relu_pool<4>") : per_item(STREAM_SCALAR, windows, "affine_relu_pool<1>");
  }

  if (q.op == STREAM_POOL_BWD) {
    if (q.H < 2 || q.W < 2) return UNETPP_EINVAL;
    if (q.bf16) {
      if (odd || q.C < 8 || (q.C & 7) || !pooled16 || !out16 || !stream_a16(q.gate_lo) || (q.idx_lo & 7) ||
          pixels * (q.C >> 3) >= kStreamLimit)
        return UNETPP_EINVAL;
      return per_item(STREAM_OCTET, pixels, "maxpool_bwd_bf16");
    }
    if (!odd && quads && stream_rows_form_ok(q.N, q.H, q.W, q.C) && pooled16 && out16 && idx4)
      return per_row(q.N * (q.H / 2), kStreamRowCap, "maxpool_bwd_rows");
    return quads ? per_item(STREAM_VEC, windows, "maxpool_bwd<4>") : per_item(STREAM_SCALAR, windows, "maxpool_bwd<1>");
  }

  // the three BatchNorm backward passes
  if ((frozen && q.has_partial && !q.has_stats) || q.has_dpooled != q.has_idx) return UNETPP_EINVAL;
  if (q.bf16) {
    // octets only; the pool gradient is routed per item (even H and W)
    if (!stream_octets_ok(q.C) || (pool && odd)) return UNETPP_EINVAL;
    if (frozen && (!in16 || !out16 || !pooled16 || (q.idx_lo & 7))) return UNETPP_EINVAL;
    if (pixels * (q.C >> 3) >= kStreamLimit) return UNETPP_EINVAL;
    static const char* const labels[3][2][2] = {  // [pass][pool][sums]
        {{"bn_bwd_reduce_bf16", "bn_bwd_reduce_bf16"}, {"bn_bwd_reduce_bf16/pool", "bn_bwd_reduce_bf16/pool"}},
        {{"bn_bwd_apply_bf16", "bn_bwd_apply_bf16"}, {"bn_bwd_apply_bf16/pool", "bn_bwd_apply_bf16/pool"}},
        {{"bn_frozen_bwd_bf16", "bn_frozen_bwd_bf16/sums"}, {"bn_frozen_bwd_bf16/pool", "bn_frozen_bwd_bf16/pool/sums"}}};
    per_item(STREAM_OCTET, pixels, labels[q.op - STREAM_BN_REDUCE][pool][sums]);
    if (q.op != STREAM_BN_APPLY) summing(kStreamSumCap);  // (the frozen pass runs this grid with or without sums)
    if (frozen && !sums) s.buf_rows = s.rows = 0;
    return UNETPP_OK;
  }
  if (pool) {
    // routed inside the pass: row-structured, every operand in 16-byte pieces and the winners four to a word
    if (!stream_bn_pool_ok(q.N, q.H, q.W, q.C) || !in16 || !coef16 || !pooled16 || !idx4) return UNETPP_EINVAL;
    if (q.op != STREAM_BN_REDUCE && !out16) return UNETPP_EINVAL;
    if ((!frozen || q.has_partial) && !stat16) return UNETPP_EINVAL;
    if (q.op == STREAM_BN_APPLY && !stream_a16(q.gamma_lo)) return UNETPP_EINVAL;
    per_row(img_rows, kStreamRowCap, q.op == STREAM_BN_REDUCE ? "bn_bwd_reduce_pool"
                                     : q.op == STREAM_BN_APPLY ? "bn_bwd_apply_pool"
                                     : sums ? "bn_frozen_bwd_pool/sums" : "bn_frozen_bwd_pool");
    if (q.op != STREAM_BN_APPLY) summing(img_rows);
    if (frozen && !sums) s.buf_rows = s.rows = 0;
    return UNETPP_OK;
  }
  const bool vec = quads && in16 && (q.op == STREAM_BN_REDUCE || out16);
  static const char* const labels[3][2][2] = {  // [pass][vec][sums]
      {{"bn_bwd_reduce<1>", "bn_bwd_reduce<1>"}, {"bn_bwd_reduce<4>", "bn_bwd_reduce<4>"}},
      {{"bn_bwd_apply<1>", "bn_bwd_apply<1>"}, {"bn_bwd_apply<4>", "bn_bwd_apply<4>"}},
      {{"bn_frozen_bwd<1>", "bn_frozen_bwd<1>/sums"}, {"bn_frozen_bwd<4>", "bn_frozen_bwd<4>/sums"}}};
  per_item(vec ? STREAM_VEC : STREAM_SCALAR, pixels, labels[q.op - STREAM_BN_REDUCE][vec][sums]);
  if (q.op != STREAM_BN_APPLY) summing(stream_sum_blocks(pixels, s.cg, (frozen ? 1L : 16L) * kStreamThreads));
  if (frozen && !sums) s.buf_rows = s.rows = 0;
  return UNETPP_OK;
}

// One BatchNorm + ReLU backward as ops.bn_backward / ops.bn_frozen_backward run it: reduce and apply around the finalize
// in training mode, one pass in frozen mode.  A pool gradient is routed inside the passes where EVERY launch of the
// sequence takes the routing form (route 1), else by unetpp_maxpool_bwd into d_act before the plain forms (route 2).
struct BnBwdQuery {
  bool frozen, bf16, sums, pool;  // sums: frozen only (training always sums)
  long N;
  int H, W, C;
  unsigned in_lo, out_lo, pooled_lo, idx_lo, coef_lo, stat_lo, gamma_lo;  // as StreamQuery
};
struct BnBwdPlan {
  int route;  // 0 no pool gradient (and refused), 1 routed inside the passes, 2 unetpp_maxpool_bwd first
  long partial_rows, partial_floats;  // rows of `partial` ([rows][C][2]); 0 for a shape no kernel takes
};
inline int bn_bwd_plan(const BnBwdQuery& b, BnBwdPlan& p) {
  p = BnBwdPlan{};
  p.partial_rows = stream_partial_rows(b.bf16, b.frozen, b.N * b.H * b.W, b.C);
  p.partial_floats = p.partial_rows * b.C * 2;
  StreamQuery q{};
  q.bf16 = b.bf16;
  q.N = b.N, q.H = b.H, q.W = b.W, q.C = b.C;
  q.has_stats = q.has_partial = !b.frozen || b.sums;
  q.in_lo = b.in_lo, q.out_lo = b.out_lo, q.coef_lo = b.coef_lo, q.stat_lo = b.stat_lo, q.gamma_lo = b.gamma_lo;
  StreamSel s;
  const auto accepts = [&](StreamOp op) {
    q.op = op;
    return stream_select(q, s) == UNETPP_OK;
  };
  const auto passes_accept = [&] {
    return b.frozen ? accepts(STREAM_BN_FROZEN) : accepts(STREAM_BN_REDUCE) && accepts(STREAM_BN_APPLY);
  };
  if (b.pool) {
    q.has_dpooled = q.has_idx = true;
    q.pooled_lo = b.pooled_lo, q.idx_lo = b.idx_lo;
    p.route = 1;
    if (passes_accept()) return UNETPP_OK;
    p.route = 2;
    q.out_lo = b.in_lo;  // into d_act
    if (!accepts(STREAM_POOL_BWD)) return p.route = 0, UNETPP_EINVAL;
    q.has_dpooled = q.has_idx = false;
    q.pooled_lo = q.idx_lo = 0;
    q.out_lo = b.out_lo;
  }
  if (passes_accept()) return UNETPP_OK;
  return p.route = 0, UNETPP_EINVAL;
}

}  // namespace unetpp
