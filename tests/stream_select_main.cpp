// Stand-alone driver of csrc/stream_select.h for tests/test_stream_select.py: one query per input line.
//   S op bf16 N H W C  scale shift act pooled idx dpooled stats partial gate  in out pooled idx coef stat gamma gate
// (the nine flags, then the low address bits of the eight pointer roles) is answered by
//   rc label grid block buf_rows rows       (label "-" and zeros for a refusal)
//   P frozen bf16 sums pool N H W C  in out pooled idx coef stat gamma
// is a whole BatchNorm backward (bn_bwd_plan), answered by
//   rc route partial_rows partial_floats
#include <stdio.h>

#include "stream_select.h"
#include "unetpp_hip.h"

int main() {
  char kind;
  while (scanf(" %c", &kind) == 1) {
    if (kind == 'S') {
      int op, bf16, f[9];
      unetpp::StreamQuery q{};
      if (scanf("%d %d %ld %d %d %d %d %d %d %d %d %d %d %d %d %u %u %u %u %u %u %u %u", &op, &bf16, &q.N, &q.H, &q.W, &q.C,
                &f[0], &f[1], &f[2], &f[3], &f[4], &f[5], &f[6], &f[7], &f[8], &q.in_lo, &q.out_lo, &q.pooled_lo, &q.idx_lo,
                &q.coef_lo, &q.stat_lo, &q.gamma_lo, &q.gate_lo) != 23)
        return 1;
      q.op = static_cast<unetpp::StreamOp>(op);
      q.bf16 = bf16 != 0;
      q.has_scale = f[0] != 0, q.has_shift = f[1] != 0, q.has_act = f[2] != 0, q.has_pooled = f[3] != 0, q.has_idx = f[4] != 0;
      q.has_dpooled = f[5] != 0, q.has_stats = f[6] != 0, q.has_partial = f[7] != 0, q.has_gate = f[8] != 0;
      unetpp::StreamSel s;
      const int rc = unetpp::stream_select(q, s);
      if (rc == UNETPP_OK)
        printf("%d %s %u %u %ld %ld\n", rc, s.label, s.grid, s.block, s.buf_rows, s.rows);
      else
        printf("%d - 0 0 0 0\n", rc);
    } else if (kind == 'P') {
      int f[4];
      unetpp::BnBwdQuery b{};
      if (scanf("%d %d %d %d %ld %d %d %d %u %u %u %u %u %u %u", &f[0], &f[1], &f[2], &f[3], &b.N, &b.H, &b.W, &b.C, &b.in_lo,
                &b.out_lo, &b.pooled_lo, &b.idx_lo, &b.coef_lo, &b.stat_lo, &b.gamma_lo) != 15)
        return 1;
      b.frozen = f[0] != 0, b.bf16 = f[1] != 0, b.sums = f[2] != 0, b.pool = f[3] != 0;
      unetpp::BnBwdPlan p;
      const int rc = unetpp::bn_bwd_plan(b, p);
      printf("%d %d %ld %ld\n", rc, p.route, p.partial_rows, p.partial_floats);
    } else {
      return 1;
    }
  }
  return 0;
}
