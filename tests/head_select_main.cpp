// Stand-alone driver of csrc/head_select.h for tests/test_head_select.py: one query per input line
//   op bf16 N H W C n_cls n_heads p_drop has_mask x_lo weight_lo dx_lo mask_lo wgs_per_cu cus
// one answer per output line
//   rc label grid block lds active          (label "-" and zeros for a refusal)
#include <stdio.h>

#include "head_select.h"
#include "unetpp_hip.h"

int main() {
  int op, bf16, has_mask, cus;
  unetpp::HeadQuery q{};
  while (scanf("%d %d %d %d %d %d %d %d %f %d %u %u %u %u %ld %d", &op, &bf16, &q.N, &q.H, &q.W, &q.C, &q.n_cls,
               &q.n_heads, &q.p_drop, &has_mask, &q.x_lo, &q.weight_lo, &q.dx_lo, &q.mask_lo, &q.wgs_per_cu, &cus) == 16) {
    q.op = static_cast<unetpp::HeadOp>(op);
    q.bf16 = bf16 != 0;
    q.has_mask = has_mask != 0;
    unetpp::HeadSel s;
    const int rc = unetpp::head_select(q, cus, s);
    if (rc == UNETPP_OK)
      printf("%d %s %u %u %zu %u\n", rc, s.label, s.grid, s.block, s.lds, s.active);
    else
      printf("%d - 0 0 0 0\n", rc);
  }
  return 0;
}
