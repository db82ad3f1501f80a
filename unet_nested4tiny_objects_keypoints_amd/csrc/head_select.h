// The deep-supervision heads: head_select decides ONCE, from the arguments of a launcher, which kernel of heads.hip takes
// the call and everything that follows from that -- every refusal and its return code, the form and the template
// coordinates, grid, workgroup, dynamic LDS, the bf16 backward's `active` count and the label.  The launchers of
// heads.hip (six, the two of the ensemble mean's backward and the training pass unetpp_head_train) check their pointers,
// fill a HeadQuery and launch what the HeadSel says.  Host only (no HIP header):
// tests/test_head_select.py compiles it with a plain C++17 compiler.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "unetpp_hip.h"

namespace unetpp {

constexpr int kHeadMaxC = 128;
constexpr int kHeadMaxCls = 8;
constexpr int kHeadThreads = 256;     // kThreads (heads.hip asserts it)
constexpr int kHeadTilePixels = 256;  // pixel tile of head_bwd_bf16_kernel up to 64 channels (128 pixels at 128 channels)

enum HeadOp {
  HEAD_FWD, HEADS_MEAN, HEAD_BWD,
  HEADS_MEAN_BWD,  // unetpp_heads_mean_bwd[_bf16], one launch per head
  HEAD_TRAIN,      // unetpp_head_train: forward, loss gradient and backward of one head in one pass (fp32 only)
};
enum HeadForm {
  HEAD_STREAM,   // fp32 forward / mean: lane = (pixel, channel quad), C = 4 * 2^log2g
  HEAD_TILED,    // fp32 forward: 64-pixel LDS tiles, any C % 4 == 0
  HEAD_POW2,     // fp32 backward: C = 4 * 2^log2g
  HEAD_VEC,      // fp32 backward: any C % 4 == 0
  HEAD_GENERIC,  // fp32, any C: scalar loads
  HEAD_OCTET,    // bf16: lane = (pixel, channel octet), C = 8 * 2^log2g
  HEAD_OCTET_GENERAL,  // bf16 mean only: any C
};

struct HeadQuery {
  HeadOp op;
  bool bf16;
  int N, H, W, C, n_cls;
  int n_heads;    // HEADS_MEAN, HEADS_MEAN_BWD and HEAD_TRAIN (the heads the loss is averaged over) only
  float p_drop;   // 0 for HEADS_MEAN
  bool has_mask;  // a mask pointer was given (whether or not p_drop uses it)
  // low four address bits per pointer role; HEADS_MEAN: x and weight OR-ed over the heads (HEADS_MEAN_BWD: and dx)
  unsigned x_lo, weight_lo, dx_lo, mask_lo;
  long wgs_per_cu;  // OPT_HEAD_WGS_PER_CU value (bf16 backward only)
};

struct HeadSel {
  HeadForm form;
  int log2g, drop, pcls;  // template coordinates: log2 of the channel groups per pixel, dropout mode 0 none / 1 hash / 2 mask, padded classes
  unsigned grid, block;
  size_t lds;       // dynamic LDS bytes
  unsigned active;  // bf16 backward: workgroups that take tiles
  const char* label;
};

// "head_bwd_pow2<3,1,8>" and the like for every (family, log2g, drop, pcls): a constant table, so that a label is a
// pointer into static storage (note_kernel keeps it) and the launch path formats nothing
struct HeadLabels {
  char s[7][6][3][3][24];  // [op + 3 * bf16, 6: the training pass][log2g][drop][pcls / 2 - 2]
};
constexpr HeadLabels make_head_labels() {
  const char* pattern[7] = {"head_fwd_stream<L,P,D>", "heads_mean_stream<L,P>", "head_bwd_pow2<L,D,P>",  // L, D, P: the
                            "head_fwd_bf16<L,D,P>",   "heads_mean_bf16<L,P>",   "head_bwd_bf16<L,D,P>",   // coordinates
                            "head_train_pow2<L,D,P>"};
  HeadLabels t{};
  for (int f = 0; f < 7; ++f)
    for (int l = 0; l < 6; ++l)
      for (int d = 0; d < 3; ++d)
        for (int p = 0; p < 3; ++p)
          for (int n = 0; pattern[f][n] != 0; ++n) {
            const char c = pattern[f][n];
            t.s[f][l][d][p][n] = static_cast<char>(c == 'L' ? '0' + l : c == 'D' ? '0' + d : c == 'P' ? '4' + 2 * p : c);
          }
  return t;
}
inline constexpr HeadLabels kHeadLabels = make_head_labels();

inline bool head_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
inline int head_log2(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}

// UNETPP_OK, UNETPP_EINVAL, or UNETPP_ELAUNCH (bf16 backward without a usable CU count).  cus_fn() is device_cu_count():
// called for the bf16 backward only, once, after every argument refusal.
template <class CusFn>
inline int head_select_with(const HeadQuery& q, CusFn&& cus_fn, HeadSel& s) {
  s = HeadSel{};
  const bool mean = q.op == HEADS_MEAN, bwd = q.op == HEAD_BWD, mean_bwd = q.op == HEADS_MEAN_BWD, train = q.op == HEAD_TRAIN;
  if (q.N < 1 || q.H < 1 || q.W < 1 || q.C < 1 || q.C > kHeadMaxC || q.n_cls < 1 || q.n_cls > kHeadMaxCls ||
      !(q.p_drop >= 0.f && q.p_drop < 1.f) ||
      ((mean || mean_bwd || train) && (q.n_heads < 1 || q.n_heads > UNETPP_MAX_HEADS)))
    return UNETPP_EINVAL;
  const long pixels = static_cast<long>(q.N) * q.H * q.W;
  const bool x16 = (q.x_lo & 15) == 0, w16 = (q.weight_lo & 15) == 0, dx16 = (q.dx_lo & 15) == 0;
  const long tiles64 = (pixels + 63) / 64;
  const long rows = (pixels + kHeadThreads - 1) / kHeadThreads;  // thread = pixel: the generic forward kernels
  s.drop = q.p_drop > 0.f ? (q.has_mask ? 2 : 1) : 0;
  s.block = kHeadThreads;
  // both backward grids (and the rows of `partial`) are unetpp_head_bwd_blocks: 64-pixel tiles, 16 workgroups per CU --
  // the tile loop is a chain of dependent loads, occupancy hides it
  s.grid = static_cast<unsigned>(tiles64 < 4096 ? tiles64 : 4096);
  if (mean_bwd) {
    // Backward of the ensemble mean: heads_mean_bwd_kernel once per head, on head_bwd_vec's 64-pixel tiles and grid.  It
    // takes what unetpp_head_bwd (fp32: anything, 16-byte pieces where rows and pointers allow) or unetpp_head_bwd_bf16
    // (octets only) takes for one head; the mean has no dropout.  LDS: x tile | dlogit | W | scratch, as head_bwd_vec.
    if (q.p_drop != 0.f) return UNETPP_EINVAL;
    if (q.bf16) {
      const int cg = q.C >> 3;
      if ((q.C & 7) != 0 || !head_pow2(cg) || !x16 || !dx16 || pixels >= 0x7fffffffL) return UNETPP_EINVAL;
      s.form = HEAD_OCTET;
      s.log2g = head_log2(cg);
      s.pcls = q.n_cls <= 4 ? 4 : q.n_cls <= 6 ? 6 : 8;
      s.label = "heads_mean_bwd_bf16";
    } else {
      const bool vec = (q.C & 3) == 0 && x16 && dx16;
      s.form = vec ? HEAD_VEC : HEAD_GENERIC;
      s.pcls = q.n_cls <= 4 ? 4 : 8;
      s.log2g = head_log2((q.C >> 2) > 0 ? (q.C >> 2) : 1);
      s.label = vec ? "heads_mean_bwd_vec" : "heads_mean_bwd";
    }
    s.lds = (64 * (q.C + 1) + 64 * kHeadMaxCls + kHeadMaxCls * q.C + 2 * q.n_cls * q.C) * sizeof(float);
    return UNETPP_OK;
  }
  if (train && q.bf16) return UNETPP_EINVAL;  // fp32 storage only
  const int family = q.op + 3 * (q.bf16 ? 1 : 0);

  if (q.bf16) {
    // bf16 has the octet kernels only (the mean also a general one): what they cannot take is refused
    const int cg = q.C >> 3;
    const bool octets = (q.C & 7) == 0 && head_pow2(cg);  // C = 8 * 2^k (k <= 4: C <= kHeadMaxC)
    const bool count32 = pixels < 0x7fffffffL;            // pixels are counted in 32 bits, element offsets are 64-bit
    if (mean) {
      if ((q.x_lo & 1) != 0) return UNETPP_EINVAL;  // not even a bf16 element boundary
      if (!(octets && x16 && count32)) {
        s.form = HEAD_OCTET_GENERAL;
        s.grid = static_cast<unsigned>(rows < 2048 * 8 ? rows : 2048 * 8);
        s.label = "heads_mean_bf16_general";
        return UNETPP_OK;
      }
    } else if (!octets || !x16 || (bwd && !dx16) || !count32 || (s.drop == 2 && (q.mask_lo & 7) != 0)) {
      return UNETPP_EINVAL;  // (a used mask is read as 8-byte octets; an unused one is never read)
    }
    s.form = HEAD_OCTET;
    s.log2g = head_log2(cg);
    s.pcls = q.n_cls <= 4 ? 4 : q.n_cls <= 6 ? 6 : 8;  // 6: the 5 key-point maps
    if (!bwd) {
      const long ppb = kHeadThreads / cg, passes = (pixels + ppb - 1) / ppb;
      s.grid = static_cast<unsigned>(passes < 256 * 16 ? passes : 256 * 16);
      if (mean) s.lds = static_cast<size_t>(q.n_heads) * s.pcls * q.C * sizeof(float);  // one padded weight tile per head
    } else {
      const int cus = cus_fn();
      if (cus <= 0) return UNETPP_ELAUNCH;
      s.lds = (kHeadTilePixels * kHeadMaxCls + 4 * (kHeadMaxCls * q.C + kHeadMaxCls)) * sizeof(float);  // dlogit tile + 4 wave rows
      // Workgroups that take tiles: at most wgs_per_cu per CU (default 4; 0 = every workgroup), and then as few as walk
      // the same number of rounds (2304 tiles: 3 rounds of 768 rather than 1024 workgroups of which 256 carry a third
      // tile).  Counted in 256-pixel tiles although the grid is sized from 64-pixel ones: the kernel's tile for C <= 64;
      // at C = 128 its tiles are 128 pixels -- twice the rounds, the same rule.
      s.active = s.grid;
      const long n_tiles = (pixels + kHeadTilePixels - 1) / kHeadTilePixels, most = q.wgs_per_cu * cus;
      if (q.wgs_per_cu > 0 && most < n_tiles) {
        const long rounds = (n_tiles + most - 1) / most;
        s.active = static_cast<unsigned>((n_tiles + rounds - 1) / rounds);
      }
      if (s.active > s.grid) s.active = s.grid;
    }
    s.label = kHeadLabels.s[family][s.log2g][s.drop][s.pcls / 2 - 2];
    return UNETPP_OK;
  }

  // fp32: every call has a kernel.  The templated forms need C = 4 * 2^k, 16-byte rows and 32-bit element offsets; a
  // mask pointer is read in 4-byte pieces there, so a misaligned one keeps the call off them even when p_drop is 0
  const int g4 = q.C >> 2;
  const bool quads = (q.C & 3) == 0;
  const bool pow2 = quads && x16 && w16 && head_pow2(g4) && g4 <= 32 && pixels * q.C < 0x7fffffffL &&
                    (!q.has_mask || (q.mask_lo & 3) == 0);
  s.pcls = q.n_cls <= 4 ? 4 : 8;
  s.log2g = head_log2(g4 > 0 ? g4 : 1);
  if (train) {
    // The training pass is head_fwd_stream's logits inside head_bwd_pow2's tile walk: it takes a call only where BOTH of
    // them take the three-launch path's calls (its results are theirs bit for bit), on the backward's grid and LDS plan.
    // Anything else is refused; the caller then runs the three launches.
    if (!(pow2 && dx16 && s.pcls <= g4)) return UNETPP_EINVAL;
    s.form = HEAD_POW2;
    s.lds = (64 * (q.C + 1) + 64 * kHeadMaxCls + 2 * q.n_cls * q.C) * sizeof(float);  // x tile | dlogit | scratch
    s.label = kHeadLabels.s[6][s.log2g][s.drop][s.pcls / 2 - 2];
    return UNETPP_OK;
  }
  if (!bwd) {
    if (pow2 && s.pcls <= g4) {  // the reduce-scatter deals the classes to the lanes of a pixel: at most one each
      s.form = HEAD_STREAM;
      const long ppb = kHeadThreads / g4, want = (pixels + ppb - 1) / ppb;
      s.grid = static_cast<unsigned>(want < 256 * 16 ? want : 256 * 16);
      s.label = kHeadLabels.s[family][s.log2g][s.drop][s.pcls / 2 - 2];
    } else if (!mean && quads && x16) {  // (the mean has no tiled form)
      s.form = HEAD_TILED;
      s.block = 64;
      s.grid = static_cast<unsigned>(tiles64 < 256 * 16 ? tiles64 : 256 * 16);
      s.lds = 64 * (q.C + 1) * sizeof(float);
      s.label = "head_fwd_tiled";
    } else {
      s.form = HEAD_GENERIC;
      s.grid = static_cast<unsigned>(rows < 2048 * 8 ? rows : 2048 * 8);
      s.label = mean ? "heads_mean" : "head_fwd";
    }
    return UNETPP_OK;
  }
  const size_t tile_floats = 64 * (q.C + 1) + 64 * kHeadMaxCls + 2 * q.n_cls * q.C;  // x tile | dlogit | scratch
  if (pow2 && dx16 && g4 >= 2) {  // classes stay in registers: no pcls <= g4 condition, but a pixel spans two lanes or more
    s.form = HEAD_POW2;
    s.lds = tile_floats * sizeof(float);
    s.label = kHeadLabels.s[family][s.log2g][s.drop][s.pcls / 2 - 2];
  } else if (quads && x16 && dx16) {
    s.form = HEAD_VEC;
    s.lds = (tile_floats + kHeadMaxCls * q.C) * sizeof(float);  // and the weights in LDS
    s.label = "head_bwd_vec";
  } else {
    s.form = HEAD_GENERIC;
    s.label = "head_bwd";
  }
  return UNETPP_OK;
}
inline int head_select(const HeadQuery& q, int cus, HeadSel& s) {
  return head_select_with(q, [cus] { return cus; }, s);
}

}  // namespace unetpp
