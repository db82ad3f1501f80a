"""The deep-supervision heads (dropout + 1x1 convolution + sigmoid, forward and backward) against float64.

The four head launchers (heads.hip: unetpp_head_fwd / unetpp_head_bwd, unetpp_head_fwd_bf16 / unetpp_head_bwd_bf16; the
choice is head_select's, head_select.h) dispatch ~140 instantiations: the dropout mode D (0 none, 1 keep flags from the in-kernel
counter hash, 2 keep flags from a mask tensor), the channel count as a power of two L and the padded class count PC,
plus general fallbacks for other channel counts.  Each launcher names its choice (unetpp_last_kernel_name).

(a) Dispatch matrix on random data: every instantiation, forward and backward, against a float64 reference that applies
    the restated keep mask (oracle/dropout_oracle.py keep_mask) for D = 1 and D = 2, under a-priori element-wise bounds
    (tests/helpers.py):
        logits    |z - z64| <= gamma_(C+2) (sum_c |x~_c w_c| + |b|)          x~ = x * keep * scale (fp32 scale)
        out       |s - s64| <= s(1-s) (that bound + EXP_ARG_ULPS u (|z| + 1)) + SIGMOID_ULPS u s
        dx        |dx - dx64| <= gamma_(n_cls+5) (scale sum_k |dl_k w_kc| + |old|)   dl from the kernel's own out
                  (3 roundings in dl = d_out out (1 - out), n_cls in the dot product, 1 for the scale, 1 for old)
    next to the suite's 1e-4 relative bar; bf16 dx keeps close_bf16; dW and db the 1e-4 bar.
(b) Generator against mask, bit for bit: a D = 1 launch with seed s, a D = 2 launch given keep_mask(s) and a D = 1
    launch given the seed as seed + device word must agree in out, dx, dW and db exactly.
(c) Production geometries in exact arithmetic: small-integer x (mostly zero), weights and biases in multiples of 1/8,
    p = 0.5 (scale 2) or 0, a synthetic out in {1/4, 1/2, 3/4} and small-integer d_out: every sum is exact in fp32
    under any order (each case asserts sum |terms| < 2^24 grid units), so dW, db and fp32 dx must equal the float64
    result exactly, bf16 dx its round-to-nearest-even, whatever the tiling, rounds and partial sums.
(d) Every COVERAGE entry ran, and each family ran above its grid cap with H*W not dividing the kernel's span.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle.dropout_oracle import keep_mask
from tests.helpers import U32, bound_ratio, gamma, rel_err, report_ratio, usable_cus

pytestmark = pytest.mark.gpu

TOL = 1e-4
BF = torch.bfloat16
P_DROP = 0.4
HEAD_SEED_STEP = 0x632BE59BD9B4E019     # engine._dropout_config: head j draws base + HEAD_SEED_STEP * (j + 1)
EXP_ARG_ULPS = 4.0   # estimate (not derived): relative error of exp(-z) is <= EXP_ARG_ULPS u (|z| + 1) (__expf, expf)
SIGMOID_ULPS = 4.0   # estimate (not derived): the add, the division / reciprocal and the store of 1 / (1 + e)
MASK64 = 0xFFFFFFFFFFFFFFFF


def _coverage():
    names = []
    for d in (0, 1, 2):
        names += ["head_fwd_stream<%d,4,%d>" % (L, d) for L in (2, 3, 4, 5)]
        names += ["head_fwd_stream<%d,8,%d>" % (L, d) for L in (3, 4, 5)]
        names += ["head_fwd_tiled/D%d" % d, "head_fwd/D%d" % d]
        names += ["head_bwd_pow2<%d,%d,%d>" % (L, d, pc) for L in (1, 2, 3, 4, 5) for pc in (4, 8)]
        names += ["head_bwd_vec/D%d" % d, "head_bwd/D%d" % d]
        names += ["head_fwd_bf16<%d,%d,%d>" % (L, d, pc) for L in (0, 1, 2, 3, 4) for pc in (4, 6, 8)]
        names += ["head_bwd_bf16<%d,%d,%d>" % (L, d, pc) for L in (0, 1, 2, 3, 4) for pc in (4, 6, 8)]
    return names


COVERAGE = _coverage()
SEEN = set()
FAMILIES = ("fp32_fwd", "fp32_bwd", "bf16_fwd", "bf16_bwd")
ABOVE_CAP = set()    # families that ran with several spans of their grid and H*W not dividing the span


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    yield torch.device("cuda:0")
    from unet_nested4tiny_objects_keypoints_amd import _lib
    phys = ctypes.c_int32(0)
    assert int(_lib.lib().unetpp_usable_cus(ctypes.byref(phys))) == phys.value   # the knob is back at 0


def last_kernel():
    from unet_nested4tiny_objects_keypoints_amd import _lib
    return _lib.lib().unetpp_last_kernel_name().decode()


def usable():
    from unet_nested4tiny_objects_keypoints_amd import _lib
    return int(_lib.lib().unetpp_usable_cus(None))


def head_seed(base, j):
    return (base + HEAD_SEED_STEP * (j + 1)) & MASK64


def keep_scale(p):
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))   # the launchers' 1.0f / (1.0f - p_drop)


def _note(name, d):
    SEEN.add(name if "<" in name else "%s/D%d" % (name, d))


def spans(bf16, pixels, c, hw):
    """(forward span, backward span) in pixels of the launchers' grids (head_select.h)."""
    if bf16:
        cg = c // 8
        ppb = 256 // cg
        fwd = min(-(-pixels // ppb), 4096) * ppb
        tp = 256 if cg <= 8 else 8 * 256 // cg                     # the kernel's tile (128 pixels at C = 128)
        grid = min(-(-pixels // 64), 4096)
        n256 = -(-pixels // 256)
        most = 4 * usable()                                        # HEAD_WGS_PER_CU (default 4) per usable CU
        active = grid
        if most < n256:
            rounds = -(-n256 // most)
            active = -(-n256 // rounds)
        active = min(active, grid)
        return fwd, active * tp
    g4 = c // 4
    if c % 4 == 0 and g4 & (g4 - 1) == 0 and 4 <= g4 <= 32:      # the stream kernel (n_cls <= g4 assumed by callers)
        ppb = 256 // g4
        fwd = min(-(-pixels // ppb), 4096) * ppb
    else:
        fwd = min(-(-pixels // 64), 4096) * 64
    return fwd, 4096 * 64


def _mark_spans(bf16, pixels, c, hw, fwd_name):
    fam = "bf16" if bf16 else "fp32"
    fs, bs = spans(bf16, pixels, c, hw)
    if fwd_name.startswith(("head_fwd_stream", "head_fwd_tiled", "head_fwd_bf16")) and pixels > fs and hw % fs:
        ABOVE_CAP.add(fam + "_fwd")
    if pixels > bs and hw % bs:
        ABOVE_CAP.add(fam + "_bwd")


# --------------------------------------------------------------------------------------------- launches
def run_fwd(x, wt, bias, p, seed, mask=None, seed_dev=None):
    from unet_nested4tiny_objects_keypoints_amd import ops
    n, h, w, _ = x.shape
    out = torch.full((n, wt.shape[0], h, w), float("nan"), device=x.device)
    ops.head_fwd(x, wt, bias, p, seed, mask, out, seed_dev=seed_dev)
    name = last_kernel()
    _note(name, 0 if p == 0 else (2 if mask is not None else 1))
    return out, name


def run_bwd(d_out, out, x, wt, p, seed, mask, old, accumulate, gate, seed_dev=None):
    from unet_nested4tiny_objects_keypoints_amd import ops
    dx = old.clone() if accumulate else torch.full_like(x, float("nan"))
    dw, db = ops.head_bwd(d_out, out, x, wt, p, seed, mask, dx, accumulate, gate_x=gate, seed_dev=seed_dev)
    name = last_kernel()
    _note(name, 0 if p == 0 else (2 if mask is not None else 1))
    torch.cuda.synchronize()
    return dx, dw.view(wt.shape).clone(), db.clone(), name


# --------------------------------------------------------------------------------------------- float64 references
def ref_forward(x64, wt64, b64, ms):
    """-> (z, sum |terms|): x64 NHWC, ms = keep * scale NHWC (None: no dropout)."""
    xt = x64 if ms is None else x64 * ms
    z = torch.einsum("nhwc,kc->nkhw", xt, wt64) + b64.view(1, -1, 1, 1)
    mag = torch.einsum("nhwc,kc->nkhw", xt.abs(), wt64.abs()) + b64.abs().view(1, -1, 1, 1)
    return z, mag


def out_bound(z, zb):
    s = torch.sigmoid(z)
    return s * (1 - s) * (zb + EXP_ARG_ULPS * U32 * (z.abs() + 1)) * 1.01 + SIGMOID_ULPS * U32 * s + 1e-300


def ref_backward(d_out64, out64, x64, wt64, ms, old64, gate):
    """-> (dx, |dx| magnitude for the bound, dW, db); dl from the kernel's own out."""
    dl = d_out64 * out64 * (1 - out64)
    s = torch.einsum("nkhw,kc->nhwc", dl, wt64)
    mag = torch.einsum("nkhw,kc->nhwc", dl.abs(), wt64.abs())
    xt = x64
    if ms is not None:
        s, mag, xt = s * ms, mag * ms.abs(), x64 * ms
    if old64 is not None:
        s, mag = s + old64, mag + old64.abs()
    if gate:
        s = torch.where(x64 > 0, s, torch.zeros_like(s))
    dw = torch.einsum("nkhw,nhwc->kc", dl, xt)
    db = dl.sum((0, 2, 3))
    return s, mag, dw, db


def close_bf16(got, want, what=""):
    from tests.test_gpu_bf16 import close_bf16 as cb
    cb(got, want, what)


# --------------------------------------------------------------------------------------------- (a) + (b)
FP32_CASES = [   # (C, n_cls): the kernels they reach forward / backward
    (16, 4), (16, 6),      # stream<2,4> / pow2<2,*,4>;   tiled (8 classes > 4 quads) / pow2<2,*,8>
    (32, 1), (32, 5),      # stream<3,4>, stream<3,8>;    pow2<3,*,4>, pow2<3,*,8>
    (64, 3), (64, 8),      # stream<4,4>, stream<4,8>;    pow2<4,*,*>
    (128, 2), (128, 7),    # stream<5,*>;                 pow2<5,*,*>
    (8, 3), (8, 8),        # tiled;                       pow2<1,*,4>, pow2<1,*,8>
    (4, 2), (24, 5),       # tiled;                       vec
    (6, 3), (3, 8),        # plain head_fwd;              plain head_bwd (C not a multiple of 4)
]
BF16_CASES = [(8, 4), (8, 6), (8, 8), (16, 1), (16, 5), (16, 7), (32, 3), (32, 6), (32, 8),
              (64, 2), (64, 5), (64, 8), (128, 4), (128, 6), (128, 8)]
MATRIX = ([("fp32", c, k, 2, 13, 29) for c, k in FP32_CASES] + [("bf16", c, k, 2, 13, 29) for c, k in BF16_CASES])
# grid-stride paths on random data: one span, 1..4 spans and more than 4 spans of the forward grids, and more than four
# 64-pixel tiles per workgroup of the fp32 backward / several rounds of the bf16 backward; H*W divides no span
SPANS = [
    ("fp32", 128, 4, 1, 181, 181),     # stream<5,4>: span 32768 pixels, 32761 pixels (one span)
    ("fp32", 128, 8, 2, 150, 200),     # 60000 pixels: 1..4 spans
    ("fp32", 128, 3, 3, 211, 223),     # 141159 pixels: > 4 spans
    ("fp32", 8, 3, 5, 250, 900),       # tiled and pow2<1>: 1.1e6 pixels, > 4 spans of 262144
    ("bf16", 8, 5, 5, 250, 900),       # bf16 forward 1.1 spans of 1048576; backward in several rounds
    ("bf16", 128, 8, 3, 211, 223),     # bf16 C = 128: 65536-pixel forward span, 128-pixel backward tiles
]


def _case_id(c):
    return "%s-C%d-k%d-%dx%dx%d" % c


@pytest.mark.parametrize("case", MATRIX + SPANS, ids=[_case_id(c) for c in MATRIX + SPANS])
def test_head_dispatch_vs_float64(dev, case):
    dt, c, n_cls, n, h, w = case
    bf16 = dt == "bf16"
    idx = (MATRIX + SPANS).index(case)
    accumulate, gate = bool(idx & 1), bool(idx & 2)
    g = torch.Generator(device=dev).manual_seed(1000 + idx)
    x = torch.randn(n, h, w, c, generator=g, device=dev)
    x = x.to(BF) if bf16 else x
    wt = torch.randn(n_cls, c, generator=g, device=dev) * (2.0 / c) ** 0.5
    bias = torch.randn(n_cls, generator=g, device=dev) * 0.5
    d_out = torch.randn(n, n_cls, h, w, generator=g, device=dev)
    old = torch.randn(n, h, w, c, generator=g, device=dev).to(x.dtype)
    x64, wt64, b64 = x.double(), wt.double(), bias.double()
    seed = head_seed(0x5EED0000 + idx, idx % 4)
    km = torch.from_numpy(keep_mask(seed, n, h, w, c, P_DROP)).to(dev)
    mask = km.to(torch.uint8).contiguous()
    ms_drop = km.double() * keep_scale(P_DROP)
    worst = {}
    results = {}
    for d, p, mk, ms in ((0, 0.0, None, None), (1, P_DROP, None, ms_drop), (2, P_DROP, mask, ms_drop)):
        out, fname = run_fwd(x, wt, bias, p, seed, mk)
        z, mag = ref_forward(x64, wt64, b64, ms)
        r = bound_ratio(out, torch.sigmoid(z), out_bound(z, gamma(c + 2) * mag))
        worst["out"] = max(worst.get("out", 0.0), r)
        assert r <= 1.0, (case, d, fname, r)
        assert rel_err(out.cpu(), torch.sigmoid(z).cpu()) < TOL, (case, d, fname)
        dx, dw, db, bname = run_bwd(d_out, out, x, wt, p, seed, mk, old, accumulate, gate)
        want_dx, dmag, want_dw, want_db = ref_backward(d_out.double(), out.double(), x64, wt64, ms,
                                                       old.double() if accumulate else None, gate)
        if bf16:
            close_bf16(dx, want_dx, (case, d, bname, "dx"))
        else:
            r = bound_ratio(dx, want_dx, gamma(n_cls + 5) * dmag)
            worst["dx"] = max(worst.get("dx", 0.0), r)
            assert r <= 1.0, (case, d, bname, r)
            assert rel_err(dx.cpu(), want_dx.cpu()) < TOL, (case, d, bname)
        assert rel_err(dw.cpu(), want_dw.cpu()) < TOL, (case, d, bname, "dW")
        assert rel_err(db.cpu(), want_db.cpu()) < TOL, (case, d, bname, "db")
        worst["dW/1e-4"] = max(worst.get("dW/1e-4", 0.0), rel_err(dw.cpu(), want_dw.cpu()) / TOL)
        results[d] = (out, dx, dw, db, fname, bname)
    # (b) the generator (D = 1) and the mask path (D = 2) given the restated mask agree bit for bit; so does the
    # graph-captured form of the seed (by-value part + device word)
    word = 0x0123456789ABCDEF
    seed_dev = torch.tensor([word - (1 << 64) if word >= 1 << 63 else word], dtype=torch.int64, device=dev)
    out_s, fname_s = run_fwd(x, wt, bias, P_DROP, (seed - word) & MASK64, None, seed_dev=seed_dev)
    dx_s, dw_s, db_s, bname_s = run_bwd(d_out, results[1][0], x, wt, P_DROP, (seed - word) & MASK64, None, old,
                                        accumulate, gate, seed_dev=seed_dev)
    (o1, dx1, dw1, db1, f1, b1), (o2, dx2, dw2, db2, f2, b2) = results[1], results[2]
    assert fname_s == f1 and bname_s == b1, (f1, fname_s, b1, bname_s)
    for what, a, b_ in (("out", o1, o2), ("dx", dx1, dx2), ("dW", dw1, dw2), ("db", db1, db2),
                        ("out seed_dev", o1, out_s), ("dx seed_dev", dx1, dx_s), ("dW seed_dev", dw1, dw_s),
                        ("db seed_dev", db1, db_s)):
        assert torch.equal(a, b_), (case, what, f1, f2, b1, b2)
    if case in SPANS:
        _mark_spans(bf16, n * h * w, c, h * w, f1)
    report_ratio("heads %s" % _case_id(case), "worst", max(worst.values()),
                 dict(worst, fwd=[results[d][4] for d in (0, 1, 2)], bwd=[results[d][5] for d in (0, 1, 2)]))


# --------------------------------------------------------------------------------------------- (c)
EXACT_CASES = [   # (label, dtype, N, H, W, C, n_cls, heads, usable CUs or None)
    ("fp32 headline", "fp32", 32, 256, 256, 32, 4, 3, None),
    ("fp32 spans across images", "fp32", 3, 250, 190, 32, 4, 3, None),
    ("bf16 configs[3]", "bf16", 8, 512, 512, 32, 4, 3, None),
    ("bf16 configs[4]", "bf16", 4, 384, 384, 64, 5, 4, None),
    ("fp32 C=128 rounds", "fp32", 3, 300, 310, 128, 4, 1, None),
    ("bf16 C=128 rounds", "bf16", 3, 300, 310, 128, 6, 1, None),
    ("bf16 C=128 rounds on 8 CUs", "bf16", 3, 300, 310, 128, 6, 1, 8),
]
GRID = 2.0 ** 24


def _exact_operands(g, dev, dt, n, h, w, c, n_cls):
    def small_ints(shape, lo, hi, density):
        v = torch.randint(lo, hi + 1, shape, generator=g, device=dev).float()
        return v * (torch.rand(shape, generator=g, device=dev) < density)
    x = small_ints((n, h, w, c), -2, 2, 0.06)
    wt = torch.randint(-16, 17, (n_cls, c), generator=g, device=dev).float() / 8
    bias = torch.randint(-16, 17, (n_cls,), generator=g, device=dev).float() / 8
    out = (torch.randint(1, 4, (n, n_cls, h, w), generator=g, device=dev).float() / 4)    # {1/4, 1/2, 3/4}
    d_out = small_ints((n, n_cls, h, w), -2, 2, 0.3)
    old = small_ints((n, h, w, c), -3, 3, 0.2) / 8
    if dt == "bf16":
        x, old = x.to(BF), old.to(BF)
    return x, wt, bias, out, d_out, old


@pytest.mark.parametrize("case", EXACT_CASES, ids=[c[0].replace(" ", "_") for c in EXACT_CASES])
def test_head_production_geometry_exact(dev, case):
    label, dt, n, h, w, c, n_cls, heads, cus = case
    bf16 = dt == "bf16"
    g = torch.Generator(device=dev).manual_seed(77 + EXACT_CASES.index(case))
    x, wt, bias, out_syn, d_out, old = _exact_operands(g, dev, dt, n, h, w, c, n_cls)
    x64, wt64, b64 = x.double(), wt.double(), bias.double()
    base = 0x0F1E2D3C4B5A6978 + 0x1000 * EXACT_CASES.index(case)
    runs = [(0.5, head_seed(base, j)) for j in range(heads)] + [(0.0, head_seed(base, 0))]
    worst = 0.0
    with usable_cus(cus) as u:
        for p, seed in runs:
            ms = None
            if p > 0:
                km = torch.from_numpy(keep_mask(seed, n, h, w, c, p)).to(dev)
                ms = km.double() * keep_scale(p)
                del km
            # forward: the logits are exact, what is left is exp and the division
            out, fname = run_fwd(x, wt, bias, p, seed)
            z, mag = ref_forward(x64, wt64, b64, ms)
            assert float(mag.max()) < GRID / 8, float(mag.max())              # premise: grid 1/8
            r = bound_ratio(out, torch.sigmoid(z), out_bound(z, torch.zeros_like(z)))
            assert r <= 1.0, (label, p, fname, r)
            worst = max(worst, r)
            del z, mag, out
            # backward on a synthetic out: dl = d_out out (1 - out) is exact (grid 1/16)
            for accumulate, gate in ((False, False), (True, True)):
                dx, dw, db, bname = run_bwd(d_out, out_syn, x, wt, p, seed, None, old, accumulate, gate)
                want_dx, dmag, want_dw, want_db = ref_backward(d_out.double(), out_syn.double(), x64, wt64, ms,
                                                               old.double() if accumulate else None, gate)
                dl = d_out.double() * out_syn.double() * (1 - out_syn.double())
                xt_abs = x64.abs() if ms is None else (x64 * ms).abs()
                assert float(dmag.max()) < GRID / 128                             # premise: grid 1/128
                assert float(torch.einsum("nkhw,nhwc->kc", dl.abs(), xt_abs).max()) < GRID / 16
                assert float(dl.abs().sum((0, 2, 3)).max()) < GRID / 16
                assert torch.equal(dw.double(), want_dw), (label, p, bname, float((dw.double() - want_dw).abs().max()))
                assert torch.equal(db.double(), want_db), (label, p, bname, float((db.double() - want_db).abs().max()))
                if bf16:
                    want_bf = want_dx.float().to(BF)                             # exact in fp32, then RNE (pack8)
                    assert torch.equal(dx, want_bf), (label, p, bname, int((dx != want_bf).sum()))
                else:
                    assert torch.equal(dx.double(), want_dx), (label, p, bname,
                                                               float((dx.double() - want_dx).abs().max()))
                del dx, want_dx, dmag, dl, xt_abs
            if p > 0:
                _mark_spans(bf16, n * h * w, c, h * w, fname)
        report_ratio("heads exact %s" % label, "out (exp/division only)", worst,
                     {"fwd": fname, "bwd": bname, "cus": u.cus, "pixels": n * h * w})


# --------------------------------------------------------------------------------------------- (d)
def test_every_head_kernel_ran(dev):
    """Runs last in this module: every instantiation the four launchers can dispatch ran (COVERAGE), and each family ran
    at least once above its grid cap with H*W not dividing the span."""
    missing = [k for k in COVERAGE if k not in SEEN]
    assert not missing, missing
    unknown = sorted(SEEN - set(COVERAGE))
    assert not unknown, unknown
    below = [f for f in FAMILIES if f not in ABOVE_CAP]
    assert not below, below
