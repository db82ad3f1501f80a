"""Both entry points of the weight-image packer of csrc/weight_image.hip, slot by slot, against tests/weight_image_oracle.py.

(a) Per image.  Every row of CASES is one image, built twice over the C ABI by the one packer body (pack_image): singly
(pack_image_job_kernel, the job passed by value, a grid of its own size: unetpp_gemm_pack_weight_image for the packed
operand, ..._from for a parameter in its torch layout) and batched (pack_image_jobs_kernel, a job table in device memory:
unetpp_gemm_pack_weight_images), ALL jobs of a group in one launch -- the largest image sizes the shared grid, so the
small ones see more workgroups than rows.  Both destinations start as a NaN bit pattern, with 64 words of it behind the
image.  Afterwards: the size unetpp_gemm_weight_image_floats gives (gemm_image_of) equals the oracle's slot count (host
selection and kernel size and walk the image by the same image_layout of csrc/gemm_units.h; the oracle restates it: a
disagreement shows as an unwritten or overrun word); no word of the image holds the pattern, the 64 behind it still do;
the two images are equal as integers; both equal the oracle; pad slots are +0.0.  fast / bf16 images are copies (roundings to bf16
aside), so the data are arbitrary bit patterns: full-mantissa values, +-0, denormals, exact bf16 ties towards both
neighbours, values that round up into the next binade (NaN is left out: its bf16 pattern is the hardware's choice).
Winograd images run on two data sets: integers times 4 (G g G^T is then an integer: both images must EQUAL float64) and
full-mantissa floats (bit-equal to each other and to the float32 restatement ((w0 +- w1) + w2) * 0.5, rows then columns,
and within gamma(4) (|G| |g| |G^T|) of float64: each of the two stages is two roundings and an exact halving).

  group   kind, taps, flags            rows (source: input views -> output views)
  fast9   fast, 9, UNETPP_GEMM_DIRECT  packed [12]->[40]; fwd [20,4,8]->[32,12]; dgrad (flip) [16,8,8]->[4]; slice of 28
                                       channels at 4 [12]->[8]; slice of 27 at 13 [20,4,8]->[4,8]; fwd with 8 + 8 views;
                                       cap: 11 tiles x 11 chunks x 9 = 1089 rows > 256 x 4 (a row is 512 slots, a
                                       workgroup of the capped grid takes 4 or 5)
  fast1   fast, 1, 0 / DIRECT          packed, fwd, dgrad (DIRECT set: no effect at one tap), slice, deconv_fwd (n_inner)
                                       [20]->4x[12], deconv_dgrad (k_inner) 4x[12]->[40], 8 + 8 views
  wino    wino, 9, 0                   the rows of fast9, each on both data sets; cap: 17 tiles x 17 chunks = 289 rows
  bf9     bf16, 9, UNETPP_GEMM_BF16    the 3x3 path through LDS (fill_bf16_3x3_block); `blocks` states which (tile,
                                       chunk) blocks take the 16-byte reads, restated in _block_class and asserted:
                                       packed [8]->[40]            not-conv (tap stride K N)
                                       fwd [32]->[32]              wide-k (k inner-most)
                                       fwd [64]->[40]              wide-k, and wide-k-short: outer_room 8 < 32
                                       fwd [40,24]->[32,24]        wide-k(-short), narrow-inner (rooms 8 and 24)
                                       dgrad [16,8,8,32]->[32,24]  wide-n-short, wide-n (flipped), narrow-inner
                                       dgrad [8]->[8]              narrow-inner
                                       slice of 48 at 8 [40,24]->[32]  wide-n, wide-n-short: in place, strides of the whole
                                       slice of 40 at 3 [8]->[32]  misaligned (origin 108 bytes into the parameter)
                                       slice of 42 at 8 [8]->[32]  odd-stride: outer stride 378 floats.  Only the slice
                                                                   factory reaches this: fwd / dgrad have outer stride
                                                                   9 x (K or N), a multiple of 72 for bf16 widths
                                       fwd [32]->[32], storage buf[1:]  misaligned (4 bytes off a 16-byte boundary)
                                       fwd, 8 + 8 views            narrow-inner only (every input view is 8 wide)
                                       cap: 17 tiles x 17 chunks = 289 blocks > 256, mixed classes
  bf1     bf16, 1, UNETPP_GEMM_BF16    packed, fwd, dgrad, slice, deconv_fwd, deconv_dgrad, 8 + 8 views (row-wise path)

No admissible shape reaches: an outer stride that is no multiple of 4 floats from pack_conv_fwd / pack_conv_dgrad (it is
9 K or 9 N, and bf16 widths are multiples of 8) -- the row above gets it from the slice factory on a parameter with 42
input channels, which the ABI admits and the network never builds; a deconvolution source at nine taps.

(b) Through ops.PackPlan: one list of ops.gemm_fwd launches on the smallest integer rows of the exact corpora
(tests/test_gpu_gemm_fp32_exact.py, tests/gemm_oracle.py), one per kernel label that reads an image, every engine.pack_*
factory among them (the in-place slice included).  Pass one records and packs singly; every image is then overwritten
with NaN; the second begin("fwd") is ONE batched launch that must reproduce the images bit for bit, and the launches
rerun on them must give the float64 results exactly.

(c) unetpp_pack_weight against `gather` for the five factories' pack= stride sets, and the argument refusals of
unetpp_gemm_pack_weight_images and of the two single entry points.
"""
import contextlib
import ctypes as C
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import pytest
import torch

from tests import gemm_oracle as go
from tests import weight_image_oracle as wo
from tests.helpers import gamma, usable_cus

pytestmark = pytest.mark.gpu

GEMM_DIRECT, GEMM_BF16 = 1, 2
NAN_WORD = 0x7FC5A5A5     # a quiet NaN as float, and a NaN in its upper bf16 half
GUARD = 64                # words of the pattern behind every image
GROUPS = {   # group -> (oracle kind, taps, flags)
    "fast9": (wo.FAST, 9, GEMM_DIRECT), "fast1": (wo.FAST, 1, 0), "wino": (wo.WINO, 9, 0),
    "bf9": (wo.BF16, 9, GEMM_BF16), "bf1": (wo.BF16, 1, GEMM_BF16),
}


@dataclass(frozen=True)
class Case:
    id: str
    group: str
    source: str                       # packed / fwd / dgrad / slice / deconv_fwd / deconv_dgrad
    in_len: Tuple[int, ...]
    out_len: Tuple[int, ...]
    slice_of: Tuple[int, int] = (0, 0)   # slice: (input channels of the whole weight, c_off)
    data: str = "bits"                # bits / int4 / full
    offset: int = 0                   # floats between a 16-byte boundary and the parameter's storage
    flags: Optional[int] = None       # overrides the group's
    blocks: Tuple[str, ...] = ()      # bf9: the block classes the row must consist of (exactly)

    @property
    def kind(self):
        return GROUPS[self.group][0]

    @property
    def taps(self):
        return GROUPS[self.group][1]

    @property
    def desc_flags(self):
        return GROUPS[self.group][2] if self.flags is None else self.flags


def _c(id, group, source, ins, outs, **kw):
    return Case(id, group, source, tuple(ins), tuple(outs), **kw)


V8F, V8F_OUT = [4] * 8, [36, 4, 4, 4, 4, 4, 4, 8]
V8B, V8B_OUT = [8] * 8, [40, 8, 8, 8, 8, 8, 8, 8]


def _fp32_rows(group, tag, cap_in, cap_out, **kw):
    return [
        _c(tag + "-packed", group, "packed", [12], [40], **kw),
        _c(tag + "-fwd", group, "fwd", [20, 4, 8], [32, 12], **kw),
        _c(tag + "-dgrad", group, "dgrad", [16, 8, 8], [4], **kw),
        _c(tag + "-slice-28at4", group, "slice", [12], [8], slice_of=(28, 4), **kw),
        _c(tag + "-slice-27at13", group, "slice", [20, 4, 8], [4, 8], slice_of=(27, 13), **kw),
        _c(tag + "-views8", group, "fwd", V8F, V8F_OUT, **kw),
        _c(tag + "-cap", group, "fwd", cap_in, cap_out, **kw),
    ]


CASES = (
    _fp32_rows("fast9", "f9", [4] * 7 + [64], [4] * 7 + [128])
    + [
        _c("f1-packed", "fast1", "packed", [12], [40]),
        _c("f1-fwd", "fast1", "fwd", [20, 4, 8], [32, 12]),
        _c("f1-dgrad-direct", "fast1", "dgrad", [16, 8, 8], [4], flags=GEMM_DIRECT),
        _c("f1-slice-27at13", "fast1", "slice", [12], [4, 8], slice_of=(27, 13)),
        _c("f1-deconv-fwd", "fast1", "deconv_fwd", [20], [12] * 4),
        _c("f1-deconv-dgrad", "fast1", "deconv_dgrad", [12] * 4, [40]),
        _c("f1-views8", "fast1", "fwd", V8F, V8F_OUT),
    ]
    + _fp32_rows("wino", "w-int4", [4] * 7 + [80], [4] * 7 + [320], data="int4")
    + _fp32_rows("wino", "w-full", [4] * 7 + [80], [4] * 7 + [320], data="full")
    + [
        _c("b9-packed", "bf9", "packed", [8], [40], blocks=("not-conv",)),
        _c("b9-fwd-wide", "bf9", "fwd", [32], [32], blocks=("wide-k",)),
        _c("b9-fwd-short-outer", "bf9", "fwd", [64], [40], blocks=("wide-k", "wide-k-short")),
        _c("b9-fwd-ragged", "bf9", "fwd", [40, 24], [32, 24], blocks=("wide-k", "wide-k-short", "narrow-inner")),
        _c("b9-dgrad-wide", "bf9", "dgrad", [16, 8, 8, 32], [32, 24], blocks=("wide-n", "wide-n-short", "narrow-inner")),
        _c("b9-dgrad-narrow", "bf9", "dgrad", [8], [8], blocks=("narrow-inner",)),
        _c("b9-slice-48at8", "bf9", "slice", [40, 24], [32], slice_of=(48, 8), blocks=("wide-n", "wide-n-short")),
        _c("b9-slice-40at3", "bf9", "slice", [8], [32], slice_of=(40, 3), blocks=("misaligned",)),
        _c("b9-slice-42at8", "bf9", "slice", [8], [32], slice_of=(42, 8), blocks=("odd-stride",)),
        _c("b9-fwd-offset4", "bf9", "fwd", [32], [32], offset=1, blocks=("misaligned",)),
        _c("b9-views8", "bf9", "fwd", V8B, V8B_OUT, blocks=("narrow-inner",)),
        _c("b9-cap", "bf9", "fwd", [8] * 7 + [320], [8] * 7 + [320], blocks=("wide-k", "wide-k-short", "narrow-inner")),
        _c("b1-packed", "bf1", "packed", [8], [40]),
        _c("b1-fwd", "bf1", "fwd", [40, 24], [32, 24]),
        _c("b1-dgrad", "bf1", "dgrad", [16, 8, 8, 32], [8]),
        _c("b1-slice-50at8", "bf1", "slice", [40, 24], [32, 8], slice_of=(50, 8)),
        _c("b1-deconv-fwd", "bf1", "deconv_fwd", [40], [24] * 4),
        _c("b1-deconv-dgrad", "bf1", "deconv_dgrad", [8] * 4, [40]),
        _c("b1-views8", "bf1", "fwd", V8B, V8B_OUT),
    ]
)
# what the rows claim about the capped grid (unetpp_gemm_pack_weight_images: at most 256 workgroups per job)
CAP_ROWS = {"f9-cap": 1089, "w-int4-cap": 289, "w-full-cap": 289, "b9-cap": 289}


# ------------------------------------------------------------------------------------------------ data and sources
SPECIALS = np.array([
    0x00000000, 0x80000000,              # +-0
    0x00000001, 0x807FFFFF, 0x00400000,  # denormals
    0x3F808000, 0xBF808000,              # ties whose even neighbour is below (1 + 2^-8 -> 1)
    0x3F818000, 0xC0018000,              # ties whose even neighbour is above
    0x3F807FFF, 0x3F808001,              # one ulp on either side of a tie
    0x3FFFFFFF, 0x407F8000, 0xC0FFC000,  # round up into the next binade (the second is a tie)
    0x7F7F0000, 0x00800000,              # the largest bf16 number, the smallest normal fp32 number
], dtype=np.uint32)


def _param_shape(c: Case):
    k, n, kk = sum(c.in_len), sum(c.out_len), (3 if c.taps == 9 else 1)
    if c.source == "packed":
        return (c.taps, k, n)
    if c.source == "fwd":
        return (n, k, kk, kk)
    if c.source == "dgrad":
        return (k, n, kk, kk)
    if c.source == "slice":
        assert c.slice_of[1] + n <= c.slice_of[0]
        return (k, c.slice_of[0], kk, kk)
    if c.source == "deconv_fwd":
        assert len(c.out_len) == 4 and len(set(c.out_len)) == 1 and len(c.in_len) == 1
        return (k, c.out_len[0], 2, 2)
    assert c.source == "deconv_dgrad" and len(c.in_len) == 4 and len(set(c.in_len)) == 1 and len(c.out_len) == 1
    return (n, c.in_len[0], 2, 2)


def _param_values(c: Case) -> np.ndarray:
    """the parameter as float32 (flat)"""
    count = int(np.prod(_param_shape(c)))
    rng = np.random.default_rng(sum(map(ord, c.id)) * 7919 + count)
    if c.data == "int4":
        return (4 * rng.integers(-8, 9, size=count)).astype(np.float32)
    b = rng.integers(0, 2 ** 32, size=count, dtype=np.uint64).astype(np.uint32)
    b = np.where(((b >> 23) & 0xFF) == 0xFF, b ^ np.uint32(0x40000000), b)       # no NaN, no infinity
    if c.data == "full":   # +-[1, 2) 2^e, e in -3 .. 3, all 23 mantissa bits in use
        e = rng.integers(124, 131, size=count).astype(np.uint32)
        return ((b & np.uint32(0x807FFFFF)) | (e << 23)).view(np.float32)
    at = np.arange(0, count, 5)
    b[at] = SPECIALS[(at // 5) % SPECIALS.size]
    return b.view(np.float32)


def _wsrc(c: Case, param):
    """the row's weight source over `param` (a torch tensor of _param_shape, or anything with its data for the host)"""
    from unet_nested4tiny_objects_keypoints_amd import engine, ops
    k, n = sum(c.in_len), sum(c.out_len)
    if c.source == "packed":
        return ops.WSrc(param, c.taps, k, n, s_t=k * n, s_k=n, s_n=1)
    if c.source == "slice":
        return engine.pack_conv_dgrad_slice(param, c.slice_of[1], n)
    return {"fwd": engine.pack_conv_fwd, "dgrad": engine.pack_conv_dgrad, "deconv_fwd": engine.pack_deconv_fwd,
            "deconv_dgrad": engine.pack_deconv_dgrad}[c.source](param)


def _block_class(ws, addr, k0, k_room, n0, n_room):
    """fill_bf16_3x3_block's choice for one (tile, chunk) block, and why: wide-k / wide-n (16-byte reads; k or n
    inner-most; -short: fewer than 32 outer indices) or the reason for the 4-byte reads"""
    k_inner_most = ws.s_k < ws.s_n
    inner_stride, outer_stride = (ws.s_k, ws.s_n) if k_inner_most else (ws.s_n, ws.s_k)
    inner_room, outer_room = (k_room, n_room) if k_inner_most else (n_room, k_room)
    origin = k0 * ws.s_k + n0 * ws.s_n
    if ws.s_t != 1 or inner_stride != 9 or ws.k_inner > 0 or ws.n_inner > 0:
        return "not-conv"
    if inner_room < 32:
        return "narrow-inner"
    if (outer_stride * 4) & 15:
        return "odd-stride"
    if (addr + 4 * origin) & 15:
        return "misaligned"
    return ("wide-k" if k_inner_most else "wide-n") + ("-short" if outer_room < 32 else "")


def block_classes(c: Case, ws, addr):
    k0, k_room = wo.pieces(c.in_len, 32)
    n0, n_room = wo.pieces(c.out_len, 32)
    return [_block_class(ws, addr, int(k0[ch]), int(k_room[ch]), int(n0[t]), int(n_room[t]))
            for t in range(len(n0)) for ch in range(len(k0))]


# ------------------------------------------------------------------------------------------------ the device side
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@dataclass
class Built:
    n_img: int
    single: np.ndarray     # uint32, image + GUARD words
    batched: np.ndarray
    want: wo.Image
    classes: list          # bf9: class of every block
    param_addr: int


_BUILT = {}


def _pattern(n, dev):
    return torch.full((n,), NAN_WORD, dtype=torch.int32, device=dev)


def _build_group(group, dev):
    """every image of the group: singly, and all of them in ONE batched launch"""
    from unet_nested4tiny_objects_keypoints_amd import _lib
    lib = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    cases = [c for c in CASES if c.group == group]
    act = torch.zeros(8 * 8 * 512, dtype=torch.float32, device=dev)   # what every view points at (never read)
    keep, jobs, out = [], [], {}
    for c in cases:
        values = _param_values(c)
        store = torch.zeros(values.size + 8, dtype=torch.float32, device=dev)
        assert store.data_ptr() % 16 == 0
        flat = store[c.offset:c.offset + values.size]
        flat.copy_(torch.from_numpy(values.copy()))
        assert np.array_equal(flat.cpu().numpy().view(np.uint32), values.view(np.uint32)), "the copy changed bits"
        param = flat.view(_param_shape(c))
        assert param.data_ptr() % 16 == 4 * c.offset
        ws = _wsrc(c, param)
        d = _lib.GemmDesc()
        d.N, d.H, d.W, d.taps, d.flags = 1, 8, 8, c.taps, c.desc_flags
        d.n_in, d.n_out = len(c.in_len), len(c.out_len)
        for views, lens in ((d.inp, c.in_len), (d.out, c.out_len)):
            for v, n in zip(views, lens):
                v.ptr, v.C, v.c_off, v.c_len, v.Hs, v.Ws, v.sy, v.sx = act.data_ptr(), n, 0, n, 8, 8, 1, 1
        n_img = int(lib.unetpp_gemm_weight_image_floats(C.byref(d)))
        assert n_img == wo.slot_count(c.kind, c.taps, c.in_len, c.out_len), c.id
        single, batched = _pattern(n_img + GUARD, dev), _pattern(n_img + GUARD, dev)
        src = _lib.WeightSrc()
        ws.fill(src)
        if c.source == "packed":
            d.weight = param.data_ptr()
            _lib.check(lib.unetpp_gemm_pack_weight_image(C.byref(d), C.c_void_p(single.data_ptr()), stream), c.id)
        else:
            _lib.check(lib.unetpp_gemm_pack_weight_image_from(C.byref(d), C.byref(src), C.c_void_p(single.data_ptr()), stream), c.id)
        job = _lib.PackJob()
        ws.fill(job.src)
        job.image = batched.data_ptr()
        job.taps, job.flags, job.n_in, job.n_out = c.taps, c.desc_flags, len(c.in_len), len(c.out_len)
        for i, n in enumerate(c.in_len):
            job.in_len[i] = n
        for i, n in enumerate(c.out_len):
            job.out_len[i] = n
        jobs.append(job)
        keep.append((c, store, ws, single, batched, n_img, values))
    table = torch.frombuffer(bytearray(bytes((_lib.PackJob * len(jobs))(*jobs))), dtype=torch.uint8).to(dev)
    largest = max(k[5] for k in keep)
    assert sum(1 for k in keep if k[5] == largest) < len(keep), "the jobs of a launch must differ in size"
    _lib.check(lib.unetpp_gemm_pack_weight_images(C.c_void_p(table.data_ptr()), len(jobs), largest, stream), group)
    torch.cuda.synchronize()
    for c, store, ws, single, batched, n_img, values in keep:
        w = wo.gather(values, ws, c.taps, sum(c.in_len), sum(c.out_len)) if c.source != "slice" else \
            wo.gather(values[c.slice_of[1] * c.taps:], ws, c.taps, sum(c.in_len), sum(c.out_len))
        classes = block_classes(c, ws, ws.t.data_ptr()) if group == "bf9" else []
        out[c.id] = Built(n_img, single.cpu().numpy().view(np.uint32), batched.cpu().numpy().view(np.uint32),
                          wo.image(c.kind, c.taps, c.in_len, c.out_len, w), classes, ws.t.data_ptr())
    return out


def _built(c: Case, dev) -> Built:
    if c.group not in _BUILT:
        _BUILT.clear()      # (one group's images at a time)
        _BUILT[c.group] = _build_group(c.group, dev)
    return _BUILT[c.group][c.id]


def _first_diff(got, want):
    bad = np.flatnonzero(got != want)
    i = int(bad[0])
    return "%d of %d words differ, first at %d (row %d, slot %d): got %08x want %08x" % (
        bad.size, want.size, i, i // 512, i % 512, int(got[i]), int(want[i]))


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_both_packers_build_the_stated_image(dev, case):
    c = case
    b = _built(c, dev)
    want = b.want
    assert want.words.size == b.n_img
    for name, got in (("single", b.single), ("batched", b.batched)):
        what = "%s %s packer" % (c.id, name)
        img, tail = got[:b.n_img], got[b.n_img:]
        assert bool((tail == NAN_WORD).all()), what + ": wrote behind the image"
        assert not bool((img == NAN_WORD).any()), "%s: %d slots left unwritten, first %d" % (
            what, int((img == NAN_WORD).sum()), int(np.flatnonzero(img == NAN_WORD)[0]))
        assert not bool(img[want.pad].any()), what + ": a pad slot is not +0.0"
    assert np.array_equal(b.single, b.batched), c.id + " single vs batched: " + _first_diff(b.batched, b.single)
    for name, got in (("single", b.single[:b.n_img]), ("batched", b.batched[:b.n_img])):
        assert np.array_equal(got, want.words), "%s %s vs oracle: %s" % (c.id, name, _first_diff(got, want.words))
    if c.kind == wo.WINO:
        got64 = b.batched[:b.n_img].view(np.float32).astype(np.float64)
        if c.data == "int4":
            assert np.array_equal(got64, want.f64), c.id + ": G g G^T of multiples of 4 must be exact"
        else:
            err, bound = np.abs(got64 - want.f64), gamma(4) * want.mag
            assert bool((err <= bound).all()), "%s: error %g above the bound %g" % (
                c.id, float(err[err > bound][0]), float(bound[err > bound][0]))
            assert float(err.max()) > 0.0, c.id + ": the data was meant to round"
    # what the row claims about itself
    ragged = any(n % wo.KC[c.kind] for n in c.in_len) or any(n % 32 for n in c.out_len)
    assert 0 < int((~want.pad).sum()) and bool(want.pad.any()) == ragged, c.id
    if c.group == "bf9":
        assert set(b.classes) == set(c.blocks), (c.id, sorted(set(b.classes)))
        assert b.param_addr % 16 == (4 * c.offset if c.source != "slice" else (36 * c.slice_of[1] + 4 * c.offset) % 16)
    if c.id in CAP_ROWS:
        rows = b.n_img // (4096 if c.kind == wo.WINO else 512)
        blocks = rows // 9 if c.group == "bf9" else rows
        assert rows == CAP_ROWS[c.id] * (9 if c.group == "bf9" else 1)
        grid = min(256, -(-b.n_img // 2048))
        assert grid == 256 and blocks > grid and blocks % grid != 0, (c.id, blocks, grid)


def test_case_table_covers_what_it_claims():
    """(no device needed, but it belongs to the table above)"""
    for group in GROUPS:
        sources = {c.source for c in CASES if c.group == group}
        want = {"packed", "fwd", "dgrad", "slice"} | ({"deconv_fwd", "deconv_dgrad"} if GROUPS[group][1] == 1 else set())
        assert sources == want, (group, sources)
        assert any(len(c.in_len) == 8 and len(c.out_len) == 8 for c in CASES if c.group == group), group
        offs = {c.slice_of[1] for c in CASES if c.group == group and c.source == "slice"}
        assert len(offs) >= (1 if GROUPS[group][1] == 1 else 2), group
    assert {c.group for c in CASES if c.id in CAP_ROWS} == {"fast9", "wino", "bf9"}
    claimed = {b for c in CASES for b in c.blocks}
    assert claimed == {"wide-k", "wide-n", "wide-k-short", "wide-n-short", "narrow-inner", "misaligned", "odd-stride", "not-conv"}
    assert len({c.id for c in CASES}) == len(CASES)


# ------------------------------------------------------------------------------------------------ (b) through PackPlan
BF = torch.bfloat16
# (row id, storage, variant, factory): variant = the switches / flags of the row's own corpus
PLAN_LAUNCHES = [
    ("f9-32-48-relu-bias", "f32", "fast", "fwd"),
    ("f9-dgrad-kinds", "f32", "wino", "dgrad"),
    ("f9-dgrad-kinds", "f32", "wino", "slice"),
    ("f9-32-48-relu-bias", "f32", "wino", "fwd"),
    ("f1-deconv-fwd-w20", "f32", "fast", "deconv_fwd"),
    ("f1-deconv-dgrad-w20", "f32", "fast", "deconv_dgrad"),
    ("f1-pw-64-64-w48", "f32", "pw", "fwd"),
    ("k9-32-32-ties-tw8", "bf16", "reg", "fwd"),
    ("k9-dgrad-kinds-tw8", "bf16", "dma4", "dgrad"),
    ("k9-dgrad-kinds-tw8", "bf16", "reg", "slice"),
    ("k1-deconv-fwd-sliced-tw8", "bf16", "reg", "deconv_fwd"),
    ("k1-deconv-dgrad-one-tile-tw16", "bf16", "dma4", "deconv_dgrad"),
    ("pw-plain-q1-c1-w16", "bf16", "pw", "fwd"),
]
IMAGE_LABELS = ("gemm_fast_kernel<9>", "gemm_fast_kernel<1>", "gemm_wino_kernel", "gemm_pw_kernel", go.REG9, go.REG1, go.DMA9,
                go.DMA1, go.PWB)


class _PlanLaunch:
    """device operands of one launch of the list (the rows take no statistics)"""

    def __init__(self, spec, dev):
        from tests import test_gpu_gemm_bf16_exact as bx
        from tests import test_gpu_gemm_fp32_exact as fx
        from unet_nested4tiny_objects_keypoints_amd import engine
        from unet_nested4tiny_objects_keypoints_amd.ops import V
        rid, storage, variant, factory = spec
        self.spec, self.dev = spec, dev
        self.bf16 = storage == "bf16"
        rows = go.ROWS if self.bf16 else fx.FP32_ROWS
        r = self.r = next(x for x in rows if x.id == rid)
        assert not r.stats and not r.fold and variant in r.variants, spec
        assert factory == r.form or (factory == "slice" and r.form == "dgrad"), spec
        self.act = BF if self.bf16 else torch.float32
        if self.bf16:
            self.switches = dict(bx.SWITCHES[variant], **({"PW_DIRECT": 0} if r.family == "k1" else {}))
            self.direct = False
            with usable_cus(None) as u:
                self.label = go.launch_plan(r, variant, u.cus)["label"]
            self.roundings = go.ROUNDINGS[self.label]
        else:
            self.label, self.switches, self.direct = fx.label_of(r, variant), fx.VARIANTS[variant][2], fx.VARIANTS[variant][3]
            self.roundings = 1
        ops = self.ops = go.operands(r)
        self.want = go.reference(r, ops, self.roundings, self.bf16)
        cache = {}

        def put(t, dt):
            if t is None:
                return None
            if (id(t), dt) not in cache:
                cache[(id(t), dt)] = t.to(dt).to(dev).contiguous()
            return cache[(id(t), dt)]
        self.in_views = [V(put(v.t, self.act), v.c_off, v.c_len, v.sy, v.sx, v.oy, v.ox, scale=put(v.scale, torch.float32),
                           shift=put(v.shift, torch.float32), relu=v.relu) for v in ops.ins]
        self.gates = [put(v.gate, self.act) for _, v, _ in ops.outs]
        param = ops.weight.float().to(dev)
        if factory == "slice":   # the row's weight as input channels [8, 8 + Ncols) of a wider parameter, read in place
            co, n = param.shape[0], param.shape[1]
            g = torch.Generator().manual_seed(co * 1000 + n)
            wide = torch.randint(-2, 3, (co, n + 16, 3, 3), generator=g).float().to(dev)
            wide[:, 8:8 + n] = param
            self.param, self.weight = wide, engine.pack_conv_dgrad_slice(wide, 8, n)
        else:
            pack = {"fwd": engine.pack_conv_fwd, "dgrad": engine.pack_conv_dgrad, "deconv_fwd": engine.pack_deconv_fwd,
                    "deconv_dgrad": engine.pack_deconv_dgrad}[factory]
            self.param, self.weight = param, pack(param)
        self.bias = None
        if ops.bias is not None:
            b = ops.bias_param.float().to(dev)
            self.bias = engine.tile_bias4(b) if r.form == "deconv_fwd" else b

    def run(self):
        """-> (output buffers between their sentinels, the library's plan of the launch, the label that ran)"""
        from tests.test_gpu_gemm_bf16_exact import PAD, _guarded_host
        from unet_nested4tiny_objects_keypoints_amd import _lib
        from unet_nested4tiny_objects_keypoints_amd import ops as lib_ops
        from unet_nested4tiny_objects_keypoints_amd.ops import V
        r, ops = self.r, self.ops
        n, h, w = r.shape
        bufs = [_guarded_host(t, self.act).to(self.dev) for t in ops.out_tensors]
        tensors = [b[PAD:PAD + t.numel()].view(t.shape) for b, t in zip(bufs, ops.out_tensors)]
        outs = [V(tensors[idx], v.c_off, v.c_len, v.sy, v.sx, v.oy, v.ox, gate=self.gates[i], relu=r.relu,
                  accumulate=kind in ("acc", "accgate"), gate_sum=kind == "accgate")
                for i, (idx, v, kind) in enumerate(ops.outs)]
        with contextlib.ExitStack() as stack:
            for name, value in self.switches.items():
                stack.enter_context(_lib.debug_switch(name, value))
            plan = lib_ops.gemm_fwd(n, h, w, r.taps, self.in_views, outs, self.weight, self.bias, None, direct=self.direct)
            ran = _lib.lib().unetpp_last_kernel_name().decode()
        return bufs, plan, ran

    def check(self, bufs, what):
        from tests.test_gpu_gemm_bf16_exact import _bits, _guarded_host, _mismatch
        for i, (buf, exp) in enumerate(zip(bufs, self.want.out_tensors)):
            got, exp_buf = buf.cpu(), _guarded_host(exp, self.act)
            assert torch.equal(_bits(got), _bits(exp_buf)), "%s output %d: %s" % (what, i, _mismatch(got, exp_buf))


def test_pack_plan_rebuilds_every_image_in_one_launch(dev):
    from unet_nested4tiny_objects_keypoints_amd import ops as lib_ops
    launches = [_PlanLaunch(spec, dev) for spec in PLAN_LAUNCHES]     # (operands first: no plan is set yet)
    assert {x.label for x in launches} == set(IMAGE_LABELS)
    assert {x.spec[3] for x in launches} == {"fwd", "dgrad", "slice", "deconv_fwd", "deconv_dgrad"}
    plan = lib_ops.PackPlan()
    lib_ops.set_pack_plan(plan)
    try:
        plan.begin("fwd")
        assert plan.launches == 0 and not plan.entries
        for x in launches:                                            # pass one: records, packs singly
            bufs, sizes, ran = x.run()
            torch.cuda.synchronize()
            assert ran == x.label and sizes.image_floats > 0 and sizes.kernel.decode() == ran, (x.spec, ran)
            x.check(bufs, "%s pass one %s" % (x.spec, ran))
        assert plan.launches == 0 and len(plan.entries) == len(launches)
        entries = list(plan.entries.values())
        assert all(e.phase == "fwd" and e.image.numel() == e.n_img for e in entries)
        first = [e.image.view(torch.int32).clone() for e in entries]
        for e in entries:
            e.image.view(torch.int32).fill_(NAN_WORD)
        plan.begin("fwd")                                             # pass two: ONE batched launch
        assert plan.launches == 1
        torch.cuda.synchronize()
        for e, img in zip(entries, first):
            got = e.image.view(torch.int32)
            assert not bool((got == NAN_WORD).any()), "the batched launch left slots unwritten"
            assert torch.equal(got, img), "batched image differs from the single one in %d of %d slots" % (
                int((got != img).sum()), img.numel())
        for x in launches:
            bufs, sizes, ran = x.run()
            torch.cuda.synchronize()
            assert ran == x.label, (x.spec, ran)
            x.check(bufs, "%s pass two %s" % (x.spec, ran))
        assert plan.launches == 1 and len(plan.entries) == len(launches)
        for e, img in zip(entries, first):                            # (pass two packed nothing by itself, and nothing else wrote)
            assert torch.equal(e.image.view(torch.int32), img)
    finally:
        lib_ops.set_pack_plan(None)


# ------------------------------------------------------------------------------------------------ (c) small neighbours
def test_pack_weight_equals_gather_for_every_factory(dev):
    """unetpp_pack_weight (pack_weight_kernel) with the stride sets of the five factories' pack= closures: the packed
    [taps][K][N] operand, every bit, on odd sizes around 256 elements"""
    from unet_nested4tiny_objects_keypoints_amd import engine
    rng = np.random.default_rng(3)

    def param(*shape):
        b = rng.integers(0, 2 ** 32, size=int(np.prod(shape)), dtype=np.uint64).astype(np.uint32)
        b = np.where(((b >> 23) & 0xFF) == 0xFF, b ^ np.uint32(0x40000000), b)
        return torch.from_numpy(b.view(np.float32).copy()).view(shape).to(dev)
    conv, conv1, deconv = param(5, 7, 3, 3), param(15, 17, 1, 1), param(9, 7, 2, 2)     # 315, 255, 252 elements
    rows = [("fwd", engine.pack_conv_fwd(conv)), ("dgrad", engine.pack_conv_dgrad(conv)),
            ("slice", engine.pack_conv_dgrad_slice(conv, 2, 3)), ("slice-0", engine.pack_conv_dgrad_slice(conv, 0, 7)),
            ("fwd-1x1", engine.pack_conv_fwd(conv1)), ("dgrad-1x1", engine.pack_conv_dgrad(conv1)),
            ("slice-1x1", engine.pack_conv_dgrad_slice(conv1, 6, 11)),
            ("deconv_fwd", engine.pack_deconv_fwd(deconv)), ("deconv_dgrad", engine.pack_deconv_dgrad(deconv))]
    for name, ws in rows:
        got = ws.packed()
        torch.cuda.synchronize()
        assert got.numel() == ws.taps * ws.k * ws.n, name
        want = wo.gather(ws.t.cpu().numpy(), ws, ws.taps, ws.k, ws.n)
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.reshape(-1).view(np.uint32)), name


def test_batched_packer_refuses_bad_arguments(dev):
    from unet_nested4tiny_objects_keypoints_amd import _lib
    lib = _lib.lib()
    table = torch.zeros(C.sizeof(_lib.PackJob), dtype=torch.uint8, device=dev)
    ptr = C.c_void_p(table.data_ptr())
    assert lib.unetpp_gemm_pack_weight_images(None, 1, 512, None) == -1
    assert lib.unetpp_gemm_pack_weight_images(ptr, 0, 512, None) == -1
    assert lib.unetpp_gemm_pack_weight_images(ptr, 65536, 512, None) == -1
    assert lib.unetpp_gemm_pack_weight_images(ptr, 1, 0, None) == -1
    torch.cuda.synchronize()


def test_single_entry_points_refuse_bad_arguments(dev):
    """(a refusal launches nothing: the destination keeps its pattern)"""
    from unet_nested4tiny_objects_keypoints_amd import _lib
    lib = _lib.lib()
    act = torch.zeros(8 * 8 * 16, dtype=torch.float32, device=dev)
    param = torch.ones(9 * 8 * 8, dtype=torch.float32, device=dev)
    image = _pattern(512, dev)
    img = C.c_void_p(image.data_ptr())

    def desc(c_in):
        d = _lib.GemmDesc()
        d.N, d.H, d.W, d.taps, d.flags, d.n_in, d.n_out = 1, 8, 8, 9, GEMM_DIRECT, 1, 1
        for v, n in ((d.inp[0], c_in), (d.out[0], 8)):
            v.ptr, v.C, v.c_off, v.c_len, v.Hs, v.Ws, v.sy, v.sx = act.data_ptr(), n, 0, n, 8, 8, 1, 1
        return d
    good, odd = desc(8), desc(6)      # 6 channels: no multiple of 4, so no image kernel takes the view
    assert lib.unetpp_gemm_weight_image_floats(C.byref(good)) == 9 * 512 and lib.unetpp_gemm_weight_image_floats(C.byref(odd)) == 0
    src, no_src = _lib.WeightSrc(), _lib.WeightSrc()
    src.src, src.s_t, src.s_k, src.s_n = param.data_ptr(), 64, 8, 1
    no_src.s_t, no_src.s_k, no_src.s_n = 64, 8, 1
    assert no_src.src is None
    assert lib.unetpp_gemm_pack_weight_image_from(C.byref(good), None, img, None) == -1
    assert lib.unetpp_gemm_pack_weight_image_from(C.byref(good), C.byref(no_src), img, None) == -1
    assert lib.unetpp_gemm_pack_weight_image_from(C.byref(good), C.byref(src), None, None) == -1
    assert lib.unetpp_gemm_pack_weight_image_from(C.byref(odd), C.byref(src), img, None) == -1
    assert good.weight is None
    assert lib.unetpp_gemm_pack_weight_image(C.byref(good), img, None) == -1
    torch.cuda.synchronize()
    assert bool((image == NAN_WORD).all()), "a refused call wrote to the destination"
