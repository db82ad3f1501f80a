"""Backward of the ensemble mean (unetpp_heads_mean_bwd / unetpp_heads_mean_bwd_bf16, ops.heads_mean_bwd) against float64.

The kernel recomputes every head's probabilities s_h = sigmoid(bias_h + x_h . w_h) from the features (the mean's forward
never wrote them), forms dl = (d_out * (1 / n)) * (s (1 - s)) and from it dx_h = W_h^T dl (+ old dx, ReLU gate of x_h),
dW_h and db_h.  A-priori element-wise bounds (tests/helpers.py gamma, bound_ratio), derived and not fitted:

    s       B_s = s(1-s) (gamma_(C+2) (sum |x w| + |b|) + EXP_ARG_ULPS u (|z| + 1)) 1.01 + SIGMOID_ULPS u s
            (tests/test_gpu_heads.py out_bound, restated with that file's two recorded estimates)
    dl      B_dl = |d_out| / n (|1 - 2 s| B_s + B_s^2) + 3 u |dl|
            (s' (1 - s') - s (1 - s) = e (1 - 2 s) - e^2 for s' = s + e; three roundings: d_out / n, s (1 - s), the product)
    dx      sum_k |W_kc| B_dl_k + gamma_(n_cls+5) (sum_k |dl_k W_kc| + |old|)
    bf16 dx close_bf16 (one rounding of the stored result); dW and db the suite's 1e-4 bar.

Shapes: the smallest that reach every form -- fp32 in 16-byte pieces (C = 4, 8, 12, 32, 64), fp32 scalar (C = 6, and C = 4
behind a pointer that is not 16-byte aligned), bf16 octets (C = 8, 64); 1, 4, 5 and 8 classes; 1 to 4 heads; 65 pixels
(a tile tail), 2 x 24 x 40, and 520 x 520 (4225 tiles of 64 pixels: more than the 4096-workgroup grid cap); accumulate and
gate_x on and off per head, mixed within one call.  Two calls on the same operands give the same bits."""
import pytest
import torch

from tests.helpers import U32, bound_ratio, close_bf16, gamma, rel_err, report_ratio

pytestmark = pytest.mark.gpu

TOL = 1e-4
BF = torch.bfloat16
EXP_ARG_ULPS = 4.0   # tests/test_gpu_heads.py: recorded estimate of exp's relative error, <= EXP_ARG_ULPS u (|z| + 1)
SIGMOID_ULPS = 4.0   # tests/test_gpu_heads.py: recorded estimate of the add, the division and the store of 1 / (1 + e)

COVERAGE = ("heads_mean_bwd", "heads_mean_bwd_vec", "heads_mean_bwd_bf16")
SEEN = set()
ABOVE_CAP = set()    # forms that ran with more 64-pixel tiles than workgroups
GRID_CAP = 4096


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def last_kernel():
    from unet_nested4tiny_objects_keypoints_amd import _lib
    return _lib.lib().unetpp_last_kernel_name().decode()


def out_bound(z, zb):
    s = torch.sigmoid(z)
    return s * (1 - s) * (zb + EXP_ARG_ULPS * U32 * (z.abs() + 1)) * 1.01 + SIGMOID_ULPS * U32 * s + 1e-300


def _misaligned(t):
    """the same values behind a pointer 4 bytes (fp32) off a 16-byte boundary: contiguous, but no 16-byte pieces"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    return view


def _operands(dev, dt, c, n_cls, n, h, w, heads, seed, misalign=False):
    g = torch.Generator(device=dev).manual_seed(seed)
    xs, wts, bs, olds = [], [], [], []
    for _ in range(heads):
        x = torch.randn(n, h, w, c, generator=g, device=dev)
        old = torch.randn(n, h, w, c, generator=g, device=dev)
        if dt == "bf16":
            x, old = x.to(BF), old.to(BF)
        if misalign:
            x = _misaligned(x)
        xs.append(x)
        olds.append(old)
        wts.append(torch.randn(n_cls, c, generator=g, device=dev) * (2.0 / c) ** 0.5)
        bs.append(torch.randn(n_cls, generator=g, device=dev) * 0.5)
    d_out = torch.randn(n, n_cls, h, w, generator=g, device=dev)
    return xs, wts, bs, olds, d_out


def _run(xs, wts, bs, olds, d_out, accs, gates):
    from unet_nested4tiny_objects_keypoints_amd import ops
    dxs = [old.clone() if a else torch.full_like(x, float("nan")) for x, old, a in zip(xs, olds, accs)]
    got = ops.heads_mean_bwd(xs, wts, bs, d_out, dxs, accs, gates)
    name = last_kernel()
    torch.cuda.synchronize()
    return dxs, [(dw.view(wt.shape).clone(), db.clone()) for (dw, db), wt in zip(got, wts)], name


def _check(dev, dt, c, n_cls, n, h, w, heads, seed, misalign=False):
    """One call against float64 -> (kernel name, worst dx err / bound, worst dW / db rel_err)."""
    xs, wts, bs, olds, d_out = _operands(dev, dt, c, n_cls, n, h, w, heads, seed, misalign)
    accs = [bool((hh + seed) & 1) for hh in range(heads)]
    gates = [bool(((hh + seed) >> 1) & 1) for hh in range(heads)]
    dxs, grads, name = _run(xs, wts, bs, olds, d_out, accs, gates)
    SEEN.add(name)
    if -(-n * h * w // 64) > GRID_CAP:
        ABOVE_CAP.add(name)
    worst_dx, worst_w = 0.0, 0.0
    d64 = d_out.double()
    for hh in range(heads):
        x64, w64, b64 = xs[hh].double(), wts[hh].double(), bs[hh].double()
        z = torch.einsum("nhwc,kc->nkhw", x64, w64) + b64.view(1, -1, 1, 1)
        mag = torch.einsum("nhwc,kc->nkhw", x64.abs(), w64.abs()) + b64.abs().view(1, -1, 1, 1)
        s = torch.sigmoid(z)
        b_s = out_bound(z, gamma(c + 2) * mag)
        dl = d64 / heads * (s * (1 - s))
        b_dl = d64.abs() / heads * ((1 - 2 * s).abs() * b_s + b_s * b_s) + 3 * U32 * dl.abs()
        want = torch.einsum("nkhw,kc->nhwc", dl, w64)
        dmag = torch.einsum("nkhw,kc->nhwc", dl.abs(), w64.abs())
        bound = torch.einsum("nkhw,kc->nhwc", b_dl, w64.abs())
        if accs[hh]:
            want, dmag = want + olds[hh].double(), dmag + olds[hh].double().abs()
        bound = bound + gamma(n_cls + 5) * dmag + 1e-300
        if gates[hh]:
            keep = x64 > 0
            want, bound = torch.where(keep, want, torch.zeros_like(want)), torch.where(keep, bound, torch.full_like(bound, 1e-300))
        what = (dt, c, n_cls, (n, h, w), heads, hh, name, accs[hh], gates[hh])
        assert bool(torch.isfinite(dxs[hh].float()).all()), what
        if dt == "bf16":
            close_bf16(dxs[hh], want, what)
        else:
            r = bound_ratio(dxs[hh], want, bound)
            worst_dx = max(worst_dx, r)
            assert r <= 1.0, (what, r)
            assert rel_err(dxs[hh].cpu(), want.cpu()) < TOL, what
        want_dw = torch.einsum("nkhw,nhwc->kc", dl, x64)
        want_db = dl.sum((0, 2, 3))
        ew, eb = rel_err(grads[hh][0].cpu(), want_dw.cpu()), rel_err(grads[hh][1].cpu(), want_db.cpu())
        worst_w = max(worst_w, ew, eb)
        assert ew < TOL and eb < TOL, (what, ew, eb)
        del x64, z, mag, s, b_s, dl, b_dl, want, dmag, bound
    return name, worst_dx, worst_w


FP32_C = (4, 8, 12, 32, 64, 6)
BF16_C = (8, 64)
MATRIX = [("fp32", c, k) for c in FP32_C for k in (1, 4, 5, 8)] + [("bf16", c, k) for c in BF16_C for k in (1, 4, 5, 8)]
SMALL = ((1, 5, 13), (2, 24, 40))


@pytest.mark.parametrize("case", MATRIX, ids=["%s-C%d-k%d" % c for c in MATRIX])
def test_heads_mean_bwd_vs_float64(dev, case):
    dt, c, n_cls = case
    idx = MATRIX.index(case)
    worst_dx, worst_w, names = 0.0, 0.0, set()
    for (n, h, w) in SMALL:
        for heads in (1, 2, 3, 4):
            name, rdx, rw = _check(dev, dt, c, n_cls, n, h, w, heads, 3000 + 16 * idx + 4 * SMALL.index((n, h, w)) + heads)
            worst_dx, worst_w = max(worst_dx, rdx), max(worst_w, rw)
            names.add(name)
    assert len(names) == 1, names                       # neither the head count nor the size changes the kernel
    want = "heads_mean_bwd_bf16" if dt == "bf16" else "heads_mean_bwd_vec" if c % 4 == 0 else "heads_mean_bwd"
    assert names == {want}, (names, want)
    report_ratio("heads_mean_bwd %s-C%d-k%d" % case, "dx err/bound, worst over sizes and 1..4 heads", worst_dx,
                 {"kernel": want, "dW_db_rel_err/1e-4": worst_w / TOL})


def test_heads_mean_bwd_scalar_form_behind_misaligned_pointers(dev):
    """C = 4 (and 8) with features 4 bytes off a 16-byte boundary: what unetpp_head_bwd takes with scalar loads."""
    for c, n_cls, heads in ((4, 4, 3), (4, 5, 2), (8, 1, 4)):
        name, rdx, rw = _check(dev, "fp32", c, n_cls, 2, 24, 40, heads, 4100 + c + heads, misalign=True)
        assert name == "heads_mean_bwd", name
        report_ratio("heads_mean_bwd misaligned C%d-k%d" % (c, n_cls), "dx err/bound", rdx, {"dW_db_rel_err/1e-4": rw / TOL})


LARGE = [("fp32", 32, 5, 3, False), ("fp32", 4, 4, 2, True), ("bf16", 8, 8, 4, False), ("bf16", 64, 1, 1, False)]


@pytest.mark.parametrize("case", LARGE, ids=["%s-C%d-k%d-h%d%s" % (c[0], c[1], c[2], c[3], "-misaligned" if c[4] else "")
                                             for c in LARGE])
def test_heads_mean_bwd_above_the_grid_cap(dev, case):
    """1 x 520 x 520: 4225 tiles of 64 pixels for 4096 workgroups -- some walk a second tile, the last tile is full."""
    dt, c, n_cls, heads, misalign = case
    name, rdx, rw = _check(dev, dt, c, n_cls, 1, 520, 520, heads, 5200 + LARGE.index(case), misalign)
    assert name in ABOVE_CAP
    report_ratio("heads_mean_bwd 520x520 %s-C%d-k%d" % (dt, c, n_cls), "dx err/bound", rdx,
                 {"kernel": name, "dW_db_rel_err/1e-4": rw / TOL})


@pytest.mark.parametrize("dt,c,n_cls,shape,misalign", [("fp32", 32, 4, (2, 24, 40), False), ("fp32", 6, 5, (1, 5, 13), False),
                                                      ("fp32", 4, 8, (2, 24, 40), True), ("bf16", 64, 5, (2, 24, 40), False),
                                                      ("fp32", 12, 4, (1, 520, 520), False), ("bf16", 8, 4, (1, 520, 520), False)])
def test_heads_mean_bwd_two_calls_give_the_same_bits(dev, dt, c, n_cls, shape, misalign):
    n, h, w = shape
    xs, wts, bs, olds, d_out = _operands(dev, dt, c, n_cls, n, h, w, 3, 77 + c, misalign)
    accs, gates = [False, True, True], [True, False, True]
    dx_a, gr_a, name_a = _run(xs, wts, bs, olds, d_out, accs, gates)
    dx_b, gr_b, name_b = _run(xs, wts, bs, olds, d_out, accs, gates)
    assert name_a == name_b
    for hh in range(3):
        assert torch.equal(dx_a[hh], dx_b[hh]), (name_a, hh)
        assert torch.equal(gr_a[hh][0], gr_b[hh][0]) and torch.equal(gr_a[hh][1], gr_b[hh][1]), (name_a, hh)


def test_heads_mean_bwd_max_heads_and_argument_errors(dev):
    """8 heads (the descriptors' capacity); the wrapper's own checks."""
    from unet_nested4tiny_objects_keypoints_amd import ops
    for dt, c in (("fp32", 32), ("fp32", 6), ("bf16", 32)):
        _check(dev, dt, c, 4, 2, 13, 29, 8, 9100 + c)
    x = torch.randn(1, 8, 8, 32, device=dev)
    wt, b, d_out = torch.randn(4, 32, device=dev), torch.randn(4, device=dev), torch.randn(1, 4, 8, 8, device=dev)
    dx = torch.empty_like(x)
    with pytest.raises(ValueError):
        ops.heads_mean_bwd([x] * 9, [wt] * 9, [b] * 9, d_out, [dx] * 9, [False] * 9, [False] * 9)
    with pytest.raises(ValueError):
        ops.heads_mean_bwd([], [], [], d_out, [], [], [])
    with pytest.raises(ValueError):
        ops.heads_mean_bwd([x, x], [wt] * 2, [b] * 2, d_out, [dx], [False] * 2, [False] * 2)
    with pytest.raises(ValueError):
        ops.heads_mean_bwd([x], [wt], [b], d_out[:, :2].contiguous(), [dx], [False], [False])
    with pytest.raises(TypeError):
        ops.heads_mean_bwd([x], [wt], [b], d_out, [dx.to(BF)], [False], [False])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.heads_mean_bwd([x], [wt], [b], d_out.cpu(), [dx], [False], [False])
    with pytest.raises(RuntimeError, match="invalid argument"):     # bf16 storage has the octet form only
        ops.heads_mean_bwd([x[..., :12].contiguous().to(BF)], [wt[:, :12].contiguous()], [b], d_out,
                           [dx[..., :12].contiguous().to(BF)], [False], [False])


def test_every_heads_mean_bwd_kernel_ran(dev):
    """Runs after the cases above (file order): every name the two launchers can report was seen, each also with more
    tiles than workgroups."""
    missing = [k for k in COVERAGE if k not in SEEN]
    assert not missing, missing
    unknown = sorted(SEEN - set(COVERAGE))
    assert not unknown, unknown
    below = [k for k in COVERAGE if k not in ABOVE_CAP]
    assert not below, below
