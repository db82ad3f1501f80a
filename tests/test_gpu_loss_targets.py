"""The caller-side kernels of the training step against plain float64, element by element (GPU only):
focal_bce_kernel, focal_bce_heads_kernel and their finish kernels (csrc/caller.hip), heatmap_kernel / heatmap_norm_kernel
(csrc/caller.hip) and pattern_map_kernel / pattern_norm_kernel (csrc/keypoints.hip).

What is pinned beyond the first-round tests of tests/test_gpu_caller.py and tests/test_keypoints.py:
  * every gradient element inside an a-priori interval (tests/loss_oracle.py: DELTA = 2^-23 on u, EPS = 16 * 2^-24
    after it), its sign, exactly 0.0 at exact hits; the loss inside the sum bound;
  * the scalar tail (numel % 4 != 0), one element, the block edges 2047 / 2048 / 2049, and a NaN guard behind grad;
  * more than 1024 blocks (the finish kernels' strided loop takes its second trip) with the whole loss placed in one
    block or in the last five elements, so a dropped block or trip changes the loss by 100 %;
  * the heads kernel bit for bit against the single-head kernel and the trainer's float32 loop, 1 to 8 heads;
  * gamma < 1 with exact hits (finite loss; gradient 0 at the hit for gamma 0);
  * contiguous views off a 16-byte boundary (copied by ops.py; the C ABI still refuses them);
  * heat maps with more than 256 blocks per image (the norm kernels' blockmax loop takes its second trip), the maximum
    decided in a block >= 256, P = 6, a 35-term float32 running sum, one-row and one-column maps: every normalised
    channel's maximum exactly 1.0 at the oracle's argmax, single-point channels within 1 float32 ulp of the oracle and
    a k-point normalised channel within k + 2 ulps (one possible flip per float32 rounding: the float64 exp and sqrt of
    the two sides differ by about 1e-16, so nothing more is possible) -- relative per element, down to the denormals.

Worst observed error / bound on an MI355X (printed by report_ratio; the bounds come from the error model, not from
these figures):
  focal gradient, tails and block edges   0.25 - 0.28 of the interval (gamma 3, 2, 2.5, 1; rows 1, 3); loss 0.06 - 0.09
  focal gradient, 1026 blocks             0.24 - 0.28 (last five elements 0.10); loss 0.001 - 0.009 of its bound
  heads 1, 2, 5, 8 and 3 at 1026 blocks   bit for bit; gradient 0.25 - 0.28, loss as the single-head kernel
  gamma 0 / 0.5                           gradient 0.03 - 0.23, loss 0.01 - 0.09 (before the fix of focal_thread: NaN
                                          loss and a NaN gradient at the exact hit, both gammas)
  create_heatmap, heatmap_pattern         0 ulps in every case, the 131414 denormal values of the 512 x 512 maps included
"""
import numpy as np
import pytest
import torch

from oracle.keypoints_oracle import create_heatmap_pattern
from oracle.step_oracle import create_heatmap_oracle
from tests import loss_oracle as lo
from tests.helpers import report_ratio

pytestmark = pytest.mark.gpu

GUARD = lo.BLOCK + 64   # floats behind grad[n]: more than the whole last block could overrun


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _dev4(a, dev):
    """float32 numpy [n] -> device tensor (1, 1, 1, n)"""
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(dev).view(1, 1, 1, -1)


def _abi_focal(pred, target, rows, gamma, want_grad=True):
    """unetpp_focal_bce through the C ABI with a NaN guard behind grad -> (loss 0-dim, grad [n] or None, guard or None)"""
    from unet_nested4tiny_objects_keypoints_amd import _lib
    from unet_nested4tiny_objects_keypoints_amd.ops import _ptr, _stream, check
    lib = _lib.lib()
    n = pred.numel()
    partial = torch.empty(int(lib.unetpp_focal_bce_blocks(n)), dtype=torch.float32, device=pred.device)
    loss = torch.empty(1, dtype=torch.float32, device=pred.device)
    buf = torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device=pred.device) if want_grad else None
    check(lib.unetpp_focal_bce(_ptr(pred), _ptr(target), n, rows, float(gamma), _ptr(buf), _ptr(partial), _ptr(loss),
                               _stream()), "unetpp_focal_bce")
    torch.cuda.synchronize()
    if not want_grad:
        return loss.reshape(()), None, None
    return loss.reshape(()), buf[:n], buf[n:]


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("gamma", [3, 2, 2.5, 1])
def test_focal_tails_and_block_edges(dev, gamma, rows):
    from unet_nested4tiny_objects_keypoints_amd import ops
    failures, worst_g, worst_l = [], 0.0, 0.0
    for n in lo.TAIL_SIZES:
        p, t = lo.tail_inputs(n)
        iv = lo.focal_interval(p, t, gamma, rows)
        if n >= 3:
            assert iv.hit.any() and (iv.d == 1).sum() == 1 and (iv.d == -1).sum() == 1
        pd, td = _dev4(p, dev), _dev4(t, dev)
        loss, grad, guard = _abi_focal(pd, td, rows, gamma)
        bad, rg = lo.check_grad(grad.cpu().numpy(), iv)
        rl = lo.loss_ratio(loss.item(), lo.loss_bound(iv))
        worst_g, worst_l = max(worst_g, rg), max(worst_l, rl)
        if not rl <= 1.0:
            bad.append("loss %r outside %r" % (loss.item(), lo.loss_bound(iv)))
        if not bool(torch.isnan(guard).all()):
            bad.append("%d elements written behind grad[n]" % int((~torch.isnan(guard)).sum()))
        # the wrapper is the same launch; without a gradient the loss has the same bits
        loss_w, grad_w = ops.focal_bce(pd, td, rows, gamma)
        loss_n, none = ops.focal_bce(pd, td, rows, gamma, want_grad=False)
        if not (_same_bits(loss_w, loss) and _same_bits(grad_w.view(-1), grad) and none is None and _same_bits(loss_n, loss)):
            bad.append("ops.focal_bce (with or without a gradient) differs from the C ABI call")
        loss_a, none, _ = _abi_focal(pd, td, rows, gamma, want_grad=False)
        if not (none is None and _same_bits(loss_a, loss)):
            bad.append("want_grad=False changes the loss bits")
        if bad:
            failures.append((n, bad))
    report_ratio("focal tails gamma=%s rows=%d" % (gamma, rows), "grad", worst_g, {"loss": worst_l})
    assert not failures, failures


@pytest.mark.parametrize("region", sorted(lo.BIG_REGIONS))
def test_focal_more_than_1024_blocks(dev, region):
    from unet_nested4tiny_objects_keypoints_amd import ops
    p, t = lo.region_inputs(region)
    rows, gamma = 3, 3
    iv = lo.focal_interval(p, t, gamma, rows)
    a, b = lo.BIG_REGIONS[region]
    outside = np.ones(p.size, bool)
    outside[a:b] = False
    assert lo.loss_blocks(p.size) == 1026 and iv.hit[outside].all() and (~iv.hit[a:b]).sum() >= 5
    loss, grad = ops.focal_bce(_dev4(p, dev), _dev4(t, dev), rows, gamma)
    bound = lo.loss_bound(iv)
    bad, rg = lo.check_grad(grad.cpu().numpy(), iv)
    rl = lo.loss_ratio(loss.item(), bound)
    report_ratio("focal 1026 blocks, loss in %s" % region, "grad", rg, {"loss": rl, "loss_value": loss.item()})
    assert not bad, bad
    assert bound[1] > 0 and rl <= 1.0, (loss.item(), bound)


# ---------------------------------------------------------------------------------------------------------------------
def _heads_against_single(dev, preds, target, rows, gamma):
    """focal_bce_heads against focal_bce per head and the trainer's float32 loop: bit for bit"""
    from unet_nested4tiny_objects_keypoints_amd import ops
    heads = len(preds)
    pd, td = [_dev4(p, dev) for p in preds], _dev4(target, dev)
    loss, grads = ops.focal_bce_heads(pd, td, rows, gamma)
    assert loss.shape == (1 + heads,) and len(grads) == heads
    inv_heads = torch.tensor(1.0 / heads, dtype=torch.float32, device=dev)
    avg = 0
    for h in range(heads):
        one, g_one = ops.focal_bce(pd[h], td, rows, gamma)
        assert _same_bits(loss[1 + h], one), (h, loss[1 + h].item(), one.item())
        assert _same_bits(grads[h], g_one * inv_heads), h
        avg = avg + one
    avg = 1.0 * avg / heads
    assert _same_bits(loss[0], avg), (loss[0].item(), avg.item())
    only_loss, none = ops.focal_bce_heads(pd, td, rows, gamma, want_grad=False)
    assert none is None and _same_bits(only_loss, loss)
    return loss, grads


@pytest.mark.parametrize("gamma", [3, 2.5])
@pytest.mark.parametrize("heads", [1, 2, 5, 8])
def test_heads_kernel_is_the_single_head_kernel_bit_for_bit(dev, heads, gamma):
    preds, t = lo.heads_inputs(heads, 2051)
    loss, grads = _heads_against_single(dev, preds, t, 3, gamma)
    worst = 0.0
    for h in range(heads):   # and every head is right, not only equal
        iv = lo.focal_interval(preds[h], t, gamma, 3)
        bad, rg = lo.check_grad(grads[h].view(-1).cpu().numpy() * np.float64(heads), _widen(iv, heads))
        assert not bad, (h, bad)
        assert lo.loss_ratio(loss[1 + h].item(), lo.loss_bound(iv)) <= 1.0
        worst = max(worst, rg)
    report_ratio("focal heads=%d gamma=%s" % (heads, gamma), "grad", worst)


def _widen(iv, heads):
    """the interval of heads * (gradient under the mean over heads): two more float32 roundings (1 / heads and the
    product with it) than the single-head gradient -- 2 * 2^-24 relative, exact when heads is a power of two"""
    if heads & (heads - 1) == 0:
        return iv
    w = 2 * 2.0 ** -24
    lo_, hi_ = iv.lo - w * np.abs(iv.lo), iv.hi + w * np.abs(iv.hi)
    return iv._replace(lo=lo_, hi=hi_)


def test_heads_kernel_more_than_1024_blocks(dev):
    regions = ("block1023", "block1024", "last5")
    preds = [lo.region_inputs(r)[0] for r in regions]
    t = lo.region_inputs(regions[0])[1]
    assert all(np.array_equal(lo.region_inputs(r)[1], t) for r in regions)
    loss, grads = _heads_against_single(dev, preds, t, 3, 3)
    for h, r in enumerate(regions):
        iv = lo.focal_interval(preds[h], t, 3, 3)
        bound = lo.loss_bound(iv)
        rl = lo.loss_ratio(loss[1 + h].item(), bound)
        bad, rg = lo.check_grad(grads[h].view(-1).cpu().numpy() * np.float64(3), _widen(iv, 3))
        report_ratio("focal heads 1026 blocks, head %d in %s" % (h, r), "grad", rg, {"loss": rl})
        assert not bad, (r, bad)
        assert bound[1] > 0 and rl <= 1.0, (r, loss[1 + h].item(), bound)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 2051])
@pytest.mark.parametrize("gamma", [0, 0.5])
def test_focal_gamma_below_one_with_exact_hits(dev, gamma, n):
    """u^gamma as powf(u, gamma - 1) * u is inf * 0 at an exact hit: the kernel takes 0^0 = 1 (torch's value) and the
    log term at its limit 0 there.  gamma 0.5: the gradient is checked where d != 0 only (torch itself has NaN at the hit)."""
    from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d, ops
    p, t = lo.tail_inputs(n)
    iv = lo.focal_interval(p, t, gamma, 3)
    assert iv.hit.any()
    loss, grad = ops.focal_bce(_dev4(p, dev), _dev4(t, dev), 3, gamma)
    got = grad.view(-1).cpu().numpy()
    assert np.isfinite(loss.item())
    rl = lo.loss_ratio(loss.item(), lo.loss_bound(iv))
    bad, rg = lo.check_grad(got, iv, where=None if gamma == 0 else ~iv.hit)
    report_ratio("focal gamma=%s n=%d" % (gamma, n), "grad", rg, {"loss": rl})
    assert rl <= 1.0, (loss.item(), lo.loss_bound(iv))
    assert not bad, bad
    if gamma == 0:
        assert np.all(got[iv.hit] == 0.0)
    # the module's own torch statement (CPU tensors, float32) is the same function: a finite loss, the same value
    cpu = FocalLoss_BCE_2d(gamma=gamma)(torch.from_numpy(p).view(1, 1, 1, -1), torch.from_numpy(t).view(1, 1, 1, -1))
    assert abs(cpu.item() / 3 - loss.item()) <= 1e-5 * loss.item()


# ---------------------------------------------------------------------------------------------------------------------
def test_misaligned_contiguous_views(dev):
    """pred / target as base[1:1 + n].view(1, 1, 1, n): contiguous, 4 bytes off a 16-byte boundary.  The module and
    mean_over_heads give the bits of aligned copies; the C ABI keeps refusing such pointers."""
    from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d, _lib
    from unet_nested4tiny_objects_keypoints_amd.ops import _ptr, _stream
    n, heads = 2051, 3
    preds, t = lo.heads_inputs(heads, n)

    def off_by_one(a):
        base = torch.zeros(n + 8, dtype=torch.float32, device=dev)
        assert base.data_ptr() % 16 == 0
        v = base[1:1 + n].view(1, 1, 1, n)
        v.copy_(torch.from_numpy(a).view(1, 1, 1, n))
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
        return v

    crit = FocalLoss_BCE_2d(gamma=3, size_average=False)
    tv, ta = off_by_one(t), _dev4(t, dev)
    pv = [off_by_one(p) for p in preds]
    pa = [_dev4(p, dev) for p in preds]
    for v, a in zip(pv, pa):
        v1, a1 = v.detach().requires_grad_(True), a.detach().requires_grad_(True)
        lv, la = crit(v1, tv), crit(a1, ta)
        lv.backward()
        la.backward()
        assert _same_bits(lv, la) and _same_bits(v1.grad, a1.grad)
    got, want = crit.mean_over_heads(tuple(pv), tv), crit.mean_over_heads(tuple(pa), ta)
    assert got is not None and want is not None
    assert _same_bits(got[0], want[0]) and all(_same_bits(g, w) for g, w in zip(got[1], want[1]))
    # the C ABI's contract stays: EINVAL, nothing launched
    lib = _lib.lib()
    partial = torch.empty(2, dtype=torch.float32, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    grad = torch.empty(n, dtype=torch.float32, device=dev)
    assert lib.unetpp_focal_bce(_ptr(pv[0]), _ptr(ta), n, 1, 3.0, _ptr(grad), _ptr(partial), _ptr(loss), _stream()) == -1
    assert lib.unetpp_focal_bce(_ptr(pa[0]), _ptr(tv), n, 1, 3.0, _ptr(grad), _ptr(partial), _ptr(loss), _stream()) == -1


# ---------------------------------------------------------------------------------------------------------------------
# Heat maps.  Cases (N, P, H, W); HEAT_CASES[0] has 265 blocks of 256 pixels per image with a ragged last one, and the
# points of its image 0 sit in rows >= 253 (pixel index >= 65536: block index >= 256) or outside the frame.
HEAT_CASES = [(2, 7, 260, 260), (1, 6, 512, 512), (3, 40, 33, 65), (1, 7, 1, 300), (1, 7, 300, 1)]
PATTERNS = [([[0], [1, 2, 3], [4], [5, 6]], 3.0), ([[2, 0], [1]], 5.0), (None, 2.5)]   # None: one map of all points


def heat_points(case):
    n, p, h, w = case
    rng = np.random.default_rng(100 + h * w + p)
    pts = np.stack([rng.uniform(-2, w + 2, (n, p)), rng.uniform(-2, h + 2, (n, p))], axis=-1).astype(np.float32)
    if case == HEAT_CASES[0]:
        pts[0, :, 0] = [30, 100, 900, -40, 160, 200, 300]      # x: 900, -40 and 300 are outside the frame
        pts[0, :, 1] = [255, 256, 256.5, 257, 254, 258, 259]   # y
        pts[1, 2] = (17, 200)                                   # exactly on a pixel of the second image
    elif min(h, w) > 1:
        pts[0, 0] = (w - 1, h - 1)          # exactly on the last pixel
        pts[0, 1] = (5, 7)                  # exactly on a pixel: the normalised channel's sum has a distance 0
        pts[0, 4] = (w + 40.5, -30.25)      # outside the frame
        pts[0, 5] = (3, h - 2)
    else:
        pts[0, 0] = (0, 0)
        pts[0, 5] = (w - 1, h - 1)
        pts[0, 2] = (-7.5, -3.25)
    return pts


_HEAT_ORACLE = {}


def heat_oracle(case):
    if case not in _HEAT_ORACLE:
        want = create_heatmap_oracle(heat_points(case), case[2], case[3])
        want.flags.writeable = False
        _HEAT_ORACLE[case] = want
    return _HEAT_ORACLE[case]


def _check_normalised(got, want, k, label, first_image_from_block=None):
    """one normalised k-point channel per leading index: maximum exactly 1.0 at the oracle's argmax, k + 2 ulps"""
    worst = 0.0
    for idx in np.ndindex(got.shape[:-2]):
        g, w = got[idx].ravel(), want[idx].ravel()
        at = int(np.argmax(w))
        assert w[at] == 1.0
        assert float(g.max()) == 1.0 and g[at] == 1.0, (label, idx, float(g.max()), g[at], at)
        if first_image_from_block is not None and idx[0] == 0:
            assert at // 256 >= first_image_from_block, (label, idx, at)   # (a check of the test's own input)
        r = float(lo.ulps(g, w).max()) / (k + 2)
        assert r <= 1.0, (label, idx, r * (k + 2), k)
        worst = max(worst, r)
    return worst


@pytest.mark.parametrize("case", HEAT_CASES, ids=lambda c: "%dx%dx%dx%d" % c)
def test_create_heatmap_ulps(dev, case):
    from unet_nested4tiny_objects_keypoints_amd import create_heatmap, ops
    n, p, h, w = case
    pts = heat_points(case)
    want = heat_oracle(case)
    got_t = ops.create_heatmap(torch.from_numpy(pts).to(dev), h, w)
    got = got_t.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32
    assert torch.equal(create_heatmap(pts, h, w), got_t)        # the package's wrapper is the same launch
    single = max(float(lo.ulps(got[:, c], want[:, c]).max()) for c in (0, 2))
    assert single <= 1.0, single
    far = 256 if case == HEAT_CASES[0] else None
    r1 = _check_normalised(got[:, 1:2], want[:, 1:2], 3, "channel 1", far)
    r3 = _check_normalised(got[:, 3:4], want[:, 3:4], p - 5, "channel 3", far)
    report_ratio("create_heatmap %dx%dx%dx%d" % case, "channels 0, 2 (ulps / 1)", single,
                 {"channel 1 (ulps / 5)": r1, "channel 3 (ulps / %d)" % (p - 3): r3, "blocks": -(-h * w // 256)})


@pytest.mark.parametrize("which", range(len(PATTERNS)))
@pytest.mark.parametrize("case", HEAT_CASES, ids=lambda c: "%dx%dx%dx%d" % c)
def test_pattern_maps_ulps(dev, case, which):
    from unet_nested4tiny_objects_keypoints_amd import Heatmap, ops
    n, p, h, w = case
    pattern, radius = PATTERNS[which]
    if pattern is None:
        pattern = [list(range(p))]
    pattern = [[i for i in m if i < p] for m in pattern]      # (P = 6: the last map keeps point 5 alone)
    pts = heat_points(case)
    want = create_heatmap_pattern(pts, pattern, h, w, radius)
    got_t = ops.heatmap_pattern(torch.from_numpy(pts).to(dev), pattern, h, w, radius)
    got = got_t.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32
    if which == 0:
        assert torch.equal(Heatmap(pattern, w, h, radius).create_heatmap(pts), got_t)
    worst = {}
    for m, hmap in enumerate(pattern):
        worst["map %d (ulps / %d)" % (m, len(hmap) + 2)] = _check_normalised(
            got[:, m:m + 1], want[:, m:m + 1], len(hmap), "map %d" % m, 256 if case == HEAT_CASES[0] else None)
    report_ratio("heatmap_pattern %dx%dx%dx%d pattern %d" % (case + (which,)), "worst", max(worst.values()), worst)
