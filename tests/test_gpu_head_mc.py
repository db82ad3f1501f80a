"""Monte-Carlo dropout at the heads on the GPU: unetpp_head_mc / ops.head_mc, UNet_Nested.infer_mc, SceneInference.uncertainty.

(a) Bit for bit against the composition through the oracle: the K samples come from K ops.head_fwd launches at the
    documented seeds (each must have run head_fwd_stream<L,P,1>), are folded by tests/mc_oracle.fold (float32 numpy, the
    stated order) and compared with the kernel's mean and variance as int32 views; two NaNs count as equal.
(b) Against float64: keep masks restated by oracle/dropout_oracle.keep_mask at the K seeds, float64 samples, mean and
    unbiased variance; the mean within the TOL tests/test_gpu_heads.py holds head_fwd to, the variance within
    mc_oracle.var_tolerance (derived there from that tolerance and |d| <= 1).
(c) The fallback composition (8 channels, bf16 storage, UNETPP_NO_FUSED_HEAD_MC in a fresh process) returns the same bits
    and launches no head_mc kernel.
(d) infer_mc on a tiny network, (e) scene.uncertainty against per-chunk infer_mc placed by torch slicing.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle.dropout_oracle import keep_mask
from tests import mc_oracle as mo
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4                      # tests/test_gpu_heads.py: rel_err(out, sigmoid(z64)) < TOL
KS = (2, 3, 8, 32)
PS = (0.1, 0.4)
SMALL = (3, 5, 7)               # 105 pixels: less than one workgroup at C = 16, a partial last group, image carries
CHANNEL_CLASSES = [(c, k) for c in (16, 32, 64, 128) for k in ((3, 4) if c == 16 else (3, 4, 5, 8))]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def last_kernel():
    from unet_nested4tiny_objects_keypoints_amd import _lib
    return _lib.lib().unetpp_last_kernel_name().decode()


def coords(c, n_cls):
    return (c // 4).bit_length() - 1, 4 if n_cls <= 4 else 8      # (L, P) of head_fwd_stream<L,P,D> / head_mc<L,P>


def operands(dev, shape, c, n_cls, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    n, h, w = shape
    x = torch.randn(n, h, w, c, generator=g).to(dev).to(dtype)
    wt = (torch.randn(n_cls, c, generator=g) * (1.5 / c ** 0.5)).to(dev)
    bias = (torch.randn(n_cls, generator=g) * 0.5).to(dev)
    return x, wt, bias


def composed_samples(x, wt, bias, p, seed, k, seed_dev=None, want_kernel=None):
    """The K maps of K ops.head_fwd launches at the documented seeds -> float32 numpy [K, N, n_cls, H, W]."""
    from unet_nested4tiny_objects_keypoints_amd import ops
    n, h, w, _ = x.shape
    maps = []
    for i in range(k):
        out = torch.full((n, wt.shape[0], h, w), float("nan"), device=x.device)
        ops.head_fwd(x, wt, bias, p, (seed + mo.SEED_STEP * i) & mo.MASK64, None, out, seed_dev=seed_dev)
        if want_kernel is not None:
            assert last_kernel() == want_kernel, (last_kernel(), want_kernel)
        maps.append(out.cpu().numpy())
    return np.stack(maps)


def run_mc(x, wt, bias, p, seed, k, seed_dev=None):
    from unet_nested4tiny_objects_keypoints_amd import ops
    n, h, w, _ = x.shape
    mean = torch.full((n, wt.shape[0], h, w), float("nan"), device=x.device)
    var = torch.full_like(mean, float("nan"))
    ops.head_mc(x, wt, bias, p, seed, k, mean, var, seed_dev=seed_dev)
    name = last_kernel()
    return mean.cpu().numpy(), var.cpu().numpy(), name


def assert_bits(got, want, what):
    ok = mo.same_bits(got, want)
    if not ok.all():
        idx = tuple(int(v[0]) for v in np.nonzero(~ok))
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %r want %r"
                             % (what, int((~ok).sum()), ok.size, idx, got[idx], want[idx]))


def check_against_composition(x, wt, bias, p, seed, k, what, seed_dev=None, mc_seed=None):
    c, n_cls = x.shape[3], wt.shape[0]
    L, P = coords(c, n_cls)
    samples = composed_samples(x, wt, bias, p, seed, k, seed_dev, "head_fwd_stream<%d,%d,1>" % (L, P))
    mean, var, name = run_mc(x, wt, bias, p, seed if mc_seed is None else mc_seed, k, seed_dev)
    assert name == "head_mc<%d,%d>" % (L, P), name
    want_mean, want_var = mo.fold(samples)
    assert_bits(mean, want_mean, (what, "mean"))
    assert_bits(var, want_var, (what, "var"))
    return samples, mean, var


# ------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("c,n_cls", CHANNEL_CLASSES)
def test_bits_against_composition(dev, c, n_cls):
    x, wt, bias = operands(dev, SMALL, c, n_cls, 100 + c + n_cls)
    for k in KS:
        for p in PS:
            seed = (0x9E3779B97F4A7C15 * (k + 1) + int(p * 1000) + c) & mo.MASK64
            samples, mean, var = check_against_composition(x, wt, bias, p, seed, k, (c, n_cls, k, p))
            assert np.isfinite(mean).all() and (var >= 0).all()
            assert (samples[0] != samples[1]).any()        # the draws differ: dropout is on


def test_bits_above_one_sweep_of_the_grid(dev):
    """1 x 368 x 368 at C = 128: 135424 pixels, more than the 4 x 4096 x 8 = 131072 of one sweep of the capped grid, H * W
    no multiple of a span: the outer loop and the carried (image, position) run."""
    x, wt, bias = operands(dev, (1, 368, 368), 128, 4, 7)
    assert 368 * 368 > 4 * 4096 * (256 // 32)
    check_against_composition(x, wt, bias, 0.4, 0xFEDCBA9876543210, 2, "368x368")


def test_bits_above_the_grid_cap_with_image_carries(dev):
    """3 images of 111 x 111 at C = 128: 36963 pixels against a span of 4096 x 8 = 32768 (two whole images and 8126
    pixels), so a thread's four pixels lie in different images and the carried (image, position) takes its carries."""
    x, wt, bias = operands(dev, (3, 111, 111), 128, 5, 8)
    assert 111 * 111 < 4096 * 8 < 3 * 111 * 111
    check_against_composition(x, wt, bias, 0.1, 12345, 2, "3x111x111")


def test_seed_dev_equals_seed_by_value(dev):
    x, wt, bias = operands(dev, SMALL, 32, 4, 9)
    seed, word = 0x0F1E2D3C4B5A6978, 0x0123456789ABCDEF
    seed_dev = torch.tensor([word], dtype=torch.int64, device=dev)
    _, mean_v, var_v = check_against_composition(x, wt, bias, 0.4, seed, 8, "by value")
    mean_d, var_d, name = run_mc(x, wt, bias, 0.4, (seed - word) & mo.MASK64, 8, seed_dev)
    assert name == "head_mc<3,4>"
    assert_bits(mean_d, mean_v, "seed_dev mean")
    assert_bits(var_d, var_v, "seed_dev var")
    # and the composition with the device word gives the same samples
    check_against_composition(x, wt, bias, 0.4, (seed - word) & mo.MASK64, 8, "device word", seed_dev=seed_dev)


def test_planted_nan_and_inf(dev):
    x, wt, bias = operands(dev, SMALL, 32, 4, 10)
    x[0, 1, 2, 5] = float("nan")
    x[2, 3, 4, 17] = float("inf")
    x[1, 0, 6, 30] = float("-inf")
    _, mean, var = check_against_composition(x, wt, bias, 0.4, 99, 8, "non-finite")
    assert np.isnan(mean[0, :, 1, 2]).all() and np.isnan(var[0, :, 1, 2]).all()     # some draw keeps channel 5
    clean = np.ones(mean.shape, dtype=bool)
    clean[0, :, 1, 2] = clean[2, :, 3, 4] = clean[1, :, 0, 6] = False
    assert np.isfinite(mean[clean]).all() and np.isfinite(var[clean]).all()         # and nothing spreads


# ------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("c,n_cls,k,p", [(16, 3, 2, 0.4), (32, 4, 8, 0.4), (64, 5, 3, 0.1), (128, 8, 32, 0.4)])
def test_against_float64(dev, c, n_cls, k, p):
    x, wt, bias = operands(dev, SMALL, c, n_cls, 200 + c)
    seed = 0xA5A5A5A55A5A5A5A ^ c
    mean, var, name = run_mc(x, wt, bias, p, seed, k)
    assert name.startswith("head_mc<")
    n, h, w = SMALL
    x64, w64, b64 = x.cpu().double().numpy(), wt.cpu().double().numpy(), bias.cpu().double().numpy()
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))      # the launcher's 1.0f / (1.0f - p_drop)
    s64 = []
    for i in range(k):
        keep = keep_mask((seed + mo.SEED_STEP * i) & mo.MASK64, n, h, w, c, p)
        z = np.einsum("nhwc,kc->nkhw", x64 * keep * scale, w64) + b64[None, :, None, None]
        s64.append(1.0 / (1.0 + np.exp(-z)))
    s64 = np.stack(s64)
    mean64, var64 = mo.fold64(s64)
    err = rel_err(torch.from_numpy(mean), torch.from_numpy(mean64))
    print("head_mc vs float64: C %d K %d mean rel err %.3e" % (c, k, err))
    assert err < TOL
    eps = TOL * float(np.abs(s64).max())
    worst = float(np.abs(var.astype(np.float64) - var64).max())
    print("head_mc vs float64: C %d K %d var err %.3e of %.3e" % (c, k, worst, mo.var_tolerance(k, eps)))
    assert worst <= mo.var_tolerance(k, eps)
    assert float(var64.max()) > 20 * mo.var_tolerance(k, eps)      # the interval is far below what is being measured


# ------------------------------------------------------------------------------------------- (c)
def test_fallback_eight_channels(dev):
    x, wt, bias = operands(dev, SMALL, 8, 4, 11)
    samples = composed_samples(x, wt, bias, 0.4, 77, 8)
    assert not last_kernel().startswith("head_fwd_stream")
    mean, var, name = run_mc(x, wt, bias, 0.4, 77, 8)
    assert not name.startswith("head_mc"), name
    want_mean, want_var = mo.fold(samples)
    assert_bits(mean, want_mean, "C = 8 mean")
    assert_bits(var, want_var, "C = 8 var")


def test_fallback_bf16_storage(dev):
    x, wt, bias = operands(dev, SMALL, 32, 4, 12, dtype=torch.bfloat16)
    samples = composed_samples(x, wt, bias, 0.4, 78, 3)
    assert last_kernel().startswith("head_fwd_bf16<")
    mean, var, name = run_mc(x, wt, bias, 0.4, 78, 3)
    assert name.startswith("head_fwd_bf16<"), name
    want_mean, want_var = mo.fold(samples)
    assert_bits(mean, want_mean, "bf16 mean")
    assert_bits(var, want_var, "bf16 var")


_CHILD = """
import sys
import numpy as np
import torch
sys.path.insert(0, %(root)r)
from unet_nested4tiny_objects_keypoints_amd import _lib, ops
from tests.test_gpu_head_mc import operands, run_mc
assert ops._FUSED_HEAD_MC is False
x, wt, bias = operands(torch.device("cuda:0"), (3, 5, 7), 32, 4, 13)
mean, var, name = run_mc(x, wt, bias, 0.4, 4242, 8)
assert name == "head_fwd_stream<3,4,1>", name
np.savez(%(out)r, mean=mean, var=var)
"""


def test_switch_takes_the_composition_with_the_fused_bits(dev, tmp_path):
    """UNETPP_NO_FUSED_HEAD_MC=1 is read once at import: a fresh process takes the composition and gets the fused bits."""
    out = str(tmp_path / "child.npz")
    env = dict(os.environ, UNETPP_NO_FUSED_HEAD_MC="1")
    done = subprocess.run([sys.executable, "-c", _CHILD % {"root": ROOT, "out": out}], env=env, cwd=ROOT,
                          capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    x, wt, bias = operands(dev, SMALL, 32, 4, 13)
    mean, var, name = run_mc(x, wt, bias, 0.4, 4242, 8)
    assert name == "head_mc<3,4>"
    child = np.load(out)
    assert_bits(child["mean"], mean, "switch mean")
    assert_bits(child["var"], var, "switch var")


# ------------------------------------------------------------------------------------------- (d)
def tiny_model(dev, feature_scale=2, seed=0):
    from unet_nested4tiny_objects_keypoints_amd import UNet_Nested
    torch.manual_seed(seed)
    model = UNet_Nested(in_channels=1, n_classes=4, feature_scale=feature_scale, depth=3).to(dev).eval()
    with torch.no_grad():       # running statistics that are not the identity
        for name, buf in model.named_buffers():
            if name.endswith("running_mean"):
                buf.normal_(0.0, 0.1)
            elif name.endswith("running_var"):
                buf.uniform_(0.5, 1.5)
    return model


def test_infer_mc_tiny_network(dev, monkeypatch):
    from unet_nested4tiny_objects_keypoints_amd import McMaps, ops
    model = tiny_model(dev)                    # 16 channels at level 0
    assert model.filters[0] == 16
    x = torch.randn(2, 1, 32, 48, generator=torch.Generator().manual_seed(1)).to(dev)
    for head in (1, 2):
        fused = model.infer_mc(x, head, samples=8, seed=1234)
        assert last_kernel() == "head_mc<2,4>"
        assert isinstance(fused, McMaps) and fused.mean.shape == fused.var.shape == (2, 4, 32, 48)
        assert fused.mean.dtype == fused.var.dtype == torch.float32
        assert fused.mean.grad_fn is None and fused.var.grad_fn is None and not fused.var.requires_grad
        assert bool((fused.var >= 0).all()) and bool((fused.var > 0).any())
        assert torch.equal(fused.std, fused.var.sqrt())
        with monkeypatch.context() as m:
            m.setattr(ops, "_FUSED_HEAD_MC", False)
            composed = model.infer_mc(x, head, samples=8, seed=1234)
            assert last_kernel() == "head_fwd_stream<2,4,1>"
        assert_bits(composed.mean.cpu().numpy(), fused.mean.cpu().numpy(), ("infer_mc mean", head))
        assert_bits(composed.var.cpu().numpy(), fused.var.cpu().numpy(), ("infer_mc var", head))
        other = model.infer_mc(x, head, samples=8, seed=1235)
        assert bool((other.var != fused.var).any())
    torch.manual_seed(5)
    a = model.infer_mc(x, samples=4)
    torch.manual_seed(5)
    b = model.infer_mc(x, samples=4)
    c = model.infer_mc(x, samples=4)
    assert torch.equal(a.mean, b.mean) and torch.equal(a.var, b.var)
    assert bool((c.var != a.var).any())
    d = model.infer_mc(x, 2, samples=4, p=0.1, seed=9)
    e = model.infer_mc(x, 2, samples=4, seed=9)          # p = None: model.drop_out.p = 0.4
    assert float(d.var.mean()) < float(e.var.mean())
    model.dropout_masks = [torch.zeros(2, 32, 48, 16, dtype=torch.uint8, device=dev)] * 2    # ignored
    f = model.infer_mc(x, 2, samples=4, seed=9)
    model.dropout_masks = None
    assert torch.equal(f.var, e.var) and torch.equal(f.mean, e.mean)
    for bad in (0, 3, True):
        with pytest.raises(ValueError):
            model.infer_mc(x, bad)
    model.train()
    with pytest.raises(RuntimeError, match="eval forward"):
        model.infer_mc(x)
    model.eval()
    getattr(model.conv00.conv1, "1").train()
    with pytest.raises(RuntimeError, match="BatchNorm layer"):
        model.infer_mc(x)


def test_infer_mc_sample_is_a_head_fwd_call(dev, monkeypatch):
    """Sample k of infer_mc(x, J, seed=s) is ops.head_fwd on X_0J with final_J's weights at the seed
    s + HEAD_SEED_STEP * J + SEED_STEP * k: the feature tensor the pass hands to ops.head_mc is caught on the way, the K
    head_fwd maps are folded by the oracle, and the bits must be infer_mc's."""
    from unet_nested4tiny_objects_keypoints_amd import engine, ops
    model = tiny_model(dev, seed=3)
    x = torch.randn(2, 1, 32, 48, generator=torch.Generator().manual_seed(2)).to(dev)
    head, seed, k = 2, 31337, 3
    final = model.final_2
    captured = {}
    real = ops.head_mc

    def spy(xf, *args, **kw):
        captured["x"] = xf
        return real(xf, *args, **kw)

    monkeypatch.setattr(ops, "head_mc", spy)
    got = model.infer_mc(x, head, samples=k, seed=seed)
    assert last_kernel() == "head_mc<2,4>" and tuple(captured["x"].shape) == (2, 32, 48, 16)
    wt, bias = final.weight.detach().view(4, -1), final.bias.detach()
    samples = composed_samples(captured["x"], wt, bias, 0.4, (seed + mo.HEAD_SEED_STEP * head) & mo.MASK64, k,
                               want_kernel="head_fwd_stream<2,4,1>")
    want_mean, want_var = mo.fold(samples)
    assert_bits(got.mean.cpu().numpy(), want_mean, "infer_mc mean")
    assert_bits(got.var.cpu().numpy(), want_var, "infer_mc var")
    assert engine.HEAD_SEED_STEP == mo.HEAD_SEED_STEP


def test_infer_mc_eight_channels_takes_the_fallback(dev):
    model = tiny_model(dev, feature_scale=4)
    assert model.filters[0] == 8
    x = torch.randn(2, 1, 32, 48, generator=torch.Generator().manual_seed(3)).to(dev)
    maps = model.infer_mc(x, 2, samples=4, seed=1)
    assert not last_kernel().startswith("head_mc"), last_kernel()
    assert bool((maps.var >= 0).all()) and bool((maps.var > 0).any()) and bool(torch.isfinite(maps.mean).all())


# ------------------------------------------------------------------------------------------- (e)
def test_scene_uncertainty(dev):
    from unet_nested4tiny_objects_keypoints_amd import SceneInference
    model = tiny_model(dev, seed=4)
    S, H, W, tile, chunk, samples, seed = 1, 96, 112, 64, 8, 4, 2024
    scene = SceneInference(model, head=2, tile=tile, chunk=chunk, mul=1.0, add=0.0)
    frames = torch.rand(S, 1, H, W, generator=torch.Generator().manual_seed(6)).to(dev)
    got = scene.uncertainty(frames, samples=samples, seed=seed)
    assert got.mean.shape == got.var.shape == (S, 4, H, W)
    tiles = scene._tiles(S, H, W)
    assert len(tiles) == 12 and -(-len(tiles) // chunk) == 2          # two chunks: 8 tiles and 4
    want_mean = torch.full((S, 4, H, W), float("nan"), device=dev)
    want_var = torch.full_like(want_mean, float("nan"))
    for i in range(0, len(tiles), chunk):
        part = tiles[i:i + chunk]
        batch = torch.stack([frames[s, :, oy:oy + tile, ox:ox + tile] for (s, oy, ox, *_r) in part]).contiguous()
        maps = model.infer_mc(batch, 2, samples=samples, seed=(seed + mo.CHUNK_SEED_STEP * (i // chunk + 1)) & mo.MASK64)
        for t, (s, oy, ox, y0, y1, x0, x1) in enumerate(part):
            want_mean[s, :, y0:y1, x0:x1] = maps.mean[t, :, y0 - oy:y1 - oy, x0 - ox:x1 - ox]
            want_var[s, :, y0:y1, x0:x1] = maps.var[t, :, y0 - oy:y1 - oy, x0 - ox:x1 - ox]
    assert_bits(got.mean.cpu().numpy(), want_mean.cpu().numpy(), "scene mean")
    assert_bits(got.var.cpu().numpy(), want_var.cpu().numpy(), "scene var")
    assert bool(torch.isfinite(got.mean).all()) and bool((got.var >= 0).all()) and bool((got.var > 0).any())
    again = scene.uncertainty(frames, samples=samples, seed=seed)
    assert torch.equal(again.var, got.var)
    assert bool((scene.uncertainty(frames, samples=samples, seed=seed + 1).var != got.var).any())
    for kw in (dict(tta="flips"), dict(ensemble=True)):
        with pytest.raises(ValueError, match="not the variance of the averaged map"):
            SceneInference(model, head=2, tile=tile, chunk=chunk, **kw).uncertainty(frames)
