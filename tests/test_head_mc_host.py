"""Monte-Carlo dropout at the heads, the part that needs no GPU: the C entry point unetpp_head_mc is declared, mirrored
and refuses what it must without touching the device; tests/mc_oracle.py -- the float32 restatement of the fold the GPU
tests hold the kernel to bit for bit -- is itself held to float64 inside its a-priori interval, pinned to the stated
order on hand-made samples, and told apart from three planted mutations."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import mc_oracle as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "unetpp_hip.h")
F32 = np.float32


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as entry
    entry.build()
    from unet_nested4tiny_objects_keypoints_amd import _lib
    return _lib


# ------------------------------------------------------------------------------------------- the ABI
_CTYPES = {"const float*": ctypes.c_void_p, "float*": ctypes.c_void_p, "const uint64_t*": ctypes.c_void_p,
           "void*": ctypes.c_void_p, "int32_t": ctypes.c_int32, "float": ctypes.c_float, "uint64_t": ctypes.c_uint64}


def test_header_and_signature_table_agree(built_lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+unetpp_head_mc\s*\(([^)]*)\)\s*;", text)
    assert m, "include/unetpp_hip.h does not declare unetpp_head_mc"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    names = [p.rsplit(" ", 1)[1] for p in params]
    assert names == ["x", "weight", "bias", "N", "H", "W", "C", "n_cls", "p_drop", "seed", "seed_dev", "samples",
                     "mean_nchw", "var_nchw", "stream"]
    want = [_CTYPES[p.rsplit(" ", 1)[0]] for p in params]
    res, args = built_lib.SIGNATURES["unetpp_head_mc"]
    assert res is ctypes.c_int and args == want
    assert re.search(r"#define\s+UNETPP_MC_MAX_SAMPLES\s+32\b", text)
    assert built_lib.MC_MAX_SAMPLES == mo.MAX_SAMPLES == 32 and built_lib.MC_SEED_STEP == mo.SEED_STEP
    lib = built_lib.lib()
    assert lib.unetpp_abi_version() == built_lib.ABI_VERSION == 14
    assert hasattr(ctypes.CDLL(built_lib.LIB_PATH), "unetpp_head_mc")


def test_refusals_without_a_device(built_lib):
    """Every refusal comes back as UNETPP_EINVAL before anything touches the device (this runs without a GPU; the pointers
    are made-up addresses that are never dereferenced)."""
    lib = built_lib.lib()
    X, WT, B, M, V = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000

    def call(x=X, wt=WT, b=B, m=M, v=V, shape=(2, 8, 8), c=32, n_cls=4, p=0.4, samples=8):
        n, h, w = shape
        return lib.unetpp_head_mc(x, wt, b, n, h, w, c, n_cls, p, 1234, None, samples, m, v, None)

    for samples in (1, 33, 0, -3):
        assert call(samples=samples) == -1, samples
    for p in (0.0, 1.0, float("nan"), -0.1, 1.5):
        assert call(p=p) == -1, p
    for role in ("x", "wt", "b", "m", "v"):
        assert call(**{role: None}) == -1, role
    assert call(c=8, n_cls=4) == -1        # four padded classes do not fit the two lanes of a pixel
    assert call(c=24) == -1                # 6 channel quads: not a power of two
    assert call(c=256) == -1               # above the heads' 128 channels
    assert call(c=16, n_cls=5) == -1       # 5 classes pad to 8, a 16-channel pixel has 4 lanes
    assert call(x=X + 4) == -1             # x off its 16-byte rows
    assert call(wt=WT + 8) == -1
    assert call(shape=(0, 8, 8)) == -1 and call(n_cls=0) == -1 and call(n_cls=9, c=64) == -1
    assert call(shape=(1, 1 << 14, 1 << 14), c=16) == -1    # 2^32 elements: past the 32-bit offsets


def test_python_argument_errors_need_no_device():
    from unet_nested4tiny_objects_keypoints_amd import ops
    x, wt, b = torch.zeros(1, 2, 2, 16), torch.zeros(4, 16), torch.zeros(4)
    out = torch.zeros(1, 4, 2, 2)
    for samples in (1, 33, True, 4.0):
        with pytest.raises(ValueError, match="samples"):
            ops.head_mc(x, wt, b, 0.4, 0, samples, out, out.clone())
    for p in (0.0, 1.0, float("nan"), -0.2):
        with pytest.raises(ValueError, match="p_drop"):
            ops.head_mc(x, wt, b, p, 0, 4, out, out.clone())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.head_mc(x, wt, b, 0.4, 0, 4, out, out.clone())
    assert ops.mc_sample_seeds(5, 3) == mo.sample_seeds(5, 3) == [5, (5 + mo.SEED_STEP) & mo.MASK64,
                                                                  (5 + 2 * mo.SEED_STEP) & mo.MASK64]


def test_package_exports_mcmaps():
    import unet_nested4tiny_objects_keypoints_amd as pkg
    maps = pkg.McMaps(torch.zeros(2), torch.tensor([4.0, 9.0]))
    assert maps._fields == ("mean", "var") and maps.std.tolist() == [2.0, 3.0]
    assert hasattr(pkg.UNet_Nested, "infer_mc") and hasattr(pkg.SceneInference, "uncertainty")
    model = pkg.UNet_Nested(in_channels=1, feature_scale=4, depth=3)
    with pytest.raises(RuntimeError, match="eval forward"):
        model.infer_mc(torch.zeros(1, 1, 8, 8))
    model.eval()
    for head in (0, 3, True, 1.0):
        with pytest.raises(ValueError, match="head"):
            model.infer_mc(torch.zeros(1, 1, 8, 8), head=head)
    with pytest.raises(ValueError, match="samples"):
        model.infer_mc(torch.zeros(1, 1, 8, 8), samples=1)
    with pytest.raises(ValueError, match="p must"):
        model.infer_mc(torch.zeros(1, 1, 8, 8), p=0.0)
    for kw in (dict(tta="flips"), dict(ensemble=True)):
        scene = pkg.SceneInference(model, head=2, tile=64, **kw)
        with pytest.raises(ValueError, match="not the variance of the averaged map"):
            scene.uncertainty(torch.zeros(1, 1, 96, 112))


# ------------------------------------------------------------------------------------------- the oracle
def _random_samples(rng, k, n):
    """sigmoid-like float32 samples [k, n]: a per-pixel level with a spread that runs from almost none to the whole range"""
    level = rng.uniform(-6.0, 6.0, size=(1, n))
    spread = rng.uniform(0.0, 4.0, size=(1, n)) * rng.integers(0, 2, size=(1, n))
    z = level + spread * rng.standard_normal((k, n))
    return (1.0 / (1.0 + np.exp(-z))).astype(F32)


def _mutant_biased(s):                   # divides by K where K - 1 belongs
    mean, var = mo.fold(s)
    k = s.shape[0]
    return mean, (var * F32(k - 1)) / F32(k)


def _mutant_pairwise(s):                 # both sums as a pairwise tree instead of the left fold
    def tree(terms):
        terms = list(terms)
        while len(terms) > 1:
            terms = [terms[i] + terms[i + 1] if i + 1 < len(terms) else terms[i] for i in range(0, len(terms), 2)]
        return terms[0]
    k = s.shape[0]
    mean = tree(s[i] for i in range(k)) / F32(k)
    return mean, tree((s[i] - mean) * (s[i] - mean) for i in range(k)) / F32(k - 1)


def _mutant_about_s0(s):                 # deviations from the first sample instead of the mean
    mean, _ = mo.fold(s)
    k = s.shape[0]
    sq = (s[0] - s[0]) * (s[0] - s[0])
    for i in range(1, k):
        sq = sq + (s[i] - s[0]) * (s[i] - s[0])
    return mean, sq / F32(k - 1)


def _accept(fold):
    """What the oracle is held to: the stated order on hand-made samples (exact expected bits), and float64 inside the
    a-priori interval on random ones.  Raises AssertionError for a fold that computes anything else."""
    t = F32(2.0 ** -24)
    # the left fold leaves 1 alone three times (ties to even); any other association reaches 1 + 2^-23
    s = np.array([[1.0], [t], [t], [t]], dtype=F32)
    mean, var = fold(s)
    assert mean[0] == F32(0.25) and mean.dtype == F32
    d0, d1 = F32(0.75), F32(t - F32(0.25))
    want = F32(F32(F32(F32(d0 * d0) + F32(d1 * d1)) + F32(d1 * d1)) + F32(d1 * d1)) / F32(3.0)
    assert var[0] == F32(want), (var[0], want)
    # two samples (K - 1 = 1): every step written out in float32 scalars
    s = np.array([[F32(1.0)], [F32(2.0 ** -12)]], dtype=F32)
    mean, var = fold(s)
    m = F32(F32(F32(1.0) + F32(2.0 ** -12)) / F32(2.0))
    da, db = F32(F32(1.0) - m), F32(F32(2.0 ** -12) - m)
    assert mean[0] == m and var[0] == F32(F32(F32(da * da) + F32(db * db)) / F32(1.0))
    rng = np.random.default_rng(20240607)
    for k in (2, 3, 8, 32):
        s = _random_samples(rng, k, 4096)
        mean, var = fold(s)
        mean64, var64 = mo.fold64(s)
        b_mean, b_var = mo.bounds(s)
        assert np.all(np.abs(mean.astype(np.float64) - mean64) <= b_mean), k
        assert np.all(np.abs(var.astype(np.float64) - var64) <= b_var), k
        assert np.all(var >= 0)


def test_oracle_fold_is_the_stated_fold_and_close_to_float64():
    _accept(mo.fold)
    s = np.array([[0.25, np.nan, 0.5], [0.75, 0.5, np.inf]], dtype=F32)
    mean, var = mo.fold(s)
    assert mean[0] == F32(0.5) and var[0] == F32(0.125) and np.isnan(mean[1]) and np.isnan(var[1]) and np.isnan(var[2])
    assert mo.same_bits(np.array([np.nan, 1.0, 0.0], F32), np.array([-np.nan, 1.0, -0.0], F32)).tolist() == [True, True, False]


@pytest.mark.parametrize("mutant", [_mutant_biased, _mutant_pairwise, _mutant_about_s0])
def test_oracle_acceptance_rejects_planted_mutations(mutant):
    with pytest.raises(AssertionError):
        _accept(mutant)


def test_variance_interval_from_a_sample_tolerance():
    """var_tolerance(K, eps) covers samples moved by eps each (the GPU test's float64 comparison), and is no wider than a
    few eps: it would not cover a variance divided by K."""
    rng = np.random.default_rng(7)
    eps = 1e-4
    for k in (2, 3, 8, 32):
        s = _random_samples(rng, k, 2048).astype(np.float64)
        moved = np.clip(s + rng.uniform(-eps, eps, size=s.shape), 0.0, 1.0)
        _, var = mo.fold(moved.astype(F32))
        _, var64 = mo.fold64(s)
        assert np.all(np.abs(var - var64) <= mo.var_tolerance(k, eps + mo.U)), k
        assert mo.var_tolerance(k, eps) < 9 * eps
