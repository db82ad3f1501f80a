"""Monte-Carlo dropout fold (csrc/heads.hip head_mc_kernel, ops.head_mc) restated in numpy float32, its float64 reference
and the a-priori intervals between them.  Shared by tests/test_head_mc_host.py and tests/test_gpu_head_mc.py (test
infrastructure; no GPU here).

The rule, per pixel and class over K >= 2 float32 samples s_0 .. s_{K-1} (sigmoid values, so 0 <= s_k <= 1):
    sum  = ((s_0 + s_1) + ...) + s_{K-1}                     a left fold, K - 1 float32 additions
    mean = sum / float32(K)                                   one float32 division
    d_k  = s_k - mean                                         one float32 subtraction each
    sq   = ((d_0 d_0 + d_1 d_1) + ...) + d_{K-1} d_{K-1}      K float32 products, each rounded, then a left fold
    var  = sq / float32(K - 1)                                one float32 division (the unbiased estimate)
No fused multiply-add anywhere: every product, sum and quotient is rounded to nearest-even on its own, which is what numpy
does with float32 arrays.  The kernel starts both folds from +0 (0 + s_0 and 0 + d_0 d_0): neither a sigmoid nor a square
is ever -0, so that first addition returns its operand.

Error model against float64 on the same float32 samples, u = 2^-24, gamma_n = n u / (1 - n u) (tests/helpers.gamma):
  mean.  K - 1 additions and one division of non-negative terms:  |mean - mean*| <= gamma_K mean* =: E_m.
  d_k.   d_k = (s_k - mean)(1 + delta), |delta| <= u, against d*_k = s_k - mean*:
             |d_k - d*_k| <= E_m + u (|d*_k| + E_m) =: e_k.
  d_k^2. |d_k^2 - d*_k^2| = |d_k - d*_k| |d_k + d*_k| <= e_k (2 |d*_k| + e_k).
  var.   K rounded products, K - 1 additions, one division of non-negative terms: a relative gamma_{K+1} on
         sum_k d_k^2 <= sum_k (|d*_k| + e_k)^2.  Together
             |var - var*| <= [ sum_k e_k (2 |d*_k| + e_k) + gamma_{K+1} sum_k (|d*_k| + e_k)^2 ] / (K - 1).
  Results below the normal range of float32 round absolutely: ABS_FLOOR = 2^-140 is added to both intervals.

When the samples themselves are only known to within eps of their float64 values (the GPU test against float64:
eps = the tolerance head_fwd is held to), each d_k moves by at most 2 eps (eps from s_k, eps from the mean) and
|d_k| <= 1 because every sample lies in [0, 1]:
             |d_k^2 - d*_k^2| <= 2 eps (2 |d*_k| + 2 eps) <= 4 eps + 4 eps^2,
and the float32 fold adds at most gamma_{K+1} sum_k d_k^2 <= gamma_{K+1} K.  Hence var_tolerance(K, eps)
             |var - var*| <= K / (K - 1) (4 eps + 4 eps^2 + gamma_{K+1}),
the mean moving by at most eps + gamma_K.
"""
import numpy as np

from tests.helpers import gamma

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
ABS_FLOOR = 2.0 ** -140
MAX_SAMPLES = 32                       # UNETPP_MC_MAX_SAMPLES
SEED_STEP = 0xD6E8FEB86659FD93         # sample k draws from seed + SEED_STEP * k (mod 2^64)
HEAD_SEED_STEP = 0x632BE59BD9B4E019    # infer_mc: head J draws from seed + HEAD_SEED_STEP * J
CHUNK_SEED_STEP = 0xA0761D6478BD642F   # scene.uncertainty: chunk i draws from seed + CHUNK_SEED_STEP * (i + 1)
MASK64 = 0xFFFFFFFFFFFFFFFF


def sample_seeds(seed, samples):
    return [(int(seed) + SEED_STEP * k) & MASK64 for k in range(samples)]


def fold(samples):
    """samples: float32 [K, ...] -> (mean, var) float32 [...], the rule above in explicit float32 operations."""
    s = np.asarray(samples)
    assert s.dtype == F32 and s.shape[0] >= 2, (s.dtype, s.shape)
    k = s.shape[0]
    with np.errstate(all="ignore"):
        total = s[0].copy()
        for i in range(1, k):
            total = total + s[i]
        mean = total / F32(k)
        d = s[0] - mean
        sq = d * d
        for i in range(1, k):
            d = s[i] - mean
            sq = sq + d * d
        var = sq / F32(k - 1)
    assert mean.dtype == F32 and var.dtype == F32
    return mean, var


def fold64(samples):
    """The same statistics in float64 on the given samples: the mean and the unbiased variance."""
    s = np.asarray(samples, dtype=F64)
    mean = s.mean(axis=0)
    var = ((s - mean) ** 2).sum(axis=0) / (s.shape[0] - 1)
    return mean, var


def bounds(samples):
    """A-priori (mean bound, var bound) per element for fold() against fold64() on the same float32 samples in [0, 1]."""
    s = np.asarray(samples, dtype=F64)
    k = s.shape[0]
    mean, _ = fold64(s)
    e_m = gamma(k) * np.abs(mean)
    d = np.abs(s - mean)
    e = e_m + U * (d + e_m)
    num = (e * (2.0 * d + e)).sum(axis=0) + gamma(k + 1) * ((d + e) ** 2).sum(axis=0)
    return e_m + ABS_FLOOR, num / (k - 1) + ABS_FLOOR


def var_tolerance(k, eps):
    """|var - var*| when every sample lies in [0, 1] and within eps of its float64 value (docstring)."""
    return k / (k - 1.0) * (4.0 * eps + 4.0 * eps * eps + gamma(k + 1))


def same_bits(got, want):
    """bool array: equal as int32 views, two NaNs counting as equal."""
    got, want = np.ascontiguousarray(got, dtype=F32), np.ascontiguousarray(want, dtype=F32)
    return (got.view(np.int32) == want.view(np.int32)) | (np.isnan(got) & np.isnan(want))
