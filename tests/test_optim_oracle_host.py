"""tests/optim_oracle.py on the CPU, before the GPU test leans on it:
  (1) fma32 against exact rational arithmetic (fractions.Fraction), on random triples and on constructed near-ties where a
      double-rounded float32(float64(a)*b + c) is wrong (asserted: the constructed set reaches that case);
  (2) the six reference fixtures (tests/golden/optim_*.npz, CPU runs of the reference's optimizers): with aten's CPU sqrt
      injected the driver reproduces every recorded element, parameters and state, bit for bit; with numpy's (correctly
      rounded) sqrt every state element still does, and the parameters that differ are counted and printed -- that count
      is a property of the torch build's sqrt, the only op of the sequence aten does not round correctly;
  (3) the branches the fixtures lack (non-default betas / eps / final_lr / gamma, dampening, a moved lr, large step
      counts, the clip multiply), on a whole 100 003-element tensor: the oracle with aten's sqrt against the same update
      written as torch CPU tensor ops in the reference's op order, bit-equal on every element.
"""
import importlib.util
import math
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import optim_oracle as oo

F32, F64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _torch_sqrt(x):
    return torch.from_numpy(np.ascontiguousarray(x)).sqrt().numpy()


# ---- 1. fma32 --------------------------------------------------------------------------------------------------------
def _round_fraction_to_f32(x):
    """The float32 nearest the Fraction x, ties to even (finite results only), by integer arithmetic."""
    if x == 0:
        return F32(0.0)
    sign, x = (-1, -x) if x < 0 else (1, x)
    e = x.numerator.bit_length() - x.denominator.bit_length()       # 2^(e-1) <= x < 2^(e+1)
    if Fraction(2) ** e > x:
        e -= 1                                                      # 2^e <= x < 2^(e+1)
    q = max(e, -126) - 23                                           # the ulp exponent (denormals: fixed at -149)
    scaled = x / Fraction(2) ** q
    n = scaled.numerator // scaled.denominator
    rem = scaled - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    assert n <= 2 ** 24
    return F32(sign * math.ldexp(n, q))                             # n * 2^q is a float32 (or the next binade's first)


def _exact_fma(a, b, c):
    return _round_fraction_to_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def _naive_fma(a, b, c):
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def _random_triples(n, seed):
    rng = np.random.default_rng(seed)

    def draw():
        mant = rng.uniform(1.0, 2.0, n) * rng.choice([-1.0, 1.0], n)
        return (mant * 2.0 ** rng.integers(-40, 21, n)).astype(F32)
    a, b, c = draw(), draw(), draw()
    # half of the addends at the product's own magnitude, where cancellation and ties live
    near = rng.random(n) < 0.5
    c = np.where(near, (a.astype(F64) * b.astype(F64) * rng.uniform(-2.0, 2.0, n)).astype(F32), c)
    return a, b, c


def _near_tie_triples(n, seed):
    """a*b + c at or next to a float32 midpoint h, two families of n/2:
    generic a, b: h = the midpoint above float32(a*b * k) for a small k, c = float32(h - a*b) nudged by -2 .. 2 float32
        ulps -- exact ties (h - a*b often fits 24 bits) and sums a few float64 ulps beside one;
    short a, b (12 and 13 significant bits, both odd, a 25-bit product): a*b IS a float32 midpoint h, so float32(h - a*b)
        is 0 and the nudged c is a tiny non-zero number of either sign, down to the denormals: a*b + c is then not a
        float64, float64 arithmetic rounds it back onto the tie and ties-to-even forgets which side it was on."""
    rng = np.random.default_rng(seed)
    m = n // 2
    a = (rng.uniform(1.0, 2.0, m) * 2.0 ** rng.integers(-20, 11, m)).astype(F32)
    b = (rng.uniform(1.0, 2.0, m) * rng.choice([-1.0, 1.0], m) * 2.0 ** rng.integers(-20, 11, m)).astype(F32)
    p = a.astype(F64) * b.astype(F64)
    target = (p * rng.choice([1.0, 1.5, 3.0, 17.0, 1025.0], m)).astype(F32)      # the sum's magnitude
    h = target.astype(F64) + 0.5 * np.spacing(target).astype(F64)                # midpoint of target and its neighbour
    c = (h - p).astype(F32)
    for _ in (1, 2):
        nudge = rng.integers(-1, 2, m)
        c = np.where(nudge > 0, np.nextafter(c, F32(np.inf)), np.where(nudge < 0, np.nextafter(c, F32(-np.inf)), c))
    ia = rng.integers(2 ** 10, 2 ** 11, 4 * m) * 2 + 1                           # odd, 12 bits
    ib = rng.integers(2 ** 11, 2 ** 12, 4 * m) * 2 + 1                           # odd, 13 bits
    keep = np.nonzero(ia * ib >= 2 ** 24)[0][:m]                                 # odd and 25 bits: a midpoint
    assert keep.size == m
    sa, sb = rng.integers(-30, 11, m), rng.integers(-30, 11, m)
    a2 = (ia[keep] * 2.0 ** sa).astype(F32)
    b2 = (ib[keep] * rng.choice([-1.0, 1.0], m) * 2.0 ** sb).astype(F32)
    shift = rng.integers(30, 90, m)
    c2 = (rng.choice([-1.0, 1.0], m) * rng.uniform(1.0, 2.0, m) * 2.0 ** (24.0 + sa + sb - shift)).astype(F32)
    return np.concatenate([a, a2]), np.concatenate([b, b2]), np.concatenate([c, c2]).astype(F32)


def test_fma32_is_correctly_rounded():
    a, b, c = _random_triples(20000, 7)
    got = oo.fma32(a, b, c)
    assert got.dtype == F32
    want = np.array([_exact_fma(*t) for t in zip(a, b, c)], dtype=F32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    naive_wrong_random = int((_naive_fma(a, b, c).view(np.uint32) != want.view(np.uint32)).sum())

    a, b, c = _near_tie_triples(4000, 8)
    got = oo.fma32(a, b, c)
    want = np.array([_exact_fma(*t) for t in zip(a, b, c)], dtype=F32)
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert bad.size == 0, [(float(a[i]).hex(), float(b[i]).hex(), float(c[i]).hex()) for i in bad[:3]]
    naive_wrong = int((_naive_fma(a, b, c).view(np.uint32) != want.view(np.uint32)).sum())
    print("naive double-rounded fma wrong on %d of 20000 random and %d of 4000 near-tie triples"
          % (naive_wrong_random, naive_wrong))
    assert naive_wrong >= 1          # the constructed set reaches the double-rounding case


def test_fma32_special_values():
    inf, nan = F32(np.inf), F32(np.nan)
    assert oo.fma32(F32(3e19), F32(3e19), F32(1.0)) == inf                       # overflow of the product itself
    assert oo.fma32(inf, F32(2.0), F32(1.0)) == inf and oo.fma32(F32(1.0), F32(2.0), -inf) == -inf
    assert np.isnan(oo.fma32(inf, F32(0.0), F32(1.0))) and np.isnan(oo.fma32(nan, F32(1.0), F32(1.0)))
    z = oo.fma32(F32(-0.0), F32(-0.0), F32(0.0))
    assert z == 0 and not np.signbit(z)
    d = oo.fma32(F32(1e-23), F32(1e-20), F32(0.0))                               # a float32 denormal
    assert 0 < d < np.finfo(F32).tiny and d == _exact_fma(F32(1e-23), F32(1e-20), F32(0.0))
    assert oo.fma32(np.zeros(0, F32), F32(1.0), np.zeros(0, F32)).shape == (0,)


def test_update_second_moment_overflow():
    """update()'s v = fma((1-b2)*g, g, v*b2), not (1-b2)*(g*g): at the default b2 a gradient of 3e19 leaves v finite
    (9e35) and 1e21 makes it +inf; it then stays +inf, denom is +inf and the parameter does not move (AdamW) or moves by
    the lower bound times m (AdaBound) -- no NaN anywhere."""
    g = np.array([3e19, 1e21], dtype=F32)
    for kind, ams in ((oo.ADAMW, False), (oo.ADAMW, True), (oo.ADABOUND, False), (oo.ADABOUND, True)):
        drv = oo.Driver(kind, [dict()], [np.array([0.5, 0.5], dtype=F32)], [0], ams=ams)
        for step in (1, 2):
            drv.step([g if step == 1 else np.zeros(2, F32)])
            st = drv.state[0]
            vs = [st[k] for k in st if k != "exp_avg"]
            assert all(np.isfinite(v[0]) and v[1] == np.inf for v in vs), (kind, ams, step, vs)
            assert np.isfinite(st["exp_avg"]).all() and np.isfinite(drv.params[0]).all()
        if kind == oo.ADAMW:
            assert drv.params[0][1] == F32(0.5)                                  # p + (-step*m)/inf = p
        else:
            assert drv.params[0][1] < F32(-1e15)                                 # p - clamp(step/inf = 0, lo, hi)*m


def test_clip_coef():
    assert oo.clip_coef(F32(1000.0), 8.0) == F32(8.0) / (F32(1000.0) + F32(1e-6))
    assert oo.clip_coef(F32(1.0), 8.0) == F32(1.0)
    assert oo.clip_coef(F32(np.inf), 8.0) == F32(0.0)
    assert np.isnan(oo.clip_coef(F32(np.nan), 8.0))
    assert oo.clip_coef(F32(0.0), 8.0) == F32(1.0)


# ---- 2. the reference's fixtures ----------------------------------------------------------------------------------------
_spec = importlib.util.spec_from_file_location("make_optim_golden", os.path.join(GOLDEN, "make_optim_golden.py"))
gm = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gm)
FIXTURE_KIND = {"AdamW": oo.ADAMW, "AdaBound": oo.ADABOUND, "SGDW": oo.SGDW}


@pytest.fixture(scope="module")
def fixture_inputs():
    return gm.make_inputs(gm.shapes())


def _run_fixture(name, inputs, sqrt):
    """The fixture's own loop (two groups at lr and lr/2, MultiStepLR([3], 0.1) after every step) through the driver ->
    (differing parameter elements, differing state elements, recorded elements)."""
    params0, grads = inputs
    cls_name, kw = gm.CONFIGS[name]
    kind = FIXTURE_KIND[cls_name]
    common = {k: v for k, v in kw.items() if k not in ("lr", "amsgrad", "amsbound", "nesterov")}
    lrs = gm.group_lrs(kw["lr"])
    drv = oo.Driver(kind, [dict(common, lr=lrs[0]), dict(common, lr=lrs[1])], params0,
                    [i % 2 for i in range(len(params0))], ams=kw.get("amsgrad", False) or kw.get("amsbound", False),
                    sqrt=sqrt)
    z = np.load(os.path.join(GOLDEN, "optim_%s.npz" % name))
    bad_p = bad_s = total = 0
    for step in range(1, gm.STEPS + 1):
        drv.step(grads[step - 1])
        if step == 3:                                   # MultiStepLR(milestones=[3], gamma=0.1), stepped after opt.step()
            for g in drv.groups:
                g["lr"] = g["lr"] * 0.1
        if step not in gm.RECORD:
            continue
        for i, p in enumerate(drv.params):
            idx = gm.sample_index(p.size)
            want = z["s%d/param/%d" % (step, i)]
            bad_p += int((p.reshape(-1)[idx].view(np.uint32) != want.view(np.uint32)).sum())
            total += want.size
            for k in gm.STATE_KEYS:
                key = "s%d/%s/%d" % (step, k, i)
                assert (key in z) == (k in drv.state[i]), (name, step, i, k)
                if key in z:
                    got = drv.state[i][k].reshape(-1)[idx]
                    bad_s += int((got.view(np.uint32) != z[key].view(np.uint32)).sum())
                    total += z[key].size
            want_step = int(z["s%d/step/%d" % (step, i)])
            if want_step >= 0:
                assert drv.count[i] == want_step, (name, step, i)
    return bad_p, bad_s, total


@pytest.mark.parametrize("name", list(gm.CONFIGS))
def test_reproduces_reference_fixture(name, fixture_inputs):
    bad_p, bad_s, total = _run_fixture(name, fixture_inputs, _torch_sqrt)
    assert (bad_p, bad_s) == (0, 0), (name, bad_p, bad_s, total)
    bad_p, bad_s, total = _run_fixture(name, fixture_inputs, np.sqrt)
    print("%s: with the correctly rounded sqrt %d of %d recorded values differ (parameters only)" % (name, bad_p, total))
    assert bad_s == 0, (name, bad_s)


# ---- 3. branches the fixtures lack, on whole tensors --------------------------------------------------------------------
N_WHOLE = 100003
OVERFLOW_AT = 7
T_SEQUENCE = (1, 2, 3, 1000, 100000)


def _torch_step(kind, ams, group, base_lr, p, g, st, t):
    """One update of one tensor as torch CPU ops in the reference's op order (in place on p and st)."""
    if kind == oo.SGDW:
        if group["momentum"] != 0:
            if "momentum_buffer" not in st:
                st["momentum_buffer"] = torch.zeros_like(p)
                st["momentum_buffer"].mul_(group["momentum"]).add_(g)
            else:
                st["momentum_buffer"].mul_(group["momentum"]).add_(g, alpha=1 - group["dampening"])
        if group["weight_decay"] != 0:
            p.add_(p, alpha=-group["weight_decay"])
        return
    if not st:
        st["exp_avg"], st["exp_avg_sq"] = torch.zeros_like(p), torch.zeros_like(p)
        if ams:
            st["max_exp_avg_sq"] = torch.zeros_like(p)
    m, v = st["exp_avg"], st["exp_avg_sq"]
    b1, b2 = group["betas"]
    if kind == oo.ADABOUND and group["weight_decay"] != 0:
        g = g.add(p, alpha=group["weight_decay"])
    m.mul_(b1).add_(g, alpha=1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    if ams:
        torch.max(st["max_exp_avg_sq"], v, out=st["max_exp_avg_sq"])
        denom = st["max_exp_avg_sq"].sqrt().add_(group["eps"])
    else:
        denom = v.sqrt().add_(group["eps"])
    step_size = group["lr"] * math.sqrt(1 - b2 ** t) / (1 - b1 ** t)
    if kind == oo.ADAMW:
        if group["weight_decay"] != 0:
            d = torch.mul(p, group["weight_decay"])
            p.addcdiv_(m, denom, value=-step_size)
            p.sub_(d)
        else:
            p.addcdiv_(m, denom, value=-step_size)
    else:
        f = group["final_lr"] * group["lr"] / base_lr
        lo, hi = f * (1 - 1 / (group["gamma"] * t + 1)), f * (1 + 1 / (group["gamma"] * t))
        s = torch.full_like(denom, step_size)
        s.div_(denom).clamp_(lo, hi).mul_(m)
        p.add_(-s)


def _whole_inputs():
    rng = np.random.default_rng(424242)
    p0 = (0.1 * rng.standard_normal(N_WHOLE)).astype(F32)
    grads = [(10.0 ** rng.uniform(-3, 1) * rng.standard_normal(N_WHOLE)).astype(F32) for _ in T_SEQUENCE]
    for g in grads:
        g[:7] = [0.0, -0.0, 1e-20, 3e-20, 1e-3, -2.5, 7.0]           # zeros and a denormal second moment
        g[OVERFLOW_AT] = 1e21                                        # (1-b2)*g*g >= 1e39: v = +inf from the first step on
    return p0, grads


WHOLE = _whole_inputs()


WHOLE_CASES = [(name, which, False) for name in oo.CONFIGS for which in (0, 1)]
WHOLE_CASES += [(name, which, True) for name in oo.CLIPPED for which in (0, 1)]       # one configuration per kind


@pytest.mark.parametrize("name,which,clipped", WHOLE_CASES,
                         ids=["%s-group%s%s" % (n, "AB"[w], "-clipped" if c else "") for n, w, c in WHOLE_CASES])
def test_oracle_equals_torch_ops_on_whole_tensor(name, which, clipped):
    kind, ams, ga, gb, lr_moves = oo.CONFIGS[name]
    group = oo.group_kwargs(kind, (ga, gb)[which])
    p0, grads = WHOLE
    drv = oo.Driver(kind, [group], [p0], [0], ams=ams, sqrt=_torch_sqrt)
    tgroup = dict(drv.groups[0])
    base_lr = tgroup["lr"]
    p, st = torch.from_numpy(p0.copy()), {}
    coef = oo.clip_coef(F32(731.25), 8.0) if clipped else None
    for k, t in enumerate(T_SEQUENCE):
        if drv.count[0] is not None:
            drv.count[0] = t - 1
        g = torch.from_numpy(grads[k].copy())
        if clipped:
            g = g * float(coef)                                       # one fp32 multiply by torch (coef is a float32 value)
        with np.errstate(all="ignore"):
            drv.step([grads[k]], coef=coef)
        _torch_step(kind, ams, tgroup, base_lr, p, g, st, t)
        assert np.array_equal(drv.params[0].view(np.uint32), p.numpy().view(np.uint32)), (name, t, "param")
        assert set(drv.state[0]) == set(st), (name, t)
        for key in st:
            assert np.array_equal(drv.state[0][key].view(np.uint32), st[key].numpy().view(np.uint32)), (name, t, key)
            if key in ("exp_avg_sq", "max_exp_avg_sq") and not clipped:       # (clipped: 1e21 * 0.011, v stays finite)
                assert float(st[key][OVERFLOW_AT]) == math.inf and drv.state[0][key][OVERFLOW_AT] == np.inf, (name, t, key)
        if (k + 1) in lr_moves:
            drv.groups[0]["lr"] = tgroup["lr"] = tgroup["lr"] * lr_moves[k + 1]
    if kind != oo.SGDW or group["weight_decay"] != 0:
        assert not np.array_equal(drv.params[0], p0)                  # the step did something
