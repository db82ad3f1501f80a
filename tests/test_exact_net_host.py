"""Preconditions of tests/test_gpu_exact_net.py, asserted on the float64 reference alone (CPU only): conditions on the
data of tests/exact_net.py, not tolerances.

* the hand-made reference equals autograd on oracle/unet_nested_oracle.py in float64, bit for bit;
* bf16 cases: every tensor the engine stores -- the node gradients after each of their read-modify-writes included -- has
  at most 8 significant bits, and so has every element of the same backward run on absolute values (the sum of the
  absolute contributions); fp32 cases: that sum and helpers.wino_magnitude, in units of the data's granule (the largest
  power of two dividing every stored value), stay below 2^22, the margin of tests/test_gemm_oracle_host.py;
* the data exercises the schedule: real gates, real pool ties, no dead parameter, no dead contribution;
* every error of the schedule the GPU test is meant to catch changes a compared tensor (the mutations below);
* unetpp_bn_eval_coeffs restated in numpy float32 gives exactly the intended dyadic scale and shift.

The seeds in exact_net.CASES are 7919 * k + n for the k-th searched case, n counted up from 0 until every assertion of
this file held for the case.
"""
import json

import numpy as np
import pytest
import torch

from oracle.unet_nested_oracle import UNetNestedOracle
from tests import exact_net as en

CUTS = [(c, norm, top) for c in en.CASES for norm in c.norms for top in [None] + list(range(1, c.ctor["depth"] - 1))]
CUT_IDS = ["%s-%s-%s" % (c.id, norm, "whole" if top is None else "head%d" % top) for c, norm, top in CUTS]


def test_the_table_covers_what_it_must():
    depths = {c.ctor["depth"] for c in en.CASES}
    assert depths == {2, 3, 4, 5}
    assert {c.ctor["in_channels"] for c in en.CASES} == {1, 3}
    for dtype in (False, True):
        for norm in en.NORMS:
            assert {c.ctor["depth"] for c in en.CASES if c.bf16 == dtype and norm in c.norms} >= {3, 4, 5}
    smallest = [c for c in en.CASES if (c.h >> (c.ctor["depth"] - 1), c.w >> (c.ctor["depth"] - 1)) in ((1, 1), (1, 2))]
    assert smallest and any(c.bf16 for c in smallest) and any(not c.bf16 for c in smallest)
    for c in en.CASES:
        m = 1 << (c.ctor["depth"] - 1)
        assert c.h % m == 0 and c.w % m == 0 and c.batch * c.h * c.w <= 2 * 32 * 32 and c.ctor["is_deconv"]
        if c.bf16:
            assert all(f % 8 == 0 and (f // 8) & (f // 8 - 1) == 0 for f in en.widths(c)) and c.ctor["in_channels"] <= 4
    assert en.CASE_BY_ID[en.EXTRA_CASE].ctor["depth"] == 4


@pytest.mark.parametrize("case,norm,top", CUTS, ids=CUT_IDS)
def test_reference_is_autograd_on_the_oracle(case, norm, top):
    """The oracle in eval mode (dropout off); its frozen BatchNorm layers get running_var = 1 - 2^-53 and eps = 2^-53, whose
    float64 sum is exactly 1, so that the module computes the intended dyadic map.  torch's max-pool backward routes to the
    first maximum, as the project does."""
    state, x, G, r = en.cached(case, norm, top, True)
    ref = UNetNestedOracle(**dict(case.ctor, is_batchnorm=norm != "none")).double().eval()
    ref.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in state.items()})
    for m in ref.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.eps = 2.0 ** -53
            m.running_var.fill_(1.0 - 2.0 ** -53)
            assert float(m.running_var[0]) < 1.0 and float(m.running_var[0] + m.eps) == 1.0
    seen = {}
    for j in range(1, case.ctor["depth"]):
        getattr(ref, "final_%d" % j).register_forward_pre_hook(lambda mod, args, j=j: seen.__setitem__(j, args[0]))
    x64 = x.double().requires_grad_(True)
    ref(x64)
    for j in range(1, r.top + 1):
        assert torch.equal(seen[j], r.X[(0, j)]), j
    sum((seen[j] * G[j]).sum() for j in range(1, r.top + 1)).backward()
    assert torch.equal(x64.grad, r.dx)
    want = dict(ref.named_parameters())
    names = en.body_names(case, "bn" if norm != "none" else "none", top)
    for n in names:
        if norm == "bn_affine" and ".1." in n:
            assert n not in r.grads
            continue
        assert torch.equal(want[n].grad, r.grads[n]), n
    assert sorted(r.grads) == sorted(en.body_names(case, norm, top))


@pytest.mark.parametrize("case,norm,top", CUTS, ids=CUT_IDS)
def test_preconditions(case, norm, top):
    m = en.measure(case, norm, top)
    print("exact-net:", json.dumps(dict(case=case.id, norm=norm, top=top, **m)))
    if case.bf16:
        assert m["bits"] <= 8, m
        assert m["bits_abs"] <= 8, m
    else:
        assert m["bits"] <= 24 and m["abs_max"] / m["granule"] < 2 ** 22 and m["wino_max"] / m["granule"] < 2 ** 22, m
    assert not m["zero_grads"], m["zero_grads"]
    assert m["dx_nonzero"]
    assert 0.30 <= m["zero_share"] <= 0.80, m
    assert m["ties"] >= 20, m
    assert m["live_contribs"] >= 2, m


# ----------------------------------------------------------------------------------------------- sensitivity
def sites(r):
    """every place of the schedule where one of the named errors can be made, for the reference r"""
    out = []
    for key, cs in r.contribs.items():
        for name, _ in cs:
            out.append(("no_pool", key) if name == "pool" else ("drop", key, name))
            out.append(("twice", key, name))
        if len(cs) > 1:
            out.append(("early_mask", key))
        out.append(("no_mask", key))
        skips = [int(name[4:]) for name, _ in cs if name.startswith("skip")]
        for a, b in zip(skips, skips[1:]):
            out.append(("swap", key, a, b))
    if r.top >= 1:
        out.append(("tie_last",))
    return out


def compared(r, names, winners=True):
    out = [r.grads[n] for n in names] + [r.dx]
    if winners:
        out += [p["idx"].double() for p in r.pairs.values() if p["idx"] is not None]
    return out


@pytest.mark.parametrize("case,norm,top", CUTS, ids=CUT_IDS)
def test_every_named_error_changes_a_compared_tensor(case, norm, top):
    state, x, G, r = en.cached(case, norm, top, True)
    names = en.body_names(case, norm, top)
    true = compared(r, names)
    kinds, silent = set(), []
    for site in sites(r):
        mutation = ("drop", site[1], "pool") if site[0] == "no_pool" else site
        m = en.reference(case, norm, state, x, G, top, True, mutation=mutation,
                         forward=None if site[0] == "tie_last" else r)
        kinds.add(site[0])
        if all(torch.equal(a, b) for a, b in zip(true, compared(m, names))):
            silent.append(site)
    assert not silent, silent
    want = {"drop", "twice", "no_mask", "tie_last", "no_pool", "early_mask"}
    if r.top >= 2:
        want.add("swap")
    assert kinds == want, kinds


# ----------------------------------------------------------------------------------------------- coefficients
@pytest.mark.parametrize("case", en.CASES, ids=[c.id for c in en.CASES])
def test_float32_coefficients_are_the_intended_dyadic_numbers(case):
    assert np.float32(0.99999) + np.float32(en.EPS) == np.float32(1.0)
    if "bn" not in case.norms:
        return
    state, _, _ = en.make_data(case, "bn")
    layers = [k[:-len(".running_var")] for k in state if k.endswith(".running_var")]
    assert len(layers) == 2 * case.ctor["depth"]
    for pre in layers:
        scale, shift, invstd = en.coeffs_float32(state, pre)
        want_scale, want_shift, _ = en.intended_coeffs(state, pre)
        assert (invstd == 1.0).all()
        assert np.array_equal(scale.astype(np.float64), want_scale.numpy()), pre
        assert np.array_equal(shift.astype(np.float64), want_shift.numpy()), pre
        assert set(np.unique(scale)) <= {0.5, 1.0, 2.0}
