"""The whole network, forward and backward, against the float64 reference of tests/exact_net.py on data where every value
the engine computes is exact in fp32 and in bf16 storage: every comparison is equality.  What makes the data exact is
asserted on the reference alone by tests/test_exact_net_host.py; that file also shows that a dropped or doubled
gradient contribution, an early or missing ReLU mask, a pool gradient sent to the last maximum or left out, and two
swapped slices of a grouped weight each change a tensor compared here.

Forward: ``engine.forward_impl(..., save=True)``; every saved tensor, the pool winners and the frozen BatchNorm
coefficients are compared.  Backward: ``engine.backward_impl`` with ``saved.head_train = {j: (G_j, dummy, dummy)}`` -- the
seam production uses after ops.head_train (``_GradBook.preset``) -- so the loss is sum_j <X[0][j], G_j> and the heads stay
out of it.  ``test_the_seam_is_the_production_path`` ties that seam to ``model(x)`` + ``backward()``.

Outside this file's exact coverage, still judged by the existing bounds: training-mode BatchNorm, the bilinear up path,
the heads and losses, the ensemble backward.
"""
import pytest
import torch

from tests import exact_net as en
from tests.helpers import usable_cus

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
ROWS = [(c, norm, grouped) for c in en.CASES for norm in c.norms for grouped in (True, False)]
ROW_IDS = ["%s-%s-%s" % (c.id, norm, "grouped" if g else "per-consumer") for c, norm, g in ROWS]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def build_model(case, norm, dev):
    from unet_nested4tiny_objects_keypoints_amd import UNet_Nested
    state, _, _ = en.cached(case, norm)[:3]
    m = UNet_Nested(**dict(case.ctor, is_batchnorm=norm != "none"))
    m.load_state_dict(state)
    m = m.to(dev).train()
    if case.bf16:
        m.set_activation_dtype(BF)
    m.drop_out.eval()
    if norm != "none":
        m.freeze_batchnorm(True, affine=norm == "bn_affine")
    return m


def nhwc64(t):
    return t.permute(0, 2, 3, 1).contiguous()


def same(dev_t, ref_nchw, what, bad):
    got = dev_t.detach().double().cpu()
    want = nhwc64(ref_nchw)
    if got.shape != want.shape or not torch.equal(got, want):
        n = int((got != want).sum()) if got.shape == want.shape else -1
        bad.append((what, "shape %s vs %s" % (tuple(got.shape), tuple(want.shape)) if n < 0 else "%d elements differ" % n))


def check_forward(case, norm, m, saved, r, state, bad):
    adt = BF if case.bf16 else torch.float32
    assert set(saved.X) == set(r.X) and set(saved.pairs) == set(r.X) and set(saved.ups) == set(r.ups)
    assert saved.top == r.top
    for key in r.X:   # forward order: the first tensor listed is the first that went wrong
        rec, p = saved.pairs[key], r.pairs[key]
        lab = "%d%d" % key
        if key in saved.ups:
            assert saved.ups[key].up.dtype == adt
            same(saved.ups[key].up, r.ups[key], "up" + lab, bad)
        for name in ("y1", "a1", "y2", "out", "pooled"):
            t = getattr(rec, name)
            if t is None:
                continue
            assert p[name] is not None and t.dtype == adt, (name, key)
            same(t, p[name], name + lab, bad)
        assert rec.out is saved.X[key]
        if norm == "none" or key[1] > 0:   # no BatchNorm: both stages store their ReLU output only
            assert rec.a1 is not None and rec.y1 is None and rec.y2 is None, key
        else:
            assert rec.y1 is not None and rec.y2 is not None, key
        same(saved.X[key], r.X[key], "X" + lab, bad)
        assert (rec.pool_idx is not None) == (p["idx"] is not None), key
        if rec.pool_idx is not None:
            same(rec.pool_idx, p["idx"].double(), "winners" + lab, bad)
        if norm != "none" and key[1] == 0:
            for stage, coeffs, frozen in ((1, rec.bn1, rec.frozen1), (2, rec.bn2, rec.frozen2)):
                assert frozen
                scale, shift, mean = en.intended_coeffs(state, "%s.conv%d.1" % (en.pair_prefix(*key), stage))
                if not (torch.equal(coeffs[2].double().cpu(), scale) and torch.equal(coeffs[3].double().cpu(), shift)):
                    bad.append(("bn%d coefficients %s" % (stage, lab), "not the dyadic numbers"))
                if coeffs[0] is not None:
                    assert torch.equal(coeffs[0].double().cpu(), mean), key
                    assert bool((coeffs[1] == 1.0).all()), key


class Sink:
    def __init__(self):
        self.got = []

    def __call__(self, pairs):
        self.got += [(p, None if g is None else g.clone()) for p, g in pairs]


def seam_gradients(case, saved, r, G, dev):
    """{j: (dX_0j, dW, db)}: G_j in the storage type and layout of X[0][j], masked with X[0][top] > 0 for the last head"""
    out = {}
    for j in range(1, r.top + 1):
        g = G[j] * (r.X[(0, j)] > 0) if j == r.top else G[j]
        t = nhwc64(g).to(saved.X[(0, j)].dtype).to(dev)
        assert t.shape == saved.X[(0, j)].shape and t.is_contiguous()
        out[j] = (t, None, None)
    return out


def run_case(case, norm, m, dev, top, want_dx, bad, forward_checked):
    from unet_nested4tiny_objects_keypoints_amd import engine
    d = case.ctor["depth"]
    ref_top = None if top in (None, d - 1) else top
    state, x, G, r = en.cached(case, norm, ref_top, True)
    tag = "%s/dx=%d" % ("whole" if top is None else "head%d" % top, want_dx)
    kw = {} if top is None else dict(head=top, all_heads=True)
    outs, saved = engine.forward_impl(m, x.to(dev), training=True, save=True, **kw)
    assert len(outs) == r.top and saved.head_train is None
    if top not in forward_checked:
        forward_checked.add(top)
        n0 = len(bad)
        check_forward(case, norm, m, saved, r, state, bad)
        bad[n0:] = [(tag,) + b for b in bad[n0:]]
        if len(bad) > n0:
            return   # the backward of a wrong forward says nothing more
    heads = {j: getattr(m, "final_%d" % j) for j in range(1, r.top + 1)}
    saved.head_train = {j: (t, torch.zeros_like(heads[j].weight), torch.zeros_like(heads[j].bias))
                        for j, (t, _, _) in seam_gradients(case, saved, r, G, dev).items()}
    sink = Sink()
    grads, dx = engine.backward_impl(m, saved, [None] * len(outs), want_dx, sink)
    torch.cuda.synchronize()
    name_of = {p: n for n, p in m.named_parameters()}
    body = en.body_names(case, "bn" if norm != "none" else "none", ref_top)
    expected = set(body) | {"final_%d.%s" % (j, s) for j in heads for s in ("weight", "bias")}
    assert {name_of[p] for p in grads} == expected, tag
    by_name = {name_of[p]: g for p, g in grads.items()}
    for n in body:   # backward order of the reference is the order of r.grads
        g = by_name[n]
        if norm == "bn_affine" and ".1." in n:
            if g is not None:
                bad.append((tag, n, "a frozen gamma / beta received a gradient"))
            continue
        if g is None or g.dtype != torch.float32 or not torch.equal(g.double().cpu(), r.grads[n]):
            bad.append((tag, n, "None" if g is None else "%d elements differ" % int((g.double().cpu() != r.grads[n]).sum())))
    if want_dx:
        assert dx is not None and dx.dtype == torch.float32
        same(dx, r.dx, "dx", bad)
        if bad and bad[-1][0] == "dx":
            bad[-1] = (tag,) + bad[-1]
    else:
        assert dx is None
    # every parameter delivered exactly once, with the bits of the final result
    assert sorted(name_of[p] for p, _ in sink.got) == sorted(expected), tag
    for p, g in sink.got:
        final = grads[p]
        assert (g is None) == (final is None), (tag, name_of[p])
        if g is not None and not torch.equal(g, final):
            bad.append((tag, name_of[p], "delivered before it was final"))


def run_matrix(case, norm, grouped, dev, monkeypatch):
    from unet_nested4tiny_objects_keypoints_amd import engine
    monkeypatch.setattr(engine, "USE_GROUPED_DGRAD", grouped)
    m = build_model(case, norm, dev)
    bad, forward_checked = [], set()
    for top in [None] + list(range(1, case.ctor["depth"])):
        for want_dx in (True, False):
            run_case(case, norm, m, dev, top, want_dx, bad, forward_checked)
    assert not bad, bad[:12]


@pytest.mark.parametrize("case,norm,grouped", ROWS, ids=ROW_IDS)
def test_exact_network(case, norm, grouped, dev, monkeypatch):
    run_matrix(case, norm, grouped, dev, monkeypatch)


@pytest.mark.parametrize("norm", en.NORMS)
@pytest.mark.parametrize("grouped", (True, False), ids=("grouped", "per-consumer"))
def test_exact_network_without_pack_plan(norm, grouped, dev, monkeypatch):
    from unet_nested4tiny_objects_keypoints_amd import engine
    monkeypatch.setattr(engine, "USE_PACK_PLAN", False)
    run_matrix(en.CASE_BY_ID[en.EXTRA_CASE], norm, grouped, dev, monkeypatch)


@pytest.mark.parametrize("norm", en.NORMS)
@pytest.mark.parametrize("grouped", (True, False), ids=("grouped", "per-consumer"))
def test_exact_network_on_eight_cus(norm, grouped, dev, monkeypatch):
    with usable_cus(8):
        run_matrix(en.CASE_BY_ID[en.EXTRA_CASE], norm, grouped, dev, monkeypatch)


@pytest.mark.parametrize("case_id,norm", [("d4-c1-f32", "bn"), ("d4-c3-bf16", "none")])
def test_the_seam_is_the_production_path(case_id, norm, dev):
    """model(x) + backward() against the same forward state run through saved.head_train, with dX_0j from a stand-alone
    ops.head_bwd call on the arguments engine._backward_impl passes: the body gradients are the same bits."""
    from unet_nested4tiny_objects_keypoints_amd import engine, ops
    case = en.CASE_BY_ID[case_id]
    _, x, _, _ = en.cached(case, norm)
    m = build_model(case, norm, dev)
    d = case.ctor["depth"]
    gen = torch.Generator().manual_seed(5)
    probes = [torch.randn(case.batch, en.N_CLASSES, case.h, case.w, generator=gen).to(dev) for _ in range(d - 1)]
    xg = x.to(dev).requires_grad_(True)
    outs = m(xg)
    sum((o * p).sum() for o, p in zip(outs, probes)).backward()
    torch.cuda.synchronize()

    outs2, saved = engine.forward_impl(m, x.to(dev), training=True, save=True)
    assert all(torch.equal(a.detach(), b) for a, b in zip(outs, outs2))
    seam = {}
    for j in range(1, d):
        head = getattr(m, "final_%d" % j)
        dx_j = torch.empty_like(saved.X[(0, j)])
        dw, db = ops.head_bwd(probes[j - 1].contiguous(), saved.outs[j - 1], saved.X[(0, j)],
                              head.weight.detach().view(en.N_CLASSES, -1), saved.p_drop, saved.seeds[j - 1], None, dx_j, False,
                              gate_x=(j == d - 1), seed_dev=saved.seed_dev)
        seam[j] = (dx_j, dw, db)
    saved.head_train = seam
    grads, dx = engine.backward_impl(m, saved, [None] * (d - 1), True, None)
    torch.cuda.synchronize()
    assert torch.equal(ops.nhwc_to_nchw(dx), xg.grad)
    checked = 0
    for n, p in m.named_parameters():
        if not p.requires_grad:
            assert p.grad is None and grads[p] is None, n
            continue
        assert torch.equal(grads[p].reshape(p.shape), p.grad), n
        checked += 1
    assert checked >= len(en.body_names(case, norm))
