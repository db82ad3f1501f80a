"""Integer networks on which the whole nested U-Net is exact, and their float64 reference (TEST INFRASTRUCTURE, like
tests/gemm_oracle.py).

A case is a constructor, a storage type, an image size and pinned seeds.  Its state has +-1 sparse convolution and
transposed-convolution weights, biases in {-1, 0}, inputs in [-2, 2] and one integer gradient G_j per head node X[0][j]:
the loss is sum_j <X[0][j], G_j>, the heads are not used.  Three normalisations: "none" (is_batchnorm=False), "bn"
(BatchNorm frozen, gamma and beta trained) and "bn_affine" (gamma and beta frozen too).  A frozen layer has
running_var = float32(0.99999), whose fp32 sum with eps = 1e-5f is exactly 1, so invstd = 1, scale = gamma (a power of
two) and shift = beta - mean * gamma exactly; the reference uses that dyadic map, not the float64 1 / sqrt(var + eps).

`reference(...)` restates the body of oracle/unet_nested_oracle.py (models/unet.py:255-280) function by function and
its backward by hand, one named gradient contribution at a time in the order engine._backward_impl makes them: the max
pool routes to the first maximum in scan order (tests/stream_rules.ref_route), ReLU passes where out > 0.  The hand-made
backward is what lets tests/test_exact_net_host.py mutate single contributions, run it on absolute values and read
every stored tensor; the same file holds it against autograd on UNetNestedOracle.  Nothing here touches the device.
"""
import re
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle.unet_nested_oracle import UNetNestedOracle
from tests.stream_rules import ref_route

F64 = torch.float64
N_CLASSES = 2
NORMS = ("none", "bn", "bn_affine")
RUNNING_VAR = float(np.float32(0.99999))
EPS = 1e-5

# id, constructor, bf16 storage, batch, H, W, seeds per data set ("none", "bn": both frozen variants share the data),
# expected taps per output of a convolution (weight density * fan_in) per data set, share of non-zero G elements,
# probabilities of gamma = 1/2, 1, 2, the normalisations the case runs
Case = namedtuple("Case", "id ctor bf16 batch h w seeds taps g_density gamma_p norms")


def _c(id_, depth, cin, fs, bf16, batch, h, w, seeds, taps=2.5, g_density=0.5, gamma_p=(0.1, 0.8, 0.1), norms=NORMS):
    return Case(id_, dict(in_channels=cin, n_classes=N_CLASSES, feature_scale=fs, is_deconv=True, depth=depth), bf16,
                batch, h, w, dict(zip(("none", "bn"), seeds)), dict(none=taps, bn=taps), g_density, gamma_p, norms)


# feature_scale 4 gives the widths 8, 16, 32, 64, 128 (2: 16 .. 256): 8 * 2^k, what bf16 storage needs.  *-min: the
# smallest legal image (the deepest level is 1x2).  The seeds were searched on the CPU until every assertion of
# tests/test_exact_net_host.py held (its docstring says how).
CASES = [
    _c("d2-c1-f32", 2, 1, 4, False, 2, 8, 12, (0, 0)),
    _c("d2-c3-bf16-min", 2, 3, 4, True, 2, 2, 4, (7989, 7926), taps=4.0),
    _c("d3-c3-f32", 3, 3, 4, False, 2, 8, 12, (15844, 15838)),
    _c("d3-c1-bf16", 3, 1, 4, True, 2, 8, 12, (23757, 23758)),
    _c("d3-c1-f32-min", 3, 1, 4, False, 2, 4, 8, (31863, 31794)),
    _c("d4-c1-f32", 4, 1, 4, False, 2, 16, 24, (39596, 39596)),
    _c("d4-c3-bf16", 4, 3, 4, True, 2, 16, 24, (47530, 47531)),
    _c("d5-c3-f32", 5, 3, 4, False, 2, 32, 32, (55436, 55446)),
    # depth 5 in bf16 storage takes two constructors: at the widths 8 .. 128 no searched data set with BatchNorm kept
    # both the 8 bits and a live gradient through the 8-channel slices of the far skips; at 16 .. 256 none without did
    _c("d5-c1-bf16", 5, 1, 4, True, 2, 32, 32, (63626, None), norms=("none",)),
    _c("d5-c1-bf16-w16", 5, 1, 2, True, 2, 32, 32, (None, 63387), taps=2.0, norms=("bn", "bn_affine")),
    _c("d4-c1-bf16-min", 4, 1, 4, True, 2, 8, 16, (71290, 71344)),
]
CASE_BY_ID = {c.id: c for c in CASES}
EXTRA_CASE = "d4-c1-f32"   # also runs without the pack plan and on a reduced persistent grid


def widths(case):
    return [int(w / case.ctor["feature_scale"]) for w in (32, 64, 128, 256, 512)][:case.ctor["depth"]]


def needed_nodes(depth, top):
    """engine.needed_nodes, restated: encoder column top down, then the decoder columns left to right"""
    return [(i, 0) for i in range(top + 1)] + [(i, j) for j in range(1, top + 1) for i in range(top + 1 - j)]


def pair_prefix(i, j):
    return "conv%d0" % i if j == 0 else "up_concat%d%d.conv" % (i, j)


_BN_KEY = re.compile(r"\.conv[12]\.1\.")


def make_data(case, norm):
    """(state dict of float32 tensors under the model's key names, x [B, C, H, W] float32, {j: G_j [B, f0, H, W] float64})"""
    data = "none" if norm == "none" else "bn"
    rng = np.random.RandomState(case.seeds[data])
    ctor = dict(case.ctor, is_batchnorm=norm != "none")
    shapes = {k: tuple(v.shape) for k, v in UNetNestedOracle(**ctor).state_dict().items()}
    state = {}
    for k, shp in shapes.items():
        if k.endswith("num_batches_tracked"):
            v = np.zeros(shp, np.int64)
        elif k.endswith("running_var"):
            v = np.full(shp, np.float32(0.99999), np.float32)
        elif k.endswith("running_mean"):
            v = rng.randint(-1, 2, shp)
        elif len(shp) == 4:
            # a transposed 2x2 stride-2 convolution gives every output pixel one tap per input channel
            fan_in = shp[0] if ".up." in k else shp[1] * shp[2] * shp[3]
            keep = rng.random_sample(shp) < min(1.0, case.taps[data] / fan_in)
            v = keep * rng.choice([-1.0, 1.0], shp)
        elif _BN_KEY.search(k) and k.endswith("weight"):
            v = rng.choice([0.5, 1.0, 2.0], shp, p=list(case.gamma_p))
        elif _BN_KEY.search(k):
            v = rng.randint(-1, 2, shp)
        else:
            v = rng.randint(-1, 1, shp)
        state[k] = torch.from_numpy(np.ascontiguousarray(v)).to(torch.int64 if k.endswith("tracked") else torch.float32)
    x = torch.from_numpy(rng.randint(-2, 3, (case.batch, case.ctor["in_channels"], case.h, case.w))).float()
    f0 = widths(case)[0]
    G = {}
    for j in range(1, case.ctor["depth"]):
        keep = rng.random_sample((case.batch, f0, case.h, case.w)) < case.g_density
        G[j] = torch.from_numpy(keep * rng.choice([-1.0, 1.0], keep.shape)).double()
    return state, x, G


def intended_coeffs(state, prefix):
    """(scale, shift, mean) float64 of the frozen layer `prefix` (e.g. "conv00.conv1.1"): the dyadic map"""
    gamma, beta = state[prefix + ".weight"].double(), state[prefix + ".bias"].double()
    mean = state[prefix + ".running_mean"].double()
    return gamma, beta - mean * gamma, mean


def coeffs_float32(state, prefix):
    """unetpp_bn_eval_coeffs in numpy float32: invstd = 1.0f / sqrtf(rv + eps); scale = gamma * invstd; shift = beta -
    mean * scale -> (scale, shift, invstd)"""
    f = np.float32
    g, b = state[prefix + ".weight"].numpy().astype(f), state[prefix + ".bias"].numpy().astype(f)
    m, rv = state[prefix + ".running_mean"].numpy().astype(f), state[prefix + ".running_var"].numpy().astype(f)
    invstd = (f(1.0) / np.sqrt((rv + f(EPS)).astype(f)).astype(f)).astype(f)
    scale = (g * invstd).astype(f)
    shift = (b - (m * scale).astype(f)).astype(f)
    return scale, shift, invstd


# ----------------------------------------------------------------------------------------------- the reference
def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def pool_winners(t, last=False):
    """NCHW -> (pooled, winner 2 * iy + ix of every window): the FIRST maximum in scan order (`last`: the mutation)"""
    cands = [t[:, :, a::2, b::2] for a in (0, 1) for b in (0, 1)]
    m = torch.maximum(torch.maximum(cands[0], cands[1]), torch.maximum(cands[2], cands[3]))
    idx = torch.zeros(m.shape, dtype=torch.int64)
    for q in ((0, 1, 2, 3) if last else (3, 2, 1, 0)):
        idx = torch.where(cands[q] == m, torch.full_like(idx, q), idx)
    ties = sum((c == m).long() for c in cands) > 1
    return m, idx, ties


class Ref:
    """What reference() returns: X, pairs (y1, a1, y2, out, pooled, idx, ties per node, None where the node has none),
    ups, grads by parameter name, dx, `stored` (label -> every tensor the engine stores, the running sums of the node
    gradients after each contribution included) and `contribs` (node -> [(name, tensor)] in engine order)."""


def reference(case, norm, state, x, G, top=None, want_dx=True, absolute=False, mutation=None, forward=None):
    """float64 forward and backward of the network cut at head `top` (None: whole).  absolute: the backward runs on |w|,
    |G|, |activations| and 0/1 gates -- every result is then the sum of the absolute values of the terms of the true one.
    mutation: one deliberate error of the schedule (tests/test_exact_net_host.py lists them).  forward: an earlier result
    for the same data and cut whose forward tensors are taken over unchanged (not with the "tie_last" mutation)."""
    d = case.ctor["depth"]
    top = d - 1 if top is None else top
    bn = norm != "none"
    f = widths(case)
    P = {k: v.double() for k, v in state.items()}
    mut = mutation or ("none",)
    r = Ref()
    r.top, r.X, r.pairs, r.ups, r.grads, r.stored, r.contribs, r.wino = top, {}, {}, {}, {}, {}, {}, {}
    A = (lambda t: t.abs()) if absolute else (lambda t: t)

    def coeff(prefix):
        if not bn or not prefix.startswith("conv"):
            return None
        return intended_coeffs(state, prefix + ".1")

    def pair_fwd(key, ins, pool):
        pre = pair_prefix(*key)
        p = dict(ins=ins, pooled=None, idx=None, ties=None, y1=None, y2=None)
        xin = torch.cat(ins, 1)
        y1 = F.conv2d(xin, P[pre + ".conv1.0.weight"], P[pre + ".conv1.0.bias"], padding=1)
        c1, c2 = coeff(pre + ".conv1"), coeff(pre + ".conv2")
        p["c1"], p["c2"] = c1, c2
        if c1 is not None:
            p["y1"] = y1
            y1 = y1 * c1[0].view(1, -1, 1, 1) + c1[1].view(1, -1, 1, 1)
        p["a1"] = y1.clamp_min(0)
        y2 = F.conv2d(p["a1"], P[pre + ".conv2.0.weight"], P[pre + ".conv2.0.bias"], padding=1)
        if c2 is not None:
            p["y2"] = y2
            y2 = y2 * c2[0].view(1, -1, 1, 1) + c2[1].view(1, -1, 1, 1)
        p["out"] = y2.clamp_min(0)
        if pool:
            p["pooled"], p["idx"], p["ties"] = pool_winners(p["out"], last=mut[0] == "tie_last")
        for name in ("y1", "a1", "y2", "out", "pooled"):
            if p[name] is not None:
                r.stored["%s%d%d" % (name, key[0], key[1])] = p[name]
        return p

    inp = x.double()
    if forward is not None:
        assert mut[0] != "tie_last" and forward.top == top
        r.X, r.pairs, r.ups = forward.X, forward.pairs, forward.ups
        r.stored = {k: v for k, v in forward.stored.items() if not k.startswith("d")}
    for (i, j) in (needed_nodes(d, top) if forward is None else ()):
        if j == 0:
            p = pair_fwd((i, 0), [inp], i < top)
            inp = p["pooled"]
        else:
            up = "up_concat%d%d.up" % (i, j)
            u = F.conv_transpose2d(r.X[(i + 1, j - 1)], P[up + ".weight"], P[up + ".bias"], stride=2)
            r.ups[(i, j)] = u
            r.stored["up%d%d" % (i, j)] = u
            p = pair_fwd((i, j), [u] + [r.X[(i, jj)] for jj in range(j)], False)
        r.pairs[(i, j)], r.X[(i, j)] = p, p["out"]

    # ------------------------------------------------------------------ backward
    dy1s, d_ups, d_pooled = {}, {}, {}

    def w1_slice(i, jc, jj):
        w = A(P["up_concat%d%d.conv.conv1.0.weight" % (i, jc)])
        return w[:, (1 + jj) * f[i]:(2 + jj) * f[i]]

    def contributions(key):
        i, j = key
        out = []
        if i == 0 and j >= 1:
            out.append(("head", A(G[j])))
        consumers = list(range(top - i, j, -1))
        for jc in consumers:
            jw = jc
            if mut[0] == "swap" and mut[1] == key and jc in mut[2:]:
                jw = mut[2] if jc == mut[3] else mut[3]
            out.append(("skip%d" % jc, F.conv_transpose2d(dy1s[(i, jc)], w1_slice(i, jw, j), padding=1)))
        if i >= 1:
            wu = A(P["up_concat%d%d.up.weight" % (i - 1, j + 1)])
            out.append(("up", F.conv2d(d_ups[(i - 1, j + 1)], wu, stride=2)))
        if j == 0 and i < top:
            idx = r.pairs[key]["idx"]
            out.append(("pool", _nchw(ref_route(_nhwc(d_pooled[i + 1]), _nhwc(idx), _nhwc(r.X[key]).shape))))
        if mut[0] == "drop" and mut[1] == key:
            out = [c for c in out if c[0] != mut[2]]
        if mut[0] == "twice" and mut[1] == key:
            out = out + [c for c in out if c[0] == mut[2]]
        return out

    def node_gradient(key):
        cs = contributions(key)
        r.contribs[key] = cs
        total = torch.zeros_like(r.X[key])
        for n, (name, t) in enumerate(cs):
            total = total + t
            r.stored["dX%d%d#%d" % (key + (n,))] = total   # the buffer after its n-th read-modify-write
        mask = (r.X[key] > 0).double()
        if mut[0] == "no_mask" and mut[1] == key:
            return total
        if mut[0] == "early_mask" and mut[1] == key:
            return (total - cs[-1][1]) * mask + cs[-1][1]
        return total * mask

    def wgrad(xin, dy, shape):
        return torch.nn.grad.conv2d_weight(xin, shape, dy, padding=1)

    def pair_bwd(key, gg, want_in):
        """gg: the gradient of the node's output, already masked"""
        pre = pair_prefix(*key)
        p = r.pairs[key]
        lab = "%d%d" % key
        w1, w2 = A(P[pre + ".conv1.0.weight"]), A(P[pre + ".conv2.0.weight"])
        sums = bn and not (norm == "bn_affine")

        def bn_bwd(stage, g_masked, y, c):
            scale, _, mean = c
            if sums:
                r.grads["%s.conv%d.1.weight" % (pre, stage)] = (g_masked * A(y - mean.view(1, -1, 1, 1))).sum((0, 2, 3))
                r.grads["%s.conv%d.1.bias" % (pre, stage)] = g_masked.sum((0, 2, 3))
            return g_masked * scale.view(1, -1, 1, 1)

        dy2 = gg if p["c2"] is None else bn_bwd(2, gg, p["y2"], p["c2"])
        r.stored["dy2_" + lab] = dy2
        r.grads[pre + ".conv2.0.weight"] = wgrad(A(p["a1"]), dy2, w2.shape)
        r.grads[pre + ".conv2.0.bias"] = dy2.sum((0, 2, 3))
        d_a1 = F.conv_transpose2d(dy2, w2, padding=1)
        if p["c1"] is not None:
            r.stored["d_a1_" + lab] = d_a1   # a BatchNorm node stores conv2's input gradient before the mask
        dy1 = d_a1 * (p["a1"] > 0).double()
        if p["c1"] is not None:
            dy1 = bn_bwd(1, dy1, p["y1"], p["c1"])
        r.stored["dy1_" + lab] = dy1
        xin = A(torch.cat(p["ins"], 1))
        r.grads[pre + ".conv1.0.weight"] = wgrad(xin, dy1, w1.shape)
        r.grads[pre + ".conv1.0.bias"] = dy1.sum((0, 2, 3))
        if absolute:   # what a Winograd kernel adds up, through its transforms taken on absolute values
            from tests.helpers import wino_magnitude
            r.wino["fwd1_" + lab] = wino_magnitude(xin, w1, A(P[pre + ".conv1.0.bias"]))
            r.wino["fwd2_" + lab] = wino_magnitude(A(p["a1"]), w2, A(P[pre + ".conv2.0.bias"]))
            r.wino["dgrad2_" + lab] = wino_magnitude(dy2, w2.flip(2, 3).transpose(0, 1))
            r.wino["dgrad1_" + lab] = wino_magnitude(dy1, w1.flip(2, 3).transpose(0, 1))
        dy1s[key] = dy1
        if want_in:
            return F.conv_transpose2d(dy1, w1[:, :p["ins"][0].shape[1]], padding=1)
        return None

    for j in range(top, 0, -1):
        for i in range(top - j, -1, -1):
            d_up = pair_bwd((i, j), node_gradient((i, j)), True)
            d_ups[(i, j)] = d_up
            r.stored["d_up%d%d" % (i, j)] = d_up
            up = "up_concat%d%d.up" % (i, j)
            src = A(r.X[(i + 1, j - 1)])
            # ConvTranspose2d(2, 2): dW[ci, co, a, b] = sum x[ci, y, x] * d_up[co, 2y + a, 2x + b]
            r.grads[up + ".weight"] = torch.stack([torch.stack([torch.einsum("nchw,nohw->co", src, d_up[:, :, a::2, b::2])
                                                                for b in (0, 1)], -1) for a in (0, 1)], -2)
            r.grads[up + ".bias"] = d_up.sum((0, 2, 3))
    r.dx = None
    for i in range(top, -1, -1):
        din = pair_bwd((i, 0), node_gradient((i, 0)), i > 0 or want_dx)
        if i > 0:
            d_pooled[i] = din
            r.stored["d_pooled%d" % i] = din
        else:
            r.dx = din
    return r


def body_names(case, norm, top=None):
    """names of the parameters the network cut at `top` gives gradients to, the heads excluded"""
    d = case.ctor["depth"]
    top = d - 1 if top is None else top
    out = []
    for (i, j) in needed_nodes(d, top):
        pre = pair_prefix(i, j)
        for stage in ("conv1", "conv2"):
            out += ["%s.%s.0.weight" % (pre, stage), "%s.%s.0.bias" % (pre, stage)]
            if norm == "bn" and j == 0:
                out += ["%s.%s.1.weight" % (pre, stage), "%s.%s.1.bias" % (pre, stage)]
        if j:
            out += ["up_concat%d%d.up.weight" % (i, j), "up_concat%d%d.up.bias" % (i, j)]
    return out


_CACHE = {}


def cached(case, norm, top=None, want_dx=True):
    """data and reference of a case, computed once per process and never written to"""
    key = (case.id, norm, top, want_dx)
    if key not in _CACHE:
        if (case.id, norm) not in _CACHE:
            _CACHE[(case.id, norm)] = make_data(case, norm)
        state, x, G = _CACHE[(case.id, norm)]
        _CACHE[key] = (state, x, G, reference(case, norm, state, x, G, top, want_dx))
    return _CACHE[key]


def sig_bits(t):
    """largest number of significant bits of an element of the float64 tensor t (0 for an all-zero tensor)"""
    a = t.detach().double().abs().reshape(-1).numpy()
    a = a[a != 0]
    if a.size == 0:
        return 0
    m, _ = np.frexp(a)                      # a = m * 2^e, 0.5 <= m < 1: m * 2^53 is an integer
    k = (m * 2.0 ** 53).astype(np.int64)
    low = k & -k                            # lowest set bit
    return int(np.max(53 - np.log2(low.astype(np.float64)).astype(np.int64)))


def granule(tensors):
    """the largest power of two that divides every element of every tensor"""
    g = None
    for t in tensors:
        a = t.detach().double().abs().reshape(-1).numpy()
        a = a[a != 0]
        if a.size == 0:
            continue
        m, e = np.frexp(a)
        k = (m * 2.0 ** 53).astype(np.int64)
        low = np.log2((k & -k).astype(np.float64)) + e - 53
        g = float(low.min()) if g is None else min(g, float(low.min()))
    return 2.0 ** (g if g is not None else 0.0)


def measure(case, norm, top=None):
    """The figures tests/test_exact_net_host.py asserts on, from the reference alone."""
    state, x, G, r = cached(case, norm, top, True)
    a = reference(case, norm, state, x, G, top, True, absolute=True)
    names = body_names(case, norm, top)
    acts = [p[k] for p in r.pairs.values() for k in ("a1", "out")]
    multi = {k: sum(bool(t.abs().max() > 0) for _, t in cs) for k, cs in r.contribs.items() if len(cs) > 1}
    g = granule(list(r.stored.values()) + list(r.grads.values()))
    return dict(
        bits=max(sig_bits(t) for t in r.stored.values()),
        bits_abs=max(sig_bits(t) for t in a.stored.values()),
        value_max=max(float(t.abs().max()) for t in r.stored.values()),
        abs_max=max(float(t.max()) for t in list(a.stored.values()) + [a.grads[n] for n in names] + [a.dx]),
        wino_max=max(float(t.max()) for t in a.wino.values()),
        grad_max=max(float(r.grads[n].abs().max()) for n in names),
        granule=g,
        zero_share=sum(int((t == 0).sum()) for t in acts) / sum(t.numel() for t in acts),
        ties=min([int(p["ties"].sum()) for p in r.pairs.values() if p["ties"] is not None]),
        zero_grads=[n for n in names if float(r.grads[n].abs().max()) == 0.0],
        dx_nonzero=bool(r.dx.abs().max() > 0),
        live_contribs=min(multi.values()) if multi else 2,
    )
