"""The fused optimizer step (optim.py, csrc/optim.hip) on the GPU against tests/optim_oracle.py: EVERY element of every
parameter and every state tensor after EVERY step, bit for bit, no tolerance.  The contract is the kernel's own (the
header of optim.hip): the reference's op sequence, every op an IEEE-754 float32 op rounded once, every element depending
on that element alone.  The oracle runs with the correctly rounded sqrt (numpy's); tests/test_optim_oracle_host.py holds
the oracle to exact arithmetic, to the reference's fixtures and to torch's CPU ops.

One parameter set (SPEC) hits every path of optim_body: tail-only segments, exactly one vector, a vector and a tail, one
element on either side of a chunk, several chunks with a remainder, the scalar path (vec = 0) through a misaligned
parameter, a misaligned gradient and both, a zero-element parameter (no segment: the eager step-count block shifts), a
parameter without a gradient at step 2 (its count falls behind, the table is rebuilt) and 270 001 elements so that a
grid sized for 8 CUs (64 workgroups) walks several of the 86 chunks.  Parameters and gradients are views inside two flat
buffers with 16 sentinel floats on each side of every view: after every step the sentinels and every gradient are
bit-unchanged (step() never writes p.grad, clipped or not).  Gradients are seeded normals scaled per tensor over
1e-3 ... 1e1; the 4097-element tensor carries +0, -0 (denom = eps), 1e-20 and 3e-20 (a denormal second moment), 3e19
(the largest second moments that stay finite: (1-b2)*g*g = 4.5e37 there, up to 2e38 after five steps) and 1e21
((1-b2)*g*g >= 1e39 for every b2 <= 0.999 here: v = +inf from step 1 on, asserted on the oracle, so sqrt(inf), m/inf,
fmax(vmax, inf) and AdaBound's clamp of step/inf run) at fixed indices.  Two parameter groups (even / odd index) differ in every hyper-parameter the
kernel reads per group.  Steps 1, 2, 3, then every count is set to 99 999 and steps 100 000 and 100 001 follow (the bias
corrections at a large t: the oracle forms them with the host's pow, the kernel with the device's, both in double).

"capturable" here is capturable=True driven by eager step() calls: device step counters advanced by the launch, the
hyper-parameter block refreshed at every step.  No HIP graph is captured or replayed in this file; a captured step is held
to the eager one in tests/test_gpu_optim.py.

Clipped steps (one configuration per kind): the oracle takes the norm the step published (tests/test_gpu_clip.py holds
it to one ulp of float64), recomputes the coefficient (optim_oracle.clip_coef), asserts the published coefficient has the
same bits and multiplies the gradients by it.  They run on the gradients above (the 1e21 entry makes the coefficient
5e-20: that entry becomes 50, nothing overflows, and nearly every other second moment is a denormal or zero) and on the
same gradients with the two large entries at 3.0 (coefficient ~0.07).
"""
import numpy as np
import pytest
import torch

from tests import optim_oracle as oo

pytestmark = pytest.mark.gpu

F32 = np.float32
GUARD = 16
GUARD_BITS = 0x4B3C2D1E        # a finite float (12332318.0) that no update here produces
# (numel, parameter offset in floats past a 16-byte boundary, gradient offset, steps without a gradient)
SPEC = [(1, 0, 0, ()), (3, 0, 0, ()), (4, 0, 0, ()), (5, 0, 0, ()), (7, 0, 0, ()),
        (4095, 0, 0, ()), (4096, 0, 0, ()), (4097, 0, 0, ()),
        (2 * 4096 + 5, 0, 0, ()),
        (3 * 4096 + 3, 1, 0, ()),          # vec = 0 through the parameter
        (4096 + 3, 0, 2, ()),              # vec = 0 through the gradient
        (1027, 3, 3, ()),                  # both misaligned
        (0, 0, 0, ()),
        (10, 0, 0, (2,)),
        (270001, 0, 0, ())]
PLANTED = 7                                # the 4097-element tensor
PLANTS = {5: 0.0, 6: -0.0, 1023: 1e-20, 1024: 3e-20, 2047: 1e21, 4095: 3e19, 4096: 1e-20}
OVERFLOW_AT = 2047                         # v = +inf from step 1 on in every unclipped run (asserted in _Oracle.snap)
SCALE_EXP = (-1, 1, -3, 0, -2)             # gradient scale 10^e per tensor, e by index mod 5
N_STEPS = 5
T_JUMP = 99999                             # every existing count after step 3
MAX_NORM = 50.0                            # below every step's gradient norm (asserted: coef < 1)
N_CHUNKS = sum((n + oo.CHUNK - 1) // oo.CHUNK for n, _, _, _ in SPEC)


def _host_inputs():
    rng = np.random.default_rng(20261018)
    params = [(0.1 * rng.standard_normal(n)).astype(F32) for n, _, _, _ in SPEC]
    grads = {"planted": [], "moderate": []}
    for step in range(1, N_STEPS + 1):
        gs = [(10.0 ** SCALE_EXP[i % 5] * rng.standard_normal(n)).astype(F32) for i, (n, _, _, _) in enumerate(SPEC)]
        for k, val in PLANTS.items():
            gs[PLANTED][k] = val
        mod = [g.copy() for g in gs]
        mod[PLANTED][4095] = mod[PLANTED][OVERFLOW_AT] = 3.0
        for key, lst in (("planted", gs), ("moderate", mod)):
            grads[key].append([None if step in SPEC[i][3] else g for i, g in enumerate(lst)])
    return params, grads


PARAMS0, GRADS = _host_inputs()
GROUP_OF = [i % 2 for i in range(len(SPEC))]


class _Oracle:
    """The driver with the correctly rounded sqrt over the N_STEPS steps, advanced on demand; snaps[k] = (params, states,
    scalars) after step k + 1.  A clipped run feeds each step's coefficient as the step publishes it."""

    def __init__(self, name, gradset):
        kind, ams, ga, gb, self.lr_moves = oo.CONFIGS[name]
        self.drv = oo.Driver(kind, [oo.group_kwargs(kind, ga), oo.group_kwargs(kind, gb)], PARAMS0, GROUP_OF, ams=ams)
        self.grads, self.snaps, self.coef_bits = GRADS[gradset], [], []

    def snap(self, step, coef=None):
        bits = None if coef is None else int(np.asarray(coef, dtype=F32).view(np.uint32))
        if step <= len(self.snaps):
            return self.snaps[step - 1] if self.coef_bits[step - 1] == bits else None
        assert step == len(self.snaps) + 1
        drv = self.drv
        with np.errstate(all="ignore"):
            if step == 4:
                drv.set_counts(T_JUMP)
            drv.step(self.grads[step - 1], coef=coef)
        if coef is None and drv.kind != oo.SGDW:          # the premise of the overflow plant: v is +inf and stays there
            st = drv.state[PLANTED]
            assert all(st[k][OVERFLOW_AT] == np.inf for k in st if k != "exp_avg"), (step, st["exp_avg_sq"][OVERFLOW_AT])
            assert np.isfinite(st["exp_avg"][OVERFLOW_AT]) and np.isfinite(drv.params[PLANTED]).all(), step
        self.snaps.append(([p.copy() for p in drv.params], [dict(s) for s in drv.state], list(drv.last_scalars)))
        self.coef_bits.append(bits)
        if step in self.lr_moves:
            for g in drv.groups:
                g["lr"] = g["lr"] * self.lr_moves[step]
        return self.snaps[-1]


_ORACLES = {}       # (name, gradient set, clipped) -> _Oracle: run once, shared by the modes and the grids


def _oracle(name, gradset="planted", clipped=False):
    key = (name, gradset, clipped)
    if key not in _ORACLES:
        _ORACLES[key] = _Oracle(name, gradset)
    return _ORACLES[key]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import __graft_entry__ as entry
    entry.build()
    return torch.device("cuda:0")


class _Layout:
    """Parameters and gradients as contiguous views inside two flat guarded device buffers."""

    def __init__(self, dev):
        self.dev = dev
        self.p_at, self.g_at = [], []
        p = g = GUARD
        for n, po, go, _ in SPEC:
            p, g = (p + 3) // 4 * 4 + po, (g + 3) // 4 * 4 + go
            self.p_at.append(p)
            self.g_at.append(g)
            p, g = p + n + GUARD, g + n + GUARD
        self.pbuf = torch.empty(p + 4, dtype=torch.float32, device=dev)
        self.gbuf = torch.empty(g + 4, dtype=torch.float32, device=dev)
        assert self.pbuf.data_ptr() % 16 == 0 and self.gbuf.data_ptr() % 16 == 0
        self.pbuf.view(torch.int32).fill_(GUARD_BITS)
        self.gbuf.view(torch.int32).fill_(GUARD_BITS)
        self.p_guard = np.ones(self.pbuf.numel(), dtype=bool)              # True outside every parameter
        for (n, _, _, _), at in zip(SPEC, self.p_at):
            self.p_guard[at:at + n] = False
        self.params = []
        for (n, po, go, _), pa, ga, p0 in zip(SPEC, self.p_at, self.g_at, PARAMS0):
            view = self.pbuf[pa:pa + n]
            view.copy_(torch.from_numpy(p0))
            assert view.is_contiguous() and self.gbuf[ga:ga + n].is_contiguous()
            if n:
                assert view.data_ptr() % 16 == 4 * po and self.gbuf[ga:ga + n].data_ptr() % 16 == 4 * go
            self.params.append(torch.nn.Parameter(view))
            assert self.params[-1].data_ptr() == view.data_ptr()
        self.g_sent = None

    def set_grads(self, grads):
        for p, (n, _, _, _), ga, g in zip(self.params, SPEC, self.g_at, grads):
            if g is None:
                p.grad = None
                continue
            view = self.gbuf[ga:ga + n]
            view.copy_(torch.from_numpy(g))
            p.grad = view
            assert p.grad.data_ptr() == view.data_ptr()
        self.g_sent = self.gbuf.clone()

    def param_bits(self):
        """-> (every parameter's bits as uint32 arrays, sentinels intact)"""
        host = self.pbuf.cpu().numpy().view(np.uint32)
        intact = bool((host[self.p_guard] == GUARD_BITS).all())
        return [host[at:at + n] for (n, _, _, _), at in zip(SPEC, self.p_at)], intact

    def grads_untouched(self):
        return torch.equal(self.gbuf.view(torch.int32), self.g_sent.view(torch.int32))


def _diff(what, got, want):
    """None, or one line naming the differing elements of a tensor: how many, the first few with their quarter of the
    chunk ((i % 4096) // 1024: which of a thread's four vectors) and their lane of the vector (i % 4), both bit patterns."""
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    if got.shape != want.shape:
        return "%s: %d elements, expected %d" % (what, got.size, want.size)
    bad = np.nonzero(got != want)[0]
    if bad.size == 0:
        return None
    first = ", ".join("i=%d (chunk %d, quarter %d, lane %d) got %08x want %08x"
                      % (i, i // oo.CHUNK, (i % oo.CHUNK) // 1024, i % 4, got[i], want[i]) for i in bad[:6])
    return "%s: %d of %d elements differ: %s" % (what, bad.size, got.size, first)


def _make_opt(name, lay, capturable, **kw):
    import unet_nested4tiny_objects_keypoints_amd as pkg
    kind, ams, ga, gb, _ = oo.CONFIGS[name]
    cls = {oo.ADAMW: pkg.AdamW, oo.ADABOUND: pkg.AdaBound, oo.SGDW: pkg.SGDW}[kind]
    if kind == oo.ADAMW:
        kw["amsgrad"] = ams
    elif kind == oo.ADABOUND:
        kw["amsbound"] = ams
    else:
        kw["lr"] = 1e-3
    return cls([dict(ga, params=lay.params[0::2]), dict(gb, params=lay.params[1::2])], capturable=capturable, **kw)


def _jump_counts(opt):
    for st in opt.state.values():
        if "step" in st:
            if opt.capturable:
                st["step"].fill_(float(T_JUMP))
            else:
                st["step"] = T_JUMP


def _check_step(name, step, lay, opt, snap):
    """Every parameter and state element against the oracle's snapshot, the sentinels, the gradients -> messages."""
    want_p, want_s, scal = snap
    torch.cuda.synchronize()
    got_p, intact = lay.param_bits()
    msgs = []
    if not intact:
        msgs.append("step %d: a sentinel beside a parameter was overwritten" % step)
    if not lay.grads_untouched():
        msgs.append("step %d: the gradient buffer (gradients or their sentinels) was written" % step)
    for i, p in enumerate(lay.params):
        bad = []
        d = _diff("step %d tensor %d (%d elements) param" % (step, i, SPEC[i][0]), got_p[i], want_p[i].view(np.uint32))
        if d:
            bad.append(d)
        st = opt.state.get(p, {})
        keys = {k for k in st if k != "step"}
        if keys != set(want_s[i]):
            bad.append("step %d tensor %d: state keys %s, expected %s" % (step, i, sorted(keys), sorted(want_s[i])))
            keys &= set(want_s[i])
        for k in sorted(keys):
            d = _diff("step %d tensor %d (%d elements) %s" % (step, i, SPEC[i][0], k),
                      st[k].cpu().numpy().view(np.uint32), want_s[i][k].view(np.uint32))
            if d:
                bad.append(d)
        if bad and scal[i] is not None:
            bad.append("    oracle scalars of tensor %d (host pow): %s"
                       % (i, " ".join("%s=%08x" % kv for kv in scal[i].bits().items())))
        msgs += bad
    return msgs


def _run(name, dev, capturable, cus, gradset="planted", clip=False):
    from tests.helpers import usable_cus
    lay = _Layout(dev)
    opt = _make_opt(name, lay, capturable, **({"max_grad_norm": MAX_NORM} if clip else {}))
    oracle, msgs = _oracle(name, gradset, clip), []
    lr_moves = oracle.lr_moves
    with usable_cus(cus) as u:
        for step in range(1, N_STEPS + 1):
            if step == 4:
                _jump_counts(opt)
            lay.set_grads(GRADS[gradset][step - 1])
            opt.step()
            if clip:
                torch.cuda.synchronize()
                block = opt._clip_block().cpu().numpy()
                coef = oo.clip_coef(F32(float(opt.last_grad_norm)), MAX_NORM)
                assert coef < F32(1.0), (step, float(block[0]), float(coef))
                assert block[1:2].view(np.uint32)[0] == np.asarray(coef).view(np.uint32), (step, block[:2], coef)
                snap = oracle.snap(step, coef)
                # the norm's bits do not depend on the mode or the grid (tests/test_gpu_clip.py): one oracle serves all
                assert snap is not None, "step %d: this run's coefficient %r differs from an earlier run's" % (step, coef)
            else:
                snap = oracle.snap(step)
            msgs += _check_step(name, step, lay, opt, snap)
            if step in lr_moves:
                for g in opt.param_groups:
                    g["lr"] = g["lr"] * lr_moves[step]
        n_chunks = max(t.n_chunks for t in opt._tables.values())
        assert n_chunks == N_CHUNKS
        if cus is not None:
            assert n_chunks > 8 * u.cus, (n_chunks, u.cus)     # optim.hip persistent_grid: min(n_chunks, 8 * cus)
    assert not msgs, "%s %s: %d findings\n%s" % (name, "capturable" if capturable else "eager", len(msgs),
                                                  "\n".join(msgs[:40]))
    return lay, opt


@pytest.mark.parametrize("cus", [None, 8], ids=["all-cus", "8-cus"])
@pytest.mark.parametrize("capturable", [False, True], ids=["eager", "capturable"])
@pytest.mark.parametrize("name", list(oo.CONFIGS))
def test_every_element_bit_equal(name, capturable, cus, dev):
    lay, opt = _run(name, dev, capturable, cus)
    for i, p in enumerate(lay.params):                     # the counts themselves
        st = opt.state.get(p, {})
        if "step" in st:
            want = T_JUMP + 2 if SPEC[i][0] or not capturable else None
            if want is not None:
                assert float(st["step"]) == want, (i, float(st["step"]))
            assert torch.is_tensor(st["step"]) == capturable
    if name == "sgdw_nesterov":                            # weight decay 0: SGDW changes no parameter
        got, _ = lay.param_bits()
        assert all(np.array_equal(g, p0.view(np.uint32)) for g, p0 in zip(got, PARAMS0))
    else:
        got, _ = lay.param_bits()
        assert not np.array_equal(got[-1], PARAMS0[-1].view(np.uint32))


@pytest.mark.parametrize("gradset", ["planted", "moderate"])
@pytest.mark.parametrize("capturable", [False, True], ids=["eager", "capturable"])
@pytest.mark.parametrize("name", list(oo.CLIPPED))
def test_clipped_step_every_element_bit_equal(name, capturable, gradset, dev):
    _run(name, dev, capturable, None, gradset=gradset, clip=True)
