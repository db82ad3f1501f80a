"""The guard-band allocator and its checker (tests/guard_alloc.py), checked on CPU tensors: in-bounds writes are never
reported, a planted single-byte write into either band is reported with its site, side and byte, the wrapped functions
return what the real ones return, pass-through cases pass through, and the real functions come back on exit.  One test
keeps the limit of the method in view: a write more than GUARD_BYTES away is not seen."""
import pytest
import torch

from tests import guard_alloc as ga

G = ga.GUARD_BYTES
CPU = ("cpu",)
DTYPES = [torch.float32, torch.bfloat16, torch.float64, torch.int32, torch.uint8, torch.bool]
POISONS = [float("nan"), 3.0e30]
SHAPE = (3, 5, 7)


@pytest.fixture(autouse=True)
def clean_registry():
    ga.reset()
    yield
    ga.reset()


def _one(dtype):
    return torch.ones((), dtype=dtype)


def _allocations(dtype, poison):
    """One tensor per wrapped function and one by guarded(), each with its registry record."""
    src = torch.zeros(SHAPE, dtype=dtype)
    out = []
    with ga.guard_allocations(poison, devices=CPU):
        for make in (lambda: torch.empty(SHAPE, dtype=dtype), lambda: torch.empty_like(src),
                     lambda: torch.zeros(SHAPE, dtype=dtype), lambda: torch.zeros_like(src),
                     lambda: torch.full(SHAPE, 1, dtype=dtype), lambda: torch.full_like(src, 1),
                     lambda: torch.ones(SHAPE, dtype=dtype)):
            t = make()
            out.append((t, ga.REGISTRY[-1]))
    out.append((ga.guarded(src, poison, name="operand"), ga.REGISTRY[-1]))
    return out


@pytest.mark.parametrize("poison", POISONS, ids=["nan", "3e30"])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
def test_writes_inside_the_tensor_are_never_reported(dtype, poison):
    got = _allocations(dtype, poison)
    assert len(ga.REGISTRY) == len(got) == 8
    for t, rec in got:
        assert t.shape == SHAPE and t.dtype == dtype and t.is_contiguous()
        assert rec.n_bytes == t.numel() * t.element_size() and rec.store.dtype == torch.uint8
        assert rec.store.numel() == rec.n_bytes + 2 * G
        assert t.data_ptr() == rec.store.data_ptr() + G           # the interior starts one band in: alignment kept
        flat = t.view(-1)
        flat[0] = _one(dtype)
        flat[-1] = _one(dtype)
        t.fill_(_one(dtype))
        t.zero_()
    assert ga.violations() == []


@pytest.mark.parametrize("poison", POISONS, ids=["nan", "3e30"])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
def test_a_planted_byte_in_either_band_is_reported(dtype, poison):
    for which, (t, rec) in enumerate(_allocations(dtype, poison)):
        n = rec.n_bytes
        for at, side, offset in ((G - 1, "before", -1), (G + n, "behind", n), (n + 2 * G - 1, "behind", n + G - 1),
                                 (0, "before", -G)):
            old = int(rec.store[at])
            rec.store[at] = old ^ 0x5A                            # plain indexing into the store: one byte
            assert ga.violations() == [(rec.site, side, offset)], (which, at)
            rec.store[at] = old
            assert ga.violations() == []
        rec.store[G - 2] ^= 1                                     # both sides at once: one entry each, first byte each
        rec.store[G + n + 3] ^= 1
        rec.store[G + n + 9] ^= 1
        assert ga.violations() == [(rec.site, "before", -2), (rec.site, "behind", n + 3)]
        rec.store[G - 2] ^= 1
        rec.store[G + n + 3] ^= 1
        rec.store[G + n + 9] ^= 1
    assert ga.violations() == []


def test_sites_name_the_allocating_line_or_the_given_name():
    with ga.guard_allocations(float("nan"), devices=CPU):
        torch.zeros(4)                                            # no frame of the package on the stack: this file's line
    assert ga.REGISTRY[-1].site.startswith("test_guard_alloc_host.py:")
    ga.guarded(torch.zeros(4), name="targets")
    assert ga.REGISTRY[-1].site == "targets"
    ga.REGISTRY[-1].store[G + 16] = 0x55
    assert ga.violations() == [("targets", "behind", 16)]


@pytest.mark.parametrize("poison", POISONS, ids=["nan", "3e30"])
def test_poison_fills_bands_and_uninitialised_interiors(poison):
    with ga.guard_allocations(poison, devices=CPU):
        f = torch.empty(6, dtype=torch.float32)
        b = torch.empty(6, dtype=torch.bfloat16)
        i = torch.empty(6, dtype=torch.int32)
        flag = torch.empty(6, dtype=torch.bool)
        z = torch.zeros(6, dtype=torch.float32)
    want = torch.full((6,), poison)
    assert torch.equal(f.isnan(), want.isnan()) and torch.equal(f.nan_to_num(1.0), want.nan_to_num(1.0))
    assert b.isnan().all() if poison != poison else (b.float() > 1e30).all()
    assert (i == -1).all() and flag.all()
    for t, rec in zip((f, b, i, flag, z), ga.REGISTRY):
        band = rec.store[:G].view(t.dtype) if t.dtype.is_floating_point else rec.store[:G]
        if t.dtype.is_floating_point:
            assert band.isnan().all() if poison != poison else (band.float() > 1e30).all()
        else:
            assert (band == 0xFF).all()
        assert torch.equal(rec.store[:G], rec.lower) and torch.equal(rec.store[G + rec.n_bytes:], rec.upper)
    # the bytes of the two poisons differ everywhere, so a write of one regime's band value shows in the other
    a = torch.full((4,), float("nan")).view(torch.uint8)
    c = torch.full((4,), 3.0e30).view(torch.uint8)
    assert (a != c).all()


def test_poison_without_guards_fills_in_place_and_registers_nothing():
    with ga.poisoned_empty(3.0e30):
        f = torch.empty(5, device="cpu")
        z = torch.zeros(5)
    assert ga.REGISTRY == [] and (z == 0).all()
    assert f.untyped_storage().nbytes() == 20                     # no bands; cpu is not in devices: left as it came
    with ga.guard_allocations(3.0e30, guard=False, devices=CPU):
        f = torch.empty(5)
        m = torch.empty(5, dtype=torch.bool)
        like = torch.empty_like(torch.zeros(3, dtype=torch.float64))
        assert torch.zeros is ga._REAL["zeros"]                   # only the uninitialised two are wrapped
    assert ga.REGISTRY == [] and (f == 3.0e30).all() and m.all() and (like == 3.0e30).all()


def test_wrapped_zeros_full_ones_return_the_requested_values():
    src = torch.arange(12, dtype=torch.float32).view(3, 4)
    with ga.guard_allocations(float("nan"), devices=CPU):
        got = [torch.zeros(2, 3), torch.zeros((2, 3), dtype=torch.int64), torch.zeros_like(src),
               torch.zeros_like(src, dtype=torch.bool), torch.full((4,), float("-inf")), torch.full((2, 2), 7, dtype=torch.int32),
               torch.full_like(src, 2.5), torch.full_like(src, 3, dtype=torch.uint8), torch.ones(5, dtype=torch.float64),
               torch.ones(2, 1, dtype=torch.bool), torch.zeros(3, requires_grad=True)]
    want = [torch.zeros(2, 3), torch.zeros((2, 3), dtype=torch.int64), torch.zeros_like(src),
            torch.zeros_like(src, dtype=torch.bool), torch.full((4,), float("-inf")), torch.full((2, 2), 7, dtype=torch.int32),
            torch.full_like(src, 2.5), torch.full_like(src, 3, dtype=torch.uint8), torch.ones(5, dtype=torch.float64),
            torch.ones(2, 1, dtype=torch.bool), torch.zeros(3, requires_grad=True)]
    assert len(ga.REGISTRY) == len(got)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and g.requires_grad == w.requires_grad and torch.equal(g, w)
    assert got[-1].is_leaf
    assert ga.violations() == []


def test_zero_size_other_devices_and_non_contiguous_requests_pass_through():
    strided = torch.zeros(4, 6).t()                               # empty_like keeps its strides: not contiguous
    with ga.guard_allocations(float("nan"), devices=CPU):
        a = torch.empty(0)
        b = torch.zeros(3, 0, 2)
        c = torch.empty_like(strided)
        d = torch.zeros_like(strided)
        into = torch.zeros(3)
        n_before = len(ga.REGISTRY)
        e = torch.zeros(3, out=into)
    assert n_before == 1 and len(ga.REGISTRY) == 1                # only `into`
    assert a.numel() == 0 and b.shape == (3, 0, 2) and c.stride() == strided.stride() and d.stride() == strided.stride()
    assert (d == 0).all() and e.data_ptr() == into.data_ptr()
    ga.reset()
    with ga.guard_allocations(float("nan")):                      # devices=("cuda",): host tensors are not touched
        h = torch.empty(8)
        z = torch.zeros(8)
    assert ga.REGISTRY == [] and h.untyped_storage().nbytes() == 32 and (z == 0).all()


def test_the_real_functions_are_back_after_the_context_also_on_an_exception():
    real = {n: getattr(torch, n) for n in ga._WRAPPED}
    with ga.guard_allocations(float("nan"), devices=CPU):
        assert all(getattr(torch, n) is not real[n] for n in ga._WRAPPED)
    assert all(getattr(torch, n) is real[n] for n in ga._WRAPPED)
    assert torch.empty is real["empty"]
    with pytest.raises(ZeroDivisionError):
        with ga.guard_allocations(3.0e30, devices=CPU):
            1 / 0
    assert all(getattr(torch, n) is real[n] for n in ga._WRAPPED)
    with pytest.raises(AssertionError):
        with ga.guard_allocations(3.0e30, devices=CPU):
            with ga.guard_allocations(3.0e30, devices=CPU):
                pass
    assert all(getattr(torch, n) is real[n] for n in ga._WRAPPED)


def test_read_only_operands_are_compared_byte_for_byte():
    x = torch.tensor([1.0, float("nan"), -0.0, 3.0])
    m = torch.tensor([True, False, True])
    gx = ga.guarded(x, 3.0e30, name="x", readonly=True)
    gm = ga.guarded(m, 3.0e30, name="mask", readonly=True)
    free = ga.guarded(x, 3.0e30, name="parameter")
    assert ga.changed_operands() == []                            # NaN equals NaN here: bytes, not values
    free.add_(1.0)
    assert ga.changed_operands() == []
    gx[2] = 0.0                                                   # -0.0 -> +0.0: equal as values, not as bytes
    assert ga.changed_operands() == ["x"]
    gm[1] = True
    assert ga.changed_operands() == ["x", "mask"]
    assert ga.violations() == []


def test_reset_forgets_and_the_registry_keeps_stores_alive():
    t = ga.guarded(torch.zeros(4), name="a")
    ptr = t.data_ptr()
    del t
    assert len(ga.REGISTRY) == 1 and ga.REGISTRY[0].store.data_ptr() + G == ptr
    ga.REGISTRY[0].store[0] = 0x55
    assert len(ga.violations()) == 1
    ga.reset()
    assert ga.REGISTRY == [] and ga.violations() == []


def test_the_limit_a_write_beyond_the_band_is_not_seen():
    """What this net cannot catch: the bands are GUARD_BYTES wide, and a stray write further away than that lands in some
    other allocation.  Here the far write goes into a neighbouring tensor carved from the same arena, GUARD_BYTES + 1 bytes
    behind the guarded tensor's store; nothing is reported, although the neighbour is damaged."""
    t = ga.guarded(torch.zeros(16, dtype=torch.float32), name="near")
    rec = ga.REGISTRY[-1]
    arena = torch.zeros(rec.store.numel() + 64, dtype=torch.uint8)           # a model of what lies behind the store
    end_of_tensor = G + rec.n_bytes
    far = end_of_tensor + G + 1                                               # more than GUARD_BYTES behind the tensor
    assert far >= rec.store.numel()                                           # ... which is outside the store
    arena[far] = 0x77
    assert ga.violations() == []
    assert int(arena[far]) == 0x77 and (t == 0).all()
    rec.store[end_of_tensor + G - 1] = 0x77                                   # the last byte that is in reach
    assert ga.violations() == [("near", "behind", rec.n_bytes + G - 1)]
