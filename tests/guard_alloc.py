"""Guard-banded, poisoned allocations with a registry, and the checker that reads the bands back.

Shared test infrastructure (no tests here).  Every tensor handed out by ``guarded()`` or, inside ``guard_allocations()``,
by the wrapped ``torch.empty`` / ``empty_like`` / ``zeros`` / ``zeros_like`` / ``full`` / ``full_like`` / ``ones`` lies in
the middle of a raw ``uint8`` store of ``n_bytes + 2 * GUARD_BYTES`` bytes whose bands hold poison:

* a READ before the first or behind the last element lands in poison and changes a result;
* a WRITE there changes the band: ``violations()`` compares both bands, byte by byte, with the copies taken when the
  tensor was handed out, and names the allocation (``file:line`` of the allocating line of the package, or the name
  given to ``guarded()``), the side and the byte.

The stores are raw bytes because a typed store does not round-trip: ``torch.bool`` filled with 0xFF comes back from
``clone()`` as 0x01.  Floating storage is poisoned with the typed value (NaN, or a large finite value that also survives
compare-and-select masking of NaN), everything else with 0xFF bytes.  A kernel that writes the very bytes a band already
holds cannot be seen under that poison: the fronts run under both, whose bytes differ.

LIMIT: a write more than ``GUARD_BYTES`` away from the tensor lands outside the store and is not seen.

The registry keeps every store alive until ``reset()``: nothing is handed back to the caching allocator, overwritten by a
later tensor and thereby forgiven.
"""
import contextlib
import os
import sys

import torch

GUARD_BYTES = 8192   # band on either side of a tensor: a multiple of 256, so the interior keeps a fresh allocation's
#                      alignment and the launchers select what they select without guards (the widest halo row of the
#                      path is 34 pixels x 256 B)

_WRAPPED = ("empty", "empty_like", "zeros", "zeros_like", "full", "full_like", "ones")
_REAL = {name: getattr(torch, name) for name in _WRAPPED}
_HERE = os.path.abspath(__file__)
_TESTS = os.path.dirname(_HERE)
_PACKAGE = os.path.join(os.path.dirname(_TESTS), "unet_nested4tiny_objects_keypoints_amd") + os.sep


class Record:
    """One guarded allocation: where it was made, its store, and what its bands held when it was handed out."""
    __slots__ = ("site", "store", "n_bytes", "lower", "upper", "original")

    def __init__(self, site, store, n_bytes, original=None):
        self.site, self.store, self.n_bytes, self.original = site, store, n_bytes, original
        self.lower = store[:GUARD_BYTES].clone()
        self.upper = store[GUARD_BYTES + n_bytes:].clone()

    def interior(self):
        return self.store[GUARD_BYTES:GUARD_BYTES + self.n_bytes]


REGISTRY = []


def reset():
    """Forget every allocation made so far (and let go of the stores)."""
    del REGISTRY[:]


def _fill(t, value, devices=("cuda",)):
    """Poison the whole of `t` in place: floating storage with `value`, everything else (integers, bool) with 0xFF bytes."""
    if t.device.type in devices and t.numel():
        if t.dtype.is_floating_point:
            t.fill_(value)
        else:
            t.view(-1).view(torch.uint8).fill_(0xFF)
    return t


def _site():
    """file:line of the innermost frame inside the package; failing that, of the innermost frame outside this file."""
    f = sys._getframe(1)
    fallback = None
    while f is not None:
        name = os.path.abspath(f.f_code.co_filename)
        if name.startswith(_PACKAGE):
            return "%s:%d" % (os.path.relpath(name, os.path.dirname(_TESTS)), f.f_lineno)
        if fallback is None and name != _HERE and not name.endswith("contextlib.py"):
            fallback = "%s:%d" % (os.path.basename(name), f.f_lineno)
        f = f.f_back
    return fallback or "?"


def _make(shape, dtype, device, value, site, original=None):
    n = _REAL["empty"]((), dtype=dtype).element_size()
    for d in shape:
        n *= int(d)
    store = _REAL["empty"](n + 2 * GUARD_BYTES, dtype=torch.uint8, device=device)
    if dtype.is_floating_point:
        store.view(dtype).fill_(value)
    else:
        store.fill_(0xFF)
    REGISTRY.append(Record(site, store, n, original))
    return store[GUARD_BYTES:GUARD_BYTES + n].view(dtype).view(tuple(shape))


def guarded(t, value=float("nan"), real_empty=None, name=None, readonly=False):
    """A copy of the tensor `t` that sits between two guard bands filled with `value` (same shape, dtype, contiguous,
    256-byte aligned): a kernel that reads before the first or past the last element of the tensor reads the guard, one
    that writes there is reported by violations() under `name`.  readonly=True: changed_operands() also reports the copy
    if its bytes ever differ from those of `t`."""
    out = _make(t.shape, t.dtype, t.device, value, name or _site(), t if readonly else None)
    out.copy_(t.detach())
    return out


def _first_difference(got, want):
    if torch.equal(got, want):
        return None
    return int((got != want).nonzero()[0])


def violations():
    """[(site, "before" | "behind", offset)] of every band byte that no longer holds what it held when the tensor was
    handed out.  The offset counts bytes from the tensor's first byte: negative before it, >= its size behind it; one
    entry per side, for the first differing byte.  Synchronise the device first."""
    bad = []
    for r in REGISTRY:
        at = _first_difference(r.store[:GUARD_BYTES], r.lower)
        if at is not None:
            bad.append((r.site, "before", at - GUARD_BYTES))
        at = _first_difference(r.store[GUARD_BYTES + r.n_bytes:], r.upper)
        if at is not None:
            bad.append((r.site, "behind", r.n_bytes + at))
    return bad


def changed_operands():
    """Sites of the guarded(..., readonly=True) copies whose bytes differ from the tensor they were copied from."""
    bad = []
    for r in REGISTRY:
        if r.original is not None:
            want = r.original.detach().contiguous().view(-1).view(torch.uint8)
            if not torch.equal(r.interior(), want):
                bad.append(r.site)
    return bad


@contextlib.contextmanager
def guard_allocations(value, guard=True, devices=("cuda",)):
    """Every tensor that Python code allocates uninitialised on one of `devices` comes back poisoned: float('nan') or a
    large finite value for floating storage, 0xFF bytes otherwise.  guard=True: it also sits between two guard bands of
    the same filling and is registered for violations(); and ``torch.zeros`` / ``zeros_like`` / ``full`` / ``full_like``
    / ``ones`` are wrapped as well -- the interior holds the requested values, the bands hold poison.  Tensors elsewhere
    (pinned host staging), empty ones and non-contiguous ones pass through unchanged.  The real functions are back on
    exit, also on an exception.  Not re-entrant."""
    assert all(getattr(torch, n) is _REAL[n] for n in _WRAPPED), "guard_allocations() is already active"

    def eligible(t, k):
        return (guard and "out" not in k and t.device.type in devices and t.numel() and t.is_contiguous()
                and t.layout == torch.strided)

    def uninitialised(real):
        def wrapper(*a, **k):
            t = real(*a, **k)
            if eligible(t, k):
                out = _make(t.shape, t.dtype, t.device, value, _site())
                return out.requires_grad_() if t.requires_grad else out
            return _fill(t, value, devices) if "out" not in k else t
        return wrapper

    def initialised(real):
        def wrapper(*a, **k):
            t = real(*a, **k)
            if eligible(t, k):
                out = _make(t.shape, t.dtype, t.device, value, _site())
                out.copy_(t.detach())
                return out.requires_grad_() if t.requires_grad else out
            return t
        return wrapper

    torch.empty, torch.empty_like = uninitialised(_REAL["empty"]), uninitialised(_REAL["empty_like"])
    if guard:
        for n in ("zeros", "zeros_like", "full", "full_like", "ones"):
            setattr(torch, n, initialised(_REAL[n]))
    try:
        yield
    finally:
        for n in _WRAPPED:
            setattr(torch, n, _REAL[n])


def poisoned_empty(value, guard=False):
    """The regime of the earlier tests: guard=False poisons ``torch.empty`` / ``empty_like`` in place and wraps nothing
    else; guard=True is guard_allocations(value)."""
    return guard_allocations(value, guard)
