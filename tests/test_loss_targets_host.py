"""The checker of tests/loss_oracle.py, tested without a GPU: a float32 restatement of focal_thread's arithmetic passes
it on every input set of tests/test_gpu_loss_targets.py and tests/test_gpu_caller.py, the input sets keep the intervals
narrow, and each of six subtly wrong kernels (mutations of the restatement) FAILS it.

Why tests/test_gpu_caller.py::test_focal_loss_value_and_gradient changed: its gradient line was
``rel_err(grad, ref) < 1e-4`` = max|a - b| / max|b| with one planted |d| = 1 element whose gradient is 1e20 / rows, so
every other element could be wrong by 1e14.  test_old_assertion_lets_the_dropped_log_term_through shows it passing a
kernel without the gamma u^(gamma-1) log e term; the per-element interval that replaces it rejects that kernel."""
import numpy as np
import pytest
import torch

from tests import loss_oracle as lo
from tests.helpers import rel_err

GAMMAS = (3, 2, 2.5, 1)
CALLER_SHAPES = [(2, 4, 16, 16), (3, 5, 24, 40), (1, 4, 7, 9), (4, 4, 64, 64)]


def _sets():
    """(label, pred, target, gamma, rows) of every input set the GPU tests use"""
    for n in lo.TAIL_SIZES:
        for gamma in GAMMAS:
            for rows in (1, 3):
                yield ("tail n=%d gamma=%s rows=%d" % (n, gamma, rows),) + lo.tail_inputs(n) + (gamma, rows)
    for gamma in (0, 0.5):
        for n in (5, 2051):
            yield ("tail n=%d gamma=%s rows=3" % (n, gamma),) + lo.tail_inputs(n) + (gamma, 3)
    for heads in (1, 2, 5, 8):
        preds, t = lo.heads_inputs(heads, 2051)
        for h, p in enumerate(preds):
            yield ("heads=%d head %d" % (heads, h), p, t, 3, 3)
    for shape in CALLER_SHAPES:
        p, t = lo.caller_inputs(shape)
        for gamma in (3, 2.5):
            yield ("caller %s gamma=%s" % (shape, gamma), p, t, gamma, shape[0] * shape[1])


def _verdict(p, t, gamma, rows, mutation=None, drop_block=0):
    """-> (complaints about the gradient, loss ratio) of the restatement (mutated or not) under the checker"""
    iv = lo.focal_interval(p, t, gamma, rows)
    loss, grad = lo.restate_f32(p, t, gamma, rows, mutation, drop_block)
    bad, _ = lo.check_grad(grad, iv)
    return bad, lo.loss_ratio(loss, lo.loss_bound(iv))


def test_restatement_passes_on_every_small_input_set():
    failures = []
    for label, p, t, gamma, rows in _sets():
        bad, lr = _verdict(p, t, gamma, rows)
        if bad or not lr <= 1.0:
            failures.append((label, bad, lr))
    assert not failures, failures[:5]


@pytest.mark.parametrize("region", sorted(lo.BIG_REGIONS))
def test_restatement_passes_on_the_1026_block_sets(region):
    p, t = lo.region_inputs(region)
    assert lo.loss_blocks(p.size) == 1026
    bad, lr = _verdict(p, t, 3, 3)
    assert not bad and lr <= 1.0, (bad, lr)


def test_intervals_are_narrow_on_the_random_elements():
    """median (hi - lo) / |want| <= 1e-3 over the elements that are neither exact hits nor |d| = 1"""
    wide = []
    sets = list(_sets()) + [("region " + r,) + lo.region_inputs(r) + (3, 3) for r in sorted(lo.BIG_REGIONS)]
    for label, p, t, gamma, rows in sets:
        iv = lo.focal_interval(p, t, gamma, rows)
        rnd = ~iv.hit & ~iv.unit
        if not rnd.any():
            continue
        if not label.startswith("caller"):   # the sets drawn for these tests: nothing else than the three kinds
            assert float(np.abs(iv.d[rnd]).max()) <= lo.MAX_D
        med = float(np.median((iv.hi[rnd] - iv.lo[rnd]) / np.abs(iv.want[rnd])))
        if not med <= 1e-3:
            wide.append((label, med))
    assert not wide, wide


def test_oracle_is_the_modules_own_cpu_statement():
    """focal_terms summed = the torch statement of FocalLoss_BCE_2d in float64, value and autograd gradient"""
    for gamma in (3, 2.5, 1):
        p, t = lo.caller_inputs((3, 5, 24, 40))
        rows = 15
        tm = lo.focal_terms(p, t, gamma, rows)
        p64 = torch.from_numpy(p).double().requires_grad_(True)
        e = 1 - torch.abs(p64 - torch.from_numpy(t).double()) + 1e-20
        loss = (-1 * (1 - e) ** gamma * torch.log(e)).sum() / rows
        loss.backward()
        # (the oracle's e at the one |d| = 1 is the kernel's float32(1e-20), within 2^-24 of torch's 1e-20: that
        # much on its log, and on its gradient below)
        assert abs(tm.loss_term.sum() / rows - loss.item()) <= 2.0 ** -24 / rows + 1e-12 * loss.item()
        got, want = tm.grad, p64.grad.numpy().ravel()
        # (torch forms 1 - e in float64: an absolute 1e-16 on u, relative gamma * 1e-16 / u on the gradient)
        assert np.all(np.abs(got - want) <= np.where(np.abs(tm.d) == 1, 2.0 ** -24, 1e-9) * np.abs(want) + 1e-15)
    # gamma < 1 at an exact hit: loss term 0, gradient 0 (torch's CPU path gives 0 for gamma 0 and NaN for 0.5)
    p, t = lo.tail_inputs(9)
    for gamma in (0, 0.5):
        tm = lo.focal_terms(p, t, gamma, 3)
        hit = tm.d == 0
        assert hit.any() and np.all(tm.loss_term[hit] == 0) and np.all(tm.grad[hit] == 0) and np.isfinite(tm.grad).all()


@pytest.mark.parametrize("mutation", ["log_term_dropped", "sign_flipped_for_negative_d", "inv_rows_twice"])
def test_elementwise_mutations_fail(mutation):
    for gamma in GAMMAS:
        for n in (5, 2051, 4099):
            p, t = lo.tail_inputs(n)
            assert not _verdict(p, t, gamma, 3)[0]
            bad, _ = _verdict(p, t, gamma, 3, mutation)
            assert bad, (mutation, gamma, n)
    for shape in CALLER_SHAPES:
        p, t = lo.caller_inputs(shape)
        bad, _ = _verdict(p, t, 3, shape[0] * shape[1], mutation)
        assert bad, (mutation, shape)


def test_tail_gradient_left_at_zero_fails():
    for n in lo.TAIL_SIZES:
        if n % 4 == 0:
            continue
        p, t = lo.tail_inputs(n)
        bad, _ = _verdict(p, t, 3, 3, "tail_gradient_left_zero")
        assert bad, n


def test_loss_missing_one_block_fails():
    for n, block in ((2049, 0), (2049, 1), (2051, 1), (4099, 1), (4099, 2)):
        p, t = lo.tail_inputs(n)
        bad, lr = _verdict(p, t, 3, 3, "loss_misses_one_block", block)
        assert not bad and lr > 1.0, (n, block, lr)
    for region in ("block0", "block1023", "block1024", "last5"):
        p, t = lo.region_inputs(region)
        _, lr = _verdict(p, t, 3, 3, "loss_misses_one_block", lo.BIG_REGIONS[region][0] // lo.BLOCK)
        assert lr > 1.0, (region, lr)


@pytest.mark.parametrize("region", ["block1024", "last5"])
def test_loss_missing_the_second_strided_trip_fails(region):
    p, t = lo.region_inputs(region)
    bad, lr = _verdict(p, t, 3, 3, "loss_misses_partials_from_1024")
    assert not bad and lr > 1.0, lr


@pytest.mark.parametrize("shape", CALLER_SHAPES)
@pytest.mark.parametrize("gamma", [3, 2.5])
def test_old_assertion_lets_the_dropped_log_term_through(shape, gamma):
    p, t = lo.caller_inputs(shape)
    rows = shape[0] * shape[1]
    ref = lo.focal_terms(p, t, gamma, rows).grad
    _, grad = lo.restate_f32(p, t, gamma, rows, "log_term_dropped")
    assert rel_err(grad, ref.astype(np.float32)) < 1e-4               # the old line: passes the wrong kernel
    assert lo.check_grad(grad, lo.focal_interval(p, t, gamma, rows))[0]  # the new check: rejects it
