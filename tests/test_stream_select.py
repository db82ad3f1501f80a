"""CPU-only: stream_select (csrc/stream_select.h) decides what the twelve streaming launchers decided for themselves
before it -- every refusal, the kernel form (as the label), grid, workgroup size and the rows of the partial buffer -- and
bn_bwd_plan decides from the same selection how a whole BatchNorm backward routes its pool gradient.  Both are pure host
functions, so tests/stream_select_main.cpp, compiled here with g++, answers a fixed list of queries, and the answers must
agree line for line with the rules as tests/stream_rules.py restates them, launcher by launcher, from commit a6066eb (the
last one whose launchers selected for themselves).  The same program runs once more under AddressSanitizer and
UndefinedBehaviorSanitizer, and unetpp_bn_bwd_plan / the five wrapper exports of the built library are held against it.

One deliberate difference to that commit, in ops.bn_backward / ops.bn_frozen_backward and not in any launcher: a fp32 call
with a pool gradient and an eligible shape in which some pointer the routing form demands is not 16-byte aligned (gamma,
dgamma, dbeta, mean, invstd, ...; pool_idx: 4 bytes) ran into the launcher's UNETPP_EINVAL in the middle of a backward,
because ops.py asked only unetpp_bn_bwd_pool_ok (frozen: plus a hand-copied part of the alignment demands).  The plan
now gives such a call route 2 -- unetpp_maxpool_bwd into d_act, then the plain forms -- so it computes exactly that
composition (tests/test_gpu_kernels.py holds it to that bit for bit)."""
import ctypes
import itertools
import os
import subprocess

import pytest

from tests import stream_rules as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "unet_nested4tiny_objects_keypoints_amd", "csrc")
LIMIT = R.LIMIT
CHANNELS = (3, 4, 8, 12, 20, 32, 64, 260, 513, 1024, 1028, 2048, 4096)
SHAPES = ((2, 8, 8), (2, 7, 8), (2, 8, 7), (3, 5, 9), (1, 1, 1), (1, 2, 2), (3, 1, 8), (3, 8, 1), (1, 2, 1), (2, 2, 64))
# items at which a grid stops growing: 2048 reduce blocks of 256 threads x 16 items (bf16: x 4), 2048 frozen blocks,
# the 16384-workgroup cap of grid_for
ITEM_CAPS = (2048 * 256 * 16, 2048 * 256 * 4, 2048 * 256, 16384 * 256)


def variants(op):
    """The optional-argument patterns of real calls (every other pattern: flag_queries)."""
    if op == R.AFFINE:
        outs = (dict(act=1), dict(act=1, pooled=1, idx=1), dict(pooled=1, idx=1), dict(act=1, pooled=1))
        return [dict(o, scale=s, shift=s) for o in outs for s in (0, 1)]
    if op == R.POOL_BWD:
        return [dict(dpooled=1, idx=1)]
    pools = (dict(), dict(dpooled=1, idx=1))
    if op == R.BN_FROZEN:
        return [dict(p, stats=1, partial=s) for p in pools for s in (0, 1)]
    return [dict(p, stats=1, partial=1) for p in pools]


def query(op, bf16, n, h, w, c, **kw):
    q = dict(op=op, bf16=bf16, N=n, H=h, W=w, C=c)
    q.update({k: 0 for k in R.FLAGS + R.ROLES})
    q.update(kw)
    # a pointer that was not given has no address bits (the launchers take them from NULL)
    absent = dict(out_lo=op == R.AFFINE and not q["act"], pooled_lo=not (q["pooled"] if op == R.AFFINE else q["dpooled"]),
                  idx_lo=not q["idx"], coef_lo=op == R.AFFINE and not (q["scale"] or q["shift"]),
                  stat_lo=op == R.BN_FROZEN and not q["stats"], gate_lo=not q["gate"])
    q.update({role: 0 for role, gone in absent.items() if gone})
    return q


def shapes_for(c):
    """(N, H, W): even, odd, 1 and 2; (W/2)*(C/4) at 63 / 64; pixel counts on both sides of every cap with a remainder;
    both 31-bit limits."""
    out = list(SHAPES)
    groups = sorted({c} | ({c // 4} if c % 4 == 0 else set()) | ({c // 8} if c % 8 == 0 else set()))
    if c % 4 == 0 and c // 4 <= 64:
        cg = c // 4
        out += [(2, 4, 2 * (63 // cg)), (2, 4, 2 * -(-64 // cg)), (2, 5, 2 * -(-64 // cg))]
    for h, w in ((1, 1), (2, 2), (2, 256)):
        for cg in groups:
            for cap in ITEM_CAPS:
                n0 = cap // (cg * h * w)
                out += [(n, h, w) for n in (n0 - 1, n0, n0 + 1, 2 * n0 + 3) if n >= 1]
            # N*H*W*C < 0x7fffffff (fp32 row forms) and pixels * (C >> 3) < 0x7fffffff (bf16): the last shape inside, the
            # first outside; with one channel group and one pixel per image the counts are 0x7fffffff - 1 and 0x7fffffff
            n0 = (LIMIT - 1) // (cg * h * w)
            out += [(n0, h, w), (n0 + 1, h, w)]
        # image rows (N * H) and window rows (N * H/2) around the 16384 rows of the row forms
        if h == 2:
            out += [(n, h, w) for n in (8191, 8192, 8193, 16383, 16384, 16385, 40001)]
    return sorted(set(out))


def flag_queries():
    """Every combination of the optional-argument flags, accepted or refused."""
    qs = []
    for op, bf16, c in itertools.product(range(5), (0, 1), (8, 64)):
        for bits in itertools.product((0, 1), repeat=len(R.FLAGS)):
            qs.append(query(op, bf16, 2, 8, 64, c, **dict(zip(R.FLAGS, bits))))
    return qs


def misaligned_queries():
    """Each pointer role misaligned in turn: by 4 bytes (and 8); the index bytes by 1, 2, 4 and 8 (fp32 reads them in
    4-byte words, bf16 in 8-byte ones)."""
    qs = []
    for op, bf16, c, (n, h, w) in itertools.product(range(5), (0, 1), (3, 8, 12, 32, 64, 1024), ((2, 8, 8), (2, 8, 64), (2, 7, 9))):
        for v in variants(op):
            if op == R.POOL_BWD and bf16:
                v = dict(v, gate=1)
            for role in R.ROLES:
                for off in ((1, 2, 4, 8) if role == "idx_lo" else (4, 8)):
                    qs.append(query(op, bf16, n, h, w, c, **dict(v, **{role: off})))
    return qs


def stream_queries():
    qs = []
    for op, bf16, c in itertools.product(range(5), (0, 1), CHANNELS):
        for (n, h, w) in shapes_for(c):
            for v in variants(op):
                qs.append(query(op, bf16, n, h, w, c, **v))
        for bad in (dict(n=0), dict(h=0), dict(w=0), dict(c=0), dict(c=-8)):
            shape = dict(dict(n=2, h=8, w=8, c=c), **bad)
            qs += [query(op, bf16, shape["n"], shape["h"], shape["w"], shape["c"], **v) for v in variants(op)]
    return qs + flag_queries() + misaligned_queries()


def plan_queries():
    """(frozen, bf16, sums, pool, N, H, W, C, bits of the seven roles)"""
    qs = []
    roles = R.ROLES[:-1]
    for frozen, bf16, pool, c in itertools.product((0, 1), (0, 1), (0, 1), CHANNELS):
        for sums in ((0, 1) if frozen else (1,)):
            for (n, h, w) in SHAPES + ((2, 4, 256), (8193, 2, 64), ((LIMIT - 1) // (4 * c), 2, 2), ((LIMIT - 1) // (4 * c) + 1, 2, 2),
                                       (0, 8, 8), (2 * 2048 * 4096 // c + 3, 1, 1)):
                qs.append((frozen, bf16, sums, pool, n, h, w, c) + (0,) * len(roles))
            for i, role in enumerate(roles):
                for off in ((1, 2, 4, 8) if role == "idx_lo" else (4, 8)):
                    bits = tuple(off if j == i else 0 for j in range(len(roles)))
                    for (n, h, w) in ((2, 6, 10), (2, 6, 16), (2, 7, 9)):
                        qs.append((frozen, bf16, sums, pool, n, h, w, c) + bits)
    return qs


def plan_expect(p):
    frozen, bf16, sums, pool, n, h, w, c = p[:8]
    bits = dict(zip(R.ROLES[:-1], p[8:]))
    rows = R.partial_rows(bf16, frozen, n * h * w, c)

    def accept(op, **kw):
        q = query(op, bf16, n, h, w, c, **dict(bits, stats=1, partial=int(not frozen or sums), **kw))
        return R.launcher_of(q)(q)[0] == R.OK

    def passes(**kw):
        return accept(R.BN_FROZEN, **kw) if frozen else accept(R.BN_REDUCE, **kw) and accept(R.BN_APPLY, **kw)

    fused = pool and passes(dpooled=1, idx=1)
    plain = passes(pooled_lo=0, idx_lo=0) and (not pool or accept(R.POOL_BWD, dpooled=1, idx=1, out_lo=bits["in_lo"]))   # into d_act
    route = (0 if plain else None) if not pool else 1 if fused else 2 if plain else None
    return "%d %d %d %d" % (((R.EINVAL, 0) if route is None else (R.OK, route)) + (rows, rows * c * 2))


def line_of(q):
    return "S %d %d %d %d %d %d " % (q["op"], q["bf16"], q["N"], q["H"], q["W"], q["C"]) + \
        " ".join(str(q[k]) for k in R.FLAGS + R.ROLES)


def build(tmp, name, *flags):
    exe = str(tmp / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC, "-I",
                    os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "stream_select_main.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("stream_select")
    qs, ps = stream_queries(), plan_queries()
    text = "\n".join([line_of(q) for q in qs] + ["P " + " ".join(map(str, p)) for p in ps]) + "\n"
    out = subprocess.run([build(tmp, "stream_select_main")], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(qs) + len(ps)
    return tmp, qs, ps, text, out


def test_selection_matches_the_launchers_rules(work):
    _, qs, _, _, out = work
    seen = set()
    for q, got in zip(qs, out):
        fn = R.launcher_of(q)
        rc, ans = fn(q)
        want = "%d %s %d %d %d %d" % ((rc,) + ans)
        assert got == want, (line_of(q), got, want)
        seen.add((fn.__name__, rc))
    launchers = {"affine", "affine_bf16", "maxpool_bwd", "maxpool_bwd_bf16", "bn_bwd_reduce", "bn_bwd_reduce_pool",
                 "bn_bwd_reduce_bf16", "bn_bwd_apply", "bn_bwd_apply_pool", "bn_bwd_apply_bf16", "bn_frozen_bwd",
                 "bn_frozen_bwd_bf16"}
    assert {name for name, _ in seen} == launchers
    for name in launchers:      # every launcher both accepted and refused
        assert (name, R.OK) in seen and (name, R.EINVAL) in seen, name


def test_labels_are_those_the_gpu_tests_cover(work):
    from tests.test_gpu_bn_frozen import COVERAGE as FROZEN
    from tests.test_gpu_streaming import COVERAGE as STREAMING
    others = ("bn_finalize", "bn_eval_coeffs", "bn_bwd_finalize", "bilinear2x", "nchw_to_nhwc", "nhwc_to_nchw")
    want = {name for name in STREAMING + FROZEN if not name.startswith(others)}
    _, qs, _, _, out = work
    got = {line.split()[1] for line in out[:len(qs)]} - {"-"}
    assert want - got == set(), "labels no query produced"
    assert got - want == set(), "labels no GPU test covers"


def test_plan_routes_by_the_launchers_rules(work):
    _, qs, ps, _, out = work
    seen = set()
    for p, got in zip(ps, out[len(qs):]):
        want = plan_expect(p)
        assert got == want, (p, got, want)
        seen.add((p[0], p[1], p[3], got.split()[0], got.split()[1]))
    for frozen, bf16 in itertools.product((0, 1), (0, 1)):
        assert (frozen, bf16, 0, "0", "0") in seen and (frozen, bf16, 1, "0", "1") in seen and (frozen, bf16, 1, "-1", "0") in seen
        assert ((frozen, bf16, 1, "0", "2") in seen) == (not bf16)     # bf16 storage has no form that routes by a pass of its own


def test_sanitized_build_gives_the_same_answers(work):
    tmp, _, _, text, out = work
    exe = build(tmp, "stream_select_main_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    run = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    assert run.stdout.splitlines() == out


def test_library_plan_and_wrapper_exports_agree(work):
    """unetpp_bn_bwd_plan of the built library (it loads without a GPU) against the stand-alone program on the same plan
    queries, with made-up addresses that carry the queries' low bits; the five wrapper exports against the plan."""
    from unet_nested4tiny_objects_keypoints_amd import _lib
    _lib.build_library()
    lib = _lib.lib()
    _, qs, ps, _, out = work
    base = 0x7f0000001000
    for p, want in zip(ps, out[len(qs):]):
        frozen, bf16, sums, pool, n, h, w, c = p[:8]
        if not -2 ** 31 <= n < 2 ** 31:
            continue
        in_lo, out_lo, pooled_lo, idx_lo, coef_lo, stat_lo, gamma_lo = p[8:]
        ptrs = [base + in_lo, base, base + out_lo, base + coef_lo, base, base + stat_lo, base, base + gamma_lo, base, base,
                base + pooled_lo if pool else None, base + idx_lo if pool else None]
        q = _lib.BnBwdQuery(frozen, bf16, sums, n, h, w, c, 0, *ptrs)
        sizes = _lib.BnBwdSizes()
        rc = lib.unetpp_bn_bwd_plan(ctypes.byref(q), ctypes.byref(sizes))
        assert "%d %d %d %d" % (rc, sizes.route, sizes.partial_rows, sizes.partial_floats) == want, p
        blocks = {(0, 0): lib.unetpp_bn_bwd_blocks, (0, 1): lib.unetpp_bn_bwd_blocks_bf16,
                  (1, 0): lib.unetpp_bn_frozen_bwd_blocks, (1, 1): lib.unetpp_bn_frozen_bwd_blocks_bf16}[(frozen, bf16)]
        assert blocks(n * h * w, c) == sizes.partial_rows, p
        if pool and not bf16 and not any(p[8:]):
            assert lib.unetpp_bn_bwd_pool_ok(n, h, w, c) == (sizes.route == 1) == R.bn_bwd_pool_ok(n, h, w, c), p
    sizes = _lib.BnBwdSizes()
    good = _lib.BnBwdQuery(0, 0, 1, 2, 6, 10, 8, 0, *([base] * 12))
    assert lib.unetpp_bn_bwd_plan(None, ctypes.byref(sizes)) == -1 and lib.unetpp_bn_bwd_plan(ctypes.byref(good), None) == -1
    assert lib.unetpp_bn_bwd_plan(ctypes.byref(good), ctypes.byref(sizes)) == 0 and sizes.route == 1
    good.pool_idx = None        # half a pool gradient
    assert lib.unetpp_bn_bwd_plan(ctypes.byref(good), ctypes.byref(sizes)) == -1
