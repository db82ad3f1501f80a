"""CPU-only: head_select (csrc/head_select.h) decides what the six head launchers decided for themselves before it --
every refusal and its return code, the kernel form and its template coordinates (as the label), grid, workgroup size,
dynamic LDS bytes and the bf16 backward's `active` count.  It is a pure host function, so tests/head_select_main.cpp,
compiled here with g++, answers a fixed list of queries, and the rules are restated below launcher by launcher as
commit 353cdf6 (the last one whose launchers selected for themselves) states them in pointwise.hip and
pointwise_bf16.hip, in the manner of spans() in tests/test_gpu_heads.py.  The answers must agree line for line.

One deliberate difference to that commit: unetpp_head_bwd_bf16 asked for the CU count before its last argument check, so
a call with a misaligned mask and no device returned UNETPP_ELAUNCH; every refusal now comes first (UNETPP_EINVAL)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "unet_nested4tiny_objects_keypoints_amd", "csrc")
OK, EINVAL, ELAUNCH = 0, -1, -2
FWD, MEAN, BWD = 0, 1, 2
MAX_C, MAX_CLS, MAX_HEADS, THREADS = 128, 8, 8, 256
LIMIT = 0x7fffffff
REFUSED = ("-", 0, 0, 0, 0)

CHANNELS = (3, 4, 8, 12, 16, 20, 32, 64, 128, 132, 256)
DROPS = ((0.0, 0), (0.4, 0), (0.4, 1), (0.0, 1))     # (p_drop, mask given): modes 0, 1, 2, and an unused mask


def cdiv(a, b):
    return -(-a // b)


def pow2(v):
    return v > 0 and v & (v - 1) == 0


def log2(v):
    return v.bit_length() - 1


def grid_for(items, cap=2048 * 8):
    return max(1, min(cdiv(items, THREADS), cap))


def head_args_ok(q):       # pointwise.hip head_args_ok
    return (q["N"] >= 1 and q["H"] >= 1 and q["W"] >= 1 and 1 <= q["C"] <= MAX_C and 1 <= q["n_cls"] <= MAX_CLS and
            0.0 <= q["p"] < 1.0)


def head_bf16_ok(q):       # pointwise_bf16.hip head_bf16_ok
    c = q["C"]
    return head_args_ok(q) and c >= 8 and c % 8 == 0 and pow2(c >> 3)


def a16(lo):
    return lo & 15 == 0


def head_bwd_blocks(pixels):
    return min(cdiv(pixels, 64), 4096)


def drop_mode(q):
    return 0 if not q["p"] > 0 else (2 if q["mask"] else 1)


def fp32_fwd(q):
    if not head_args_ok(q):
        return EINVAL, REFUSED
    pixels, c, g4 = q["N"] * q["H"] * q["W"], q["C"], q["C"] >> 2
    pcls = 4 if q["n_cls"] <= 4 else 8
    if (c % 4 == 0 and a16(q["x"]) and a16(q["w"]) and pow2(g4) and g4 <= 32 and pcls <= g4 and pixels * c < LIMIT and
            (not q["mask"] or q["mask_lo"] & 3 == 0)):
        ppb = THREADS // g4
        return OK, ("head_fwd_stream<%d,%d,%d>" % (log2(g4), pcls, drop_mode(q)), min(cdiv(pixels, ppb), 4096), 256, 0, 0)
    if c % 4 == 0 and a16(q["x"]):
        return OK, ("head_fwd_tiled", min(cdiv(pixels, 64), 4096), 64, 64 * (c + 1) * 4, 0)
    return OK, ("head_fwd", grid_for(pixels), 256, 0, 0)


def fp32_mean(q):
    if not (1 <= q["heads"] <= MAX_HEADS) or not head_args_ok(q):
        return EINVAL, REFUSED
    pixels, c, g4 = q["N"] * q["H"] * q["W"], q["C"], q["C"] >> 2
    pcls = 4 if q["n_cls"] <= 4 else 8
    vec = c % 4 == 0 and a16(q["x"]) and a16(q["w"])     # every head's x and weight
    if vec and pow2(g4) and g4 <= 32 and pcls <= g4 and pixels * c < LIMIT:
        ppb = THREADS // g4
        return OK, ("heads_mean_stream<%d,%d>" % (log2(g4), pcls), min(cdiv(pixels, ppb), 4096), 256, 0, 0)
    return OK, ("heads_mean", grid_for(pixels), 256, 0, 0)


def fp32_bwd(q):
    if not head_args_ok(q):
        return EINVAL, REFUSED
    pixels, c, g4, k = q["N"] * q["H"] * q["W"], q["C"], q["C"] >> 2, q["n_cls"]
    grid = head_bwd_blocks(pixels)
    if (c % 4 == 0 and a16(q["x"]) and a16(q["dx"]) and a16(q["w"]) and pow2(g4) and 2 <= g4 <= 32 and
            pixels * c < LIMIT and (not q["mask"] or q["mask_lo"] & 3 == 0)):
        lds = (64 * (c + 1) + 64 * MAX_CLS + 2 * k * c) * 4
        return OK, ("head_bwd_pow2<%d,%d,%d>" % (log2(g4), drop_mode(q), 4 if k <= 4 else 8), grid, 256, lds, 0)
    if c % 4 == 0 and a16(q["x"]) and a16(q["dx"]):
        return OK, ("head_bwd_vec", grid, 256, (64 * (c + 1) + 64 * MAX_CLS + MAX_CLS * c + 2 * k * c) * 4, 0)
    return OK, ("head_bwd", grid, 256, 0, 0)


def pcls_bf16(k):
    return 4 if k <= 4 else 6 if k <= 6 else 8


def bf16_fwd(q):
    if not a16(q["x"]) or not head_bf16_ok(q):
        return EINVAL, REFUSED
    pixels, cg = q["N"] * q["H"] * q["W"], q["C"] >> 3
    if pixels >= LIMIT:
        return EINVAL, REFUSED
    drop = drop_mode(q)
    if drop == 2 and q["mask_lo"] & 7:
        return EINVAL, REFUSED
    grid = min(cdiv(pixels, THREADS // cg), 4096)
    return OK, ("head_fwd_bf16<%d,%d,%d>" % (log2(cg), drop, pcls_bf16(q["n_cls"])), grid, 256, 0, 0)


def bf16_mean(q):
    c = q["C"]
    if (not (1 <= q["heads"] <= MAX_HEADS) or q["N"] < 1 or q["H"] < 1 or q["W"] < 1 or not 1 <= c <= MAX_C or
            not 1 <= q["n_cls"] <= MAX_CLS):
        return EINVAL, REFUSED
    if q["x"] & 1:
        return EINVAL, REFUSED
    pixels, cg = q["N"] * q["H"] * q["W"], c >> 3
    if a16(q["x"]) and c % 8 == 0 and pow2(cg) and pixels < LIMIT:
        pc = pcls_bf16(q["n_cls"])
        grid = min(cdiv(pixels, THREADS // cg), 4096)
        return OK, ("heads_mean_bf16<%d,%d>" % (log2(cg), pc), grid, 256, q["heads"] * pc * c * 4, 0)
    return OK, ("heads_mean_bf16_general", grid_for(pixels), 256, 0, 0)


def bf16_bwd(q):
    if not a16(q["x"]) or not a16(q["dx"]) or not head_bf16_ok(q):
        return EINVAL, REFUSED
    pixels, c = q["N"] * q["H"] * q["W"], q["C"]
    if pixels >= LIMIT:
        return EINVAL, REFUSED
    drop = drop_mode(q)
    if drop == 2 and q["mask_lo"] & 7:       # (the parent checked this after the CU count: see the module docstring)
        return EINVAL, REFUSED
    if q["cus"] <= 0:
        return ELAUNCH, REFUSED
    grid = min(cdiv(pixels, 64), 4096)
    lds = (256 * MAX_CLS + 4 * (MAX_CLS * c + MAX_CLS)) * 4
    active = grid
    n_tiles, most = cdiv(pixels, 256), q["wgs"] * q["cus"]
    if q["wgs"] > 0 and most < n_tiles:
        rounds = cdiv(n_tiles, most)
        active = cdiv(n_tiles, rounds)
    active = min(active, grid)
    return OK, ("head_bwd_bf16<%d,%d,%d>" % (log2(c >> 3), drop, pcls_bf16(q["n_cls"])), grid, 256, lds, active)


LAUNCHERS = {(FWD, 0): fp32_fwd, (MEAN, 0): fp32_mean, (BWD, 0): fp32_bwd,
             (FWD, 1): bf16_fwd, (MEAN, 1): bf16_mean, (BWD, 1): bf16_bwd}


def pixel_counts(c):
    under = (LIMIT - 1) // c       # fp32 templated forms: pixels * C < 2^31 - 1; bf16: pixels < 2^31 - 1
    return sorted({1, 63, 64, 65, 4096 * 64 + 1, 2304 * 256, under, under + 1, LIMIT - 1, LIMIT})


def query(op, bf16, c, k, pixels=65, p=0.0, mask=0, heads=3, x=0, w=0, dx=0, mask_lo=0, wgs=4, cus=256, n=1, h=1):
    return dict(op=op, bf16=bf16, N=n, H=h, W=pixels, C=c, n_cls=k, heads=heads if op == MEAN else 0, p=p, mask=mask,
                x=x, w=w, dx=dx, mask_lo=mask_lo, wgs=wgs, cus=cus)


def queries():
    qs = []
    for (op, bf16) in LAUNCHERS:
        drops = ((0.0, 0),) if op == MEAN else DROPS
        for c in CHANNELS:
            for k in range(10):
                for p, mask in drops:
                    for pixels in pixel_counts(c):
                        qs.append(query(op, bf16, c, k, pixels, p, mask))
            # each pointer role misaligned in turn: x by 4 bytes (a mean source also by 1 and by 2), weight, dx, the
            # mask by 1 and by 4
            for k in (1, 5, 8):
                for p, mask in drops:
                    for role in (dict(x=4), dict(x=1), dict(x=2), dict(w=4), dict(dx=4), dict(mask_lo=1), dict(mask_lo=4)):
                        qs.append(query(op, bf16, c, k, 65, p, mask, **role))
            # the bf16 backward's active count; the CU count must not matter anywhere else
            for pixels in pixel_counts(c):
                for cus in (0, 8, 256):
                    for wgs in (0, 4):
                        qs.append(query(op, bf16, c, 5, pixels, 0.0 if op == MEAN else 0.4, cus=cus, wgs=wgs))
        # argument refusals, with and without a device
        for bad in (dict(n=0), dict(h=0), dict(pixels=0), dict(p=1.0), dict(p=-0.25), dict(heads=0), dict(heads=9),
                    dict(heads=8), dict(heads=1), dict(p=0.4, mask=1, mask_lo=1), dict(p=0.4, mask=1, mask_lo=4)):
            if op == MEAN and "p" in bad:
                continue
            for cus in (0, 256):
                qs.append(query(op, bf16, 32, 5, cus=cus, **bad))
    return qs


def line_of(q):
    return "%d %d %d %d %d %d %d %d %.9g %d %d %d %d %d %d %d" % (
        q["op"], q["bf16"], q["N"], q["H"], q["W"], q["C"], q["n_cls"], q["heads"], q["p"], q["mask"], q["x"], q["w"],
        q["dx"], q["mask_lo"], q["wgs"], q["cus"])


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("head_select") / "head_select_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "head_select_main.cpp"), "-o", exe], check=True)
    qs = queries()
    out = subprocess.run([exe], input="\n".join(line_of(q) for q in qs) + "\n", capture_output=True, text=True,
                         check=True).stdout.splitlines()
    assert len(out) == len(qs)
    return qs, out


def test_selection_matches_the_launchers_rules(answers):
    qs, out = answers
    seen = set()
    for q, got in zip(qs, out):
        rc, (label, grid, block, lds, active) = LAUNCHERS[(q["op"], q["bf16"])](q)
        want = "%d %s %d %d %d %d" % (rc, label, grid, block, lds, active)
        assert got == want, (line_of(q), got, want)
        seen.add((q["op"], q["bf16"], rc))
    # every launcher was asked, accepted and refused; the bf16 backward also without a device
    for key in LAUNCHERS:
        assert key + (OK,) in seen and key + (EINVAL,) in seen
    assert (BWD, 1, ELAUNCH) in seen
    assert not any(rc == ELAUNCH for op, bf16, rc in seen if (op, bf16) != (BWD, 1))


def test_labels_are_those_the_gpu_tests_cover(answers):
    from tests.test_gpu_heads import _coverage
    from tests.test_gpu_infer import KERNEL_COVERAGE
    want = {name.split("/D")[0] for name in _coverage()} | set(KERNEL_COVERAGE)
    got = {line.split()[1] for line in answers[1]} - {"-"}
    assert want - got == set(), "labels no query produced"
    assert got - want == set(), "labels no GPU test covers"
