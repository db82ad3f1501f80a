"""CPU-only: head_select's seventh query, HEAD_TRAIN (csrc/head_select.h) -- what unetpp_head_train takes and what it
refuses, in the manner of tests/test_head_select.py for the other six: tests/head_select_main.cpp answers a list of
queries, the launcher's rules are restated here, and the answers must agree line for line.

The training pass is head_fwd_stream's logits inside head_bwd_pow2's tile walk and promises their bits, so it takes a call
exactly where unetpp_head_fwd picks its streaming kernel AND unetpp_head_bwd its power-of-two kernel (both restated in
tests/test_head_select.py and reused here), with the backward's grid, workgroup and LDS bytes and the same template
coordinates; everything else -- bf16 storage included -- is UNETPP_EINVAL, after which the caller runs the three launches."""
import os
import subprocess

import pytest

from tests.test_head_select import (CHANNELS, CSRC, DROPS, EINVAL, LIMIT, MAX_CLS, MAX_HEADS, OK, REFUSED, ROOT, a16, cdiv,
                                    drop_mode, fp32_bwd, fp32_fwd, head_args_ok, head_bwd_blocks, line_of, log2,
                                    pixel_counts, pow2)

TRAIN = 4      # HeadOp HEAD_TRAIN


def fp32_train(q):
    """unetpp_head_train's rules (include/unetpp_hip.h), restated."""
    if q["bf16"] or not head_args_ok(q) or not 1 <= q["heads"] <= MAX_HEADS:
        return EINVAL, REFUSED
    pixels, c, g4, k = q["N"] * q["H"] * q["W"], q["C"], q["C"] >> 2, q["n_cls"]
    pcls = 4 if k <= 4 else 8
    if not (c % 4 == 0 and pow2(g4) and g4 <= 32 and pcls <= g4 and a16(q["x"]) and a16(q["w"]) and a16(q["dx"]) and
            pixels * c < LIMIT and (not q["mask"] or q["mask_lo"] & 3 == 0)):
        return EINVAL, REFUSED
    lds = (64 * (c + 1) + 64 * MAX_CLS + 2 * k * c) * 4
    return OK, ("head_train_pow2<%d,%d,%d>" % (log2(g4), drop_mode(q), pcls), head_bwd_blocks(pixels), 256, lds, 0)


def query(c, k, pixels=65, p=0.0, mask=0, heads=3, bf16=0, x=0, w=0, dx=0, mask_lo=0, cus=256, n=1, h=1):
    return dict(op=TRAIN, bf16=bf16, N=n, H=h, W=pixels, C=c, n_cls=k, heads=heads, p=p, mask=mask, x=x, w=w, dx=dx,
                mask_lo=mask_lo, wgs=4, cus=cus)


def queries():
    qs = []
    for c in CHANNELS:
        for k in range(10):
            for p, mask in DROPS:
                for pixels in pixel_counts(c):
                    qs.append(query(c, k, pixels, p, mask))
        for k in (1, 4, 5, 8):
            for p, mask in DROPS:
                for role in (dict(x=4), dict(w=4), dict(dx=4), dict(mask_lo=1), dict(mask_lo=2), dict(mask_lo=4)):
                    qs.append(query(c, k, 65, p, mask, **role))
            for heads in (0, 1, 2, 8, 9):
                qs.append(query(c, k, heads=heads))
            qs.append(query(c, k, bf16=1))
            qs.append(query(c, k, cus=0))      # the CU count does not matter
    for bad in (dict(n=0), dict(h=0), dict(pixels=0), dict(p=1.0), dict(p=-0.25), dict(heads=-1)):
        qs.append(query(32, 4, **bad))
    return qs


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("head_train_select") / "head_select_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "head_select_main.cpp"), "-o", exe], check=True)
    qs = queries()
    out = subprocess.run([exe], input="\n".join(line_of(q) for q in qs) + "\n", capture_output=True, text=True,
                         check=True).stdout.splitlines()
    assert len(out) == len(qs)
    return qs, out


def test_train_selection_matches_the_restated_rules(answers):
    qs, out = answers
    seen, labels = set(), set()
    for q, got in zip(qs, out):
        rc, (label, grid, block, lds, active) = fp32_train(q)
        want = "%d %s %d %d %d %d" % (rc, label, grid, block, lds, active)
        assert got == want, (line_of(q), got, want)
        seen.add(rc)
        labels.add(label)
    assert seen == {OK, EINVAL}
    # every instantiation heads.hip builds is reached: C = 16 .. 128, three dropout modes, 4 or 8 padded classes (8 from C = 32)
    want = {"head_train_pow2<%d,%d,%d>" % (L, d, pc) for L in (2, 3, 4, 5) for d in (0, 1, 2) for pc in (4, 8) if pc <= 1 << L}
    assert labels - {"-"} == want


def test_train_takes_what_the_stream_forward_and_the_pow2_backward_both_take(answers):
    """Accepted iff the three-launch path would run head_fwd_stream and head_bwd_pow2 on the same arguments, and then with
    their template coordinates and the backward's grid, workgroup and LDS bytes."""
    qs, out = answers
    for q, got in zip(qs, out):
        if q["bf16"] or not 1 <= q["heads"] <= MAX_HEADS:
            assert got.split()[0] == str(EINVAL), (line_of(q), got)
            continue
        (frc, fwd), (brc, bwd) = fp32_fwd(q), fp32_bwd(q)
        both = frc == OK and brc == OK and fwd[0].startswith("head_fwd_stream<") and bwd[0].startswith("head_bwd_pow2<")
        rc, label, grid, block, lds, active = got.split()
        assert (int(rc) == OK) == both, (line_of(q), got, fwd, bwd)
        if both:
            fl, fp_, fd = fwd[0][len("head_fwd_stream<"):-1].split(",")
            assert bwd[0] == "head_bwd_pow2<%s,%s,%s>" % (fl, fd, fp_)
            assert label == "head_train_pow2<%s,%s,%s>" % (fl, fd, fp_)
            assert (int(grid), int(block), int(lds), int(active)) == bwd[1:]
            assert int(grid) == min(cdiv(q["N"] * q["H"] * q["W"], 64), 4096)
