"""CPU checks of the fused optimizers (optim.py, csrc/optim.hip): the reference's constructor contract, no CPU fallback,
the C entry points' argument checks without a GPU, the segment struct's layout, and the golden fixtures."""
import ctypes
import importlib.util
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _golden_module():
    spec = importlib.util.spec_from_file_location("make_optim_golden", os.path.join(GOLDEN, "make_optim_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as entry
    entry.build()
    from unet_nested4tiny_objects_keypoints_amd import _lib
    return _lib


def _p():
    return [torch.nn.Parameter(torch.zeros(3))]


def test_defaults_and_group_keys():
    from unet_nested4tiny_objects_keypoints_amd import AdaBound, AdamW, SGDW
    g = AdamW(_p()).param_groups[0]
    assert {k: g[k] for k in ("lr", "betas", "eps", "weight_decay", "amsgrad")} == dict(
        lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False)
    a = AdaBound([{"params": _p(), "lr": 2e-3}, {"params": _p()}])
    assert a.base_lrs == [2e-3, 1e-3]
    assert {k: a.param_groups[1][k] for k in ("betas", "final_lr", "gamma", "eps", "weight_decay", "amsbound")} == dict(
        betas=(0.9, 0.999), final_lr=0.1, gamma=1e-3, eps=1e-8, weight_decay=0, amsbound=False)
    s = SGDW(_p(), lr=0.1).param_groups[0]
    assert {k: s[k] for k in ("lr", "momentum", "dampening", "weight_decay", "nesterov")} == dict(
        lr=0.1, momentum=0, dampening=0, weight_decay=0, nesterov=False)
    for opt in (AdamW(_p()), AdaBound(_p()), SGDW(_p(), lr=0.1)):     # no extra key in the groups: checkpoints move both ways
        assert "capturable" not in opt.param_groups[0] and opt.capturable is False
    with pytest.raises(ValueError):
        SGDW(_p())            # lr is required, as in the reference


@pytest.mark.parametrize("ctor,msg", [
    (lambda AdamW, AdaBound, SGDW: AdamW(_p(), betas=(1.0, 0.999)), "Invalid beta parameter at index 0: 1.0"),
    (lambda AdamW, AdaBound, SGDW: AdamW(_p(), betas=(0.9, -0.1)), "Invalid beta parameter at index 1: -0.1"),
    (lambda AdamW, AdaBound, SGDW: AdaBound(_p(), lr=-1.0), "Invalid learning rate: -1.0"),
    (lambda AdamW, AdaBound, SGDW: AdaBound(_p(), eps=-1.0), "Invalid epsilon value: -1.0"),
    (lambda AdamW, AdaBound, SGDW: AdaBound(_p(), betas=(0.9, 1.0)), "Invalid beta parameter at index 1: 1.0"),
    (lambda AdamW, AdaBound, SGDW: AdaBound(_p(), final_lr=-0.1), "Invalid final learning rate: -0.1"),
    (lambda AdamW, AdaBound, SGDW: AdaBound(_p(), gamma=1.0), "Invalid gamma parameter: 1.0"),
    (lambda AdamW, AdaBound, SGDW: SGDW(_p(), lr=0.1, nesterov=True), "Nesterov momentum requires a momentum and zero dampening"),
    (lambda AdamW, AdaBound, SGDW: SGDW(_p(), lr=0.1, momentum=0.9, dampening=0.1, nesterov=True), "Nesterov momentum requires"),
])
def test_reference_value_errors(ctor, msg):
    from unet_nested4tiny_objects_keypoints_amd import AdaBound, AdamW, SGDW
    with pytest.raises(ValueError, match=msg.replace("(", r"\(")):
        ctor(AdamW, AdaBound, SGDW)


@pytest.mark.parametrize("name", ["AdamW", "AdaBound", "SGDW"])
def test_cpu_parameters_have_no_fallback(name, built_lib):
    import unet_nested4tiny_objects_keypoints_amd as pkg
    p = torch.nn.Parameter(torch.randn(5))
    p.grad = torch.randn(5)
    opt = getattr(pkg, name)([p], lr=0.1, weight_decay=1e-4)
    before = p.detach().clone()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()
    assert torch.equal(p.detach(), before)


def test_entry_points_reject_bad_arguments(built_lib):
    L = built_lib.lib()
    assert L.unetpp_optim_chunk_elems() == 4096
    segs = (built_lib.OptimSegment * 1)()
    cmap = (ctypes.c_int32 * 1)()
    hyper = (ctypes.c_double * 8)()
    steps = (ctypes.c_double * 1)()
    done = ctypes.c_int32(0)
    S, M, H, T = ctypes.byref(segs), ctypes.byref(cmap), ctypes.byref(hyper), ctypes.byref(steps)
    A, CAP = built_lib.OPTIM_AMS, built_lib.OPTIM_CAPTURABLE
    bad = [
        (0, 0, None, 1, M, 1, H, T, None),          # null table
        (0, 0, S, 0, M, 1, H, T, None),             # zero segments
        (0, 0, S, 1, None, 1, H, T, None),          # null chunk map
        (0, 0, S, 1, M, 0, H, T, None),             # zero chunks
        (0, 0, S, 1, M, 1, None, T, None),          # null hyper-parameters
        (3, 0, S, 1, M, 1, H, T, None),             # unknown kind
        (-1, 0, S, 1, M, 1, H, T, None),
        (0, 4, S, 1, M, 1, H, T, None),             # unknown flag
        (2, A, S, 1, M, 1, H, T, None),             # SGDW has no AMS variant
        (0, 0, S, 1, M, 1, H, None, None),          # eager needs the step counts
        (0, 0, S, 1, M, 1, H, T, ctypes.byref(done)),   # ... and no arrival counter
        (0, CAP, S, 1, M, 1, H, None, None),        # capturable needs the arrival counter
        (1, CAP | A, S, 1, M, 1, H, T, ctypes.byref(done)),  # ... and no host step counts
    ]
    for args in bad:
        assert L.unetpp_optim_step(*args, None) == -1, args
    assert L.unetpp_optim_upload(None, H, 8, None) == -1
    assert L.unetpp_optim_upload(H, None, 8, None) == -1
    assert L.unetpp_optim_upload(H, H, 0, None) == -1


def test_segment_layout_matches_header(built_lib, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "unetpp_hip.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu %zu %d %d %d %d %d %d\\n", sizeof(unetpp_optim_segment),'
                   'offsetof(unetpp_optim_segment, step), offsetof(unetpp_optim_segment, numel),'
                   'offsetof(unetpp_optim_segment, chunk_begin), offsetof(unetpp_optim_segment, group),'
                   'offsetof(unetpp_optim_segment, vec), UNETPP_OPTIM_ADAMW, UNETPP_OPTIM_ADABOUND, UNETPP_OPTIM_SGDW,'
                   'UNETPP_OPTIM_AMS, UNETPP_OPTIM_CAPTURABLE, UNETPP_OPTIM_HYPER);return 0;}')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S = built_lib.OptimSegment
    want = [ctypes.sizeof(S), S.step.offset, S.numel.offset, S.chunk_begin.offset, S.group.offset, S.vec.offset,
            built_lib.OPTIM_ADAMW, built_lib.OPTIM_ADABOUND, built_lib.OPTIM_SGDW, built_lib.OPTIM_AMS,
            built_lib.OPTIM_CAPTURABLE, built_lib.OPTIM_HYPER]
    assert got == want


def test_golden_fixtures_are_self_consistent():
    gm = _golden_module()
    shapes = gm.shapes()
    assert len(shapes) == 75 and shapes[-1] == (gm.BIG,) and gm.BIG % 2 == 1 and gm.BIG > 100000
    params0, grads = gm.make_inputs(shapes)
    assert grads[gm.NO_GRAD[0] - 1][gm.NO_GRAD[1]] is None
    total = 0
    for name, (cls, kw) in gm.CONFIGS.items():
        path = os.path.join(GOLDEN, "optim_%s.npz" % name)
        total += os.path.getsize(path)
        z = np.load(path)
        assert int(z["n_tensors"]) == len(shapes)
        for step in gm.RECORD:
            for i, s in enumerate(shapes):
                n = int(np.prod(s))
                idx = gm.sample_index(n)
                p = z["s%d/param/%d" % (step, i)]
                assert p.shape == idx.shape and np.isfinite(p).all()
                st = int(z["s%d/step/%d" % (step, i)])
                behind = 1 if (i == gm.NO_GRAD[1] and step >= gm.NO_GRAD[0]) else 0
                if cls == "SGDW":
                    assert st == -1                                   # the reference's SGDW keeps no count
                    assert ("s%d/momentum_buffer/%d" % (step, i) in z) == (kw.get("momentum", 0) != 0)
                    continue
                assert st == step - behind
                m, v = z["s%d/exp_avg/%d" % (step, i)], z["s%d/exp_avg_sq/%d" % (step, i)]
                assert (v >= 0).all() and np.isfinite(m).all()
                ams = kw.get("amsgrad", False) or kw.get("amsbound", False)
                assert ("s%d/max_exp_avg_sq/%d" % (step, i) in z) == ams
                if ams:
                    assert (z["s%d/max_exp_avg_sq/%d" % (step, i)] >= v).all()
        # the parameters moved -- except under SGDW without weight decay: the reference never applies the gradient
        p6 = z["s6/param/0"]
        p0 = params0[0].reshape(-1)[gm.sample_index(params0[0].size)]
        assert np.array_equal(p6, p0) == (cls == "SGDW" and kw.get("weight_decay", 0) == 0)
    assert total < 2.5e6
