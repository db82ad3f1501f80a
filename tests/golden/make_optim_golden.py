"""Generate tests/golden/optim_*.npz by RUNNING THE REFERENCE'S OPTIMIZERS (tools/optimizers/{adamw,adabound,sgdw}.py).

Build-container only: imports the reference's optimizer classes as they are (CPU torch) and records, for every
configuration of CONFIGS, the parameters and the full optimizer state after steps 1, 3 and 6.  Only data is stored: the
inputs are re-made from a numpy seed by ``make_inputs`` (tests/test_gpu_optim.py imports this file for it), and the
recorded values are the elements at ``sample_index`` of every tensor (first and last elements, chunk boundaries of the
fused kernel, a seeded spread in between) -- the whole state would be ~30 MB.  Re-run with:

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python /path/to/repo/tests/golden/make_optim_golden.py

The reference does not exist on the GPU box; nothing at test time calls ``main``.

Case: the parameter shapes of UNet_Nested(1, 4, feature_scale=8) plus one tensor of odd length 100003 (tails, several
4096-element chunks); two parameter groups (even / odd tensor index, the odd group at half the lr); seeded gradients for
6 steps, tensor 3 has no gradient at step 2 (its count falls behind); MultiStepLR(milestones=[3], gamma=0.1) stepped
after every optimizer step.
"""
import os
import sys

import numpy as np

REF = os.environ.get("UNETPP_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))

STEPS = 6
RECORD = (1, 3, 6)
NO_GRAD = (2, 3)           # (step, tensor index): grad None
BIG = 100003
SAMPLES = 48
CONFIGS = {
    # name: (class, kwargs)
    "adamw": ("AdamW", dict(lr=1e-3, weight_decay=1e-4)),
    "adamw_amsgrad": ("AdamW", dict(lr=1e-3, amsgrad=True, weight_decay=0)),
    "adabound": ("AdaBound", dict(lr=1e-3, weight_decay=1e-4)),
    "adabound_amsbound": ("AdaBound", dict(lr=1e-3, amsbound=True)),
    "sgdw": ("SGDW", dict(lr=1e-3, weight_decay=1e-4)),
    "sgdw_nesterov": ("SGDW", dict(lr=1e-3, momentum=0.9, nesterov=True)),
}
STATE_KEYS = ("exp_avg", "exp_avg_sq", "max_exp_avg_sq", "momentum_buffer")


def shapes():
    """UNet_Nested(1, 4, feature_scale=8)'s parameter shapes (this package's module tree equals the reference's)."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from unet_nested4tiny_objects_keypoints_amd import UNet_Nested
    return [tuple(p.shape) for p in UNet_Nested(1, 4, feature_scale=8).parameters()] + [(BIG,)]


def make_inputs(shape_list):
    """-> initial parameters [n] and gradients [STEPS][n] (None where NO_GRAD says), float32 numpy, seeded."""
    rng = np.random.default_rng(20261015)
    params = [(0.1 * rng.standard_normal(s)).astype(np.float32) for s in shape_list]
    grads = []
    for step in range(1, STEPS + 1):
        scale = 10.0 ** rng.uniform(-3, -1)
        gs = [(scale * rng.standard_normal(s)).astype(np.float32) for s in shape_list]
        grads.append([None if (step, i) == NO_GRAD else g for i, g in enumerate(gs)])
    return params, grads


def sample_index(numel):
    """Flat indices recorded for a tensor of `numel` elements."""
    if numel <= SAMPLES:
        return np.arange(numel)
    rng = np.random.default_rng(numel)
    fixed = [0, 1, 2, 3, numel - 4, numel - 3, numel - 2, numel - 1]
    fixed += [c + d for c in range(4096, numel, 4096) for d in (-1, 0)][:16]
    spread = rng.choice(numel, SAMPLES, replace=False)
    return np.unique(np.asarray(fixed + list(spread), dtype=np.int64) % numel)


def groups_of(params):
    return [list(params[0::2]), list(params[1::2])]


def group_lrs(lr):
    return [lr, 0.5 * lr]


def run(cls, kwargs, shape_list, params0, grads):
    """The reference's loop on CPU -> {step: {"param/i", "<state key>/i", "step/i"}} sampled."""
    import torch
    params = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in params0]
    lr = kwargs["lr"]
    ga, gb = groups_of(params)
    opt = cls([{"params": ga, "lr": group_lrs(lr)[0]}, {"params": gb, "lr": group_lrs(lr)[1]}],
              **{k: v for k, v in kwargs.items() if k != "lr"}, lr=lr)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[3], gamma=0.1)
    out = {}
    for step in range(1, STEPS + 1):
        for p, g in zip(params, grads[step - 1]):
            p.grad = None if g is None else torch.from_numpy(g.copy())
        opt.step()
        sched.step()
        if step in RECORD:
            rec = {}
            for i, p in enumerate(params):
                idx = sample_index(p.numel())
                rec["param/%d" % i] = p.detach().reshape(-1)[idx].numpy().copy()
                st = opt.state.get(p, {})
                for k in STATE_KEYS:
                    if k in st:
                        rec["%s/%d" % (k, i)] = st[k].reshape(-1)[idx].numpy().copy()
                rec["step/%d" % i] = np.asarray(st.get("step", -1), dtype=np.int64)
            out[step] = rec
    return out


def main():
    import warnings
    import torch
    torch.set_num_threads(1)
    warnings.simplefilter("ignore")          # the reference's add_(scalar, tensor) overloads are deprecated
    sys.path.insert(0, REF)
    from tools.optimizers.adabound import AdaBound
    from tools.optimizers.adamw import AdamW
    from tools.optimizers.sgdw import SGDW
    classes = {"AdamW": AdamW, "AdaBound": AdaBound, "SGDW": SGDW}
    shape_list = shapes()
    params0, grads = make_inputs(shape_list)
    for name, (cls_name, kwargs) in CONFIGS.items():
        rec = run(classes[cls_name], kwargs, shape_list, params0, grads)
        arrays = {"n_tensors": np.asarray(len(shape_list))}
        for step, r in rec.items():
            arrays.update({"s%d/%s" % (step, k): v for k, v in r.items()})
        path = os.path.join(OUT, "optim_%s.npz" % name)
        np.savez_compressed(path, **arrays)
        print("wrote", path, os.path.getsize(path))


if __name__ == "__main__":
    main()
