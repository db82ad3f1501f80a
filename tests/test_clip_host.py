"""Host side of gradient clipping in the fused optimizers (optim.py): argument checks, the state_dict format and the
package's exports.  No GPU: the optimizers are only constructed."""
import pytest
import torch

import unet_nested4tiny_objects_keypoints_amd as pkg
from unet_nested4tiny_objects_keypoints_amd import AdaBound, AdamW, SGDW

CLASSES = [(AdamW, {}), (AdaBound, {}), (SGDW, {"lr": 0.1, "momentum": 0.9})]


def _params():
    return [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))]


@pytest.mark.parametrize("cls,kw", CLASSES, ids=[c.__name__ for c, _ in CLASSES])
@pytest.mark.parametrize("bad", [0, 0.0, -1.0])
def test_max_grad_norm_must_be_positive(cls, kw, bad):
    with pytest.raises(ValueError):
        cls(_params(), **kw, max_grad_norm=bad)
    opt = cls(_params(), **kw, max_grad_norm=1.0)
    with pytest.raises(ValueError):
        opt.max_grad_norm = bad
    assert opt.max_grad_norm == 1.0


@pytest.mark.parametrize("cls,kw", CLASSES, ids=[c.__name__ for c, _ in CLASSES])
def test_skip_nonfinite_needs_capturable(cls, kw):
    with pytest.raises(ValueError, match="capturable"):
        cls(_params(), **kw, skip_nonfinite=True)
    with pytest.raises(ValueError, match="capturable"):
        cls(_params(), **kw, skip_nonfinite=True, max_grad_norm=1.0, capturable=False)
    opt = cls(_params(), **kw, skip_nonfinite=True, capturable=True)      # allowed without max_grad_norm
    assert opt.skip_nonfinite and opt.max_grad_norm is None


@pytest.mark.parametrize("cls,kw", CLASSES, ids=[c.__name__ for c, _ in CLASSES])
def test_defaults_and_keyword_only(cls, kw):
    opt = cls(_params(), **kw)
    assert opt.max_grad_norm is None and opt.skip_nonfinite is False
    opt.max_grad_norm = 2
    assert opt.max_grad_norm == 2.0 and isinstance(opt.max_grad_norm, float)
    opt.max_grad_norm = None
    assert opt.max_grad_norm is None
    import inspect
    sig = inspect.signature(cls.__init__).parameters
    assert sig["max_grad_norm"].kind is inspect.Parameter.KEYWORD_ONLY and sig["max_grad_norm"].default is None
    assert sig["skip_nonfinite"].kind is inspect.Parameter.KEYWORD_ONLY and sig["skip_nonfinite"].default is False


@pytest.mark.parametrize("cls,kw", CLASSES, ids=[c.__name__ for c, _ in CLASSES])
def test_state_dict_keeps_the_reference_format(cls, kw):
    """Optimizer attributes, not param-group keys: the dict of a clipping optimizer has the keys of a plain one."""
    plain = cls(_params(), **kw).state_dict()
    clipped = cls(_params(), **kw, max_grad_norm=0.5, skip_nonfinite=True, capturable=True).state_dict()
    assert plain.keys() == clipped.keys()
    assert len(plain["param_groups"]) == len(clipped["param_groups"])
    for a, b in zip(plain["param_groups"], clipped["param_groups"]):
        assert a.keys() == b.keys()
        assert a == b
    assert plain["state"] == clipped["state"] == {}
    hyper = cls(_params(), **kw, max_grad_norm=0.5)._hyper()              # the value travels in the hyper block instead
    assert hyper[pkg._lib.OPTIM_H_MAX_NORM] == 0.5
    assert cls(_params(), **kw)._hyper()[pkg._lib.OPTIM_H_MAX_NORM] == 0.0


def test_exports():
    assert "clip_grad_norm_" in pkg.__all__ and callable(pkg.clip_grad_norm_)
    from unet_nested4tiny_objects_keypoints_amd.optim import clip_grad_norm_
    assert clip_grad_norm_ is pkg.clip_grad_norm_
    for name in ("unetpp_grad_norm", "unetpp_optim_step_clip", "unetpp_grad_scale"):
        assert name in pkg._lib.SIGNATURES


def test_clip_grad_norm_refuses_what_it_does_not_do():
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    with pytest.raises(ValueError, match="norm_type"):
        pkg.clip_grad_norm_([p], 1.0, norm_type=1.0)
    with pytest.raises(ValueError, match="norm_type"):
        pkg.clip_grad_norm_([p], 1.0, norm_type=float("inf"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.clip_grad_norm_([p], 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.clip_grad_norm_(p, 1.0)                                       # a single tensor, as torch accepts it
    with pytest.raises(ValueError):
        pkg.clip_grad_norm_([p], 0.0)
    assert torch.equal(p.grad, torch.ones(4))
    q = torch.nn.Parameter(torch.zeros(4))                                # nothing to clip: torch's 0.
    assert float(pkg.clip_grad_norm_([q], 1.0)) == 0.0


def test_entry_points_validate_arguments_without_a_gpu():
    import ctypes as C

    import __graft_entry__ as entry
    entry.build()
    lib = pkg._lib.lib()
    x = C.c_void_p(0x1000)
    assert lib.unetpp_grad_norm(None, 1, x, 1, x, None) == -1
    assert lib.unetpp_grad_norm(x, 0, x, 1, x, None) == -1
    assert lib.unetpp_grad_norm(x, 1, x, 1, None, None) == -1
    assert lib.unetpp_grad_scale(x, 1, x, 1, None, 1.0, x, None) == -1
    assert lib.unetpp_grad_scale(x, 1, x, 1, x, 0.0, x, None) == -1
    assert lib.unetpp_grad_scale(x, 1, x, 1, x, 1.0, None, None) == -1
    cap = pkg._lib.OPTIM_CAPTURABLE
    skip = pkg._lib.OPTIM_SKIP_NONFINITE
    assert lib.unetpp_optim_step_clip(0, 0, x, 1, x, 1, x, x, None, None, x, None) == -1      # no partials
    assert lib.unetpp_optim_step_clip(0, 0, x, 1, x, 1, x, x, None, x, None, None) == -1      # no state block
    assert lib.unetpp_optim_step_clip(0, skip, x, 1, x, 1, x, x, None, x, x, None) == -1      # skip needs capturable
    assert lib.unetpp_optim_step_clip(0, cap | skip, x, 1, x, 1, x, None, None, x, x, None) == -1   # capturable: done
    assert lib.unetpp_optim_step_clip(3, 0, x, 1, x, 1, x, x, None, x, x, None) == -1         # kind
    assert lib.unetpp_optim_step_clip(0, 8, x, 1, x, 1, x, x, None, x, x, None) == -1         # flag
    assert C.sizeof(pkg._lib.ClipState) == 16
