"""Checkpoint compatibility with the reference trainer.

The module tree and parameter names of :class:`UNet_Nested` equal the reference's, so a reference-trained
``state_dict`` loads directly.  This file mirrors the two on-disk formats the reference trainer reads and writes
(/root/reference/trainer/trainer.py):

* ``*.pth`` -- a bare ``state_dict`` (``torch.save(model_state_dic, ...)``, trainer.py:240-249, loaded at :415-419);
  the trainer names it ``best_epoch_{epoch}_heatmaploss_{h}_landmarkloss_{l}.pth``;
* ``*.tar`` -- ``{'model_state_dict', 'optimizer_state_dict', 'epoch'}`` (loaded at trainer.py:403-413).

Files saved from a ``nn.DataParallel`` wrapper without unwrapping carry a ``module.`` prefix on every key; it is
stripped on load (the reference unwraps with ``model.module`` when ``device_count > 1``, trainer.py:240).

Pruned checkpoints (``save_pruned`` / ``load_pruned``) keep only what ``UNet_Nested.infer(x, head)`` runs: the nodes of
``engine.needed_nodes(depth, head)`` and the heads ``final_1 .. final_head``, under the reference's key names -- a plain
``.pth`` that is a subset of the full one (4.6 % of the parameters for head 1, 23 % for head 2 at depth 4).
"""
from __future__ import annotations

import os
from typing import Optional

import torch


def _unwrap(model):
    return model.module if hasattr(model, "module") and isinstance(model.module, torch.nn.Module) else model


def _strip_module_prefix(state):
    if state and all(k.startswith("module.") for k in state):
        return {k[len("module."):]: v for k, v in state.items()}
    return state


def best_model_name(epoch, heatmap_loss, landmark_loss) -> str:
    return "best_epoch_{}_heatmaploss_{}_landmarkloss_{}.pth".format(epoch, heatmap_loss, landmark_loss)


def save_best(model, save_dir: str, epoch, heatmap_loss, landmark_loss) -> str:
    """trainer.py:240-249: the unwrapped state_dict as a .pth named after the validation losses."""
    path = os.path.join(save_dir, best_model_name(epoch, heatmap_loss, landmark_loss))
    torch.save(_unwrap(model).state_dict(), path)
    return path


def average_model_name(epoch, heatmap_loss, landmark_loss) -> str:
    return "average_epoch_{}_heatmaploss_{}_landmarkloss_{}.pth".format(epoch, heatmap_loss, landmark_loss)


def save_average(avg, save_dir: str, epoch, heatmap_loss, landmark_loss) -> str:
    """The ``model_save == "average"`` strategy trainer.py:243-252 names and does not implement: the averaged weights of
    a ``WeightAverager`` as a bare state_dict under the model's key names -- a plain .pth like ``save_best``'s, which the
    reference's model loads."""
    path = os.path.join(save_dir, average_model_name(epoch, heatmap_loss, landmark_loss))
    torch.save(avg.averaged_state_dict(), path)
    return path


def save_checkpoint(model, optimizer, epoch: int, path: str, averager=None) -> str:
    """The .tar layout trainer.py:403-413 resumes from.  With a ``WeightAverager`` its state travels along under
    ``average_state_dict`` (the reference ignores keys it does not know); without one the file is what it always was."""
    ckpt = {"model_state_dict": _unwrap(model).state_dict(),
            "optimizer_state_dict": None if optimizer is None else optimizer.state_dict(),
            "epoch": int(epoch)}
    if averager is not None:
        ckpt["average_state_dict"] = averager.state_dict()
    torch.save(ckpt, path)
    return path


def resume(model, path: str, optimizer=None, resume_opt: bool = False, map_location: Optional[str] = "cpu",
           averager=None) -> int:
    """trainer.py:399-419.  Loads `path` (suffix .tar or .pth) into `model` (and the optimizer when `resume_opt`);
    returns the epoch to start from (0 unless a .tar is resumed together with its optimizer state).  `averager`: a
    ``WeightAverager`` that takes the file's ``average_state_dict`` together with the optimizer state."""
    suf = path.rsplit(".", 1)[-1]
    start_epoch = 0
    target = _unwrap(model)
    if suf == "tar":
        ckpt = torch.load(path, map_location=map_location)
        target.load_state_dict(_strip_module_prefix(ckpt["model_state_dict"]))
        if resume_opt:
            if optimizer is None:
                raise ValueError("resume_opt needs the optimizer")
            optimizer.load_state_dict(ckpt["optimizer_state_dict"])
            if averager is not None:
                if "average_state_dict" not in ckpt:
                    raise KeyError("%s was saved without an averager: it has no average_state_dict" % path)
                averager.load_state_dict(ckpt["average_state_dict"])
            start_epoch = int(ckpt["epoch"]) + 1
    elif suf == "pth":
        target.load_state_dict(_strip_module_prefix(torch.load(path, map_location=map_location)))
    else:
        raise ValueError("unknown checkpoint suffix %r (the reference trainer reads .tar and .pth)" % suf)
    return start_epoch


def _pruned_prefixes(depth: int, head: int):
    from .engine import needed_nodes
    names = ["conv%d0." % i if j == 0 else "up_concat%d%d." % (i, j) for (i, j) in needed_nodes(depth, head)]
    return tuple(names + ["final_%d." % j for j in range(1, head + 1)])


def pruned_state_dict(model, head: int):
    """The entries of ``model.state_dict()`` that inference cut at `head` reads: the nodes of needed_nodes(depth, head) and
    final_1 .. final_head (all of them, so that ``infer(x, J, ensemble=True)`` works for every J <= head), in the full
    dict's order and under its names.  ``head = depth - 1`` gives the full dict."""
    target = _unwrap(model)
    prefixes = _pruned_prefixes(target.depth, head)
    return type(target.state_dict())((k, v) for k, v in target.state_dict().items() if k.startswith(prefixes))


def save_pruned(model, head: int, path: str) -> str:
    """``pruned_state_dict(model, head)`` as a plain .pth."""
    torch.save(pruned_state_dict(model, head), path)
    return path


def load_pruned(model, path: str, map_location: Optional[str] = "cpu") -> int:
    """Loads a ``save_pruned`` file into `model` and returns the head it was pruned to.  The file's key set must be exactly
    the pruned key set of some head of this model: any other missing or unexpected key is an error that names the keys.
    Records ``model.pruned_to = head``: from then on ``forward`` and ``infer(head > pruned_to)`` raise, because the nodes
    that were not loaded still hold their initialisation; a full ``load_state_dict`` lifts that.  ``forward_pruned(x, head <=
    pruned_to)`` / ``train_step(..., head=)`` train such a model, and ``save_pruned`` of it round-trips."""
    target = _unwrap(model)
    state = _strip_module_prefix(torch.load(path, map_location=map_location))
    own = target.state_dict()
    have = set(state)
    best = None   # (number of keys that differ, head, missing, unexpected)
    for head in range(1, target.depth):
        want = {k for k in own if k.startswith(_pruned_prefixes(target.depth, head))}
        missing, unexpected = sorted(want - have), sorted(have - want)
        if not missing and not unexpected:
            best = (0, head, missing, unexpected)
            break
        if best is None or len(missing) + len(unexpected) < best[0]:
            best = (len(missing) + len(unexpected), head, missing, unexpected)
    if best[0]:
        raise RuntimeError("%s is not a checkpoint pruned to any head of this model; closest is head %d: missing keys %s, "
                           "unexpected keys %s" % (path, best[1], best[2], best[3]))
    head = best[1]
    target.load_state_dict(state, strict=False)   # (shape mismatches still raise)
    target.pruned_to = None if head == target.depth - 1 else head
    return head
