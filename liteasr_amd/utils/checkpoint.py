"""Checkpoint loading and averaging for inference (liteasr/utils/checkpoint.py).

``load_ckpt(cfg.inference)`` returns a state dict for ``model.load_state_dict``:

* without ``model_avg``: ``{ckpt_path}/model.ep.{ckpt_name}.pt`` as saved by the trainer;
* with ``model_avg``: every file of ``ckpt_path`` is listed by modification time, ``pos`` is
  the place of the named checkpoint in that list and ``pos - avg_num + 1 >= 0`` is asserted.
  With ``avg_policy=None`` the ``avg_num`` checkpoints ending at ``pos`` are taken.  Otherwise
  ``avg_policy`` names a training log; its ``valid loss:`` numbers, in file order, belong to
  the listed files in mtime order, and the ``avg_num`` lowest-loss ones among the first
  ``pos + 1`` are taken (stable: equal losses keep mtime order).  The tensors are summed in
  pick-up order, then divided: ``/=`` for floating tensors, ``//=`` for integer ones
  (BatchNorm's ``num_batches_tracked``).
"""

import logging
import os
import re

import torch

logger = logging.getLogger(__name__)

_VALID_LOSS = re.compile(r".*valid loss: ([\d\.]+)")


def _read(path):
    return torch.load(path, map_location="cpu")


def average_states(paths, avg_num):
    """The first state dict of ``paths`` with every later one added to it in order, each tensor
    then divided in place by ``avg_num`` (true division for floating tensors, floor division
    for integer ones)."""
    paths = list(paths)
    acc = _read(paths[0])
    for path in paths[1:]:
        for name, t in _read(path).items():
            acc[name] += t
    for t in acc.values():
        if t is None:
            continue
        if t.is_floating_point():
            t.div_(avg_num)
        else:
            t.floor_divide_(avg_num)
    return acc


def valid_losses(log_path):
    """The numbers of the trainer's ``valid loss:`` lines, in file order."""
    with open(log_path) as log:
        hits = (_VALID_LOSS.match(line.strip()) for line in log)
        return [float(m.group(1)) for m in hits if m]


def _by_mtime(directory):
    """Every visible entry of ``directory`` as ``directory/name``, oldest first."""
    with os.scandir(directory) as it:
        entries = [(e.stat().st_mtime, f"{directory}/{e.name}") for e in it if not e.name.startswith(".")]
    entries.sort(key=lambda e: e[0])
    return [path for _, path in entries]


def pickup(cfg):
    """The checkpoint files ``load_ckpt`` averages, in pick-up order."""
    files = _by_mtime(cfg.ckpt_path)
    named = f"{cfg.ckpt_path}/model.ep.{cfg.ckpt_name}.pt"
    if named not in files:
        raise ValueError(f"{named} is not in {cfg.ckpt_path}")
    upto = files.index(named) + 1  # candidates: everything up to the named checkpoint
    first = upto - cfg.avg_num
    assert first >= 0, f"avg_num {cfg.avg_num} reaches before the oldest file ({upto} candidates)"
    if cfg.avg_policy is None:
        return files[first:upto]
    losses = valid_losses(cfg.avg_policy)
    ranked = sorted(range(min(upto, len(losses))), key=losses.__getitem__)  # stable: ties keep mtime order
    return [files[i] for i in ranked[: cfg.avg_num]]


def load_ckpt(cfg):
    if not cfg.model_avg:
        path = f"{cfg.ckpt_path}/model.ep.{cfg.ckpt_name}.pt"
        logger.info("checkpoint: %s", path)
        return _read(path)
    picked = pickup(cfg)
    logger.info("average of %d checkpoints:\n  %s", len(picked), "\n  ".join(picked))
    return average_states(picked, cfg.avg_num)
