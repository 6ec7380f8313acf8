"""Forced-alignment CLI: ``python -m liteasr_amd.align task=... model=... inference.ckpt_name=N ...``.

The config is composed, and the checkpoint loaded, exactly as ``liteasr_amd.infer`` does it (same
groups, overrides, run directory and logging; the log file is ``align.log``; ``load_ckpt`` with
``inference.model_avg``; the test sets of ``task.test``).  Every utterance's reference transcript is
aligned to its audio through the model's CTC head (``U2.align``: the Viterbi pass of
csrc/ctc_align.hip), in ``infer.batch_plan``'s groups of ``inference.batch_size`` utterances, each
group zero-padded to its longest (``infer.pad_batch``).  A padded row is the computation training
sees for that row, so its times may differ from ``inference.batch_size=1``'s by a frame; a group's
longest row is the unpadded computation.

Per test set two files are written under ``inference.align_dir`` (default ``align``, relative to
the run directory), named after the set's directory:

    <set name>.ctm     ``uttid 1 start dur token``, one line per token, dataset order
    <set name>.scores  ``uttid score score/frames``, one line per utterance

Times are seconds from the start of the utterance in steps of one encoder frame (0.04 s: the
10 ms frame shift times the subsampling of 4, ``ASRTask.align``); ``frames`` counts encoder frames.
An utterance whose transcript does not fit its frames is logged and listed in ``.scores`` with
``-inf``.  A model without ``align`` (no CTC head: Paraformer, Transducer) is refused before any
data is read."""

import logging
import os

import torch

from . import tasks
from .config.compose import ConfigError
from .infer import NEEDS, batch_plan, pad_batch
from .models import MODEL_REGISTRY
from .train import prepare
from .utils.checkpoint import load_ckpt

logger = logging.getLogger("liteasr_amd.align")

CTM_FORMAT = "{} 1 {:.2f} {:.2f} {}"
SCORE_FORMAT = "{} {:.4f} {:.4f}"


def pad_targets(tokenids):
    """Token-id lists as training pads them: int64 (B, Lmax) filled with -1, and the lengths."""
    lens = [len(t) for t in tokenids]
    ys = torch.full((len(tokenids), max(lens + [1])), -1, dtype=torch.int64)
    for b, t in enumerate(tokenids):
        if lens[b]:
            ys[b, :lens[b]] = torch.tensor(list(t), dtype=torch.int64)
    return ys, lens


def align_dataset(task, model, dataset, device, batch_size=1):
    """Align one test set; returns per utterance, in dataset order, the ``(tokens, score)`` of
    ``ASRTask.align``: ``tokens`` a list of (token, start_s, dur_s), or None."""
    xlens = [dataset[i].xlen for i in range(len(dataset))]
    out = [None] * len(dataset)
    with torch.no_grad():
        for group in batch_plan(xlens, batch_size):
            xs, lens = pad_batch([dataset[i].x for i in group])
            ys, ylens = pad_targets([dataset[i].tokenids for i in group])
            for i, row in zip(group, task.align(xs.to(device), lens, ys, ylens, model)):
                out[i] = row
    return out


def write_alignment(dataset, rows, frames, ctm_path, scores_path):
    with open(ctm_path, "w") as ctm, open(scores_path, "w") as scores:
        for i, (tokens, score) in enumerate(rows):
            uttid = dataset.uttids[i]
            if tokens is None:
                logger.warning("{}: the transcript does not fit the utterance's {} encoder frames, not aligned"
                               .format(uttid, frames[i]))
                scores.write("{} -inf -inf\n".format(uttid))
                continue
            for token, start, dur in tokens:
                ctm.write(CTM_FORMAT.format(uttid, start, dur, token) + "\n")
            scores.write(SCORE_FORMAT.format(uttid, score, score / max(frames[i], 1)) + "\n")


def encoder_frames(dataset, i):
    """The encoder frames utterance i's score covers (get_pred_len of its feature frames)."""
    return max(((int(dataset[i].xlen) - 1) // 2 - 1) // 2, 0)


def align(cfg):
    device = torch.device("cuda")
    task = tasks.setup_task(cfg.task)
    logger.info("setting {} task...".format(task.__class__.__name__))
    # refused before any data is read: the registered class says whether the model can align
    cls = MODEL_REGISTRY.get(str(cfg.model.get("name", "")))
    if cls is None:
        raise ConfigError("model.name={} is not a registered model".format(cfg.model.get("name")))
    if not hasattr(cls, "align"):
        raise ConfigError("model {} has no align: forced alignment needs a CTC head (model=U2)".format(cls.__name__))

    logger.info("1. load data...")
    task.load_dataset("test", task.cfg.test, None, cfg.postprocess)

    model = task.build_model(cfg.model)
    model.load_state_dict(load_ckpt(cfg.inference))
    model = model.to(device=device).eval()

    out_dir = str(cfg.inference.get("align_dir", "align") or "align")
    os.makedirs(out_dir, exist_ok=True)
    batch_size = int(cfg.inference.get("batch_size", 1) or 1)
    test_sets = task.dataset("test")
    test_sets = test_sets if isinstance(test_sets, (list, tuple)) else [test_sets]
    for data_dir, test_set in zip(task.cfg.test, test_sets):
        name = os.path.basename(os.path.normpath(str(data_dir)))
        rows = align_dataset(task, model, test_set, device, batch_size=batch_size)
        frames = [encoder_frames(test_set, i) for i in range(len(test_set))]
        ctm, scores = os.path.join(out_dir, name + ".ctm"), os.path.join(out_dir, name + ".scores")
        write_alignment(test_set, rows, frames, ctm, scores)
        done = sum(t is not None for t, _ in rows)
        logger.info("{}: aligned {} of {} utterances -> {}, {}".format(name, done, len(rows), ctm, scores))


def main(argv=None):
    """What alignment reads must be set: the vocabulary, the test sets and the checkpoint."""
    cfg, _ = prepare(argv, job_name="align", description=__doc__.splitlines()[0], mandatory=NEEDS.__contains__)
    if cfg is None:
        return
    if not cfg.task.get("test"):
        raise ConfigError("task.test names no test set")
    align(cfg)


def cli_main():
    main()


if __name__ == "__main__":
    cli_main()
