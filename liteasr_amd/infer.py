"""Evaluation CLI (liteasr/infer.py): ``python -m liteasr_amd.infer task=... model=... inference.ckpt_name=N ...``.

The config is composed exactly as ``liteasr_amd.train`` composes it (same groups, overrides,
run directory and logging; the log file is ``infer.log``).  Then, as the reference does: the
task, the test sets of ``task.test``, the model, ``load_ckpt(cfg.inference)`` (one checkpoint
or an average), and per test set one block per utterance

    [X] <hypothesis>          ([ ] when it differs from the reference text)
    <edit distance> <reference text>

followed by ``Error rate: <errors> / <reference length> = <percent>``.

A test set may be a raw-audio directory (wav.scp, no feats.scp): its utterances reach
``task.inference`` as int16 PCM and go through the task's device front end (``task.frontend``:
Kaldi fbank and optional CMVN) there; they are ordered and graph-planned by their frame counts.

Differences from the reference, on purpose:

* it decodes utterance by utterance (``load_dataset("test", ..., None, ...)``).  The reference
  hands ``cfg.dataset`` to the test loader and then slices the batchified set per rank, which
  yields lists of utterances where its loop expects one;
* one process on one device: ``inference.thread_num`` is accepted and ignored (the
  reference's pool of CPU workers has no counterpart on a single accelerator);
* the encoder hipGraph is used only for frame counts that occur at least ``GRAPH_MIN_USES``
  times in the set: a capture costs two extra encoder passes and a replay saves about 0.59 of
  one, so it pays from the fourth use.  Utterances are decoded in frame-count order, so equal
  shapes are adjacent and a captured graph is not evicted between its uses; the blocks are
  logged in dataset order;
* ``inference.batch_size`` (default 1: the loop above, unchanged).  Above 1, models that have
  ``inference_batch`` (U2, Paraformer) decode ``batch_plan``'s groups: utterances in frame-count
  order, cut into consecutive groups of ``batch_size``, each zero-padded to its longest.  A padded
  row is the computation training sees for that row, not the unpadded single-utterance one
  (``decoding.attention_rescore_batch``), so a hypothesis may differ from ``batch_size`` 1's.
  Models without ``inference_batch`` (Transducer) are decoded utterance by utterance.
"""

import logging
from collections import Counter

import torch

from . import tasks
from .config.compose import ConfigError
from .train import prepare
from .utils.checkpoint import load_ckpt
from .utils.score import levenshtein

logger = logging.getLogger("liteasr_amd.infer")

GRAPH_MIN_USES = 4
UTT_FORMAT = "\n{} {}\n{:>3} {}"
RATE_FORMAT = "Error rate: {} / {} = {:.2%}"


def utt_line(ref, hyp):
    """The reference's per-utterance block and the utterance's edit distance."""
    err = levenshtein(ref, hyp)
    return UTT_FORMAT.format("[X]" if ref == hyp else "[ ]", hyp, err, ref), err


def rate_line(total_err, total_len):
    return RATE_FORMAT.format(total_err, total_len, total_err / total_len)


def graph_plan(xlens, min_uses=GRAPH_MIN_USES):
    """(decode order, per-utterance encoder_graph flag): equal frame counts adjacent (stable
    in dataset order), a graph only where the frame count occurs at least ``min_uses`` times."""
    uses = Counter(xlens)
    order = sorted(range(len(xlens)), key=lambda i: xlens[i])
    return order, [uses[n] >= min_uses for n in xlens]


def batch_plan(xlens, batch_size):
    """The groups of a batched decode: utterance indices in frame-count order (stable in dataset
    order, ``graph_plan``'s order), cut into consecutive groups of ``batch_size``; the last may be
    short.  Neighbours in that order differ least in length, so this pads least."""
    if batch_size < 1:
        raise ValueError(f"inference.batch_size must be at least 1, got {batch_size}")
    order = sorted(range(len(xlens)), key=lambda i: xlens[i])
    return [order[a:a + batch_size] for a in range(0, len(order), batch_size)]


def pad_batch(xs):
    """Utterances (features (T_i, F) or int16 PCM (n_i,)) zero-padded along their first dimension
    to the longest, stacked: (batch, per-row lengths)."""
    lens = [int(x.shape[0]) for x in xs]
    out = xs[0].new_zeros((len(xs), max(lens)) + tuple(xs[0].shape[1:]))
    for b, x in enumerate(xs):
        out[b, :lens[b]] = x
    return out, lens


def infer_dataset(task, model, dataset, device, batch_size=1):
    """Decode one test set; returns (errors, reference length, hypotheses in dataset order)."""
    xlens = [dataset[i].xlen for i in range(len(dataset))]
    hyps = [None] * len(dataset)
    if batch_size > 1 and not hasattr(model, "inference_batch"):
        logger.info("{} has no inference_batch: decoding utterance by utterance (inference.batch_size={} ignored)"
                    .format(type(model).__name__, batch_size))
        batch_size = 1
    with torch.no_grad():
        if batch_size > 1:
            for group in batch_plan(xlens, batch_size):
                xs, lens = pad_batch([dataset[i].x for i in group])
                for i, hyp in zip(group, task.inference_batch(xs.to(device), lens, model)):
                    hyps[i] = hyp
        else:
            order, graphed = graph_plan(xlens)
            for i in order:
                feat = dataset[i].x.unsqueeze(0).to(device)
                hyps[i] = task.inference(feat, model, encoder_graph=graphed[i])
    total_len = total_err = 0
    for i, hyp in enumerate(hyps):
        ref = dataset[i].text
        line, err = utt_line(ref, hyp)
        total_len += len(ref)
        total_err += err
        logger.info(line)
    logger.info(rate_line(total_err, total_len))
    return total_err, total_len, hyps


def infer(cfg):
    device = torch.device("cuda")
    task = tasks.setup_task(cfg.task)
    logger.info("setting {} task...".format(task.__class__.__name__))

    logger.info("1. load data...")
    task.load_dataset("test", task.cfg.test, None, cfg.postprocess)

    model = task.build_model(cfg.model)
    model.load_state_dict(load_ckpt(cfg.inference))
    model = model.to(device=device).eval()

    test_sets = task.dataset("test")
    for test_set in test_sets if isinstance(test_sets, (list, tuple)) else [test_sets]:
        infer_dataset(task, model, test_set, device, batch_size=int(cfg.inference.get("batch_size", 1) or 1))


NEEDS = ("task.vocab", "task.test", "inference.ckpt_name", "inference.ckpt_path")


def main(argv=None):
    """What evaluation reads must be set: the vocabulary, the test sets and the checkpoint.
    ``task.train`` / ``task.valid`` and the other training-only values may stay ``???``."""
    cfg, _ = prepare(argv, job_name="infer", description=__doc__.splitlines()[0], mandatory=NEEDS.__contains__)
    if cfg is None:
        return
    if not cfg.task.get("test"):
        raise ConfigError("task.test names no test set")
    infer(cfg)


def cli_main():
    main()


if __name__ == "__main__":
    cli_main()
