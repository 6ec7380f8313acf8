"""Inputs shared by the pretraining-path CPU and GPU tests: the reference-made fixture
(tests/golden/pretrain.npz over tests/golden/pretrain_data/) and its data directories realised
under a temporary path."""

import functools
import os
import shutil
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DATA = os.path.join(HERE, "golden", "pretrain_data")
WAV = os.path.join(DATA, "wav")
SMALL_BUDGET = 20000  # Wav2VecBatch.max_batch_frame the fixture's batches were made with


@functools.lru_cache(None)
def golden():
    return dict(np.load(os.path.join(HERE, "golden", "pretrain.npz")))


def data_dir(tmp_path, form):
    """tests/golden/pretrain_data/<form> ("seg" / "whole") copied to tmp_path/<form>, its
    wav.scp pointing at the committed WAV files."""
    d = os.path.join(str(tmp_path), form)
    if not os.path.isdir(d):
        shutil.copytree(os.path.join(DATA, form), d)
        scp = open(os.path.join(d, "wav.scp.in")).read().replace("@WAV@", WAV)
        with open(os.path.join(d, "wav.scp"), "w") as f:
            f.write(scp)
    return d


def small_cfg():
    return SimpleNamespace(max_batch_frame=SMALL_BUDGET)


def golden_batches(form):
    g = golden()
    sizes = g[form + ".batch_size"].tolist()
    flat = g[form + ".batch_flat"].tolist()
    out, at = [], 0
    for n in sizes:
        out.append(flat[at:at + n])
        at += n
    return out
