"""Generate tests/golden/pretrain_data/ and tests/golden/pretrain.npz by running the *reference's*
own AudioSheet, RawAudioFileDataset, Wav2VecBatch and collator (imported through refshim) on a
small Kaldi-style directory of WAV files.  Data only; the tests read the fixtures and never the
reference.

    python tests/golden/make_golden_pretrain.py

``soundfile`` is not installed where this runs.  After ``refshim.install()`` the stand-in module's
``read`` is replaced by a reader built on the standard library's ``wave`` module that returns
``int16 / 32768`` as float64 (and the rate).  That is libsndfile's rule for PCM_16 read as
double, stated from its documentation: it is the one thing in these fixtures that is not pinned
by running the reference's own dependency.

pretrain_data/ (seeded, 16 kHz, 16-bit mono; ``wav.scp.in`` lines hold ``@WAV@`` for the wav/
directory, which a test replaces with where it is):
  wav/recA.wav, recB.wav    two recordings cut by seg/segments
  wav/u0.wav .. u6.wav      seven short files (1200..11000 samples)
  seg/wav.scp.in, segments  form (a): 32 segments of 800..6000 samples, times with enough
                            decimals that round(t * 16000) rounds both ways
  whole/wav.scp.in          form (b): wav.scp alone

pretrain.npz, for f in ("seg", "whole"), with the reference class attribute
``Wav2VecBatch.max_batch_frame`` set to 20000 so these files make several batches:
  f.uttid, f.wav, f.start, f.shape   the sheet tuples (wav: the file's base name)
  f.order                            indices sorted by length, descending, stable
  f.batch_flat, f.batch_size         the batches' index lists, concatenated, and their sizes
  f.xs.<i>                           batch i as the collator returns it (float32)
and for the policy alone, at the default 1400000, over 200 seeded lengths in 30000..400000 (records
only, no audio): syn.len, syn.order, syn.batch_flat, syn.batch_size.  Asserted here: each form
makes at least three batches of differing size; the synthetic list makes at least four, and at
least one of them has a shortest length above 250000 (the crop cap bounds its size).
"""

import os
import shutil
import sys
import tempfile
import types
import wave

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import refshim  # noqa: E402

refshim.install()


def _sf_read(path, *a, **k):
    with wave.open(path, "rb") as w:
        assert w.getnchannels() == 1 and w.getsampwidth() == 2
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
        return pcm.astype(np.float64) / 32768.0, w.getframerate()


sys.modules["soundfile"].read = _sf_read

from liteasr.dataclass.sheet import AudioSheet  # noqa: E402
from liteasr.dataset.pretrain_dataset import RawAudioFileDataset  # noqa: E402
from liteasr.dataclass.audio_data import Audio  # noqa: E402
from liteasr.utils.batchify import Wav2VecBatch  # noqa: E402

DATA = os.path.join(HERE, "pretrain_data")
SMALL_BUDGET = 20000
RECS = {"recA": 24000, "recB": 22000}
WHOLE = {"u0": 11000, "u1": 10500, "u2": 8000, "u3": 6800, "u4": 6003, "u5": 4001, "u6": 1200}


def _signal(n, rng):
    t = np.arange(n) / 16000.0
    f0, f1 = rng.uniform(90, 400), rng.uniform(500, 3000)
    x = 0.45 * np.sin(2 * np.pi * f0 * t) + 0.25 * np.sin(2 * np.pi * f1 * t + 1.0) + 0.12 * rng.standard_normal(n)
    pcm = np.clip(np.round(x * 32768), -32768, 32767).astype("<i2")
    pcm[:3] = (-32768, 32767, 0)
    return pcm


def _write_wav(path, pcm):
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(pcm.tobytes())


def write_data():
    rng = np.random.default_rng(20240)
    shutil.rmtree(DATA, ignore_errors=True)
    for d in ("wav", "seg", "whole"):
        os.makedirs(os.path.join(DATA, d))
    for name, n in {**RECS, **WHOLE}.items():
        _write_wav(os.path.join(DATA, "wav", name + ".wav"), _signal(n, rng))
    with open(os.path.join(DATA, "seg", "wav.scp.in"), "w") as f:
        for name in RECS:
            f.write(f"{name} @WAV@/{name}.wav\n")
    with open(os.path.join(DATA, "whole", "wav.scp.in"), "w") as f:
        for name in WHOLE:
            f.write(f"{name} @WAV@/{name}.wav\n")
    # 32 segments, 800..6000 samples long, inside their recording; the first three are >= 4001
    # samples (the model test takes 3 x 4000 from them)
    lens = [4500, 4001, 6000] + [int(v) for v in rng.integers(800, 6001, size=29)]
    lens[5], lens[9] = 800, 801
    with open(os.path.join(DATA, "seg", "segments"), "w") as f:
        for i, n in enumerate(lens):
            rec = "recA" if i % 2 == 0 else "recB"
            s0 = int(rng.integers(0, RECS[rec] - n - 2))
            jit = rng.uniform(-0.45, 0.45, size=2) / 16000.0  # round() must absorb these
            start, end = max(s0 / 16000.0 + jit[0], 0.0), (s0 + n + 1) / 16000.0 + jit[1]
            f.write(f"utt{i:02d} {rec} {start:.7f} {end:.7f}\n")


def realise(form, tmp):
    """The committed directory of a form with wav.scp written for where the files are."""
    d = os.path.join(tmp, form)
    shutil.copytree(os.path.join(DATA, form), d)
    scp = open(os.path.join(d, "wav.scp.in")).read().replace("@WAV@", os.path.join(DATA, "wav"))
    with open(os.path.join(d, "wav.scp"), "w") as f:
        f.write(scp)
    return d


def flat(batches):
    return (np.array([i for b in batches for i in b], dtype=np.int64), np.array([len(b) for b in batches], dtype=np.int64))


def main():
    write_data()
    out = {}
    cfg = types.SimpleNamespace()
    with tempfile.TemporaryDirectory() as tmp:
        Wav2VecBatch.max_batch_frame = SMALL_BUDGET
        for form in ("seg", "whole"):
            d = realise(form, tmp)
            rows = list(AudioSheet(d))
            out[form + ".uttid"] = np.array([r[0] for r in rows])
            out[form + ".wav"] = np.array([os.path.basename(r[1]) for r in rows])
            out[form + ".start"] = np.array([r[2] for r in rows], dtype=np.int64)
            out[form + ".shape"] = np.array([r[3] for r in rows], dtype=np.int64)
            ds = RawAudioFileDataset(d, cfg, None)
            order = sorted(range(len(ds.data)), key=lambda i: ds.data[i].xlen, reverse=True)
            batches = [list(b) for b in ds.batchify_policy.data]
            assert [i for b in batches for i in b] == order
            out[form + ".order"] = np.array(order, dtype=np.int64)
            out[form + ".batch_flat"], out[form + ".batch_size"] = flat(batches)
            sizes = out[form + ".batch_size"]
            assert len(batches) >= 3 and len(set(sizes.tolist())) >= 2 and sizes.min() >= 1, sizes
            for i in range(len(ds)):
                xs, a, b, c = ds.collator([ds[i]])
                assert a is None and b is None and c is None and xs.dtype.is_floating_point
                assert xs.shape == (len(batches[i]), min(ds[i][-1].xlen, 250000)), xs.shape
                out[f"{form}.xs.{i}"] = xs.numpy().astype(np.float32, copy=True)
            print(form, "rows", len(rows), "batch sizes", sizes.tolist())
        Wav2VecBatch.max_batch_frame = 1400000

    rng = np.random.default_rng(7)
    lens = rng.integers(30000, 400001, size=200).astype(np.int64)
    lens[17] = lens[18]  # a tie: the sort is stable
    recs = [Audio("none", 0, int(n), None, None) for n in lens]
    pol = Wav2VecBatch(cfg)
    assert pol.max_batch_frame == 1400000
    order = [i for i, _ in sorted(enumerate(recs), key=lambda d: d[1].xlen, reverse=True)]
    pol.batchify(order, recs)
    batches = [list(b) for b in pol.data]
    assert len(batches) >= 4, len(batches)
    assert any(min(recs[i].xlen for i in b) > 250000 for b in batches)
    out["syn.len"] = lens
    out["syn.order"] = np.array(order, dtype=np.int64)
    out["syn.batch_flat"], out["syn.batch_size"] = flat(batches)
    print("synthetic batch sizes", out["syn.batch_size"].tolist())

    path = os.path.join(HERE, "pretrain.npz")
    np.savez_compressed(path, **out)
    audio = sum(os.path.getsize(os.path.join(DATA, "wav", f)) for f in os.listdir(os.path.join(DATA, "wav")))
    assert audio < 200 * 1024, audio
    print("wrote", path, os.path.getsize(path), "bytes; audio", audio, "bytes")


if __name__ == "__main__":
    main()
