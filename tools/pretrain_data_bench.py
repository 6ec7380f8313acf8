"""Pretraining data path timing on one MI355X (task=pretrain, model=wav2vec2_base).

  python tools/pretrain_data_bench.py [--repeats 15] [--steps 24] [--rounds 3] [--out FILE]

It writes its own seeded 16 kHz, 16-bit mono WAV files into a temporary directory, measures, and
prints one JSON line (appended to --out when given):

* ``batch_to_device``: per minibatch, from the list of records to an fp32 (B, S) tensor in HBM,
  host clock around work that ends in a device synchronisation, the two paths alternating,
  median / min / max over --repeats after warm-up (the files are in the page cache by then):
    ``pcm``    the product path: one native batched read into an int16 (B, S) tensor, pinned,
               one host-to-device copy of int16, lasr_pcm_to_float;
    ``float``  the reference's path restated here from numpy / torch ops only (no product code):
               per utterance the whole file decoded to float64 / 32768, cast to float32, sliced
               and cropped, then pad_sequence, pinned, one host-to-device copy of float32.
  Two sets: ``uniform`` (8 utterances of 64000 samples) and ``tail`` (16 utterances whose
  lengths spread from 48000 to 240000 samples, cropped to the shortest, as the collator does).
  ``pcm_faster_beyond_spread`` is pcm's median below float's minimum.  Both results are compared
  bit for bit first.
* ``loader``: ms per step of ``wav2vec2_base`` bf16 eager steps through ``Trainer.run`` (96
  files of 64000 samples listed 320 times so that a run stays inside one epoch (the loader starts
  its workers anew every epoch), dataset.max_batch_frame 512000: batches of 8 x 64000), fed by
  RawAudioFileDataset at num_workers 0 and 4 and, for comparison, by the same int16 batches held
  in memory; the three alternate for --rounds rounds of --steps steps, the first 4 steps of every
  run are dropped, median / min / max of the rest.  A step is timed from one optimizer step's
  return (it reads the skipped flag back, a device synchronisation) to the next.
"""

import argparse
import hashlib
import json
import os
import statistics
import sys
import tempfile
import time
import wave

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DROP = 4  # steps dropped at the start of every loader run (worker start-up, first launches)


def _stats(ts):
    return {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}


def write_set(d, name, lengths, seed, lines=None):
    """A wav.scp data directory d/name of len(lengths) seeded files; returns its path.  With
    ``lines`` the scp has that many entries, cycling over the files (a longer epoch)."""
    rng = np.random.default_rng(seed)
    root = os.path.join(d, name)
    os.makedirs(root)
    paths = []
    with open(os.path.join(root, "wav.scp"), "w") as scp:
        for i, n in enumerate(lengths):
            p = os.path.join(root, f"utt{i:03d}.wav")
            paths.append(p)
            pcm = np.clip(np.round(rng.standard_normal(n) * 3000), -32768, 32767).astype("<i2")
            with wave.open(p, "wb") as w:
                w.setnchannels(1)
                w.setsampwidth(2)
                w.setframerate(16000)
                w.writeframes(pcm.tobytes())
            scp.write(f"utt{i:03d} {p}\n")
        for j in range(len(lengths), lines or 0):
            scp.write(f"utt{j:03d} {paths[j % len(paths)]}\n")
    return root


def reference_batch(records, S):
    """The reference's collation (audio_data.py:30-33, pretrain_dataset.py:51-56) from numpy / torch."""
    xs = []
    for fd, start, xlen in records:
        with wave.open(fd, "rb") as w:
            pcm = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
        x = torch.from_numpy(pcm.astype(np.float64) / 32768.0).float()
        xs.append(x[start:start + xlen][:S])
    return torch.nn.utils.rnn.pad_sequence(xs, batch_first=True)


def batch_to_device(data_dir, repeats, warmup=3):
    from liteasr_amd import kernels as K
    from liteasr_amd.dataclass.sheet import AudioSheet
    from liteasr_amd.utils import wavio

    records = sorted(((fd, start, n) for _, fd, start, n in AudioSheet(data_dir)), key=lambda r: -r[2])
    S = min(records[-1][2], 250000)
    B = len(records)

    def pcm_path():
        xs = torch.empty(B, S, dtype=torch.int16)
        wavio.read_batch([r[0] for r in records], [r[1] for r in records], S, out=xs.numpy())
        out = K.pcm_to_float(xs.pin_memory().to("cuda", non_blocking=True))
        torch.cuda.synchronize()
        return out

    def float_path():
        out = reference_batch(records, S).pin_memory().to("cuda", non_blocking=True)
        torch.cuda.synchronize()
        return out

    fns = {"pcm": pcm_path, "float": float_path}
    for _ in range(warmup):
        a, b = pcm_path(), float_path()
    assert a.dtype == b.dtype == torch.float32 and torch.equal(a, b), "the two paths disagree"
    ts = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():  # alternating
            t0 = time.perf_counter()
            fn()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    out = {"B": B, "S": S, "bytes_h2d": {"pcm": 2 * B * S, "float": 4 * B * S}, "bit_equal": True}
    out.update({k + "_ms": _stats(v) for k, v in ts.items()})
    out["pcm_faster_beyond_spread"] = out["pcm_ms"]["median"] < out["float_ms"]["min"]
    return out


class _Held(torch.utils.data.Dataset):
    """Collated batches held in memory (what the loader would deliver, at no cost)."""

    def __init__(self, batches):
        self.batches = batches

    def __len__(self):
        return len(self.batches)

    def __getitem__(self, i):
        return self.batches[i]

    @staticmethod
    def collator(items):
        return items[0]


def loader_steps(data_dir, steps, rounds):
    from types import SimpleNamespace

    from liteasr_amd.config.compose import compose
    from liteasr_amd.criterions import build_criterion
    from liteasr_amd.dataset import RawAudioFileDataset
    from liteasr_amd.models import build_model
    from liteasr_amd.optims.noam import Noam, NoamConfig
    from liteasr_amd.trainer import Trainer

    cfg = compose(overrides=["task=pretrain_wav", "model=wav2vec2_base", "criterion=wav2vec", "optimizer=noam_d256"])
    torch.manual_seed(42)
    np.random.seed(42)
    model = build_model(cfg.model, None).cuda().train()
    crit = build_criterion(cfg.criterion, None)
    opt = Noam(model.parameters(), NoamConfig(model_dim=cfg.model.encoder_embed_dim))
    ds = RawAudioFileDataset(data_dir, SimpleNamespace(max_batch_frame=512000), None, raw_pcm=True)
    shapes = sorted({tuple(ds.collator([ds[i]])[0].shape) for i in range(len(ds))})
    held = _Held([ds.collator([ds[i]]) for i in range(len(ds))])
    feeds = {"in_memory": (held, 0), "workers_0": (ds, 0), "workers_4": (ds, 4)}
    ts = {k: [] for k in feeds}
    skipped = {k: 0 for k in feeds}
    for _ in range(rounds):
        for name, (data, workers) in feeds.items():  # alternating
            tcfg = SimpleNamespace(distributed=SimpleNamespace(num_workers=workers), common=SimpleNamespace(trigger=[]),
                                   optimization=SimpleNamespace(max_epoch=-1, max_iter=steps, accum_grad=1,
                                                                clip_grad_norm=5.0))
            tr = Trainer(tcfg, SimpleNamespace(dataset=lambda split, data=data: data), model, crit, opt, device="cuda")
            stamps = []
            inner = tr._optimizer_step

            def stepped():
                took = inner()
                stamps.append(time.perf_counter())
                return took

            tr._optimizer_step = stepped
            tr.run()
            assert tr.iter == steps and tr.epoch == 0, (name, tr.iter, tr.epoch)
            skipped[name] += tr.skipped  # a NaN-skipped step does the same work up to the update
            ts[name] += [(b - a) * 1e3 for a, b in zip(stamps[DROP - 1:], stamps[DROP:])]
            del tr
    out = {"batch_shapes": [list(s) for s in shapes], "batches": len(ds), "steps_per_run": steps, "rounds": rounds,
           "dropped_per_run": DROP, "nan_skipped_steps": skipped}
    out.update({k + "_ms_per_step": _stats(v) for k, v in ts.items()})
    spread = out["in_memory_ms_per_step"]["max"] - out["in_memory_ms_per_step"]["min"]
    for k in ("workers_0", "workers_4"):
        out[k + "_slower_beyond_spread"] = (out[k + "_ms_per_step"]["median"]
                                            - out["in_memory_ms_per_step"]["median"]) > spread
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-loader", action="store_true", help="only the batch-to-device part")
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pretrain_data_bench: no GPU (nothing is measured on the host)")
    lib = os.path.join(ROOT, "liteasr_amd", "lib", "libliteasr_hip.so")
    out = {"workload": "pretraining data path: WAV on disk -> fp32 (B, S) in HBM; wav2vec2_base bf16 Trainer steps",
           "host_threads_for_reads": "lasr_wav_read_batch default (at most 16)"}
    with tempfile.TemporaryDirectory() as d:
        tail = [int(v) for v in np.linspace(240000, 48000, 16)]
        sets = {"uniform": write_set(d, "uniform", [64000] * 8, 1), "tail": write_set(d, "tail", tail, 2)}
        out["batch_to_device"] = {k: batch_to_device(v, a.repeats) for k, v in sets.items()}
        if not a.skip_loader:
            out["loader"] = loader_steps(write_set(d, "train", [64000] * 96, 3, lines=320), a.steps, a.rounds)
    out["repeats"] = a.repeats
    out["build"] = hashlib.sha256(open(lib, "rb").read()).hexdigest()[:16]
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
