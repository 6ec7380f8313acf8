"""Front-end timing on one MI355X: ``lasr_fbank`` against the same transform composed from torch
ops, and task=asr Trainer steps fed from wav.scp against the same utterances fed from feats.scp.

  python tools/fbank_bench.py [--repeats 15] [--iters 20] [--steps 24] [--rounds 3] [--out FILE]

It writes its own seeded 16 kHz, 16-bit mono WAV files into a temporary directory, measures, and
prints one JSON line (appended to --out when given):

* ``kernel``: B = 32 utterances of 160400 samples (T = 1001 frames, F = 80) already in HBM as
  int16.  ``fbank`` is one ``lasr_fbank`` launch, ``fbank_graph`` the same launch replayed from a
  captured hipGraph, ``torch`` the composition ``unfold`` -> DC removal -> pre-emphasis -> povey
  window -> ``torch.fft.rfft(n=512)`` -> power -> matmul with the [256, F] mel matrix -> log, on
  the identical input, launched eagerly (a dozen device-bound kernels on 51 MB of frames: the
  queue never runs dry, so nothing is lost to launch gaps; it is not captured because the FFT
  library may allocate inside a capture).  Each sample is device time by events around --iters
  back-to-back calls, divided by --iters; the three alternate for --repeats samples; median /
  min / max.  ``fbank_faster_beyond_spread``: the torch minimum minus the kernel median exceeds
  the torch spread (max - min).  The two results are compared first (largest difference of the
  log values over the bins within 1e-6 of each frame's peak energy).
* ``loader``: ms per eager ``conformer_small`` bf16 step through ``Trainer.run`` (batches of 32
  utterances of 160400 samples, SpecAugment on), fed by AudioFileDataset over a wav.scp directory
  and over a feats.scp directory holding the front end's own output for the same files, at
  num_workers 0 and 4; the four alternate for --rounds rounds of --steps steps, the first 4 steps
  of every run are dropped; median / min / max.  A step is timed from one optimizer step's return
  (it reads the skipped flag back, a device synchronisation) to the next.
"""

import argparse
import hashlib
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DROP = 4
B, S, F = 32, 160400, 80


def _stats(ts, nd=4):
    return {"median": round(statistics.median(ts), nd), "min": round(min(ts), nd), "max": round(max(ts), nd)}


def torch_fbank(pcm, window, mel_t):
    """The transform from torch ops: pcm int16 (B, S) on the device -> fp32 (B, T, F)."""
    x = pcm.float().unfold(1, 400, 160)
    x = x - x.mean(dim=-1, keepdim=True)
    x = x - 0.97 * torch.cat([x[..., :1], x[..., :-1]], dim=-1)
    spec = torch.fft.rfft(x * window, n=512)
    power = spec.real.square() + spec.imag.square()
    return torch.log(torch.clamp(power[..., :256] @ mel_t, min=torch.finfo(torch.float32).eps))


def kernel_bench(repeats, iters):
    from liteasr_amd import kernels as K

    rng = np.random.default_rng(0)
    pcm = np.clip(np.round(rng.standard_normal((B, S)) * 3000), -32768, 32767).astype(np.int16)
    pcm = torch.from_numpy(pcm).cuda()
    T = K.fbank_num_frames(S)
    nf = torch.full((B,), T, dtype=torch.int32, device="cuda")
    out = torch.empty(B, T, F, device="cuda")
    tab, seg = K.fbank_tables(F)
    mel = np.zeros((F, 256), dtype=np.float64)
    for f in range(F):
        mel[f, seg[f]:seg[f + 1]] += tab[1536:1792][seg[f]:seg[f + 1]]
        mel[f, seg[f + 1]:seg[f + 2]] += tab[1792:2048][seg[f + 1]:seg[f + 2]]
    window = torch.from_numpy(tab[:400].copy()).cuda()
    mel_t = torch.from_numpy(mel.T.astype(np.float32).copy()).cuda()

    def run_fbank():
        K.fbank(pcm, nf, F, out=out, max_frames=T)

    for _ in range(3):
        run_fbank()
        ref = torch_fbank(pcm, window, mel_t)
    torch.cuda.synchronize()
    strong = ref >= ref.amax(dim=-1, keepdim=True) - 13.8  # bins within 1e-6 of the frame's peak energy
    diff = float((out - ref).abs()[strong].max())
    assert diff < 1e-3, f"kernel and torch composition disagree: {diff}"
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run_fbank()
    fns = {"fbank": run_fbank, "fbank_graph": graph.replay, "torch": lambda: torch_fbank(pcm, window, mel_t)}
    ts = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():  # alternating
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b) / iters)
    res = {"B": B, "S": S, "T": T, "F": F, "iters_per_sample": iters, "max_log_diff_strong_bins": diff}
    res.update({k + "_ms": _stats(v) for k, v in ts.items()})
    spread = res["torch_ms"]["max"] - res["torch_ms"]["min"]
    res["fbank_faster_beyond_spread"] = res["torch_ms"]["min"] - res["fbank_graph_ms"]["median"] > spread
    return res


def dump_feats(wav_dir, out_dir):
    """The front end's features of every file of wav_dir as a feats.scp directory with the same
    utterance list (entries that share a file share its features)."""
    from liteasr_amd.dataclass.sheet import AudioSheet
    from liteasr_amd.utils import wavio
    from liteasr_amd.utils.frontend import Fbank, num_frames
    from liteasr_amd.utils.kaldiio import save_ark

    fe = Fbank(F)
    os.makedirs(out_dir)
    entries = list(AudioSheet(wav_dir))
    files = sorted({fd for _, fd, _, _ in entries})
    feats, pos = {}, {}
    for fd in files:
        pcm, got = wavio.read(fd)
        x = torch.from_numpy(pcm[:got]).unsqueeze(0).cuda()
        t = num_frames(got)
        nf = torch.tensor([t], dtype=torch.int32, device="cuda")
        feats[os.path.basename(fd)] = fe(x, nf, max_frames=t)[0].cpu().numpy()
    ark = os.path.join(out_dir, "feats.ark")
    save_ark(ark, feats, scp=os.path.join(out_dir, "files.scp"))
    for line in open(os.path.join(out_dir, "files.scp")):
        k, v = line.split(None, 1)
        pos[k] = v.strip()
    with open(os.path.join(out_dir, "feats.scp"), "w") as scp, \
            open(os.path.join(out_dir, "utt2num_frames"), "w") as u2n:
        for uttid, fd, _, _ in entries:
            k = os.path.basename(fd)
            scp.write(f"{uttid} {pos[k]}\n")
            u2n.write(f"{uttid} {feats[k].shape[0]}\n")
    os.remove(os.path.join(out_dir, "files.scp"))
    for fn in ("text", "vocab.txt"):
        shutil.copy(os.path.join(wav_dir, fn), out_dir)
    return out_dir


def loader_bench(wav_dir, feats_dir, steps, rounds, save_dir):
    from types import SimpleNamespace

    from liteasr_amd import tasks
    from liteasr_amd.config.compose import compose

    over = ["model=conformer_small", "criterion=hybrid_ctc_w03", "optimizer=noam_d256", "dataset.batch_count=seq",
            f"dataset.batch_size={B}", "dataset.min_batch_size=1", "dataset.max_len_in=100000",
            "dataset.max_len_out=1000", f"task.save_dir={save_dir}"]
    trainers = {}
    model = crit = opt = None
    for kind, d in (("wav", wav_dir), ("feats", feats_dir)):
        cfg = compose(overrides=["task=asr_wav", f"task.vocab={d}/vocab.txt", f"task.train={d}", f"task.valid={d}"]
                      + over)
        task = tasks.setup_task(cfg.task)
        task.load_dataset("train", d, cfg.dataset, cfg.postprocess, False)
        if model is None:
            torch.manual_seed(42)
            model = task.build_model(cfg.model).cuda().train()
            opt = task.build_optimizer(model.parameters(), cfg.optimizer)
            crit = task.build_criterion(cfg.criterion)
        trainers[kind] = task
    shapes = {k: sorted({tuple(t.dataset("train").collator([t.dataset("train")[i]])[0].shape)
                         for i in range(min(len(t.dataset("train")), 4))}) for k, t in trainers.items()}
    from liteasr_amd.trainer import Trainer

    feeds = [(k, w) for w in (0, 4) for k in ("wav", "feats")]
    ts = {f"{k}_workers_{w}": [] for k, w in feeds}
    skipped = dict.fromkeys(ts, 0)
    for _ in range(rounds):
        for kind, workers in feeds:  # alternating
            name = f"{kind}_workers_{workers}"
            task = trainers[kind]
            data = task.dataset("train")
            tcfg = SimpleNamespace(distributed=SimpleNamespace(num_workers=workers), common=SimpleNamespace(trigger=[]),
                                   optimization=SimpleNamespace(max_epoch=-1, max_iter=steps, accum_grad=1,
                                                                clip_grad_norm=5.0))
            shim = SimpleNamespace(dataset=lambda split, data=data: data, frontend=task.frontend)
            tr = Trainer(tcfg, shim, model, crit, opt, device="cuda")
            stamps, inner = [], tr._optimizer_step

            def stepped(inner=inner, stamps=stamps):
                took = inner()
                stamps.append(time.perf_counter())
                return took

            tr._optimizer_step = stepped
            tr.run()
            assert tr.iter + tr.skipped == steps and tr.epoch == 0, (name, tr.iter, tr.skipped, tr.epoch)
            skipped[name] += tr.skipped
            ts[name] += [(b - a) * 1e3 for a, b in zip(stamps[DROP - 1:], stamps[DROP:])]
            del tr
    out = {"batch_shapes": {k: [list(s) for s in v] for k, v in shapes.items()}, "steps_per_run": steps,
           "rounds": rounds, "dropped_per_run": DROP, "nan_skipped_steps": skipped}
    out.update({k + "_ms_per_step": _stats(v, 3) for k, v in ts.items()})
    for w in (0, 4):
        a, b = out[f"wav_workers_{w}_ms_per_step"], out[f"feats_workers_{w}_ms_per_step"]
        out[f"wav_slower_beyond_spread_workers_{w}"] = a["median"] - b["median"] > b["max"] - b["min"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-loader", action="store_true", help="only the kernel part")
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fbank_bench: no GPU (nothing is measured on the host)")
    lib = os.path.join(ROOT, "liteasr_amd", "lib", "libliteasr_hip.so")
    out = {"workload": "fbank front end: int16 PCM in HBM -> fp32 (B, T, 80); conformer_small bf16 Trainer steps "
                       "from wav.scp and from feats.scp"}
    out["kernel"] = kernel_bench(a.repeats, a.iters)
    if not a.skip_loader:
        from liteasr_amd.utils.synthetic import synthetic_wav_dir

        with tempfile.TemporaryDirectory() as d:
            lines = B * (a.steps + 2)  # a run stays inside one epoch
            wav = synthetic_wav_dir(os.path.join(d, "wav"), [S] * (2 * B), seed=3, lines=lines)
            feats = dump_feats(wav, os.path.join(d, "feats"))
            out["loader"] = loader_bench(wav, feats, a.steps, a.rounds, os.path.join(d, "ckpts"))
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
