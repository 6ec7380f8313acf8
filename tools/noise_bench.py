"""Additive-noise timing on one MI355X: ``lasr_mix_i16`` against the same transform composed from
torch ops, the device front end (mix + fbank) as a share of a training step fed from wav.scp with
``frontend.noise`` on, and what the same mixing costs a loader on the host.

  python tools/noise_bench.py [--repeats 15] [--iters 20] [--steps 24] [--rounds 3] [--out FILE]
                              [--kernel-stats FILE]

It writes its own seeded 16 kHz, 16-bit mono WAV files into a temporary directory, measures, and
prints one JSON line (appended to --out when given):

* ``kernel``: B = 32 rows of up to 160400 int16 samples already in HBM (row 0 full, the others 50 to
  100 % of it), rows 0, 2, 4, ... with 1 source, rows 1, 5, 9, ... with 5 and the rest with none,
  SNRs 0 to 20 dB, out of a resident bank of 300 recordings of 5 to 60 s.  ``mix`` is one
  ``lasr_mix_i16`` call (two launches) in place, ``mix_graph`` the same replayed from a captured
  hipGraph, ``torch`` the composition on the identical input, launched eagerly: per source slot a
  modular gather out of the bank, int64 sums of squares, the gain in float64, ``addcmul``, then
  ``round``, ``clamp``, the cast to int16 and the zero padding.  Each sample is device time by events
  around --iters back-to-back calls, divided by --iters, after one untimed pass; the three alternate
  for --repeats samples; median / min / max.  ``mix_faster_beyond_spread``: the torch minimum minus
  the kernel median exceeds the torch spread (max - min).  The two results are compared first (at
  most 1 LSB apart: the composition may round the product).  ``bytes`` is what the two launches
  move (every row's samples read twice and each of its sources' read twice, the whole output
  written), ``achieved_gbps`` that over the graph-replayed median, ``share_of_8tbps`` its share of
  the HBM roofline.
* ``loader``: ms per eager ``conformer_small`` bf16 step through ``Trainer.run`` (batches of 32
  utterances of 80200 .. 160400 samples, SpecAugment on) fed by AudioFileDataset over a wav.scp
  directory with two noise directories on and with the option off, at num_workers 0 and 4; the four
  alternate for --rounds rounds of --steps steps, the first 4 steps of every run are dropped; median
  / min / max.  ``frontend_share``: device time of mix + fbank (events around the calls) over the
  wall time of the same steps.
* ``host``: as context, one such batch mixed with numpy the way a collator would have to (gather,
  energies, gain, multiply-add, round, clip per row); ms per batch, median / min / max of 5.

--kernel-stats FILE: one more run of the kernel part alone under ``rocprofv3 --kernel-trace
--stats`` in a child process; the rows of its kernel statistics that belong to the two mix kernels
are written to FILE (CSV).  --trace-leg is that child's mode: the kernel part, no output.
"""

import argparse
import glob
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DROP = 4
B, S = 32, 160400
NREC = 300


def _stats(ts, nd=4):
    return {"median": round(statistics.median(ts), nd), "min": round(min(ts), nd), "max": round(max(ts), nd)}


def torch_mix(pcm, bank, n, slots, out):
    """The transform from torch ops.  n int64 [B]; slots: per source slot (row indices, offset,
    length, start int64 [rows], r float64 [rows])."""
    m = torch.arange(pcm.shape[1], device=pcm.device)
    valid = m[None, :] < n[:, None]
    x = pcm.long() * valid
    ex = (x * x).sum(1)
    acc = pcm.float()
    for idx, off, length, start, r in slots:
        v = bank[off[:, None] + (start[:, None] + m[None, :]) % length[:, None]]
        vl = v.long() * valid[idx]
        ev = (vl * vl).sum(1)
        e = ex[idx]
        g = torch.sqrt(e.double() / ev.double() * r)
        g = torch.where((e > 0) & (ev > 0), g, torch.zeros_like(g)).float()
        acc[idx] = torch.addcmul(acc[idx], g[:, None], v.float())
    out.copy_(acc.round().clamp(-32768, 32767).to(torch.int16) * valid)
    return out


def kernel_case():
    from liteasr_amd import kernels as K

    rng = np.random.default_rng(0)
    gen = torch.Generator(device="cuda").manual_seed(0)
    pcm0 = (torch.randn(B, S, device="cuda", generator=gen) * 6000).round().clamp(-32768, 32767).to(torch.int16)
    lengths = rng.integers(5 * 16000, 60 * 16000 + 1, NREC)
    offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    bank = (torch.randn(int(lengths.sum()), device="cuda", generator=gen) * 3000).round().to(torch.int16)
    ns = [S] + rng.integers(S // 2, S + 1, B - 1).tolist()
    for b, n in enumerate(ns):
        pcm0[b, n:] = 0
    counts = [1 if b % 2 == 0 else (5 if b % 4 == 1 else 0) for b in range(B)]
    srcs = []
    for k in counts:
        recs = rng.integers(NREC, size=k)
        srcs.append([(int(offsets[r]), int(lengths[r]), int(rng.integers(lengths[r])),
                      10.0 ** (-float(rng.uniform(0, 20)) / 10.0)) for r in recs])
    rows_h, table_h = K.mix_plan(ns, srcs)
    nbytes = sum(2 * 2 * n * (1 + k) for n, k in zip(ns, counts)) + 2 * B * S
    return pcm0, bank, ns, counts, srcs, torch.from_numpy(rows_h).cuda(), torch.from_numpy(table_h).cuda(), nbytes


def kernel_bench(repeats, iters, trace_only=False):
    from liteasr_amd import kernels as K

    pcm0, bank, ns, counts, srcs, rows, table, nbytes = kernel_case()
    work = pcm0.clone()
    out, ref = torch.empty_like(pcm0), torch.empty_like(pcm0)

    def run_kernel():  # in place, as the trainer calls it; the timed calls mix what the last one left
        K.mix_i16(work, bank, rows, table, out=work)

    K.mix_i16(pcm0, bank, rows, table, out=out)
    if trace_only:
        for _ in range(iters):
            run_kernel()
        torch.cuda.synchronize()
        return None, None
    n_dev = torch.tensor(ns, device="cuda")
    slots = []
    for j in range(max(counts)):
        idx = [b for b in range(B) if counts[b] > j]
        cols = [torch.tensor([srcs[b][j][c] for b in idx], device="cuda") for c in range(3)]
        slots.append((torch.tensor(idx, device="cuda"), *cols,
                      torch.tensor([srcs[b][j][3] for b in idx], dtype=torch.float64, device="cuda")))
    torch_mix(pcm0, bank, n_dev, slots, ref)
    torch.cuda.synchronize()
    diff = int((out.int() - ref.int()).abs().max())
    differing = float((out != ref).float().mean())
    assert diff <= 1, f"kernel and torch composition disagree by {diff} LSB"
    assert not torch.equal(out, pcm0)
    run_kernel()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run_kernel()
    fns = {"mix": run_kernel, "mix_graph": graph.replay, "torch": lambda: torch_mix(pcm0, bank, n_dev, slots, ref)}
    for fn in fns.values():  # the untimed pass
        fn()
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
    res = {"B": B, "S": S, "rows_with_1_source": counts.count(1), "rows_with_5_sources": counts.count(5),
           "bank_recordings": NREC, "bank_mb": round(2 * bank.numel() / (1 << 20), 1), "iters_per_sample": iters,
           "max_diff_lsb": diff, "share_differing": differing, "bytes": nbytes}
    res.update({k + "_ms": _stats(v) for k, v in ts.items()})
    spread = res["torch_ms"]["max"] - res["torch_ms"]["min"]
    res["mix_faster_beyond_spread"] = res["torch_ms"]["min"] - res["mix_ms"]["median"] > spread
    gbps = nbytes / (res["mix_graph_ms"]["median"] * 1e-3) / 1e9
    res["achieved_gbps"], res["share_of_8tbps"] = round(gbps, 1), round(gbps / 8000.0, 4)
    host = (pcm0.cpu().numpy(), bank.cpu().numpy(), ns, srcs, out.cpu().numpy())
    return res, host


class TimedCall(object):
    def __init__(self, owner, fn):
        self.owner, self.fn = owner, fn

    def __call__(self, *a, **k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        y = self.fn(*a, **k)
        e1.record()
        self.owner.events.append((e0, e1))
        return y


class TimedFrontend(object):
    """The task's front end with device events around its calls."""

    def __init__(self, inner):
        self.inner, self.events = inner, []
        self.num_mel_bins = inner.num_mel_bins
        self.speed = TimedCall(self, inner.speed)
        self.noise = TimedCall(self, inner.noise) if inner.noise is not None else None
        self._fbank = TimedCall(self, inner)

    def __call__(self, *a, **k):
        return self._fbank(*a, **k)


def loader_bench(wav_dir, noise_dirs, steps, rounds, save_dir):
    from types import SimpleNamespace

    from liteasr_amd import tasks
    from liteasr_amd.config.compose import compose
    from liteasr_amd.trainer import Trainer

    over = ["model=conformer_small", "criterion=hybrid_ctc_w03", "optimizer=noam_d256", "dataset.batch_count=seq",
            f"dataset.batch_size={B}", "dataset.min_batch_size=1", "dataset.max_len_in=100000",
            "dataset.max_len_out=1000", f"task.save_dir={save_dir}", "task=asr_wav", f"task.vocab={wav_dir}/vocab.txt",
            f"task.train={wav_dir}", f"task.valid={wav_dir}", "task.frontend.noise_snr=[0,15,13,20]",
            "task.frontend.noise_sources=[1,1,3,7]"]
    trainers = {}
    model = crit = opt = None
    for kind, noise in (("on", "[" + ",".join(noise_dirs) + "]"), ("off", "null")):
        cfg = compose(overrides=over + [f"task.frontend.noise={noise}"])
        task = tasks.setup_task(cfg.task)
        task.load_dataset("train", wav_dir, cfg.dataset, cfg.postprocess, False)
        if model is None:
            torch.manual_seed(42)
            model = task.build_model(cfg.model).cuda().train()
            opt = task.build_optimizer(model.parameters(), cfg.optimizer)
            crit = task.build_criterion(cfg.criterion)
        trainers[kind] = task
    trainers["on"].frontend.noise.bank_on("cuda")  # the one-time read and upload is not a step's cost
    feeds = [(k, w) for w in (0, 4) for k in ("on", "off")]
    ts = {f"{k}_workers_{w}": [] for k, w in feeds}
    share = {k: [] for k in ts}
    skipped = dict.fromkeys(ts, 0)
    for _ in range(rounds):
        for kind, workers in feeds:  # alternating
            name = f"{kind}_workers_{workers}"
            task = trainers[kind]
            data = task.dataset("train")
            tcfg = SimpleNamespace(distributed=SimpleNamespace(num_workers=workers), common=SimpleNamespace(trigger=[]),
                                   optimization=SimpleNamespace(max_epoch=-1, max_iter=steps, accum_grad=1,
                                                                clip_grad_norm=5.0))
            fe = TimedFrontend(task.frontend)
            shim = SimpleNamespace(dataset=lambda split, data=data: data, frontend=fe)
            tr = Trainer(tcfg, shim, model, crit, opt, device="cuda")
            stamps, marks, inner = [], [], tr._optimizer_step

            def stepped(inner=inner, stamps=stamps, marks=marks, fe=fe):
                took = inner()
                stamps.append(time.perf_counter())
                marks.append(len(fe.events))
                return took

            tr._optimizer_step = stepped
            tr.run()
            torch.cuda.synchronize()
            assert tr.iter + tr.skipped == steps and tr.epoch == 0, (name, tr.iter, tr.skipped, tr.epoch)
            skipped[name] += tr.skipped
            ts[name] += [(b - a) * 1e3 for a, b in zip(stamps[DROP - 1:], stamps[DROP:])]
            dev = sum(e0.elapsed_time(e1) for e0, e1 in fe.events[marks[DROP - 1]:marks[-1]])
            share[name].append(dev / ((stamps[-1] - stamps[DROP - 1]) * 1e3))
            del tr
    idx = trainers["on"].frontend.noise.index
    out = {"steps_per_run": steps, "rounds": rounds, "dropped_per_run": DROP, "nan_skipped_steps": skipped,
           "noise_recordings": len(idx.paths), "noise_bank_mb": round(2 * idx.total / (1 << 20), 1)}
    out.update({k + "_ms_per_step": _stats(v, 3) for k, v in ts.items()})
    out.update({k + "_frontend_share": _stats(v, 5) for k, v in share.items()})
    return out


def host_bench(pcm, bank, ns, srcs, device_out, repeats=5):
    def one(b):
        n = ns[b]
        x = pcm[b, :n]
        acc = x.astype(np.float32)
        ex = int((x.astype(np.int64) ** 2).sum())
        for off, length, start, r in srcs[b]:
            v = bank[off + (start + np.arange(n)) % length]
            ev = int((v.astype(np.int64) ** 2).sum())
            g = np.float32(np.sqrt(np.float64(ex) / np.float64(ev) * r)) if ex and ev else np.float32(0)
            acc = acc + g * v.astype(np.float32)
        y = np.zeros(pcm.shape[1], dtype=np.int16)
        y[:n] = np.clip(np.rint(acc), -32768, 32767).astype(np.int16)
        return y

    got = np.stack([one(b) for b in range(len(ns))])
    diff = int(np.abs(got.astype(np.int32) - device_out.astype(np.int32)).max())
    assert diff <= 1, f"host and device mixing disagree by {diff} LSB"
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for b in range(len(ns)):
            one(b)
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"max_diff_lsb_to_device": diff, "numpy_ms_per_batch": _stats(ts, 2)}


def kernel_stats(path, iters):
    """The kernel part once more under the profiler, in a child process; the mix kernels' rows of its
    kernel statistics go to ``path``."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--",
               sys.executable, os.path.abspath(__file__), "--trace-leg", "--iters", str(iters)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        found = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))
        if r.returncode != 0 or not found:
            raise RuntimeError(f"rocprofv3 run failed ({r.returncode}): {r.stderr[-2000:]}")
        lines = open(found[0]).read().splitlines()
    keep = [lines[0]] + [ln for ln in lines[1:] if "mix_energy_kernel" in ln or "mix_apply_kernel" in ln]
    if len(keep) != 3:
        raise RuntimeError(f"expected the two mix kernels in the statistics, got {keep[1:]}")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write("\n".join(keep) + "\n")
    return keep[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-loader", action="store_true", help="only the kernel and host parts")
    ap.add_argument("--trace-leg", action="store_true", help="the kernel part alone, no output (the profiled child)")
    ap.add_argument("--kernel-stats", default=None, help="write the mix kernels' rocprofv3 statistics to this CSV file")
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    a = ap.parse_args()
    if a.trace_leg:
        kernel_bench(a.repeats, a.iters, trace_only=True)
        return
    if a.kernel_stats:  # before this process opens the GPU
        kernel_stats(a.kernel_stats, a.iters)
    if not torch.cuda.is_available():
        raise SystemExit("noise_bench: no GPU (the device parts are not measured on the host)")
    lib = os.path.join(ROOT, "liteasr_amd", "lib", "libliteasr_hip.so")
    out = {"workload": "additive noise: int16 PCM in HBM + sources of a resident int16 bank at drawn SNRs -> int16, in "
                       "place; conformer_small bf16 Trainer steps from wav.scp with frontend.noise on"}
    out["kernel"], host_case = kernel_bench(a.repeats, a.iters)
    out["host"] = host_bench(*host_case)
    if not a.skip_loader:
        from liteasr_amd.utils.synthetic import synthetic_wav_dir

        with tempfile.TemporaryDirectory() as d:
            rng = np.random.default_rng(5)
            lengths = rng.integers(S // 2, S + 1, 2 * B).tolist()
            lines = B * (a.steps + 2)  # a run stays inside one epoch
            wav = synthetic_wav_dir(os.path.join(d, "wav"), lengths, seed=3, lines=lines)
            noise = [synthetic_wav_dir(os.path.join(d, f"noise{i}"), rng.integers(5 * 16000, 20 * 16000, 20).tolist(),
                                       seed=7 + i) for i in range(2)]
            out["loader"] = loader_bench(wav, noise, a.steps, a.rounds, os.path.join(d, "ckpts"))
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
