"""Room-reverberation timing on one MI355X: ``lasr_reverb_i16`` against the same transform composed
from torch ops, and the device front end (reverb + mix + fbank) as a share of a training step fed
from wav.scp with ``frontend.rir`` on.

  python tools/reverb_bench.py [--repeats 15] [--iters 20] [--steps 24] [--rounds 3] [--out FILE]
                               [--kernel-stats FILE]

It writes its own seeded 16 kHz, 16-bit mono WAV files into a temporary directory, measures, and
prints one JSON line (appended to --out when given):

* ``kernel``: B = 32 rows of 80200 to 160400 int16 samples already in HBM (row 0 full), 24 of them
  reverberated (every fourth row is only copied), out of a resident bank of 200 RIRs of 4000 to 16000
  taps (decaying Gaussian noise with a direct-path peak).  ``reverb`` is one ``lasr_reverb_i16``
  call (three launches) in place, ``reverb_graph`` the same replayed from a captured hipGraph,
  ``torch`` the composition on the identical input, launched eagerly: ``torch.fft.rfft`` of the rows
  and of their RIRs at the next power of two above S + Lmax, the product, ``irfft``, a per-row
  gather at the peak, the energies (int64 and float64), the gain in float64, then ``round``,
  ``clamp``, the cast to int16 and the zero padding.  Each sample is device time by events around
  --iters back-to-back calls, divided by --iters, after one untimed pass; the three alternate for
  --repeats samples; median / min / max.  ``reverb_faster_beyond_spread``: the torch minimum minus
  the kernel median exceeds the torch spread (max - min).  The two results are compared first: the
  share of samples that differ is logged and none may differ by more than 1 LSB.
* ``loader``: ms per eager ``conformer_small`` bf16 step through ``Trainer.run`` (batches of 32
  utterances of 80200 .. 160400 samples, SpecAugment on, one noise directory on throughout) fed by
  AudioFileDataset over a wav.scp directory with an RIR directory on and with the option off, at
  num_workers 0 and 4; the four alternate for --rounds rounds of --steps steps, the first 4 steps of
  every run are dropped; median / min / max.  ``frontend_share``: device time of reverb + mix +
  fbank (events around the calls) over the wall time of the same steps.

--kernel-stats FILE: one more run of the kernel part alone under ``rocprofv3 --kernel-trace
--stats`` in a child process; the rows of its kernel statistics that belong to the three reverb
kernels are written to FILE (CSV).  --trace-leg is that child's mode: the kernel part, no output.
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
NRIR, LMIN, LMAX = 200, 4000, 16000
KERNELS = ("reverb_fwd_kernel", "reverb_acc_kernel", "reverb_apply_kernel")


def _stats(ts, nd=4):
    return {"median": round(statistics.median(ts), nd), "min": round(min(ts), nd), "max": round(max(ts), nd)}


def torch_reverb(pcm, n, idx, h, peak, nfft, out):
    """The transform from torch ops.  n int64 [B]; idx: the reverberated rows; h fp32 [rows, Lmax]:
    their RIRs, scaled by 2^-15 and zero-padded; peak int64 [rows]."""
    m = torch.arange(pcm.shape[1], device=pcm.device)
    valid = m[None, :] < n[:, None]
    out.copy_(pcm * valid)
    x = (pcm[idx] * valid[idx]).float()
    full = torch.fft.irfft(torch.fft.rfft(x, n=nfft) * torch.fft.rfft(h, n=nfft), n=nfft)
    c = torch.gather(full, 1, m[None, :] + peak[:, None]) * valid[idx]
    xl = x.long()
    ex = (xl * xl).sum(1)
    ec = (c.double() ** 2).sum(1)
    g = torch.sqrt(ex.double() / ec)
    g = torch.where((ex > 0) & (ec > 0), g, torch.zeros_like(g)).float()
    out[idx] = (g[:, None] * c).round().clamp(-32768, 32767).to(torch.int16) * valid[idx]
    return out


def kernel_case():
    from liteasr_amd import kernels as K

    rng = np.random.default_rng(0)
    gen = torch.Generator(device="cuda").manual_seed(0)
    pcm0 = (torch.randn(B, S, device="cuda", generator=gen) * 3000).round().clamp(-32768, 32767).to(torch.int16)
    lengths = rng.integers(LMIN, LMAX + 1, NRIR)
    offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    recs, peaks = [], []
    for L in lengths:
        h = 0.1 * rng.standard_normal(L) * 10.0 ** (-3.0 * np.arange(L) / 4800.0)
        p = int(rng.integers(0, 80))
        h[p] = 1.0
        recs.append(np.clip(np.round(h * 30000), -32768, 32767).astype(np.int16))
        peaks.append(int(np.argmax(recs[-1])))
    bank_h = np.concatenate(recs)
    table_h = np.stack([offsets, lengths, np.asarray(peaks)], axis=1).astype(np.int64)
    ns = [S] + rng.integers(S // 2, S + 1, B - 1).tolist()
    for b, n in enumerate(ns):
        pcm0[b, n:] = 0
    ids = [-1 if b % 4 == 3 else int(rng.integers(NRIR)) for b in range(B)]
    rows = torch.from_numpy(K.reverb_plan(ns, ids)).cuda()
    return pcm0, torch.from_numpy(bank_h).cuda(), bank_h, table_h, ns, ids, rows, torch.from_numpy(table_h).cuda()


def kernel_bench(repeats, iters, trace_only=False):
    from liteasr_amd import kernels as K

    pcm0, bank, bank_h, table_h, ns, ids, rows, table = kernel_case()
    work = pcm0.clone()
    out, ref = torch.empty_like(pcm0), torch.empty_like(pcm0)

    def run_kernel():  # in place, as the trainer calls it; the timed calls reverberate what the last one left
        K.reverb_i16(work, bank, rows, table, out=work, max_taps=LMAX)

    K.reverb_i16(pcm0, bank, rows, table, out=out, max_taps=LMAX)
    if trace_only:
        for _ in range(iters):
            run_kernel()
        torch.cuda.synchronize()
        return None
    n_dev = torch.tensor(ns, device="cuda")
    idx_h = [b for b in range(B) if ids[b] >= 0]
    h_host = np.zeros((len(idx_h), LMAX), dtype=np.float32)
    for k, b in enumerate(idx_h):
        off, L, _ = table_h[ids[b]]
        h_host[k, :L] = bank_h[off:off + L].astype(np.float32) * np.float32(2.0 ** -15)
    idx, h = torch.tensor(idx_h, device="cuda"), torch.from_numpy(h_host).cuda()
    peak = torch.tensor([int(table_h[ids[b], 2]) for b in idx_h], device="cuda")
    nfft = 1 << int(S + LMAX).bit_length()
    torch_reverb(pcm0, n_dev, idx, h, peak, nfft, ref)
    torch.cuda.synchronize()
    diff = int((out.int() - ref.int()).abs().max())
    differing = float((out != ref).float().mean())
    assert diff <= 1, f"kernel and torch composition disagree by {diff} LSB"
    assert not torch.equal(out, pcm0) and torch.equal(out[3], pcm0[3])
    run_kernel()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run_kernel()
    fns = {"reverb": run_kernel, "reverb_graph": graph.replay,
           "torch": lambda: torch_reverb(pcm0, n_dev, idx, h, peak, nfft, ref)}
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
    taps = [int(table_h[i, 1]) for i in ids if i >= 0]
    res = {"B": B, "S": S, "rows_reverberated": len(idx_h), "bank_rirs": NRIR, "taps_min": min(taps),
           "taps_max": max(taps), "block": K.REVERB_BLOCK, "torch_fft_points": nfft, "iters_per_sample": iters,
           "max_diff_lsb": diff, "share_differing": differing,
           "workspace_mb": round(K.N.load().lasr_reverb_ws_bytes(B, S, LMAX) / (1 << 20), 1)}
    res.update({k + "_ms": _stats(v) for k, v in ts.items()})
    spread = res["torch_ms"]["max"] - res["torch_ms"]["min"]
    res["reverb_faster_beyond_spread"] = res["torch_ms"]["min"] - res["reverb_ms"]["median"] > spread
    return res


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
        self.reverb = TimedCall(self, inner.reverb) if inner.reverb is not None else None
        self._fbank = TimedCall(self, inner)

    def __call__(self, *a, **k):
        return self._fbank(*a, **k)


def loader_bench(wav_dir, rir_dir, noise_dir, steps, rounds, save_dir, workers_list):
    from types import SimpleNamespace

    from liteasr_amd import tasks
    from liteasr_amd.config.compose import compose
    from liteasr_amd.trainer import Trainer

    over = ["model=conformer_small", "criterion=hybrid_ctc_w03", "optimizer=noam_d256", "dataset.batch_count=seq",
            f"dataset.batch_size={B}", "dataset.min_batch_size=1", "dataset.max_len_in=100000",
            "dataset.max_len_out=1000", f"task.save_dir={save_dir}", "task=asr_wav", f"task.vocab={wav_dir}/vocab.txt",
            f"task.train={wav_dir}", f"task.valid={wav_dir}", f"task.frontend.noise=[{noise_dir}]",
            "task.frontend.rir_prob=0.75"]
    trainers = {}
    model = crit = opt = None
    for kind, rir in (("on", f"[{rir_dir}]"), ("off", "null")):
        cfg = compose(overrides=over + [f"task.frontend.rir={rir}"])
        task = tasks.setup_task(cfg.task)
        task.load_dataset("train", wav_dir, cfg.dataset, cfg.postprocess, False)
        if model is None:
            torch.manual_seed(42)
            model = task.build_model(cfg.model).cuda().train()
            opt = task.build_optimizer(model.parameters(), cfg.optimizer)
            crit = task.build_criterion(cfg.criterion)
        trainers[kind] = task
        task.frontend.noise.bank_on("cuda")  # the one-time reads and uploads are not a step's cost
    trainers["on"].frontend.reverb.tables_on("cuda")
    feeds = [(k, w) for w in workers_list for k in ("on", "off")]
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
    idx = trainers["on"].frontend.reverb.index
    out = {"steps_per_run": steps, "rounds": rounds, "dropped_per_run": DROP, "nan_skipped_steps": skipped,
           "rir_prob": 0.75, "rirs": len(idx.paths), "rir_bank_mb": round(2 * idx.total / (1 << 20), 1)}
    out.update({k + "_ms_per_step": _stats(v, 3) for k, v in ts.items()})
    out.update({k + "_frontend_share": _stats(v, 5) for k, v in share.items()})
    return out


def kernel_stats(path, iters):
    """The kernel part once more under the profiler, in a child process; the reverb kernels' rows of
    its kernel statistics go to ``path``."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--",
               sys.executable, os.path.abspath(__file__), "--trace-leg", "--iters", str(iters)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        found = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))
        if r.returncode != 0 or not found:
            raise RuntimeError(f"rocprofv3 run failed ({r.returncode}): {r.stderr[-2000:]}")
        lines = open(found[0]).read().splitlines()
    keep = [lines[0]] + [ln for ln in lines[1:] if any(k in ln for k in KERNELS)]
    if len(keep) != 1 + len(KERNELS):
        raise RuntimeError(f"expected the three reverb kernels in the statistics, got {keep[1:]}")
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
    ap.add_argument("--workers", type=int, nargs="+", default=[0, 4], help="num_workers of the loader runs")
    ap.add_argument("--skip-loader", action="store_true", help="only the kernel part")
    ap.add_argument("--trace-leg", action="store_true", help="the kernel part alone, no output (the profiled child)")
    ap.add_argument("--kernel-stats", default=None,
                    help="write the reverb kernels' rocprofv3 statistics to this CSV file")
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    a = ap.parse_args()
    if a.trace_leg:
        kernel_bench(a.repeats, a.iters, trace_only=True)
        return
    if a.kernel_stats:  # before this process opens the GPU
        kernel_stats(a.kernel_stats, a.iters)
    if not torch.cuda.is_available():
        raise SystemExit("reverb_bench: no GPU (the device parts are not measured on the host)")
    lib = os.path.join(ROOT, "liteasr_amd", "lib", "libliteasr_hip.so")
    out = {"workload": "room reverberation: int16 PCM in HBM convolved with RIRs of a resident int16 bank, shifted, "
                       "cut and normalised -> int16, in place; conformer_small bf16 Trainer steps from wav.scp with "
                       "frontend.rir on"}
    out["kernel"] = kernel_bench(a.repeats, a.iters)
    if not a.skip_loader:
        from liteasr_amd.utils.synthetic import synthetic_rir_dir, synthetic_wav_dir

        with tempfile.TemporaryDirectory() as d:
            rng = np.random.default_rng(5)
            lengths = rng.integers(S // 2, S + 1, 2 * B).tolist()
            lines = B * (a.steps + 2)  # a run stays inside one epoch
            wav = synthetic_wav_dir(os.path.join(d, "wav"), lengths, seed=3, lines=lines)
            rir = synthetic_rir_dir(os.path.join(d, "rir"), rng.integers(LMIN, LMAX + 1, NRIR).tolist(), seed=9)
            noise = synthetic_wav_dir(os.path.join(d, "noise"), rng.integers(5 * 16000, 20 * 16000, 20).tolist(), seed=7)
            out["loader"] = loader_bench(wav, rir, noise, a.steps, a.rounds, os.path.join(d, "ckpts"), a.workers)
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
