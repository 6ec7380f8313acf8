"""Speed perturbation timing on one MI355X: ``lasr_resample_i16`` against the same transform
composed from torch ops, the device front end (resample + fbank) as a share of a training step fed
from wav.scp with ``speed_perturb`` on, and what the same resampling costs a loader on the host.

  python tools/resample_bench.py [--repeats 15] [--iters 20] [--steps 24] [--rounds 3] [--out FILE]

It writes its own seeded 16 kHz, 16-bit mono WAV files into a temporary directory, measures, and
prints one JSON line (appended to --out when given):

* ``kernel``: B = 32 rows of 160400 int16 samples already in HBM, speeds 0.9 / 1.0 / 1.1 mixed
  across the rows (row r takes factor r mod 3).  ``resample`` is one ``lasr_resample_i16`` launch,
  ``resample_graph`` the same launch replayed from a captured hipGraph, ``torch`` the composition,
  per ratio group: gather the group's rows, convert to fp32, pad, ``conv1d`` with the ratio's q
  phases as output channels (the same fp32 taps, stride p), interleave the phases, ``round``,
  ``clamp``, cast to int16 and scatter into the zero-padded output (the 1.0 group is a copy), on
  the identical input, launched eagerly.  Each sample is device time by events around --iters
  back-to-back calls, divided by --iters; the three alternate for --repeats samples; median / min
  / max.  ``resample_faster_beyond_spread``: the torch minimum minus the kernel median exceeds the
  torch spread (max - min).  The two results are compared first (at most 1 LSB apart: conv1d sums
  in another order).  ``bytes`` is what the transform must move (the rows' own input samples and
  the whole output), ``achieved_gbps`` that over the graph-replayed median, ``share_of_8tbps`` its
  share of the HBM roofline.
* ``loader``: ms per eager ``conformer_small`` bf16 step through ``Trainer.run`` (batches of 32
  utterances of 80200 .. 160400 samples, SpecAugment on) fed by AudioFileDataset over a wav.scp
  directory with speed_perturb [0.9, 1.0, 1.1] and, as context, with it off (other frame counts:
  not a bar), at num_workers 0 and 4; the four alternate for --rounds rounds of --steps steps, the
  first 4 steps of every run are dropped; median / min / max.  ``frontend_share``: device time of
  resample + fbank (events around the two calls) over the wall time of the same steps.
* ``host``: one such batch resampled on the host the way a collator would have to:
  ``scipy.signal.upfirdn`` per row with the same windowed sinc as prototype filter, rounded and
  saturated, rows spread over 1 and over 16 threads; ms per batch, median / min / max of 5.
"""

import argparse
import hashlib
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DROP = 4
B, S = 32, 160400
SPEEDS = [0.9, 1.0, 1.1]


def _stats(ts, nd=4):
    return {"median": round(statistics.median(ts), nd), "min": round(min(ts), nd), "max": round(max(ts), nd)}


def torch_resample(pcm, groups, out):
    """The transform from torch ops.  groups: (row indices, p, q, width, weight [q, 1, nt], M)."""
    for idx, p, q, width, weight, M in groups:
        x = pcm[idx]
        if p == q:
            y = x
        else:
            J = -(-M // q)
            nt = weight.shape[2]
            right = max((J - 1) * p + nt - width - x.shape[1], 0)
            xf = torch.nn.functional.pad(x.float(), (width, right)).unsqueeze(1)
            y = torch.nn.functional.conv1d(xf, weight, stride=p)[:, :, :J]  # [rows, q, J]
            y = y.transpose(1, 2).reshape(x.shape[0], J * q)[:, :M]
            y = y.round().clamp(-32768, 32767).to(torch.int16)
        out[idx, :M] = y[:, :M]
        out[idx, M:] = 0
    return out


def kernel_bench(repeats, iters):
    from liteasr_amd import kernels as K
    from liteasr_amd.utils.frontend import resampled_samples

    rng = np.random.default_rng(0)
    host = np.clip(np.round(rng.standard_normal((B, S)) * 9000), -32768, 32767).astype(np.int16)
    pcm = torch.from_numpy(host).cuda()
    ratios = [K.resample_ratio(s) for s in SPEEDS]
    table_h, taps_h = K.resample_tables(ratios)
    table, taps = torch.from_numpy(table_h).cuda(), torch.from_numpy(taps_h).cuda()
    rows = [[S, resampled_samples(S, *ratios[r % 3]), r % 3] for r in range(B)]
    plan = torch.tensor(rows, dtype=torch.int32, device="cuda")
    s_out = max(r[1] for r in rows)
    out = torch.empty(B, s_out, dtype=torch.int16, device="cuda")
    ref = torch.empty_like(out)
    groups = []
    for g, (p, q, width, off) in enumerate(table_h.tolist()):
        nt = 2 * width + p
        idx = torch.tensor([r for r in range(B) if r % 3 == g], device="cuda")
        groups.append((idx, p, q, width, taps[off:off + q * nt].reshape(q, 1, nt).contiguous(), rows[g][1]))

    def run_kernel():
        K.resample_i16(pcm, plan, table, taps, out=out)

    for _ in range(3):
        run_kernel()
        torch_resample(pcm, groups, ref)
    torch.cuda.synchronize()
    diff = int((out.int() - ref.int()).abs().max())
    differing = float((out != ref).float().mean())
    assert diff <= 1, f"kernel and torch composition disagree by {diff} LSB"
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run_kernel()
    fns = {"resample": run_kernel, "resample_graph": graph.replay, "torch": lambda: torch_resample(pcm, groups, ref)}
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
    nbytes = 2 * (B * S + B * s_out)
    res = {"B": B, "S_in": S, "S_out": s_out, "speeds": SPEEDS, "iters_per_sample": iters, "max_diff_lsb": diff,
           "share_differing": differing, "bytes": nbytes}
    res.update({k + "_ms": _stats(v) for k, v in ts.items()})
    spread = res["torch_ms"]["max"] - res["torch_ms"]["min"]
    res["resample_faster_beyond_spread"] = res["torch_ms"]["min"] - res["resample_graph_ms"]["median"] > spread
    gbps = nbytes / (res["resample_graph_ms"]["median"] * 1e-3) / 1e9
    res["achieved_gbps"], res["share_of_8tbps"] = round(gbps, 1), round(gbps / 8000.0, 4)
    return res, (host, rows, ratios, out.cpu().numpy())


class TimedFrontend(object):
    """The task's front end with device events around its two calls."""

    def __init__(self, inner):
        self.inner, self.events = inner, []
        self.num_mel_bins = inner.num_mel_bins

    def _timed(self, fn, *a, **k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        y = fn(*a, **k)
        e1.record()
        self.events.append((e0, e1))
        return y

    def speed(self, pcm, plan):
        return self._timed(self.inner.speed, pcm, plan)

    def __call__(self, *a, **k):
        return self._timed(self.inner, *a, **k)


def loader_bench(wav_dir, steps, rounds, save_dir):
    from types import SimpleNamespace

    from liteasr_amd import tasks
    from liteasr_amd.config.compose import compose
    from liteasr_amd.trainer import Trainer

    over = ["model=conformer_small", "criterion=hybrid_ctc_w03", "optimizer=noam_d256", "dataset.batch_count=seq",
            f"dataset.batch_size={B}", "dataset.min_batch_size=1", "dataset.max_len_in=100000",
            "dataset.max_len_out=1000", f"task.save_dir={save_dir}", "task=asr_wav", f"task.vocab={wav_dir}/vocab.txt",
            f"task.train={wav_dir}", f"task.valid={wav_dir}"]
    trainers = {}
    model = crit = opt = None
    for kind, speed in (("on", "[0.9,1.0,1.1]"), ("off", "null")):
        cfg = compose(overrides=over + [f"task.frontend.speed_perturb={speed}"])
        task = tasks.setup_task(cfg.task)
        task.load_dataset("train", wav_dir, cfg.dataset, cfg.postprocess, False)
        if model is None:
            torch.manual_seed(42)
            model = task.build_model(cfg.model).cuda().train()
            opt = task.build_optimizer(model.parameters(), cfg.optimizer)
            crit = task.build_criterion(cfg.criterion)
        trainers[kind] = task
    mixed = [len({a.ratio for a in trainers["on"].dataset("train")[i]}) for i in range(len(trainers["on"].dataset("train")))]
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
    out = {"steps_per_run": steps, "rounds": rounds, "dropped_per_run": DROP, "nan_skipped_steps": skipped,
           "batches": len(mixed), "batches_with_mixed_speeds": sum(m > 1 for m in mixed)}
    out.update({k + "_ms_per_step": _stats(v, 3) for k, v in ts.items()})
    out.update({k + "_frontend_share": _stats(v, 5) for k, v in share.items()})
    return out


def host_bench(host, rows, ratios, device_out, threads=(1, 16), repeats=5):
    from concurrent.futures import ThreadPoolExecutor

    from scipy.signal import upfirdn

    from liteasr_amd.kernels import RESAMPLE_ROLLOFF, RESAMPLE_WIDTH

    protos = {}
    for p, q in ratios:
        if p == q:
            continue
        c = RESAMPLE_ROLLOFF * min(1.0, q / p)
        half = p * int(np.ceil(RESAMPLE_WIDTH * q / c / p))  # a multiple of p: a whole-sample delay
        u = c * np.arange(-half, half + 1, dtype=np.float64) / q
        h = np.where(np.abs(u) < RESAMPLE_WIDTH, c * np.sinc(u) * np.cos(np.pi * u / (2.0 * RESAMPLE_WIDTH)) ** 2, 0.0)
        protos[(p, q)] = (h.astype(np.float32), half // p)

    def one(r):
        n, m, g = rows[r]
        p, q = ratios[g]
        if p == q:
            return host[r, :n].copy()
        h, delay = protos[(p, q)]
        y = upfirdn(h, host[r, :n].astype(np.float32), up=q, down=p)[delay:delay + m]
        return np.clip(np.rint(y), -32768, 32767).astype(np.int16)

    got = [one(r) for r in range(len(rows))]
    diff = max(int(np.abs(got[r].astype(np.int32) - device_out[r, :rows[r][1]].astype(np.int32)).max())
               for r in range(len(rows)))
    assert diff <= 1, f"host and device resampling disagree by {diff} LSB"
    res = {"max_diff_lsb_to_device": diff}
    for t in threads:
        ts = []
        with ThreadPoolExecutor(max_workers=t) as pool:
            for _ in range(repeats):
                t0 = time.perf_counter()
                list(pool.map(one, range(len(rows))))
                ts.append((time.perf_counter() - t0) * 1e3)
        res[f"threads_{t}_ms_per_batch"] = _stats(ts, 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-loader", action="store_true", help="only the kernel and host parts")
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resample_bench: no GPU (the device parts are not measured on the host)")
    lib = os.path.join(ROOT, "liteasr_amd", "lib", "libliteasr_hip.so")
    out = {"workload": "speed perturbation 0.9 / 1.0 / 1.1: int16 PCM in HBM -> resampled int16; conformer_small bf16 "
                       "Trainer steps from wav.scp with speed_perturb on"}
    out["kernel"], host_case = kernel_bench(a.repeats, a.iters)
    out["host"] = host_bench(*host_case)
    if not a.skip_loader:
        from liteasr_amd.utils.synthetic import synthetic_wav_dir

        with tempfile.TemporaryDirectory() as d:
            lengths = np.random.default_rng(5).integers(S // 2, S + 1, 2 * B).tolist()
            lines = B * (a.steps + 2)  # a run stays inside one epoch, with the option off too
            wav = synthetic_wav_dir(os.path.join(d, "wav"), lengths, seed=3, lines=lines)
            out["loader"] = loader_bench(wav, a.steps, a.rounds, os.path.join(d, "ckpts"))
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
