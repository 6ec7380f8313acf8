"""Global CMVN statistics of a raw-audio data directory, through the device front end.

  python tools/compute_cmvn.py DATA_DIR OUT [--num-mel-bins 80] [--batch 32] [--text]
                               [--speed-perturb 0.9,1.0,1.1]

DATA_DIR holds wav.scp (with or without segments; 16 kHz, 16-bit mono WAV).  Every utterance goes
through the front end of task=asr_wav (``lasr_fbank``, no CMVN); the per-bin sums and sums of
squares are accumulated in float64 on the device and written to OUT as the 2 x (F + 1) matrix
Kaldi's ``compute-cmvn-stats`` writes for one global speaker (row 0: sums, then the frame count;
row 1: sums of squares, then 0), binary unless --text.  Use it as ``task.frontend.cmvn=OUT``.
With --speed-perturb the statistics are taken over what training with
``task.frontend.speed_perturb`` of the same factors sees: one copy of every utterance per factor,
resampled on the device (``lasr_resample_i16``) in front of the fbank kernel.
"""

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def accumulate_perturbed(records, speeds, num_mel_bins=80, batch=32, device="cuda"):
    """records: (wav file, first sample, samples) triples, ``speeds`` the speed factors -> float64
    [2, F + 1] statistics over one resampled copy of every utterance per factor."""
    from liteasr_amd.utils import wavio
    from liteasr_amd.utils.frontend import Fbank, ResamplePlan, num_frames, resampled_samples, speed_ratios

    fe = Fbank(num_mel_bins)
    F = fe.num_mel_bins
    sums = torch.zeros(2, F, dtype=torch.float64, device=device)
    count = 0
    ratios = list(dict.fromkeys(speed_ratios(speeds)))
    copies = [(fd, start, n, r, resampled_samples(n, *pq)) for r, pq in enumerate(ratios) for fd, start, n in records]
    copies = sorted((c for c in copies if num_frames(c[4]) > 0), key=lambda c: -c[4])
    for at in range(0, len(copies), batch):
        part = copies[at:at + batch]
        frames = [num_frames(c[4]) for c in part]
        smax = max(c[2] for c in part)
        xs = torch.zeros(len(part), smax, dtype=torch.int16)
        _, got = wavio.read_batch([c[0] for c in part], [c[1] for c in part], smax, out=xs.numpy())
        for i, (fd, start, n, _, _) in enumerate(part):
            if got[i] < n:
                raise ValueError(f"{fd}: {int(got[i])} samples from {start} on disk, {n} needed")
            xs[i, n:] = 0
        plan = ResamplePlan(torch.tensor([[c[2], c[4], c[3]] for c in part], dtype=torch.int32), ratios, part[0][4])
        pcm = fe.speed(xs.to(device), plan)
        xlens = torch.tensor(frames, dtype=torch.int32)
        feats = fe(pcm, xlens.to(device), max_frames=frames[0]).double()  # padding rows are zero
        sums[0] += feats.sum(dim=(0, 1))
        sums[1] += (feats * feats).sum(dim=(0, 1))
        count += sum(frames)
    stats = np.zeros((2, F + 1), dtype=np.float64)
    stats[:, :F] = sums.cpu().numpy()
    stats[0, F] = count
    return stats


def accumulate(records, num_mel_bins=80, batch=32, device="cuda"):
    """records: (wav file, first sample, samples) triples -> float64 [2, F + 1] statistics."""
    from liteasr_amd.utils import wavio
    from liteasr_amd.utils.frontend import Fbank, num_frames, used_samples

    fe = Fbank(num_mel_bins)
    F = fe.num_mel_bins
    sums = torch.zeros(2, F, dtype=torch.float64, device=device)
    count = 0
    records = sorted((r for r in records if num_frames(r[2]) > 0), key=lambda r: -r[2])
    for at in range(0, len(records), batch):
        part = records[at:at + batch]
        frames = [num_frames(n) for _, _, n in part]
        smax = used_samples(frames[0])
        xs = torch.zeros(len(part), smax, dtype=torch.int16)
        _, got = wavio.read_batch([r[0] for r in part], [r[1] for r in part], smax, out=xs.numpy())
        for i, (fd, start, n) in enumerate(part):
            if got[i] < used_samples(frames[i]):
                raise ValueError(f"{fd}: {int(got[i])} samples from {start} on disk, {used_samples(frames[i])} needed")
            xs[i, used_samples(frames[i]):] = 0
        xlens = torch.tensor(frames, dtype=torch.int32)
        feats = fe(xs.to(device), xlens.to(device), max_frames=frames[0]).double()  # padding rows are zero
        sums[0] += feats.sum(dim=(0, 1))
        sums[1] += (feats * feats).sum(dim=(0, 1))
        count += sum(frames)
    stats = np.zeros((2, F + 1), dtype=np.float64)
    stats[:, :F] = sums.cpu().numpy()
    stats[0, F] = count
    return stats


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("data_dir")
    ap.add_argument("out")
    ap.add_argument("--num-mel-bins", type=int, default=80)
    ap.add_argument("--batch", type=int, default=32, help="utterances per device call")
    ap.add_argument("--text", action="store_true", help="write a Kaldi text matrix")
    ap.add_argument("--speed-perturb", default=None, metavar="S1,S2,...",
                    help="speed factors, e.g. 0.9,1.0,1.1: statistics over one resampled copy per factor")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("compute_cmvn: no GPU (the front end runs on the device only)")
    from liteasr_amd.dataclass.sheet import AudioSheet
    from liteasr_amd.utils.frontend import write_cmvn_stats

    sheet = AudioSheet(a.data_dir)
    if not sheet.scp.endswith("wav.scp"):
        raise SystemExit(f"compute_cmvn: {a.data_dir} has feats.scp; this tool is for raw-audio directories")
    records = [(fd, start, n) for _, fd, start, n in sheet]
    if a.speed_perturb:
        stats = accumulate_perturbed(records, [s for s in a.speed_perturb.split(",") if s.strip()], a.num_mel_bins,
                                     a.batch)
    else:
        stats = accumulate(records, a.num_mel_bins, a.batch)
    if stats[0, -1] == 0:
        raise SystemExit(f"compute_cmvn: no utterance of {a.data_dir} holds a frame")
    write_cmvn_stats(a.out, stats, binary=not a.text)
    print(f"{a.out}: {int(stats[0, -1])} frames, {a.num_mel_bins} bins")


if __name__ == "__main__":
    main()
