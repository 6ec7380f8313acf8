"""Feature front end of task=asr on raw audio: Kaldi fbank (+ global CMVN) on the device.

The reference has no front end (its ``Audio.x`` hands bare samples to the feature models); a data
directory with ``wav.scp`` and no ``feats.scp`` is turned into log-mel features here, on the GPU,
from the int16 batch the collator delivers: ``lasr_fbank`` (csrc/fbank.hip) through
``kernels.fbank``.  The Kaldi options are fixed, ``compute-fbank-feats --snip-edges=true
--dither=0 --remove-dc-offset=true --preemphasis-coefficient=0.97 --window-type=povey
--use-power=true --use-energy=false --low-freq=20 --high-freq=0 --sample-frequency=16000
--frame-length=25 --frame-shift=10``, with samples at int16 scale; ``num_mel_bins`` and the
CMVN statistics are the configuration.

CMVN statistics are Kaldi's global matrix, ``2 x (F + 1)`` as ``compute-cmvn-stats`` writes it
(row 0: sums and the frame count, row 1: sums of squares and 0), binary or text:
``mean = s / c`` and ``istd = 1 / sqrt(max(ss / c - mean^2, 1e-20))``.

Speed perturbation (``frontend.speed_perturb``, e.g. [0.9, 1.0, 1.1]; the train split only) runs in
front of it, on the device too: the collator still delivers the source int16 batch, with a
ResamplePlan, and ``lasr_resample_i16`` (csrc/resample.hip) makes the int16 batch the fbank kernel
reads: Kaldi's LinearResample (Hann-windowed sinc, filter width 6, roll-off 0.99), rounded and
saturated to 16 bits like the WAV file an offline ``speed`` + ``rate`` pipeline writes.
"""

import numpy as np

FRAME_LEN, FRAME_SHIFT, SAMPLE_RATE = 400, 160, 16000


def num_frames(nsamples: int) -> int:
    """snip-edges frame count: 0 below 400 samples, else 1 + (n - 400) // 160."""
    return 0 if nsamples < FRAME_LEN else 1 + (nsamples - FRAME_LEN) // FRAME_SHIFT


def used_samples(frames: int) -> int:
    """Samples that ``frames`` frames read."""
    return 0 if frames <= 0 else FRAME_SHIFT * (frames - 1) + FRAME_LEN


def read_cmvn_stats(path: str) -> np.ndarray:
    """The float64 [2, F + 1] statistics matrix at ``path`` (Kaldi binary or text matrix)."""
    with open(path, "rb") as f:
        head = f.read(2)
    if head == b"\0B":
        from .kaldiio import load_mat

        stats = np.asarray(load_mat(path), dtype=np.float64)
    else:
        with open(path, "r") as f:
            body = f.read()
        if "[" not in body or "]" not in body:
            raise ValueError(f"{path}: not a Kaldi matrix")
        body = body[body.index("[") + 1:body.rindex("]")]
        rows = [[float(v) for v in line.split()] for line in body.strip().splitlines() if line.strip()]
        stats = np.asarray(rows, dtype=np.float64)
    if stats.ndim != 2 or stats.shape[0] != 2 or stats.shape[1] < 2:
        raise ValueError(f"{path}: CMVN statistics must be a 2 x (F + 1) matrix, got {stats.shape}")
    return stats


def write_cmvn_stats(path: str, stats, binary: bool = True):
    """Write the [2, F + 1] statistics as a Kaldi double matrix (binary) or a text matrix."""
    stats = np.ascontiguousarray(stats, dtype=np.float64)
    assert stats.ndim == 2 and stats.shape[0] == 2
    if binary:
        from .kaldiio import save_mat

        save_mat(path, stats)
    else:
        with open(path, "w") as f:
            f.write(" [\n" + "\n".join("  " + " ".join(repr(float(v)) for v in row) for row in stats) + " ]\n")


def cmvn_from_stats(stats):
    """(mean, istd), float64 [F]."""
    stats = np.asarray(stats, dtype=np.float64)
    F = stats.shape[1] - 1
    count = stats[0, F]
    if not count > 0:
        raise ValueError("CMVN statistics hold no frames")
    mean = stats[0, :F] / count
    var = stats[1, :F] / count - mean * mean
    return mean, 1.0 / np.sqrt(np.maximum(var, 1e-20))


def speed_ratios(speed_perturb):
    """``frontend.speed_perturb`` as the list of reduced fractions (p, q), in the listed order;
    None or an empty list is None.  A factor outside [0.5, 2] or with p, q above 32 is refused."""
    if not speed_perturb:
        return None
    from ..kernels import resample_ratio

    return [resample_ratio(s) for s in speed_perturb]


def resampled_samples(nsamples: int, p: int, q: int) -> int:
    """Samples of an utterance of ``nsamples`` at speed p / q: ceil(q n / p)."""
    return -((-q * int(nsamples)) // p)


class ResamplePlan(object):
    """What the collator of a speed-perturbed dataset adds to its batch, as the last element:
    ``rows`` int32 (B, 3) on the host, per row its source samples, its resampled samples and the
    index of its ratio in ``ratios``, the dataset's distinct (p, q); ``max_out`` the largest
    resampled count.  Trainer._features takes it off the batch again."""

    __slots__ = ("rows", "ratios", "max_out")

    def __init__(self, rows, ratios, max_out: int):
        self.rows, self.ratios, self.max_out = rows, tuple(tuple(r) for r in ratios), int(max_out)


class SpeedPerturb(object):
    """int16 (B, S) PCM on the device + a ResamplePlan -> the resampled int16 (B, max_out) batch,
    zero past every row's own samples (``lasr_resample_i16``).  The ratio and tap tables are made
    once per set of ratios and device."""

    def __init__(self):
        self._dev = {}

    def tables_on(self, ratios, device):
        import torch

        from .. import kernels as K

        key = (tuple(tuple(r) for r in ratios), torch.device(device))
        if key not in self._dev:
            self._dev[key] = tuple(torch.from_numpy(v).to(key[1]) for v in K.resample_tables(key[0]))
        return self._dev[key]

    def __call__(self, pcm, plan: ResamplePlan, out=None):
        from .. import kernels as K

        table, taps = self.tables_on(plan.ratios, pcm.device)
        return K.resample_i16(pcm, plan.rows.to(pcm.device), table, taps, out=out, max_out=plan.max_out)


class Fbank(object):
    """int16 (B, S) PCM on the device + frame counts -> fp32 (B, T, F) features, zero-padded.
    ``speed``: the speed perturbation that runs in front of it on training batches that carry a
    ResamplePlan."""

    def __init__(self, num_mel_bins: int = 80, cmvn: str = None, dither: float = 0.0):
        self.speed = SpeedPerturb()
        if dither != 0:
            raise NotImplementedError("frontend.dither: dithering (a device RNG in the front end) is not supported")
        self.num_mel_bins = int(num_mel_bins)
        if not 1 <= self.num_mel_bins <= 128:
            raise ValueError(f"frontend.num_mel_bins must be in 1..128, got {num_mel_bins}")
        self.cmvn_path = cmvn
        self.cmvn = None
        if cmvn is not None:
            mean, istd = cmvn_from_stats(read_cmvn_stats(cmvn))
            if mean.shape[0] != self.num_mel_bins:
                raise ValueError(f"{cmvn}: statistics of {mean.shape[0]} bins, frontend.num_mel_bins is "
                                 f"{self.num_mel_bins}")
            self.cmvn = (mean.astype(np.float32), istd.astype(np.float32))
        self._dev = {}

    def _cmvn_on(self, device):
        if self.cmvn is None:
            return None
        import torch

        key = torch.device(device)
        if key not in self._dev:
            self._dev[key] = tuple(torch.from_numpy(v).to(key) for v in self.cmvn)
        return self._dev[key]

    def __call__(self, pcm, xlens, max_frames=None, out=None):
        """``xlens``: frame counts on the device of ``pcm`` (any integer dtype).  ``max_frames``:
        their largest, when the caller knows it on the host (spares the read-back)."""
        import torch

        from .. import kernels as K

        nframes = xlens if xlens.dtype == torch.int32 else xlens.to(torch.int32)
        return K.fbank(pcm, nframes.contiguous(), self.num_mel_bins, self._cmvn_on(pcm.device), out=out,
                       max_frames=max_frames)

    def __repr__(self):
        return f"Fbank(num_mel_bins={self.num_mel_bins}, cmvn={self.cmvn_path!r})"
