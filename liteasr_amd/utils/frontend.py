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

Additive noise (``frontend.noise``, a list of wav.scp directories of 16 kHz 16-bit mono recordings,
MUSAN-style; the train split only; the reference has none) runs between the two, in place on the
int16 batch: the recordings stay resident in HBM as one int16 bank (NoiseMixer), the collator draws
per utterance whether it is augmented, a directory, the number of sources and per source a
recording, a start and an SNR (NoisePlan), and ``lasr_mix_i16`` (csrc/mix.hip) scales every source
to its SNR against the utterance's own energy and adds it, rounded and saturated to 16 bits.

Room reverberation (``frontend.rir``, a list of wav.scp directories of 16 kHz 16-bit mono room
impulse responses of at most 65536 samples; the train split only; the reference has none) runs
between the resampler and the mixer, in place too: the RIRs stay resident in HBM as one int16 bank
with the index of every RIR's peak (Reverberator), the collator draws per utterance whether it is
reverberated, a directory and an RIR of it (ReverbPlan), and ``lasr_reverb_i16`` (csrc/reverb.hip)
convolves, shifts to the peak, keeps the utterance's duration and energy, rounds and saturates:
Kaldi's ``wav-reverberate --shift-output=true --normalize-output=true``.  With noise on too, the
SNR is taken against the reverberated utterance, whose energy is the clean one's up to rounding;
Kaldi takes the early-reverberation energy there and reverberates point-source noises with RIRs of
their own: neither is done here.
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


def _ranges(name, values, ndirs, integer):
    """``values`` (two numbers, or two per directory) as one (lo, hi) per directory."""
    vals = None if values is None or isinstance(values, (str, int, float)) else list(values)
    if (vals is None or any(isinstance(v, str) for v in vals) or len(vals) < 2 or len(vals) % 2
            or (ndirs is not None and len(vals) not in (2, 2 * ndirs))):
        raise ValueError(f"frontend.{name} must hold two values, or two per noise directory, got {values!r}")
    pairs = [(vals[i], vals[i + 1]) for i in range(0, len(vals), 2)]
    for lo, hi in pairs:
        if integer and (int(lo) != lo or int(hi) != hi or not 1 <= lo <= 8 or not 1 <= hi <= 8):
            raise ValueError(f"frontend.{name}: source counts must be integers in 1..8, got {values!r}")
        if not lo <= hi:  # a NaN fails too
            raise ValueError(f"frontend.{name}: the lower bound {lo} is above the upper bound {hi}")
    pairs = [(int(lo), int(hi)) if integer else (float(lo), float(hi)) for lo, hi in pairs]
    return pairs * ndirs if ndirs is not None and len(pairs) == 1 else pairs


class NoiseIndex(object):
    """Where every recording of the noise directories lies in the bank: ``paths``, ``offsets`` and
    ``lengths`` (samples, int64) in the order of the directories and of their wav.scp lines,
    ``dir_of`` the directory of each and ``by_dir`` the recordings of each directory.  No sample is
    read for it: the lengths come from the WAV headers.  ``key`` names the option in the messages
    (``frontend.noise`` or ``frontend.rir``); ``max_frames``: the longest recording taken."""

    __slots__ = ("paths", "offsets", "lengths", "dir_of", "by_dir", "total")

    def __init__(self, dirs, max_mb, key="noise", max_frames=None):
        import os

        from ..dataclass.sheet import AudioSheet
        from . import wavio

        self.paths, lengths, dir_of, self.by_dir = [], [], [], []
        for d, data_dir in enumerate(dirs):
            scp = os.path.join(data_dir, "wav.scp")
            if not os.path.isfile(scp):
                raise FileNotFoundError(f"frontend.{key}: wav.scp not found in {data_dir}")
            first = len(self.paths)
            with open(scp, "r") as f:
                for _, path in AudioSheet._wav_entries(ln for ln in f if ln.strip()):
                    info = wavio.probe(path)
                    if (info.rate, info.bits, info.channels) != (SAMPLE_RATE, 16, 1) or info.frames < 1:
                        raise ValueError(f"frontend.{key}: {path} is {info.rate} Hz, {info.bits} bits, {info.channels} "
                                         f"channel(s), {info.frames} samples; 16 kHz 16-bit mono recordings are needed")
                    if max_frames is not None and info.frames > max_frames:
                        raise ValueError(f"frontend.{key}: {path} holds {info.frames} samples, at most {max_frames} "
                                         "are taken (nothing is truncated silently)")
                    self.paths.append(path)
                    lengths.append(info.frames)
                    dir_of.append(d)
            if len(self.paths) == first:
                raise ValueError(f"frontend.{key}: {data_dir} lists no recording")
            self.by_dir.append(np.arange(first, len(self.paths), dtype=np.int64))
        self.lengths = np.asarray(lengths, dtype=np.int64)
        self.offsets = np.concatenate([[0], np.cumsum(self.lengths)[:-1]]).astype(np.int64)
        self.dir_of = np.asarray(dir_of, dtype=np.int32)
        self.total = int(self.lengths.sum())
        if 2 * self.total > int(max_mb) * (1 << 20):
            raise ValueError(f"frontend.{key}: the {len(self.paths)} recordings hold {self.total} samples, "
                             f"{2 * self.total / (1 << 20):.1f} MB, above frontend.{key}_max_mb = {max_mb}; raise the "
                             "cap or list fewer recordings (nothing is left out silently)")


class NoiseSpec(object):
    """``frontend.noise*`` checked: the directories, the probability that an utterance is augmented,
    per directory its SNR range in dB and its range of source counts, the seed and the cap on the
    resident bank.  ``index()`` is the NoiseIndex over the directories, made on first use and kept
    (the train dataset and the NoiseMixer share it)."""

    def __init__(self, dirs, prob=0.5, snr=(0.0, 15.0), sources=(1, 1), seed=0, max_mb=2048):
        self.dirs = [dirs] if isinstance(dirs, str) else [str(d) for d in dirs]
        if not self.dirs:
            raise ValueError("frontend.noise lists no directory")
        self.prob, self.seed, self.max_mb = check_noise_options(prob, snr, sources, seed, max_mb, len(self.dirs))
        self.snr, self.sources = _ranges("noise_snr", snr, len(self.dirs), False), _ranges(
            "noise_sources", sources, len(self.dirs), True)
        self._index = None

    def index(self) -> NoiseIndex:
        if self._index is None:
            self._index = NoiseIndex(self.dirs, self.max_mb)
        return self._index


def check_noise_options(prob, snr, sources, seed, max_mb, ndirs=None):
    """Refuses a probability outside [0, 1], lo > hi, source counts outside 1..8, a wrong list
    length, a negative seed or cap; returns (prob, seed, max_mb)."""
    prob = float(prob)
    if not 0.0 <= prob <= 1.0:
        raise ValueError(f"frontend.noise_prob must lie in [0, 1], got {prob}")
    _ranges("noise_snr", snr, ndirs, False)
    _ranges("noise_sources", sources, ndirs, True)
    if int(seed) != seed or int(seed) < 0:
        raise ValueError(f"frontend.noise_seed must be an integer >= 0, got {seed!r}")
    if int(max_mb) != max_mb or int(max_mb) < 0:
        raise ValueError(f"frontend.noise_max_mb must be an integer >= 0, got {max_mb!r}")
    return prob, int(seed), int(max_mb)


class NoisePlan(object):
    """What the collator of a noise-augmented dataset adds to its batch, as the last element (after
    a ResamplePlan if there is one): the host tables of ``kernels.mix_plan``, ``rows`` int32 (B, 3)
    (samples, first source and source count of every row; the samples are those after speed
    perturbation) and ``sources`` int64 (n, 4) (offset, length and start in the bank, the bits of
    r = 10^(-snr / 10)), and ``snr`` the drawn dB values per row.  Trainer._features takes it off
    the batch again."""

    __slots__ = ("rows", "sources", "snr")

    def __init__(self, rows, sources, snr):
        self.rows, self.sources, self.snr = rows, sources, snr


def draw_noise_plan(rng, spec: NoiseSpec, index: NoiseIndex, ns) -> NoisePlan:
    """One NoisePlan for rows of ``ns`` samples from the numpy Generator ``rng``.  Per row, in this
    order: a uniform number (augmented when below ``noise_prob``; nothing else is drawn
    otherwise), a directory, the source count in the directory's range, then per source a
    recording of the directory, a start in [0, length) and an SNR in the directory's range."""
    import torch

    from ..kernels import mix_plan

    srcs, snrs = [], []
    for _ in ns:
        row, row_snr = [], []
        if rng.random() < spec.prob:
            d = int(rng.integers(len(spec.dirs)))
            lo, hi = spec.sources[d]
            for _ in range(int(rng.integers(lo, hi + 1))):
                rec = int(index.by_dir[d][int(rng.integers(len(index.by_dir[d])))])
                start = int(rng.integers(int(index.lengths[rec])))
                snr = float(rng.uniform(*spec.snr[d]))
                row.append((int(index.offsets[rec]), int(index.lengths[rec]), start, 10.0 ** (-snr / 10.0)))
                row_snr.append(snr)
        srcs.append(row)
        snrs.append(row_snr)
    rows, table = mix_plan([int(n) for n in ns], srcs)
    return NoisePlan(torch.from_numpy(rows), torch.from_numpy(table), snrs)


class NoiseMixer(object):
    """Additive noise of the train split (``task.frontend.noise``): owns the resident bank, every
    recording of the noise directories back to back as int16 on the device.  On first use it reads
    them with the native WAV reader into one pinned buffer and uploads that with one copy; a call
    mixes the rows of an int16 (B, S) batch with the sources of a NoisePlan (``lasr_mix_i16``)."""

    def __init__(self, spec: NoiseSpec):
        self.spec = spec
        self._dev = {}

    @property
    def index(self) -> NoiseIndex:
        return self.spec.index()

    def read_bank(self, pin: bool = False):
        """The bank on the host, an int16 vector of ``index.total`` samples."""
        import torch

        from . import wavio

        idx = self.index
        bank = torch.empty(idx.total, dtype=torch.int16, pin_memory=pin)
        arr = bank.numpy()
        for path, off, n in zip(idx.paths, idx.offsets.tolist(), idx.lengths.tolist()):
            got = wavio.read_into(path, arr[off:off + n])
            if got != n:
                raise IOError(f"{path}: {got} samples on disk, its header says {n}")
        return bank

    def bank_on(self, device):
        import torch

        key = torch.device(device)
        if key.index is None:
            key = torch.device(key.type, torch.cuda.current_device())
        if key not in self._dev:
            self._dev[key] = self.read_bank(pin=True).to(key, non_blocking=True)
            torch.cuda.current_stream(key).synchronize()  # the pinned buffer goes away here
        return self._dev[key]

    def __call__(self, pcm, plan: NoisePlan, out=None, gains=None):
        from .. import kernels as K

        return K.mix_i16(pcm, self.bank_on(pcm.device), plan.rows.to(pcm.device), plan.sources.to(pcm.device),
                         out=out, gains=gains)

    def __repr__(self):
        s = self.spec
        return f"NoiseMixer(dirs={s.dirs!r}, prob={s.prob}, snr={s.snr}, sources={s.sources})"


RIR_MAX_SAMPLES = 65536


def check_rir_options(prob, seed, max_mb):
    """Refuses a probability outside [0, 1], a negative seed or cap; returns (prob, seed, max_mb)."""
    if isinstance(prob, str) or not 0.0 <= float(prob) <= 1.0:  # a NaN fails too
        raise ValueError(f"frontend.rir_prob must lie in [0, 1], got {prob!r}")
    if isinstance(seed, str) or int(seed) != seed or int(seed) < 0:
        raise ValueError(f"frontend.rir_seed must be an integer >= 0, got {seed!r}")
    if isinstance(max_mb, str) or int(max_mb) != max_mb or int(max_mb) < 0:
        raise ValueError(f"frontend.rir_max_mb must be an integer >= 0, got {max_mb!r}")
    return float(prob), int(seed), int(max_mb)


class RirSpec(object):
    """``frontend.rir*`` checked: the directories, the probability that an utterance is
    reverberated, the seed and the cap on the resident bank.  ``index()`` is the NoiseIndex over
    the directories (16 kHz 16-bit mono, at most 65536 samples each), made on first use and kept
    (the train dataset and the Reverberator share it)."""

    def __init__(self, dirs, prob=0.5, seed=0, max_mb=512):
        self.dirs = [dirs] if isinstance(dirs, str) else [str(d) for d in dirs]
        if not self.dirs:
            raise ValueError("frontend.rir lists no directory")
        self.prob, self.seed, self.max_mb = check_rir_options(prob, seed, max_mb)
        self._index = None

    def index(self) -> NoiseIndex:
        if self._index is None:
            self._index = NoiseIndex(self.dirs, self.max_mb, key="rir", max_frames=RIR_MAX_SAMPLES)
        return self._index


class ReverbPlan(object):
    """What the collator of a reverberated dataset adds to its batch (after a ResamplePlan, before
    a NoisePlan): ``rows`` int32 (B, 2) on the host, the table of ``kernels.reverb_plan``: per row
    its samples (those after speed perturbation) and the index of its RIR in the bank's table, -1
    for a row that stays as it is.  Trainer._features takes it off the batch again."""

    __slots__ = ("rows",)

    def __init__(self, rows):
        self.rows = rows


def draw_reverb_plan(rng, spec: RirSpec, index: NoiseIndex, ns) -> ReverbPlan:
    """One ReverbPlan for rows of ``ns`` samples from the numpy Generator ``rng``.  Per row, in this
    order: a uniform number (reverberated when below ``rir_prob``; nothing else is drawn
    otherwise), a directory, an RIR of the directory."""
    import torch

    from ..kernels import reverb_plan

    ids = []
    for _ in ns:
        rir = -1
        if rng.random() < spec.prob:
            d = int(rng.integers(len(spec.dirs)))
            rir = int(index.by_dir[d][int(rng.integers(len(index.by_dir[d])))])
        ids.append(rir)
    return ReverbPlan(torch.from_numpy(reverb_plan([int(n) for n in ns], ids)))


class Reverberator(object):
    """Room reverberation of the train split (``task.frontend.rir``): owns the resident bank, every
    RIR of the directories back to back as int16 on the device, and the int64 table (offset, length,
    peak) of the RIRs.  On first use it reads them with the native WAV reader into one pinned buffer,
    finds every peak (the first index of the largest sample; an all-zero recording is refused) and
    uploads the bank with one copy; a call reverberates the rows of an int16 (B, S) batch as a
    ReverbPlan says (``lasr_reverb_i16``)."""

    def __init__(self, spec: RirSpec):
        self.spec = spec
        self._dev = {}

    @property
    def index(self) -> NoiseIndex:
        return self.spec.index()

    def read_bank(self, pin: bool = False):
        """(bank, rirs) on the host: the int16 vector of ``index.total`` samples and the int64
        (n_rir, 3) table of offset, length and peak."""
        import torch

        from . import wavio

        idx = self.index
        bank = torch.empty(idx.total, dtype=torch.int16, pin_memory=pin)
        arr = bank.numpy()
        table = np.zeros((len(idx.paths), 3), dtype=np.int64)
        for i, (path, off, n) in enumerate(zip(idx.paths, idx.offsets.tolist(), idx.lengths.tolist())):
            got = wavio.read_into(path, arr[off:off + n])
            if got != n:
                raise IOError(f"{path}: {got} samples on disk, its header says {n}")
            h = arr[off:off + n]
            peak = int(np.argmax(h))  # the first index of the largest sample
            if h[peak] == 0 and not h.any():
                raise ValueError(f"frontend.rir: {path} holds {n} samples, all zero: no impulse response")
            table[i] = (off, n, peak)
        return bank, torch.from_numpy(table)

    def tables_on(self, device):
        import torch

        key = torch.device(device)
        if key.index is None:
            key = torch.device(key.type, torch.cuda.current_device())
        if key not in self._dev:
            bank, table = self.read_bank(pin=True)
            self._dev[key] = (bank.to(key, non_blocking=True), table.to(key))
            torch.cuda.current_stream(key).synchronize()  # the pinned buffer goes away here
        return self._dev[key]

    def __call__(self, pcm, plan: ReverbPlan, out=None, gains=None):
        from .. import kernels as K

        bank, table = self.tables_on(pcm.device)
        return K.reverb_i16(pcm, bank, plan.rows.to(pcm.device), table, out=out, gains=gains,
                            max_taps=int(self.index.lengths.max()))

    def __repr__(self):
        return f"Reverberator(dirs={self.spec.dirs!r}, prob={self.spec.prob})"


class Fbank(object):
    """int16 (B, S) PCM on the device + frame counts -> fp32 (B, T, F) features, zero-padded.
    ``speed``: the speed perturbation that runs in front of it on training batches that carry a
    ResamplePlan.  ``noise``: the NoiseMixer of ``frontend.noise`` (None: off), which runs between
    the two on batches that carry a NoisePlan.  ``reverb``: the Reverberator of ``frontend.rir``
    (None: off), which runs between the resampler and the mixer on batches that carry a
    ReverbPlan."""

    def __init__(self, num_mel_bins: int = 80, cmvn: str = None, dither: float = 0.0, noise: "NoiseSpec" = None,
                 rir: "RirSpec" = None):
        self.speed = SpeedPerturb()
        self.noise = NoiseMixer(noise) if noise is not None else None
        self.reverb = Reverberator(rir) if rir is not None else None
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
