"""Shared inputs of the fbank tests: the seeded signals, the batch of row lengths and the
float64 references (computed once per process).  Run as a script it prints what the float32
restatement of tests/fbank_ref.py loses against float64 on these inputs, per signal and metric:
the figures next to the bars in tests/test_fbank_gpu.py."""

import functools

import numpy as np

import fbank_ref as R

LENGTHS = [399, 400, 559, 560, 4000, 16000]  # 0, 1, 1, 2, 23 and 98 frames
SMAX = max(LENGTHS)
BROADBAND = ("noise_full", "noise_small", "square", "tone_noise")
FLOOR = ("zeros", "constant")
SIGNALS = BROADBAND + ("sine_bin64", "sine_1234") + FLOOR


@functools.lru_cache(maxsize=None)
def signal(name):
    """SMAX int16 samples."""
    rng = np.random.default_rng(2024 + SIGNALS.index(name))
    n = np.arange(SMAX, dtype=np.float64)
    if name == "noise_full":
        x = rng.integers(-32768, 32768, SMAX)
    elif name == "noise_small":
        x = rng.integers(-30, 31, SMAX)
    elif name == "square":
        x = np.where((n % 74) < 37, 32767, -32767)
    elif name == "tone_noise":
        x = 8000.0 * np.exp(-n / 4000.0) * np.sin(2 * np.pi * 180.0 * n / R.FS) + rng.normal(0.0, 20.0, SMAX)
    elif name == "sine_bin64":
        x = 20000.0 * np.sin(2 * np.pi * 64.0 * n / R.NFFT)
    elif name == "sine_1234":
        x = 12000.0 * np.sin(2 * np.pi * 1234.5 * n / R.FS)
    elif name == "zeros":
        x = np.zeros(SMAX)
    elif name == "constant":
        x = np.full(SMAX, 1000.0)
    else:
        raise KeyError(name)
    x = np.round(x).astype(np.int16)
    x.setflags(write=False)
    return x


def batch(name):
    """int16 [len(LENGTHS), SMAX]: row i holds the signal's first LENGTHS[i] samples, then zeros."""
    x = np.zeros((len(LENGTHS), SMAX), dtype=np.int16)
    for i, n in enumerate(LENGTHS):
        x[i, :n] = signal(name)[:n]
    return x


@functools.lru_cache(maxsize=None)
def reference(name, F=80, dtype=np.float64):
    """Per row of LENGTHS the [frames, F] features of tests/fbank_ref.py (read-only)."""
    out = []
    for n in LENGTHS:
        y = R.fbank(signal(name)[:n], F, dtype)
        y.setflags(write=False)
        out.append(y)
    return tuple(out)


def energy_error(y, ref):
    """Metric (a): |exp(y) - exp(ref)| / the frame's largest exp(ref), the largest over all bins."""
    if ref.shape[0] == 0:
        return 0.0
    e, r = np.exp(np.asarray(y, dtype=np.float64)), np.exp(ref)
    return float((np.abs(e - r) / r.max(axis=1, keepdims=True)).max())


def log_error(y, ref):
    """Metric (b): the largest absolute error of the log values."""
    return float(np.abs(np.asarray(y, dtype=np.float64) - ref).max()) if ref.size else 0.0


def fp32_loss(name, F=80):
    """(metric a, metric b) of the float32 restatement against float64, the largest over the rows."""
    pairs = list(zip(reference(name, F, np.float32), reference(name, F)))
    return max(energy_error(y, r) for y, r in pairs), max(log_error(y, r) for y, r in pairs)


if __name__ == "__main__":
    for s in SIGNALS:
        a, b = fp32_loss(s)
        print(f"{s:12s} (a) {a:.3e}  (b) {b:.3e}")
