"""Kaldi ``compute-fbank-feats`` restated in numpy, the reference of the fbank tests.

Settings (the only ones the project's front end has): 16 kHz, 25 ms / 10 ms frames (400 / 160
samples), snip-edges, no dither, DC removal, pre-emphasis 0.97, povey window, 512-point FFT,
power spectrum, mel filters from 20 Hz to 8000 Hz, no energy, no VTLN, samples at int16 scale.

``dtype`` selects the arithmetic: float64 is the reference; float32 (numpy float32 and
``scipy.fft`` on float32 input) is one sample of what an fp32 pipeline can reach, and its error
against float64 sets the bars of tests/test_fbank_gpu.py.  The tables (window, mel weights) are
always computed in float64 and then cast, as the kernel's are.
"""

import numpy as np
import scipy.fft

FRAME_LEN, FRAME_SHIFT, NFFT, FS = 400, 160, 512, 16000
PREEMPH, LOW_FREQ, HIGH_FREQ = 0.97, 20.0, 8000.0
FLT_EPSILON = float(np.finfo(np.float32).eps)
LOG_EPS32 = np.float32(np.log(np.float64(FLT_EPSILON)))


def num_frames(n):
    """snip-edges frame count of n samples."""
    return 0 if n < FRAME_LEN else 1 + (n - FRAME_LEN) // FRAME_SHIFT


def povey_window():
    i = np.arange(FRAME_LEN, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * i / (FRAME_LEN - 1))) ** 0.85


def mel(f):
    return 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def mel_banks(F):
    """[F, NFFT/2 + 1] float64 triangular weights; a bin counts for a filter only when its mel
    frequency lies strictly inside (left, right)."""
    edges = np.linspace(mel(LOW_FREQ), mel(HIGH_FREQ), F + 2)
    m = mel(np.arange(NFFT // 2 + 1) * (FS / NFFT))
    W = np.zeros((F, NFFT // 2 + 1), dtype=np.float64)
    for f in range(F):
        left, center, right = edges[f], edges[f + 1], edges[f + 2]
        inside = (m > left) & (m < right)
        up = (m - left) / (center - left)
        down = (right - m) / (right - center)
        W[f] = np.where(inside, np.where(m <= center, up, down), 0.0)
    return W


def cmvn_from_stats(stats):
    """(mean, istd) float64 [F] from a Kaldi global CMVN matrix [2, F + 1]."""
    stats = np.asarray(stats, dtype=np.float64)
    F = stats.shape[1] - 1
    c = stats[0, F]
    mean = stats[0, :F] / c
    var = stats[1, :F] / c - mean * mean
    return mean, 1.0 / np.sqrt(np.maximum(var, 1e-20))


def fbank(pcm, F=80, dtype=np.float64, cmvn=None):
    """pcm: int16 [n] -> [num_frames(n), F] in ``dtype``; cmvn: (mean, istd) or None."""
    pcm = np.asarray(pcm)
    assert pcm.dtype == np.int16 and pcm.ndim == 1
    dt = np.dtype(dtype).type
    T = num_frames(pcm.shape[0])
    if T == 0:
        return np.zeros((0, F), dtype=dt)
    idx = FRAME_SHIFT * np.arange(T)[:, None] + np.arange(FRAME_LEN)[None, :]
    w = pcm.astype(dt)[idx]
    w = w - w.sum(axis=1, keepdims=True, dtype=dt) / dt(FRAME_LEN)
    pre = np.empty_like(w)
    pre[:, 1:] = w[:, 1:] - dt(PREEMPH) * w[:, :-1]
    pre[:, 0] = w[:, 0] - dt(PREEMPH) * w[:, 0]
    pre = pre * povey_window().astype(dt)
    padded = np.zeros((T, NFFT), dtype=dt)
    padded[:, :FRAME_LEN] = pre
    X = scipy.fft.rfft(padded, axis=1)
    assert X.dtype == (np.complex64 if dt is np.float32 else np.complex128)
    P = X.real * X.real + X.imag * X.imag
    e = P[:, : NFFT // 2] @ mel_banks(F)[:, : NFFT // 2].astype(dt).T
    y = np.log(np.maximum(e, dt(FLT_EPSILON)))
    assert y.dtype == dt
    if cmvn is not None:
        y = (y - np.asarray(cmvn[0], dtype=dt)) * np.asarray(cmvn[1], dtype=dt)
    return y
