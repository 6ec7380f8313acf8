"""Restatement of the speed perturbation transform (csrc/resample.hip) straight from its formula,
independent of the library's tap tables: the Hann-windowed sinc of Kaldi's LinearResample with
filter width L = 6 and roll-off 0.99.  A speed factor p / q (reduced) turns N samples into
M = ceil(q N / p):

    y[m] = sum_n x[n] c sinc(u) cos^2(pi u / 2L),   u = c (n - m p / q),   over |u| < L,
    c = 0.99 min(1, q / p),   sinc(u) = sin(pi u) / (pi u),   x[n] = 0 outside [0, N)

evaluated over each output's support only (a dense M x N matrix at 16000 samples is gigabytes).
n - m p / q is formed as (n q - m p) / q, the numerator an exact integer.  ``dtype`` float64 is
the reference; float32 runs the same expressions in float32 and shows what that precision loses.
p = q is a copy.  ``quantise`` is the 16-bit WAV file in between: nearest-even, saturated."""

from fractions import Fraction

import numpy as np

L, ROLLOFF = 6, 0.99


def ratio(speed):
    """(p, q) of a speed factor, the reduced Fraction(str(speed))."""
    f = Fraction(str(speed))
    return f.numerator, f.denominator


def num_samples(n, p, q):
    return (q * n + p - 1) // p


def resample(x, p, q, dtype=np.float64):
    """The unrounded output, ``dtype`` [M], of int16 (or any real) samples ``x`` at speed p / q."""
    x = np.asarray(x)
    N = x.shape[0]
    M = num_samples(N, p, q)
    if p == q:
        return x.astype(dtype)
    if M == 0:
        return np.zeros(0, dtype=dtype)
    T = np.dtype(dtype).type
    c = T(ROLLOFF) * T(min(1.0, q / p))
    reach = int(np.ceil(L / float(c))) + 1  # |n - m p / q| < L / c lies inside
    m = np.arange(M, dtype=np.int64)[:, None]
    n = (m * p) // q + np.arange(-reach, reach + 2, dtype=np.int64)[None, :]
    u = c * ((n * q - m * p).astype(dtype) / T(q))
    live = (np.abs(u) < L) & (n >= 0) & (n < N)
    pu = T(np.pi) * u
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(u == 0, T(1), np.sin(pu) / pu)
    w = c * sinc * np.cos(pu / T(2 * L)) ** 2
    xs = np.where(live, x[np.clip(n, 0, max(N - 1, 0))].astype(dtype), T(0))
    return (np.where(live, w, T(0)) * xs).sum(axis=1, dtype=dtype)


def quantise(y):
    """int16: round to nearest-even, saturate to [-32768, 32767]."""
    return np.clip(np.rint(np.asarray(y, dtype=np.float64)), -32768, 32767).astype(np.int16)


def boundary_distance(y):
    """Distance of each float64 value from the nearest point where ``quantise`` changes: a
    half-integer inside the int16 range, the saturation point outside it."""
    y = np.asarray(y, dtype=np.float64)
    inside = np.abs((y - np.floor(y)) - 0.5)
    return np.where(y > 32767.5, y - 32767.5, np.where(y < -32768.5, -32768.5 - y, inside))
