"""Restatement of the reverberation transform (csrc/reverb.hip) straight from its definition.  A row
of n int16 samples x, a room impulse response h of L int16 samples whose peak index is p (the first
index of its largest sample):

    c[m] = sum_{k<L} (h[k] 2^-15) x[m + p - k],  0 <= m < n,  x = 0 outside [0, n)
    Ex = sum x^2 (an exact integer),  Ec = sum_{m<n} c[m]^2
    g = float32(sqrt(Ex / Ec)) in float64;  0 when Ex = 0 or Ec = 0
    y[m] = g c[m]                                            (the product in float64)

``convolve`` with float64 is the reference: ``np.convolve``, then the shift and the cut.  Two float32
restatements show what that precision loses: the direct convolution in float32, and uniformly
partitioned overlap-save with ``scipy.fft`` in float32 at a block size.  ``quantise`` is the int16
the kernel stores: nearest-even, saturated."""

import numpy as np


def peak(h):
    """The first index of the largest sample of h."""
    return int(np.argmax(np.asarray(h)))


def energy(x):
    """sum x^2 as a Python integer."""
    return int((np.asarray(x).astype(np.int64) ** 2).sum())


def convolve(x, h, p, dtype=np.float64):
    """c[0 .. n) by direct convolution in ``dtype``."""
    x, h = np.asarray(x), np.asarray(h)
    n = x.shape[0]
    if n == 0:
        return np.zeros(0, dtype=dtype)
    full = np.convolve(x.astype(dtype), h.astype(dtype) * dtype(2.0 ** -15))
    return full[p:p + n].astype(dtype)


def convolve_overlap_save32(x, h, p, block):
    """c[0 .. n) in float32 by uniformly partitioned overlap-save: 2 ``block``-point real transforms
    of scipy.fft (float32 natively), the partitions accumulated in complex64."""
    import scipy.fft

    x, h = np.asarray(x), np.asarray(h)
    n, L, P = x.shape[0], h.shape[0], int(block)
    parts, blocks = -(-L // P), -(-n // P)
    hp = np.zeros(parts * P, dtype=np.float32)
    hp[:L] = h.astype(np.float32) * np.float32(2.0 ** -15)
    H = [scipy.fft.rfft(np.concatenate([hp[c * P:(c + 1) * P], np.zeros(P, dtype=np.float32)])) for c in range(parts)]
    lead = parts * P  # x[m] sits at xp[lead + m]: every window index below is inside xp
    xp = np.zeros(lead + (blocks + 1) * P + L, dtype=np.float32)
    xp[lead:lead + n] = x.astype(np.float32)
    X = {}
    out = np.zeros(blocks * P, dtype=np.float32)
    for a in range(blocks):
        acc = np.zeros(P + 1, dtype=np.complex64)
        for c in range(parts):
            j = a - c
            if j not in X:
                lo = lead + j * P + p - P
                X[j] = scipy.fft.rfft(xp[lo:lo + 2 * P])
            acc = acc + X[j] * H[c]
        y = scipy.fft.irfft(acc, 2 * P)
        assert y.dtype == np.float32 and acc.dtype == np.complex64
        out[a * P:(a + 1) * P] = y[P:]
    return out[:n]


def gain64(ex, c):
    """sqrt(Ex / Ec) in float64, Ec summed in float64 over the values c; 0.0 when either is 0."""
    ec = float((np.asarray(c).astype(np.float64) ** 2).sum())
    if ex == 0 or ec == 0.0:
        return 0.0
    return float(np.sqrt(np.float64(ex) / np.float64(ec)))


def reverb(x, h, p, method="float64", block=None):
    """(the unrounded output [n], the gain as float32).  ``method``: "float64" (the reference),
    "direct32" or "overlap_save32" (the convolution and the final product in float32)."""
    if method == "float64":
        c = convolve(x, h, p, np.float64)
    elif method == "direct32":
        c = convolve(x, h, p, np.float32)
    elif method == "overlap_save32":
        c = convolve_overlap_save32(x, h, p, block)
    else:
        raise ValueError(method)
    g = np.float32(gain64(energy(x), c))
    if method == "float64":
        return np.float64(g) * c, g
    return (g * c.astype(np.float32)).astype(np.float32), g


def exact_gain(x, h, p):
    """sqrt(Ex / Ec) of the float64 convolution, before its rounding to float32."""
    return gain64(energy(x), convolve(x, h, p, np.float64))


def quantise(y):
    """int16: round to nearest-even, saturate to [-32768, 32767]."""
    return np.clip(np.rint(np.asarray(y, dtype=np.float64)), -32768, 32767).astype(np.int16)


def boundary_distance(y):
    """Distance of each float64 value from the nearest point where ``quantise`` changes: a
    half-integer inside the int16 range, the saturation point outside it."""
    y = np.asarray(y, dtype=np.float64)
    inside = np.abs((y - np.floor(y)) - 0.5)
    return np.where(y > 32767.5, y - 32767.5, np.where(y < -32768.5, -32768.5 - y, inside))
