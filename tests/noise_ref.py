"""Restatement of the additive-noise transform (csrc/mix.hip) straight from its definition.  A
row of n int16 samples x and k sources, source j the recording w_j of L_j samples read from phase
s_j and wrapped, v_j[m] = w_j[(s_j + m) mod L_j], at r_j = 10^(-snr_j / 10):

    Ex = sum x[m]^2,   Ev_j = sum_{m<n} v_j[m]^2            (exact integers)
    g_j = float32(sqrt(Ex / Ev_j * r_j))  in float64;  0 when Ex = 0 or Ev_j = 0
    y[m] = x[m] + sum_j g_j v_j[m]                          (products and sums in float64)

``dtype`` float64 is the reference; float32 runs the sum in float32, a rounded product and a rounded
sum per source, and shows what that precision loses.  ``quantise`` is the int16 the kernel stores:
nearest-even, saturated."""

import numpy as np


def ratio_of(snr_db):
    """r = 10^(-snr / 10), float64, as the plan carries it."""
    return 10.0 ** (-float(snr_db) / 10.0)


def source(bank, offset, length, start, n):
    """v[m] = w[(start + m) mod length], m < n, of the recording at bank[offset : offset + length]."""
    return np.asarray(bank)[offset + (start + np.arange(n, dtype=np.int64)) % length]


def energy(v):
    """sum v^2 as a Python integer."""
    return int((np.asarray(v).astype(np.int64) ** 2).sum())


def gain64(ex, ev, r):
    """sqrt(Ex / Ev * r) in float64; 0.0 when either energy is 0."""
    if ex == 0 or ev == 0:
        return 0.0
    return float(np.sqrt(np.float64(ex) / np.float64(ev) * np.float64(r)))


def gains(x, vs, rs):
    """float32 [k]: the gains of the sources ``vs`` (their first len(x) samples) at ``rs``."""
    ex = energy(x)
    return np.asarray([gain64(ex, energy(v), r) for v, r in zip(vs, rs)], dtype=np.float64).astype(np.float32)


def mix(x, vs, rs, dtype=np.float64):
    """The unrounded output, ``dtype`` [n]."""
    acc = np.asarray(x).astype(dtype)
    for g, v in zip(gains(x, vs, rs), vs):
        acc = acc + dtype(g) * np.asarray(v).astype(dtype)
    return acc


def measured_snr_db(x, noise):
    """10 log10(sum x^2 / sum noise^2) of float64 arrays."""
    x, noise = np.asarray(x, dtype=np.float64), np.asarray(noise, dtype=np.float64)
    return 10.0 * np.log10(np.sum(x ** 2) / np.sum(noise ** 2))


def quantise(y):
    """int16: round to nearest-even, saturate to [-32768, 32767]."""
    return np.clip(np.rint(np.asarray(y, dtype=np.float64)), -32768, 32767).astype(np.int16)


def boundary_distance(y):
    """Distance of each float64 value from the nearest point where ``quantise`` changes: a
    half-integer inside the int16 range, the saturation point outside it."""
    y = np.asarray(y, dtype=np.float64)
    inside = np.abs((y - np.floor(y)) - 0.5)
    return np.where(y > 32767.5, y - 32767.5, np.where(y < -32768.5, -32768.5 - y, inside))
