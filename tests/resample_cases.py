"""Shared inputs of the resampler tests: the seeded signals (the generators of tests/fbank_cases.py),
the row lengths, the ratios and the float64 references (computed once per process).  Every
signal is one batch of len(LENGTHS) x len(RATIOS) rows, row r the first LENGTHS[r // 5] samples at
ratio RATIOS[(r + r // 5) % 5], so neighbouring rows carry different ratios.

Run as a script it prints, per signal and ratio, what the float32 restatement of
tests/resample_ref.py loses against float64 (in LSB of the int16 output), the share of int16
samples that differ, the share of samples whose float64 value lies within BAR_FACTOR x that loss of
a rounding (x.5) or saturation boundary (the samples the GPU test excuses from exactness) and the
share that saturates; and it asserts that the excused share stays within EXCUSED_CAP.  The
FP32_LOSS table of tests/test_resample_gpu.py is copied from this output."""

import functools

import numpy as np

import fbank_cases as FC
import resample_ref as R

LENGTHS = [0, 1, 9, 10, 399, 400, 4000, 16000]
RATIOS = [(9, 10), (11, 10), (1, 1), (4, 5), (5, 4)]
SIGNALS = ("noise_full", "sine_1234", "square", "noise_small")
SATURATING = ("noise_full", "square")
BAR_FACTOR = 4.0
EXCUSED_CAP = 0.10
SMAX = max(LENGTHS)


def signal(name):
    """16000 int16 samples (read-only)."""
    return FC.signal(name)


def rows():
    """[(samples, (p, q))] of the batch."""
    out = []
    for r in range(len(LENGTHS) * len(RATIOS)):
        li = r // len(RATIOS)
        out.append((LENGTHS[li], RATIOS[(r + li) % len(RATIOS)]))
    return out


def batch(name):
    """int16 [rows, SMAX]: row r holds the signal's first samples, then zeros."""
    x = np.zeros((len(rows()), SMAX), dtype=np.int16)
    for r, (n, _) in enumerate(rows()):
        x[r, :n] = signal(name)[:n]
    return x


@functools.lru_cache(maxsize=None)
def reference(name, n, ratio, dtype=np.float64):
    """The unrounded output of tests/resample_ref.py for the signal's first n samples (read-only)."""
    y = R.resample(signal(name)[:n], ratio[0], ratio[1], dtype)
    y.setflags(write=False)
    return y


def figures(name, ratio):
    """(largest float32 loss in LSB, share of int16 samples differing, share within BAR_FACTOR x
    loss of a boundary, share saturated), over all LENGTHS."""
    y64 = np.concatenate([reference(name, n, ratio) for n in LENGTHS])
    y32 = np.concatenate([reference(name, n, ratio, np.float32) for n in LENGTHS]).astype(np.float64)
    loss = float(np.abs(y32 - y64).max())
    differ = float((R.quantise(y32) != R.quantise(y64)).mean())
    near = float((R.boundary_distance(y64) <= BAR_FACTOR * loss).mean()) if loss else 0.0
    sat = float(((y64 > 32767.5) | (y64 < -32768.5)).mean())
    return loss, differ, near, sat


if __name__ == "__main__":
    for s in SIGNALS:
        for pq in RATIOS:
            loss, differ, near, sat = figures(s, pq)
            print(f"{s:12s} {pq[0]:2d}/{pq[1]:<2d} loss {loss:.3e} LSB  differ {100 * differ:.3f} %  "
                  f"excused {100 * near:.3f} %  saturated {100 * sat:.2f} %")
            assert near <= EXCUSED_CAP, (s, pq, near)
        if s in SATURATING:
            q = R.quantise(np.concatenate([reference(s, SMAX, pq) for pq in RATIOS if pq != (1, 1)]))
            assert (q == 32767).any() and (q == -32768).any(), s
