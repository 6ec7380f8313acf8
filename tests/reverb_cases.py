"""Shared inputs of the reverberation tests: the seeded signals, the bank of room impulse responses,
the rows of one batch per signal, and the float64 references (computed once per process).

The bank holds RIRs of 1 (a delta), 2, 257, BLOCK - 1, BLOCK, BLOCK + 1, 4000, 2 BLOCK + 1000 and
4000 samples and a delta at index 123 of 300, back to back: decaying Gaussian noise (T60 0.3 s) with
a direct-path peak at index 0, at L - 1 or inside.  The two Gaussian signals are one batch each of
len(LENGTHS) x len(RIR_SPECS) rows, row r the signal's first LENGTHS[r // R] samples with RIR
(r + r // R) mod R, every fourth row with none (a copy), so neighbouring rows carry different RIRs
and every RIR meets every length but those it loses to the copies.  The two saturating signals
(160-sample bursts of +-24000 in Gaussian noise: full scale broke the cap; a +-20000 square wave of period 74) meet the two 4000-tap RIRs
only, four rows per length, the fourth a copy.  One more row per batch is all zero with an RIR.

Run as a script it prints, per signal and RIR length, what the float32 restatements of
tests/reverb_ref.py (direct, and overlap-save at BLOCK; the larger counts) lose against float64 (in
LSB of the int16 output, over the samples that do not saturate either way), the share of int16
samples that differ, the share of samples whose float64 value lies within BAR_FACTOR x that loss of
a rounding (x.5) or saturation boundary (the samples the GPU test excuses from exactness) and the
share that saturates, then the largest relative deviation of the float32 restatements' gains from
the float64 gain; and it asserts that the excused share stays within EXCUSED_CAP.  The FP32_LOSS
and GAIN_DEV tables of tests/test_reverb_gpu.py are copied from this output."""

import functools

import numpy as np

import reverb_ref as R

BLOCK = 2048  # kernels.REVERB_BLOCK (tests/test_reverb_cpu.py checks that)
LENGTHS = [0, 1, 399, 400, 4000, 16000]
# (taps, peak index; None: a delta of that amplitude at the index)
RIR_SPECS = [(1, 0, 12345), (2, 1, None), (257, 100, None), (BLOCK - 1, 0, None), (BLOCK, BLOCK - 1, None),
             (BLOCK + 1, 700, None), (4000, 40, None), (2 * BLOCK + 1000, 3000, None), (4000, 0, None),
             (300, 123, 32767)]
DELTAS = (0, 9)
SIGNALS = ("gauss", "gauss_small", "bursts", "square")
SATURATING = ("bursts", "square")
BAR_FACTOR = 4.0
EXCUSED_CAP = 0.10
SMAX = max(LENGTHS)
METHODS = ("direct32", "overlap_save32")


@functools.lru_cache(maxsize=None)
def signal(name):
    """16000 int16 samples (read-only)."""
    rng = np.random.default_rng({"gauss": 11, "gauss_small": 12, "bursts": 13, "square": 14}[name])
    if name == "gauss":
        x = 2700.0 * rng.standard_normal(SMAX)
    elif name == "gauss_small":
        x = 10.0 * rng.standard_normal(SMAX)
    elif name == "bursts":
        x = 2500.0 * rng.standard_normal(SMAX)
        for start, v in ((150, 24000), (2000, -24000), (9000, 24000)):
            x[start:start + 160] = v
    else:
        x = np.where((np.arange(SMAX) // 37) % 2 == 0, 20000.0, -20000.0)
    x = np.clip(np.rint(x), -32768, 32767).astype(np.int16)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def bank():
    """(int16 samples back to back, the int64 [n, 3] table of offset, length, peak) (read-only)."""
    rng = np.random.default_rng(2024)
    recs, table, off = [], [], 0
    for L, p, delta in RIR_SPECS:
        if delta is not None:
            h = np.zeros(L)
            h[p] = delta
        else:
            t = np.arange(L) - p  # the tail decays from the direct path on: 60 dB in 0.3 s
            h = 0.1 * rng.standard_normal(L) * 10.0 ** (-3.0 * np.abs(t) / 4800.0)
            h[p] = 1.0
            h = np.clip(np.rint(h * 20000), -32768, 32767)
        h = h.astype(np.int16)
        assert R.peak(h) == p
        recs.append(h)
        table.append((off, L, p))
        off += L
    flat = np.concatenate(recs)
    flat.setflags(write=False)
    return flat, np.asarray(table, dtype=np.int64)


def rir(i):
    flat, table = bank()
    off, L, p = (int(v) for v in table[i])
    return flat[off:off + L], p


@functools.lru_cache(maxsize=None)
def rows(name):
    """[(samples, RIR index or -1, zero row?)] of the signal's batch."""
    out = []
    if name in SATURATING:  # the two 4000-tap RIRs only
        for r in range(len(LENGTHS) * 4):
            out.append((LENGTHS[r // 4], (6, 8, 6, -1)[r % 4], False))
    else:
        nr = len(RIR_SPECS)
        for r in range(len(LENGTHS) * nr):
            li = r // nr
            out.append((LENGTHS[li], -1 if r % 4 == 3 else (r + li) % nr, False))
    out.append((4000, 6, True))  # an all-zero row
    return tuple(out)


def batch(name):
    """int16 [rows, SMAX]: row r holds the signal's first samples (or zeros), then zeros."""
    x = np.zeros((len(rows(name)), SMAX), dtype=np.int16)
    for r, (n, _, zero) in enumerate(rows(name)):
        if not zero:
            x[r, :n] = signal(name)[:n]
    return x


@functools.lru_cache(maxsize=None)
def reference(name, r, method="float64"):
    """(the unrounded output, the float32 gain) of tests/reverb_ref.py for row r (read-only); a
    row without an RIR is its input, at gain 1."""
    n, i, _ = rows(name)[r]
    x = batch(name)[r, :n]
    if i < 0:
        y, g = x.astype(np.float64), np.float32(1.0)
    else:
        y, g = R.reverb(x, *rir(i), method=method, block=BLOCK)
    y.setflags(write=False)
    return y, g


@functools.lru_cache(maxsize=None)
def exact_gain(name, r):
    n, i, _ = rows(name)[r]
    return R.exact_gain(batch(name)[r, :n], *rir(i)) if i >= 0 else 1.0


def rows_of_length(name, L):
    return [r for r, (_, i, _) in enumerate(rows(name)) if i >= 0 and RIR_SPECS[i][0] == L]


def figures(name, L):
    """(largest float32 loss in LSB over the samples that do not saturate, share of int16 samples
    differing, share within BAR_FACTOR x loss of a boundary, share saturated), over the rows of the
    signal's batch whose RIR has L taps; the loss and the differing share are the larger of the two
    float32 restatements'."""
    rs = rows_of_length(name, L)
    y64 = np.concatenate([reference(name, r)[0] for r in rs])
    inside = (y64 >= -32768.5) & (y64 <= 32767.5)
    loss = differ = 0.0
    for method in METHODS:
        y32 = np.concatenate([reference(name, r, method)[0] for r in rs]).astype(np.float64)
        loss = max(loss, float(np.abs(y32 - y64)[inside].max(initial=0.0)))
        differ = max(differ, float((R.quantise(y32) != R.quantise(y64)).mean()))
    near = float((R.boundary_distance(y64) <= BAR_FACTOR * loss).mean()) if loss else 0.0
    return loss, differ, near, float((~inside).mean())


def gain_deviation(name):
    """The largest relative deviation of a float32 restatement's gain from the float64 gain (before
    its rounding to float32), over the rows of the signal's batch."""
    dev = 0.0
    for r, (_, i, _) in enumerate(rows(name)):
        g64 = exact_gain(name, r)
        if i < 0 or g64 == 0.0:
            continue
        for method in METHODS:
            dev = max(dev, abs(float(reference(name, r, method)[1]) - g64) / g64)
    return dev


def taps(name):
    """The RIR lengths of the signal's batch, ascending."""
    return sorted({RIR_SPECS[i][0] for _, i, _ in rows(name) if i >= 0})


if __name__ == "__main__":
    for s in SIGNALS:
        for L in taps(s):
            loss, differ, near, sat = figures(s, L)
            print(f"{s:12s} L={L:5d} loss {loss:.3e} LSB  differ {100 * differ:.3f} %  excused {100 * near:.3f} %  "
                  f"saturated {100 * sat:.2f} %")
            assert near <= EXCUSED_CAP, (s, L, near)
        print(f"{s:12s} gain deviation {gain_deviation(s):.3e}")
        if s in SATURATING:
            q = R.quantise(np.concatenate([reference(s, r)[0] for r in range(len(rows(s)))]))
            assert (q == 32767).any() and (q == -32768).any(), s
