"""Inputs of the CTC alignment tests, shared by the CPU and the GPU file.

Recipe: logits = 3 N(0, 1) as fp32 over V = 50 entries from numpy.random.default_rng(seed);
targets uniform in 1..V-1 with y[1] = y[0] when L >= 3 (an adjacent repeat); lp = log-softmax in
float64 rounded to fp32, gathered to the kernel's [T, L+1] layout (column 0 blank, 1+i target i).

Run as a script it prints, per shape, how often the float32 and float64 restatements take the
same path and the largest |s32 - s64|."""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_align_ref as R  # noqa: E402

V = 50

# The move words of a T x (2L+1) launch stay in LDS while 4 (2L+1) (2 + ceil(T/16)) <= 65536
# (liteasr_amd.kernels.ctc_align_workspace).  At L = 255 (511 states) that is ceil(T/16) <= 30:
# T = 480 is the last LDS shape, T = 481 the first spilled one.
LDS_EDGE_IN = (480, 255)
LDS_EDGE_OUT = (481, 255)

SHAPES = [
    (8, 3),      # small
    (5, 5),      # infeasible because of the repeat
    (12, 4),     # small
    (5, 4),      # exactly feasible: T = L + repeats
    (62, 20),    # medium
    (250, 100),  # long
    (64, 0),     # empty target
    (1, 1),      # single frame, single label
    (1, 0),      # single frame, empty target
    (600, 256),  # 307 800 states: past what 64 KB of 2-bit moves holds, the spill path
    LDS_EDGE_IN,
    LDS_EDGE_OUT,
]


def repeats(y):
    y = np.asarray(y)
    return int(np.sum(y[1:] == y[:-1]))


def feasible(T, y):
    return T >= len(y) + repeats(y)


def make_logits(T, L, seed):
    """(logits [T, V] fp32, y [L] int32) of the recipe."""
    rng = np.random.default_rng(seed)
    logits = (3.0 * rng.standard_normal((T, V))).astype(np.float32)
    y = rng.integers(1, V, size=L).astype(np.int32)
    if L >= 3:
        y[1] = y[0]
    return logits, y


def make_case(T, L, seed):
    """(lp [T, L+1] fp32, y [L] int32) of the recipe."""
    logits, y = make_logits(T, L, seed)
    x = logits.astype(np.float64)
    m = x.max(axis=1, keepdims=True)
    logp = x - (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True)))
    cols = np.concatenate([[0], y]).astype(np.int64)
    return logp[:, cols].astype(np.float32), y


def make_batch(shapes, seed):
    """A padded batch of one case per (T, L): lp [B, Tmax, Lmax+1] fp32 (0 past a row's lengths, as
    the first CTC stage leaves it), targets [B, Lmax] int32 (0 padded), ilen, tlen int32 [B]."""
    B = len(shapes)
    Tmax = max(t for t, _ in shapes)
    Lmax = max(l for _, l in shapes)
    lp = np.zeros((B, Tmax, Lmax + 1), dtype=np.float32)
    targets = np.zeros((B, Lmax), dtype=np.int32)
    ilen = np.array([t for t, _ in shapes], dtype=np.int32)
    tlen = np.array([l for _, l in shapes], dtype=np.int32)
    for b, (T, L) in enumerate(shapes):
        r, y = make_case(T, L, seed + b)
        lp[b, :T, :L + 1] = r
        targets[b, :L] = y
    return lp, targets, ilen, tlen


def survey(shapes=None, seeds=20, big_seeds=6):
    """rows of (T, L, feasible cases, cases with the same path in fp32 and fp64, max |s32 - s64|)."""
    rows = []
    for T, L in shapes or SHAPES:
        n = big_seeds if T * (2 * L + 1) > 100000 else seeds
        feas = same = 0
        worst = 0.0
        for seed in range(n):
            lp, y = make_case(T, L, seed)
            s32, st32, _ = R.align_row(lp, y, T, np.float32)
            s64, st64, _ = R.align_row(lp, y, T, np.float64)
            if st64 is None:
                assert st32 is None and not feasible(T, y)
                continue
            feas += 1
            same += int(st32 is not None and np.array_equal(st32, st64))
            worst = max(worst, abs(float(s32) - float(s64)))
        rows.append((T, L, feas, same, worst))
    return rows


if __name__ == "__main__":
    print(f"{'T':>5} {'L':>4} {'feasible':>8} {'same path':>9} {'max |s32-s64|':>14}")
    for T, L, feas, same, worst in survey():
        print(f"{T:>5} {L:>4} {feas:>8} {same:>9} {worst:>14.3e}")
