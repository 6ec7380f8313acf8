"""CTC forced alignment restated in numpy, parameterised by dtype (lasr_ctc_align's semantics,
include/liteasr_hip.h).

``float32`` is the yardstick the kernel must match bit for bit: per step a max of fp32 values and
one fp32 add, which numpy rounds exactly as the device does.  ``float64`` on the same fp32 ``lp``
cast up shows the yardstick is sound.  Vectorised over the lattice states; the ties are the
kernel's: stay unless the step from s-1 is strictly greater, then the skip from s-2 only if
strictly greater again."""

import numpy as np


def extended(y):
    """blank-interleaved labels of target y: [0, y0, 0, y1, ..., 0]."""
    ext = np.zeros(2 * len(y) + 1, dtype=np.int64)
    ext[1::2] = y
    return ext


def skip_allowed(y):
    """bool [S]: the move from s-2 exists (ctc.hip's rule: s odd, s >= 2, label(s) != label(s-2))."""
    ext = extended(y)
    ok = np.zeros(len(ext), dtype=bool)
    ok[3::2] = ext[3::2] != ext[1:-2:2]
    return ok


def align_row(lp, y, Tb, dtype=np.float32):
    """One utterance.  lp [T, >= L+1] fp32 (column 0 blank, 1+i target i), y the L labels, Tb
    frames.  Returns (score as dtype scalar, states int32 [Tb] or None, spans int32 [L, 2] or
    None); None where the score is not finite."""
    y = np.asarray(y, dtype=np.int64)
    L = len(y)
    S = 2 * L + 1
    ninf = dtype(-np.inf)
    if Tb <= 0:
        return (dtype(0) if L == 0 else ninf), None, None
    col = np.zeros(S, dtype=np.int64)
    col[1::2] = 1 + np.arange(L)
    e = np.asarray(lp[:Tb], dtype=np.float32)[:, col].astype(dtype)  # [Tb, S]
    skip = skip_allowed(y)
    v = np.full(S, ninf, dtype=dtype)
    v[0] = e[0, 0]
    if L >= 1:
        v[1] = e[0, 1]
    moves = np.zeros((Tb, S), dtype=np.int8)
    with np.errstate(invalid="ignore"):
        for t in range(1, Tb):
            best = v.copy()
            mv = np.zeros(S, dtype=np.int8)
            a1 = np.full(S, ninf, dtype=dtype)
            a1[1:] = v[:-1]
            take = a1 > best
            take[0] = False
            best = np.where(take, a1, best)
            mv[take] = 1
            a2 = np.full(S, ninf, dtype=dtype)
            a2[2:] = v[:-2]
            take = skip & (a2 > best)
            best = np.where(take, a2, best)
            mv[take] = 2
            v = (best + e[t]).astype(dtype)
            moves[t] = mv
        if S == 1:
            end = 0
        else:
            end = S - 1 if v[S - 1] >= v[S - 2] else S - 2
    score = v[end]
    if not np.isfinite(score):
        return score, None, None
    states = np.empty(Tb, dtype=np.int32)
    s = end
    for t in range(Tb - 1, -1, -1):
        states[t] = s
        s -= int(moves[t, s])
    spans = np.full((L, 2), -1, dtype=np.int32)
    for i in range(L):
        at = np.nonzero(states == 2 * i + 1)[0]
        spans[i] = (at[0], at[-1] + 1)
    return score, states, spans


def align_batch(lp, targets, ilen, tlen, dtype=np.float32):
    """The kernel's three outputs for a padded batch: states [B, T] int32, spans [B, Lmax, 2]
    int32 and score [B] dtype, with its -1 conventions."""
    lp = np.asarray(lp)
    B, T, L1 = lp.shape
    Lmax = L1 - 1
    states = np.full((B, T), -1, dtype=np.int32)
    spans = np.full((B, Lmax, 2), -1, dtype=np.int32)
    score = np.zeros(B, dtype=dtype)
    for b in range(B):
        Tb, Lb = int(ilen[b]), int(tlen[b])
        sc, st, sp = align_row(lp[b], np.asarray(targets[b][:Lb]), Tb, dtype)
        score[b] = sc
        if st is not None:
            states[b, :Tb] = st
            spans[b, :Lb] = sp
    return states, spans, score


def brute_force_best(lp, y, Tb):
    """max over every valid CTC path of its float64 log-prob (exponential: tiny shapes only)."""
    ext = extended(np.asarray(y, dtype=np.int64))
    S = len(ext)
    skip = skip_allowed(y)
    col = np.zeros(S, dtype=np.int64)
    col[1::2] = 1 + np.arange(len(y))
    e = np.asarray(lp[:Tb], dtype=np.float64)[:, col]
    best = -np.inf

    def rec(t, s, acc):
        nonlocal best
        if t == Tb:
            if s >= S - 2 or S == 1:
                best = max(best, acc)
            return
        for d in (0, 1, 2):
            n = s + d
            if n >= S or (d == 2 and not skip[n]):
                continue
            rec(t + 1, n, acc + e[t, n])

    for s0 in range(min(2, S)):
        rec(1, s0, e[0, s0])
    return best
