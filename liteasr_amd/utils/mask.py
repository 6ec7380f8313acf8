"""Host-side draws of the wav2vec 2.0 step: the span mask (liteasr/utils/mask.py:93-230) and the
negative indices (liteasr/models/wav2vec2.py:336-357).

Both consume their generators call for call like the reference -- ``np.random`` for the mask,
torch's CPU generator for the indices -- so seeding them reproduces the reference's mask and
indices exactly.  They are small (B x T' bools, B x M x N ints) and cost one host-to-device copy
each per step.
"""

from __future__ import annotations

import numpy as np
import torch


def _span_lengths(policy, count, length):
    if policy == "static":
        return np.full(count, length)
    if policy == "uniform":
        return np.random.randint(0.0, length * 2 + 1, size=count)
    if policy == "normal":
        return [max(1, int(round(v))) for v in np.random.normal(length, 0.0, size=count)]
    if policy == "poisson":
        return [int(round(v)) for v in np.random.poisson(length, size=count)]
    raise Exception("unknown mask selection " + policy)


def _place_without_overlap(frame, spans, min_interval):
    """Spans placed longest first into the free intervals, each interval drawn with probability
    proportional to its length (only intervals that still fit the span count)."""
    taken = []
    free = [(0, frame)]
    shortest = min(spans)
    for size in sorted(spans, reverse=True):
        room = np.fromiter((hi - lo if hi - lo >= size + min_interval else 0 for lo, hi in free), int)
        total = np.sum(room)
        if total == 0:
            break
        lo, hi = free.pop(np.random.choice(len(free), p=room / total))
        start = np.random.randint(lo, hi - size)
        taken.extend(start + i for i in range(size))
        if lo + shortest + min_interval <= start:
            free.append((lo, start - min_interval + 1))
        if start + size + min_interval + shortest < hi:
            free.append((start + size + min_interval, hi))
    return np.asarray(taken)


def span_mask(batch, frame, prob, length, policy="static", no_overlap=False, min_mask_num=0, min_interval=0):
    """(batch, frame) bool mask of random spans; every row masks the same number of frames (rows
    with more are thinned at random to the shortest row's count)."""
    count = max(min_mask_num, int(prob * frame / float(length) + np.random.rand()))
    rows = []
    for _ in range(batch):
        spans = _span_lengths(policy, count, length)
        if sum(spans) == 0:
            spans[0] = min(length, frame - 1)
        if no_overlap:
            idx = _place_without_overlap(frame, spans, min_interval)
        else:
            shortest = min(spans)
            if frame - shortest <= count:
                shortest = frame - count - 1
            starts = np.random.choice(frame - shortest, count, replace=False)
            idx = np.asarray([starts[j] + o for j in range(len(starts)) for o in range(spans[j])])
        rows.append(np.unique(idx[idx < frame]))
    keep = min(len(r) for r in rows)
    mask = torch.zeros((batch, frame), dtype=torch.bool)
    for i, r in enumerate(rows):
        if len(r) > keep:
            r = np.random.choice(r, keep, replace=False)
        mask[i, r] = True
    return mask


def negative_indices(batch, num_mask, num_negatives):
    """(batch, num_mask * num_negatives) int64 rows of the flattened (batch * num_mask) targets:
    for masked position m of utterance b, ``num_negatives`` draws from the utterance's other
    masked positions (uniform over num_mask - 1, shifted past m), offset by b * num_mask."""
    own = torch.arange(num_mask).unsqueeze(-1).expand(-1, num_negatives).flatten()
    idx = torch.randint(low=0, high=num_mask - 1, size=(batch, num_mask * num_negatives))
    idx[idx >= own] += 1
    for b in range(1, batch):
        idx[b] += b * num_mask
    return idx
