"""Host restatement of inference-mode integrate-and-fire (lasr_cif_infer, csrc/cif.hip;
liteasr/nets/paraformer/predictor.py:41-118 with ``ylens=None``), written from the
reference's update rules in numpy, independent of the device code.

``cif_infer_ref(z, plen, h)`` takes the predictor logits z [B, T'], the kept frames plen
[B] and the encoder output h [B, T', D] and returns (sum_alpha [B], ulen [B] int, fired
[B, T'] bool, row [B, T'] int, out [B, T', D], extra) with extra.alpha [B, T'], extra.count
[B] (the counted fired states) and extra.beta [B].

dtype float32 (default) follows the kernel's operation order, so equal inputs give equal
bits wherever numpy's float32 ``exp`` agrees with the device's ``expf``:
  * alpha = 1 / (1 + exp(-z)) for t < plen, else 0;
  * sum_alpha = the 64 strided partials (lane l adds t = l, l + 64, ... in order), then the
    xor-butterfly tree over offsets 32, 16, ..., 1;
  * ulen = rint(sum_alpha) (half to even, torch.round); beta = sum_alpha / ulen - 1e-4, each
    operation rounded once (ulen = 0: +inf, or NaN for a zero sum; nothing fires);
  * per frame: new = prev + alpha; fire = new >= beta; left = beta - prev; right = new - beta;
    state o = s + left * h (product and sum rounded separately); on a fire o is the fired
    state, s = right * h, prev = right; otherwise s = o, prev = new;
  * a fired state whose entries are all zero does not count (predictor.py:105); counted
    states fill out[b] from row 0 in frame order, every later row is zero.
dtype float64 runs the same rules in double (the yardstick for error bars).
"""

from types import SimpleNamespace

import numpy as np


def _wave_sum(alpha_row, dt):
    parts = np.zeros(64, dtype=dt)
    for t in range(alpha_row.shape[0]):  # lane t % 64 adds its frames in order
        parts[t % 64] = dt(parts[t % 64] + alpha_row[t])
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        parts = (parts + parts[lanes ^ o]).astype(dt)
    return parts[0]


def cif_infer_ref(z, plen, h, dtype=np.float32):
    dt = np.dtype(dtype).type
    z = np.asarray(z, dtype=dt)
    h = np.asarray(h, dtype=dt)
    B, T, D = h.shape
    z = z.reshape(B, T)
    plen = np.asarray(plen).reshape(B)
    alpha = np.zeros((B, T), dtype=dt)
    sum_alpha = np.zeros(B, dtype=dt)
    ulen = np.zeros(B, dtype=np.int64)
    fired = np.zeros((B, T), dtype=bool)
    row = np.full((B, T), -1, dtype=np.int64)
    out = np.zeros((B, T, D), dtype=dt)
    count = np.zeros(B, dtype=np.int64)
    beta_of = np.zeros(B, dtype=dt)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for b in range(B):
            a = (dt(1) / (dt(1) + np.exp(-z[b]))).astype(dt)
            a[np.arange(T) >= plen[b]] = 0
            alpha[b] = a
            s_a = _wave_sum(a, dt)
            sum_alpha[b] = s_a
            ulen[b] = int(np.rint(s_a))
            beta = dt(dt(s_a / dt(ulen[b])) - dt(1e-4))
            beta_of[b] = beta
            prev = dt(0)
            s = np.zeros(D, dtype=dt)
            for t in range(T):
                new = dt(prev + a[t])
                fire = bool(new >= beta)
                left, right = dt(beta - prev), dt(new - beta)
                o = (s + (left * h[b, t]).astype(dt)).astype(dt)
                if fire:
                    fired[b, t] = True
                    if np.any(o != 0):
                        row[b, t] = count[b]
                        out[b, count[b]] = o
                        count[b] += 1
                    s = (right * h[b, t]).astype(dt)
                    prev = right
                else:
                    s = o
                    prev = new
    extra = SimpleNamespace(alpha=alpha, count=count, beta=beta_of)
    return sum_alpha, ulen, fired, row, out, extra
