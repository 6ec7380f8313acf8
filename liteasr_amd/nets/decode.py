"""The U2 inference paths on the HIP kernels, eval mode, no saved state: the encoder's
after_norm, the CTC head, the decoder over whole hypotheses (decoder_logits) and advanced one
position per step through a key/value cache (DecoderStepCache), on the attention and FFN
sub-blocks of nets/functional.py.  liteasr_amd/decoding.py drives them."""

from __future__ import annotations

import math

from .. import kernels as K
from .._native import ACT_RELU
from .functional import F32, _e, ffn_forward, ld_scores, ln_forward, mha_forward, vocab_logits


def encoder_out(x, model, adt):
    """Encoder after_norm (transformer_encoder.py:126) without the CTC dropout branch:
    x [M, d] fp32 residual stream -> h [M, d] in the compute dtype."""
    we = model.encoder.after_norm_weights()
    h, _, _, _ = ln_forward(x.contiguous(), we.g, we.b, adt)
    return h


def ctc_logits(h, model):
    """ctc_lo(h) (ctc.py:25-26, no dropout), [M, V] padded-row view."""
    wc = model.ctc.weights()
    return vocab_logits(h, wc.W, wc.b)


def decoder_logits(model, h, ys_in, dec_mask, mem_mask, B, L1, T):
    """TransformerDecoder.forward (transformer_decoder.py:70-93) in eval mode for
    decoding: ys_in int32 [B, L1], dec_mask u8 [B, L1, L1] (1 = masked), memory h
    [B*T, d] (compute dtype), mem_mask u8 [B, T].  Returns h_attn [B*L1, V] (padded rows).
    Same kernels and order as HeadsFn.forward, without dropout and saved state."""
    wd = model.decoder.weights()
    d, adt, dev = wd.d, h.dtype, h.device
    y = _e((B * L1, d), F32, dev)
    K.embed_pe_fwd(ys_in, L1, wd.E, wd.pe, math.sqrt(d), y, 0.0, 0)
    for lw in wd.layers:
        l1, _, _, _ = ln_forward(y, lw.ln1.g, lw.ln1.b, adt)
        y1, _ = mha_forward(l1, None, lw.sa, B, L1, L1, wd.H, dec_mask, dec_mask.stride(0), dec_mask.stride(1), y,
                            0.0, 0, 0.0, 0)
        l2, _, _, _ = ln_forward(y1, lw.ln2.g, lw.ln2.b, adt)
        y2, _ = mha_forward(l2, h, lw.ca, B, L1, T, wd.H, mem_mask, T, 0, y1, 0.0, 0, 0.0, 0)
        l3, _, _, _ = ln_forward(y2, lw.ln3.g, lw.ln3.b, adt)
        y, _, _ = ffn_forward(l3, lw.ff, ACT_RELU, 0.0, 0, y2, 1.0, 0.0, 0)
    yf, _, _, _ = ln_forward(y, wd.ln_f.g, wd.ln_f.b, adt)
    return vocab_logits(yf, wd.Wout, wd.bout)


class DecoderStepCache:
    """TransformerDecoder.forward_one_step (liteasr/nets/transformer_decoder.py:58-68,
    DecoderLayer with cache: transformer_layer.py:27-47,179-221) for the attention beam
    search (u2.py:163-216), eval mode, with a key/value cache per decoder layer: each step
    runs only the new position -- its row's projections, one-query attention over the cached
    keys, the source attention over the memory keys/values (projected ONCE per utterance:
    the memory is the same for every beam and step), the FFN and the output projection --
    instead of the whole prefix.

    Cache semantics follow the reference exactly.  Its cache (each layer's outputs for the
    earlier positions) is NOT reordered when the beam reorders its hypotheses; the first
    layer recomputes its keys from the (reordered) hypothesis embeddings, while layers >= 1
    attend to the earlier rows in the previous step's slot order.  Here: the first layer's
    key/value cache is gathered by the beam's selection each step (identical to recomputing
    it from the reordered embeddings: a row's projection does not depend on other rows);
    the caches of layers >= 1 are never permuted (tests/golden/decode_cache.npz, two
    decoder layers, pins the per-step log-probs)."""

    def __init__(self, model, mem, beam, T, max_len):
        wd = model.decoder.weights()
        self.wd, self.beam, self.T = wd, beam, T
        d, adt, dev = wd.d, mem.dtype, mem.device
        self.adt, self.dev = adt, dev
        self.kv_mem = []  # per layer [T, 2d]: linear_k / linear_v of the memory (src_attn)
        for lw in wd.layers:
            kv = _e((T, 2 * d), adt, dev)
            K.linear(mem, lw.ca.Wkv, kv, bias=lw.ca.bkv)
            self.kv_mem.append(kv)
        n = len(wd.layers)
        self.kc = [_e((beam, max_len, d), adt, dev) for _ in range(n)]
        self.vc = [_e((beam, max_len, d), adt, dev) for _ in range(n)]

    def _attend(self, q, k3, v3, Tk):
        """softmax(q k^T / sqrt(dk)) v for one query row per beam: q [beam, d] (row stride
        arbitrary), k3 / v3 [beam, >=Tk, d] views (any batch stride, 0 included)."""
        wd, beam = self.wd, self.beam
        H, d = wd.H, wd.d
        dk = d // H
        ldS = ld_scores(Tk)
        q4 = q.unflatten(1, (H, dk)).unsqueeze(2)  # (beam, H, 1, dk)
        k4 = k3[:, :Tk].unflatten(2, (H, dk)).permute(0, 2, 1, 3)  # (beam, H, Tk, dk)
        v4 = v3[:, :Tk].unflatten(2, (H, dk)).permute(0, 2, 1, 3)
        S = _e((beam, H, 1, ldS), F32, self.dev)
        K.gemm(q4, k4.transpose(-1, -2), S[..., :Tk], alpha=dk ** -0.5)
        P = _e((beam, H, 1, ldS), self.adt, self.dev)
        K.attn_softmax_fwd(S, None, beam, H, 1, Tk, ldS, None, 0, 0, P)
        ctx = _e((beam, d), self.adt, self.dev)
        K.gemm(P[..., :Tk], v4, ctx.unflatten(1, (H, dk)).unsqueeze(2))
        return ctx

    def step(self, ids, i, sel=None):
        """Log-probs' logits [beam, V] of step i (1-based: the new token sits at position
        i - 1); ids int32 [beam] = each hypothesis' last token; sel (int64 device [beam],
        optional) = the beam's selection that produced these hypotheses from the previous
        step's slots."""
        wd, beam, adt, dev = self.wd, self.beam, self.adt, self.dev
        d = wd.d
        if sel is not None and i > 1:
            for c in (self.kc[0], self.vc[0]):
                c[:, :i - 1] = c[:, :i - 1].index_select(0, sel)
        y = _e((beam, d), F32, dev)
        K.embed_pe_fwd(ids, 1, wd.E, wd.pe[i - 1:], math.sqrt(d), y, 0.0, 0)
        for j, lw in enumerate(wd.layers):
            l1, _, _, _ = ln_forward(y, lw.ln1.g, lw.ln1.b, adt)
            qkv = _e((beam, 3 * d), adt, dev)
            K.linear(l1, lw.sa.Wqkv, qkv, bias=lw.sa.bqkv)
            self.kc[j][:, i - 1] = qkv[:, d:2 * d]
            self.vc[j][:, i - 1] = qkv[:, 2 * d:]
            ctx = self._attend(qkv[:, :d], self.kc[j], self.vc[j], i)
            y1 = _e((beam, d), F32, dev)
            K.linear(ctx, lw.sa.Wo, y1, bias=lw.sa.bo, res=y, res_scale=1.0)
            l2, _, _, _ = ln_forward(y1, lw.ln2.g, lw.ln2.b, adt)
            q = _e((beam, d), adt, dev)
            K.linear(l2, lw.ca.Wq, q, bias=lw.ca.bq)
            kv = self.kv_mem[j]
            ctx2 = self._attend(q, kv[:, :d].unsqueeze(0).expand(beam, self.T, d),
                                kv[:, d:].unsqueeze(0).expand(beam, self.T, d), self.T)
            y2 = _e((beam, d), F32, dev)
            K.linear(ctx2, lw.ca.Wo, y2, bias=lw.ca.bo, res=y1, res_scale=1.0)
            l3, _, _, _ = ln_forward(y2, lw.ln3.g, lw.ln3.b, adt)
            y, _, _ = ffn_forward(l3, lw.ff, ACT_RELU, 0.0, 0, y2, 1.0, 0.0, 0)
        yf, _, _, _ = ln_forward(y, wd.ln_f.g, wd.ln_f.b, adt)
        return vocab_logits(yf, wd.Wout, wd.bout)
