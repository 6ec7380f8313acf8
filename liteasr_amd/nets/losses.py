"""The criterions' loss nodes on the HIP kernels (csrc/loss.hip, ctc.hip, rnnt.hip): forward
computes the loss only, backward writes the logits gradients scaled by the incoming device
gradient, without a host round trip.
  HybridLossFn     label-smoothed KL + CTC, combined      criterions/hybrid_ctc_attn.py:39-79
  ParaformerLossFn cross-entropy + L1 on the CIF's sum    criterions/paraformer_loss.py:39-56
  RNNTLossFn       transducer loss of the joint logits     criterions/rnnt.py:53-72
"""

from __future__ import annotations

from types import SimpleNamespace

import torch

from .. import kernels as K
from ..utils.markers import ranged
from .functional import F32, _e


@ranged
class ParaformerLossFn(torch.autograd.Function):
    """ParaformerLoss.__call__ (liteasr/criterions/paraformer_loss.py:39-56):
    gamma * CE(hs_attn, ys; ignore -1, mean over targets) + mean |sum_alpha - ylens|."""

    @staticmethod
    def forward(ctx, hs_attn, sum_alpha, ys, ylens, count, gamma, cif):
        dev = hs_attn.device
        R, V = hs_attn.shape
        B = sum_alpha.shape[0]
        tgt = ys.reshape(-1).to(torch.int32).contiguous()
        lse, rows = _e(R, F32, dev), _e(R, F32, dev)
        K.lsm_kl_fwd(hs_attn, tgt, -1, 0.0, lse, rows)
        loss = _e(1, F32, dev)
        K.loss_combine(rows, gamma / max(count, 1), cif.mae, 1.0 / B, loss)
        ctx.sv = SimpleNamespace(ha=hs_attn, tgt=tgt, lse=lse, scale=gamma / max(count, 1), B=B,
                                 sign=torch.sign(sum_alpha.detach() - ylens.to(F32)))
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        sv = ctx.sv
        g = g.contiguous().float()
        ga = K.padded_rows(sv.ha.shape[0], sv.ha.shape[1], sv.ha.dtype, g.device)
        K.lsm_kl_bwd(sv.ha, sv.tgt, -1, 0.0, sv.lse, ga, sv.scale, gdev=g)
        gsum = sv.sign * (g / sv.B)
        ctx.sv = None
        return ga, gsum, None, None, None, None, None


@ranged
class HybridLossFn(torch.autograd.Function):
    """HybridCTCLoss.__call__ (liteasr/criterions/hybrid_ctc_attn.py:39-79):
    ctc_weight * CTC(sum)/B + (1 - ctc_weight) * smoothed-KL(sum)/B.
    Forward computes losses only; backward computes both logits gradients scaled by the
    incoming (device) gradient without a host round trip."""

    @staticmethod
    def forward(ctx, h_attn, h_ctc, prep, ctc_weight, smoothing, ignore):
        dev = h_attn.device
        B, L1 = prep.ys_in.shape
        V = h_attn.shape[-1]
        Tp = h_ctc.shape[1]
        ha = h_attn.reshape(B * L1, V)
        hc = h_ctc.reshape(B, Tp, V)
        L = prep.tgt_ctc.shape[1]
        lse_a = _e(B * L1, F32, dev)
        rows = _e(B * L1, F32, dev)
        K.lsm_kl_fwd(ha, prep.tgt, ignore, smoothing, lse_a, rows)
        S = 2 * L + 1
        lse = _e(B * Tp, F32, dev)
        lp = _e(B * Tp * (L + 1), F32, dev)
        alpha = _e(B * Tp * S, F32, dev)
        beta = _e(B * Tp * S, F32, dev)  # computed alongside alpha (one launch)
        nll = _e(B, F32, dev)
        K.ctc_fwd(hc, prep.tgt_ctc, prep.pred_len, prep.ylen, lse, lp, alpha, nll, beta=beta)
        loss = _e(1, F32, dev)
        K.loss_combine(nll, ctc_weight / B, rows, (1.0 - ctc_weight) / B, loss)
        ctx.sv = SimpleNamespace(ha=ha, hc=hc, prep=prep, lse_a=lse_a, lse=lse, lp=lp, alpha=alpha,
                                 beta=beta, nll=nll, w=ctc_weight, s=smoothing, ign=ignore, B=B,
                                 shapes=(h_attn.shape, h_ctc.shape))
        ctx.parts = (nll, rows)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        sv = ctx.sv
        g = g.contiguous().float()
        dev = g.device
        B = sv.B
        ga = K.padded_rows(sv.ha.shape[0], sv.ha.shape[1], sv.ha.dtype, dev)
        K.lsm_kl_bwd(sv.ha, sv.prep.tgt, sv.ign, sv.s, sv.lse_a, ga, (1.0 - sv.w) / B, gdev=g)
        gc = K.padded_rows(sv.hc.shape[0] * sv.hc.shape[1], sv.hc.shape[2], sv.hc.dtype, dev).view(sv.hc.shape)
        K.ctc_bwd(sv.hc, sv.prep.tgt_ctc, sv.prep.pred_len, sv.prep.ylen, sv.lse, sv.lp, sv.alpha,
                  sv.nll, sv.beta, gc, sv.w / B, gdev=g, beta_ready=True)
        ctx.sv = None
        return ga.view(sv.shapes[0]), gc.view(sv.shapes[1]), None, None, None, None


@ranged
class RNNTLossFn(torch.autograd.Function):
    """RNNTLoss (liteasr/criterions/rnnt.py:53-72): batch mean of -log P(y|x) over the raw
    joint logits [B, T, U1, V] with the log-softmax fused (csrc/rnnt.hip); the backward
    writes d loss / d logits scaled by the incoming device gradient, no host sync."""

    @staticmethod
    def forward(ctx, logits, targets, ilen, tlen, blank):
        dev = logits.device
        B, T, U1, V = logits.shape
        rows = B * T * U1
        lse, lp = _e(rows, F32, dev), _e(rows * 2, F32, dev)
        alpha, beta, nll = _e(rows, F32, dev), _e(rows, F32, dev), _e(B, F32, dev)
        K.rnnt_fwd(logits, targets, ilen, tlen, blank, lse, lp, alpha, beta, nll)
        loss = _e(1, F32, dev)
        K.loss_combine(nll, 1.0 / B, None, 0.0, loss)
        ctx.sv = (logits, targets, ilen, tlen, blank, lse, lp, alpha, beta, nll)
        ctx.nll = nll
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        logits, targets, ilen, tlen, blank, lse, lp, alpha, beta, nll = ctx.sv
        B, T, U1, V = logits.shape
        grad = K.padded_rows(B * T * U1, V, logits.dtype, logits.device).view(B, T, U1, V)
        K.rnnt_bwd(logits, targets, ilen, tlen, blank, lse, lp, alpha, beta, nll, grad, 1.0 / B,
                   gdev=g.contiguous().float())
        ctx.sv = None
        return grad, None, None, None, None
