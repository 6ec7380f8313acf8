"""Paraformer's heads on the HIP kernels: everything of the model after the conformer layers, in
training (ParaformerHeadsFn) and in its one-pass decoding (paraformer_decode), on the decoder
layers and the after_norm tail of nets/functional.py and the integrate-and-fire scan of
csrc/cif.hip."""

from __future__ import annotations

import math
from types import SimpleNamespace

import torch

from .. import kernels as K
from .._native import ACT_RELU
from ..utils.markers import ranged
from .functional import (F32, LN_EPS, _e, _ln_bufs, _rows2d, after_norm_backward, decoder_layers_bwd,
                         decoder_layers_fwd, decoder_rates)


def predictor_logits(pr, hm, B, T):
    """The predictor's logits (predictor.py:32-33 before the sigmoid): conv1d(k3, pad 1) as
    one GEMM over overlapping row windows of a zero-padded copy, then the scalar head.
    hm [B*T, d] in the compute dtype -> (z [B*T, 1] fp32, xpad, cv: what the backward keeps)."""
    dev, adt = hm.device, hm.dtype
    d = hm.shape[-1]
    M = B * T
    wp = pr.weights()
    xpad = torch.zeros(B, T + 2, d, dtype=adt, device=dev)
    xpad[:, 1:T + 1] = hm.view(B, T, d)
    wc = _e((d, 3 * d), adt, dev)
    K.permute_last2(wp.Wc.reshape(d, d, 3), d, d, 3, wc)  # [out][in][tap] -> [out][tap][in]
    win = xpad.as_strided((B, T, 3 * d), ((T + 2) * d, d, 1))
    cv = _e((B, T, d), adt, dev)
    K.gemm(win, wc.t().unsqueeze(0).expand(B, 3 * d, d), cv, bias=wp.bc, act=ACT_RELU)
    z = _e((M, 1), F32, dev)
    K.gemm(cv.view(M, d), wp.Wl.t(), z, bias=wp.bl)
    return z, xpad, cv


def paraformer_decode(model, h32, plen, mask_k, B, T):
    """Paraformer's one-pass decoding after the encoder (liteasr/models/paraformer.py:126-128,
    the predictor in its inference branch, predictor.py:41-53): h32 [B*T, d] fp32 encoder
    output, plen int32 [B] frames the predictor keeps, mask_k u8 [B, T] the memory key mask
    (1 = padding).  Returns (cif: the K.cif_infer state, ulens: host list, ids: host int32
    [B, L] with L = max ulens, logits [B*L, V]); ids and logits are None when L = 0.  One
    device->host copy of ulen [B] sizes the decoder pass (the reference's max(ulens)); the
    decoder's self-attention over the L rows is unmasked, as in the reference."""
    dev, adt = h32.device, model.compute_dtype
    dec = model.decoder
    d = h32.shape[1]
    hm = h32.to(adt)
    z, _, _ = predictor_logits(model.predictor, hm, B, T)
    cif = K.cif_infer(z, plen, h32.view(B, T, d))
    ulens = cif.ulen.cpu().tolist()
    L = max(ulens)
    if L == 0:
        return cif, ulens, None, None
    nomask = torch.zeros(B, L, dtype=torch.uint8, device=dev)
    rows = cif.out[:, :L].contiguous().view(B * L, d)
    hat, _ = decoder_layers_fwd(dec, dec.weights(), rows, hm, B, L, T, (nomask, L, 0, mask_k),
                                (0.0, 0.0, 0.0, 0.0), adt, seed_shift=8)
    _, ids, _ = K.logsoftmax_topk(hat, 1)
    return cif, ulens, ids.view(B, L).cpu(), hat


@ranged
class ParaformerHeadsFn(torch.autograd.Function):
    """Everything of Paraformer.forward after the conformer layers (liteasr/models/
    paraformer.py:97-113): encoder after_norm, the CIF predictor (predictor.py:24-118:
    conv1d k3 + ReLU and linear + sigmoid as GEMMs, the integrate-and-fire scan in
    csrc/cif.hip), target embedding + PE, the no-grad first decoder pass and its argmax,
    the glancing sampler (host ``random.sample`` per utterance, the reference's RNG calls),
    the mix and the second decoder pass.  Returns (hs_attn [B*L, V], sum_alpha [B])."""

    @staticmethod
    def forward(ctx, x, anchor, model, env, ys, ylens_host, rng):
        dev, adt = x.device, env.adt
        enc, dec, pr = model.encoder, model.decoder, model.predictor
        B, T = env.B, env.T
        L = ys.shape[1]
        M, R = B * T, B * L
        tr = env.training
        x = x.contiguous()
        d = x.shape[1]
        # ---- encoder after_norm: fp32 for the predictor, compute dtype for the decoder memory
        we = enc.after_norm_weights()
        h32, me, re = _ln_bufs(M, d, F32, dev)
        K.layernorm_fwd(x, we.g, we.b, LN_EPS, h32, me, re)
        hm = h32.to(adt)
        z, xpad, cv = predictor_logits(pr, hm, B, T)
        # ---- CIF
        plen = env.pred_len
        ylen = env.ylen
        cs = SimpleNamespace(alpha=_e(M, F32, dev), acc=_e(M, F32, dev), fired=_e(M, torch.uint8, dev),
                             row=_e(M, torch.int32, dev), sum_alpha=_e(B, F32, dev), mae=_e(B, F32, dev),
                             out=_e((B, L, d), F32, dev))
        K.cif_fwd(z, plen, ylen, h32, B, T, L, cs)
        # ---- target embedding + PE (paraformer.py:103)
        eos = model.eos
        ys_in = ys.masked_fill(ys == model.ignore, eos).to(torch.int32).contiguous()
        emb = _e((R, d), F32, dev)
        p_pos = model.pos_dropout_rate if tr else 0.0
        K.embed_pe_fwd(ys_in, L, model.embed_weight(), model.pe.table(L), math.sqrt(d), emb, p_pos, env.seed + 5)
        # ---- first decoder pass, no grad (paraformer.py:106-109)
        wd = dec.weights()
        p = decoder_rates(dec, tr)
        nomask = torch.zeros(B, L, dtype=torch.uint8, device=dev)
        masks = (nomask, L, 0, env.mask_k)
        cif_rows = cs.out.view(R, d)
        hat, _ = decoder_layers_fwd(dec, wd, cif_rows, hm, B, L, T, masks, p, adt, seed_shift=8)
        _, ids, _ = K.logsoftmax_topk(hat, 1)
        # ---- glancing sampler on the host (glancing_sampler.py:16-30)
        ys_hat = ids.view(B, L).long().cpu()
        ys_in_h = ys_in.cpu().long()
        pad = torch.arange(L)[None, :] >= ylens_host[:, None]
        ys_hat = ys_hat.masked_fill(pad, eos)
        num = torch.ceil(model.sample_ratio * (ys_hat != ys_in_h).sum(-1)).long()
        rep = torch.zeros(B, L, dtype=torch.uint8)
        for b in range(B):
            rep[b, rng.sample(range(int(ylens_host[b])), int(num[b]))] = 1
        rep = rep.to(dev)
        mix = _e((R, d), F32, dev)
        K.glancing_mix(rep, emb, cif_rows, mix)
        # ---- second pass, with gradients
        hs_attn, dsv = decoder_layers_fwd(dec, wd, mix, hm, B, L, T, masks, p, adt)
        model.last_glance = SimpleNamespace(ys_hat=ys_hat, replace=rep.cpu().bool(), cif=cs)
        ctx.sv = SimpleNamespace(x=x, st=(me, re), h32=h32, hm=hm, xpad=xpad, cv=cv, cs=cs, rep=rep,
                                 ys_in=ys_in, dec=dsv, dims=(B, T, L, d), p_pos=p_pos)
        ctx.model, ctx.env = model, env
        return hs_attn, cs.sum_alpha

    @staticmethod
    def backward(ctx, g_attn, g_sum):
        sv, model, env = ctx.sv, ctx.model, ctx.env
        enc, dec, pr = model.encoder, model.decoder, model.predictor
        B, T, L, d = sv.dims
        M, R = B * T, B * L
        dev, adt = sv.x.device, env.adt
        dh = torch.zeros(M, d, dtype=F32, device=dev)  # gradient of the after_norm output
        wd, gd = dec.weights(), dec.grads()
        with K.deferred_reductions():
            if g_attn is not None:
                dmix = decoder_layers_bwd(_rows2d(g_attn, R), sv.dec, dec, wd, gd, sv.hm, B, L, T, dh, adt)
            else:
                dmix = torch.zeros(R, d, dtype=F32, device=dev)
        dec.on_grads_ready()
        g_emb, g_cif = _e((R, d), F32, dev), _e((R, d), F32, dev)
        K.glancing_mix(sv.rep, dmix, None, g_emb, g_cif, backward=True)
        K.embed_bwd(sv.ys_in, g_emb, math.sqrt(d), model.embed_grad(), sv.p_pos, env.seed + 5)
        model.unit_ready("embed")
        # ---- CIF backward -> predictor logits / encoder output
        dz = _e(M, F32, dev)
        dh_cif = _e((B, T, d), F32, dev)
        gs = g_sum.contiguous().float() if g_sum is not None else None
        K.cif_bwd(env.pred_len, env.ylen, sv.h32, B, T, L, sv.cs, g_cif, gs, dz, dh_cif)
        # ---- predictor head and conv1d backward
        wp, gp = pr.weights(), pr.grads()
        dza = dz.to(adt).view(M, 1)
        K.gemm(dza.t(), sv.cv.view(M, d), gp.Wl, beta=1.0, rowsum=gp.bl)
        dpre = _e((M, d), adt, dev)
        K.gemm(dza, wp.Wl, dpre, aux=sv.cv.view(M, d), aux_act=ACT_RELU)
        P = torch.zeros(B, T + 2, d, dtype=adt, device=dev)
        P[:, 1:T + 1] = dpre.view(B, T, d)
        Pk = P.view(-1, d)[1:-1]
        kw = Pk.shape[0]
        win = sv.xpad.view(-1)[: (kw - 1) * d + 3 * d].as_strided((kw, 3 * d), (d, 1))
        dwc = _e((d, 3 * d), F32, dev)
        K.gemm(Pk.t(), win, dwc, split_k=0, rowsum=gp.bc)
        K.permute_last2(dwc, d, d, 3, gp.Wc.view(d, d, 3), reverse=True, accumulate=True)
        wflip = wp.Wc.reshape(d, d, 3).flip(-1).permute(1, 2, 0).reshape(d, 3 * d).to(adt)
        pwin = P.as_strided((B, T, 3 * d), ((T + 2) * d, d, 1))
        dh_pred = _e((B, T, d), F32, dev)
        K.gemm(pwin, wflip.t().unsqueeze(0).expand(B, 3 * d, d), dh_pred)
        pr.on_grads_ready()
        dh += dh_cif.view(M, d)
        dh += dh_pred.view(M, d)
        dx = after_norm_backward(enc, sv.x, sv.st, dh)
        ctx.sv = None
        return dx, None, None, None, None, None, None
