"""Fused forward/backward of the encoder stack and the U2 heads on the HIP kernels: the part of
the host path every model family goes through.

Granularity (one autograd node each, so torch's engine only chains a handful of
nodes and never casts/sums tensors itself):
  EmbedConvFn      Conv2d subsampling convolutions                      subsampling.py:42-46
  EmbedOutFn       its output projection + x*sqrt(d) (+dropout)        subsampling.py:47-48, positional_encoding.py:68-75
  ConformerLayerFn one RelativeEncoderLayer (macaron FFN, rel-pos MHSA,  conformer_layer.py:130-147
                   conv module, FFN, final LN)
  TransformerLayerFn one Transformer encoder layer                       transformer_layer.py:64-76,119-136
  HeadsFn          encoder after_norm + CTC head (input dropout always   transformer_encoder.py:126, ctc.py:28-30,
                   on) + the whole Transformer decoder                  transformer_decoder.py:70-93
  EncoderOutFn     encoder after_norm alone, for the other families' heads

This module keeps the helpers and the LayerNorm-fusion plumbing (PostLN, res_proj, LnBwd, dx_ln),
the attention / convolution / FFN sub-blocks, the nodes above, decoder_layers_fwd / _bwd, and
every A/B switch with every function that reads one.  The families build on it, one module each
(they import from here, never the other way round):
  nets/losses.py      HybridLossFn, ParaformerLossFn, RNNTLossFn
  nets/paraformer.py  ParaformerHeadsFn, predictor_logits, paraformer_decode
  nets/transducer.py  TransducerHeadsFn, lstm_layer_fwd / _bwd
  nets/decode.py      encoder_out, ctc_logits, decoder_logits, DecoderStepCache
  nets/wav2vec2.py    the wav2vec 2.0 front end and head

Weight gradients never travel through autograd: the backward kernels accumulate them
(beta = 1) straight into the flat fp32 grad buffer of FlatParams; autograd only
carries the residual-stream gradient between nodes.  Each node takes one "anchor"
parameter as an input so that its output requires grad whenever the model does.
What neighbouring encoder layer nodes hand each other (a chained norm, its gradient, queued
reductions, the batched positional projection) goes through one LayerLink per layer (links.py).

Storage: residual streams fp32; GEMM operands / activations in the model's compute
dtype ``adt`` (bf16, or fp32 for the parity build); attention scores fp32.
"""

from __future__ import annotations

import math
from types import SimpleNamespace

import torch

from .. import kernels as K
from .._native import ACT_GATE, ACT_RELU
from ..utils.markers import ranged
from .links import LayerLink

F32 = torch.float32
LN_EPS = 1e-12

# ==================================================================== switches ===
# Every A/B switch of this host path: a module attribute read at call time by the function that
# branches on it (all in this module), set by tests and tools/flag_ab.py.  True is the product path.
#
# Full-row GEMM tiles with the next LayerNorm in the epilogue (gemm_row.hip): a residual
# projection and the norm after it, or an input-gradient GEMM and the norm backward before
# it, in one launch, bit-identical to the two launches.  False keeps two launches
# (tests/test_switches_gpu.py pins the pair); shapes the kernel does not take (fp32 build, other
# widths) keep them too.
ROW_LN = True
# the decoder's norms after / before its attention projections on the row kernel
DEC_ROW_LN = True
# K >= 1024 GEMMs whose plan splits K (the decoder's FFN on B*(L+1) rows) run the following
# LayerNorm (forward) / the preceding one's backward in their split-K reduction launch
# (gemm_ln.hip); False: separate launches (tests/test_fusions_gpu.py pins the two bit for bit)
SPLITK_LN = True
# the encoder attention's positional-bias gradient (qbias_bwd) in the positional-projection
# gradient GEMM's split-K reduction launch (gemm_ln.hip lasr_gemm_qbias_bwd); False: its own launch
QBIAS_IN_REDUCE = True
# a Conformer layer's first-norm backward and the previous layer's final-norm backward in one
# launch (lasr_layernorm2_bwd, the reverse of FUSED_LN2's chained forward): the previous layer
# receives its final norm's input gradient instead of computing it; False: two launches with
# the fp32 gradient between them (tests/test_fusions_gpu.py pins the two bit for bit)
LN2_BWD_CHAIN = True
# the conv module's BatchNorm + activation backward folded into the depthwise-conv / GLU
# backward (lasr_bn_act_glu_dwconv_bwd: dy computed in its window load, never stored); False: the
# two launches with the fp32 dy between them (tests/test_fusions_gpu.py pins the two bit for bit)
BN_GLU_FUSED = True
# the encoder layers' parameter-gradient reductions (LayerNorm gamma / beta, split-K weight
# slabs, positional biases, depthwise conv) queued across layer nodes and launched together at
# the lowest layer of each backward segment (kernels.deferred_reductions(hold=True)); the
# layers' gradient-ready hooks fire after that launch.  False: one reduction launch per layer
# (tests/test_fusions_gpu.py pins the two bit for bit)
LAYER_RED_HOLD = True
# the encoder's relative-position attention on the fused kernels (attn_flash.hip: scores never
# materialised); False: the materialised-score kernels (see fused_relattn for the shapes)
FUSED_RELATTN = True
# the positional projections of every encoder layer in one batched GEMM (pos_projections);
# False: each layer projects its own
BATCH_POS_PROJ = True
# a layer's final norm and the next layer's first norm in one launch (lasr_layernorm2_fwd)
FUSED_LN2 = True
# Decoder attention on the fused kernels (attn_flash.hip, lasr_attn_fwd/bwd: the relative-
# position kernels without the positional term, Tq queries x Tk keys): scores / softmax /
# P.V (3 launches forward, 5 backward) become 1 + 2 launches, for the self attention (causal +
# padding mask) and the source attention over the encoder output (key padding).
# False keeps the materialised path (tests/test_kernels_gpu.py compares the two).
FUSED_DEC_ATTN = True
# the decoder FFN branch gradients written by the LayerNorm backward that produces each layer's
# output gradient (False: a branch_grad launch per layer; the test pins the two bit for bit)
DEC_GB_IN_LN = True


# ===================================================================== helpers ===
def _e(shape, dtype, dev):
    return torch.empty(shape, dtype=dtype, device=dev)


def ld_scores(T):
    return (T + 7) // 8 * 8


def _seed(base, k):
    return (base * 0x100000001B3 + k * 0x9E3779B1 + 1) & 0xFFFFFFFFFFFFFFFF


def _ln_bufs(rows, D, dtype, dev):
    """(y, mean, rstd) buffers of a LayerNorm over [rows, D] with its output in `dtype`."""
    return _e((rows, D), dtype, dev), _e(rows, F32, dev), _e(rows, F32, dev)


def ln_forward(x, g, b, adt, y2=False, p2=0.0, seed2=0):
    rows, D = x.shape
    y, mean, rstd = _ln_bufs(rows, D, adt, x.device)
    yd = _e((rows, D), adt, x.device) if y2 else None
    K.layernorm_fwd(x, g, b, LN_EPS, y, mean, rstd, yd, p2, seed2)
    return y, yd, mean, rstd


def _link(env, layer):
    """The layer's LayerLink of this forward (nets/links.py); None: a standalone node."""
    return env.links[layer] if env.links is not None else None


def _hold(link):
    """Whether a layer's backward node leaves its reductions queued for a layer below it."""
    return LAYER_RED_HOLD and link is not None and not link.floor


def layer_rates(env):
    """An encoder layer node's (residual, FFN, attention) dropout rates: 0 outside training."""
    return (env.p_drop, env.p_ff, env.p_att) if env.training else (0.0, 0.0, 0.0)


def decoder_rates(dec, training):
    """A Transformer decoder's (residual, FFN, self-attention, source-attention) dropout rates,
    decoder_layers_fwd's `p`: 0 outside training."""
    r = dec.rates
    return (r.drop, r.ff, r.self_att, r.src_att) if training else (0.0, 0.0, 0.0, 0.0)


def sub_dims(Tx, Fd):
    """(T1, F1, T2, F2): frames x features after each of the subsampling's two k3 s2 convolutions."""
    T1, F1 = (Tx - 3) // 2 + 1, (Fd - 3) // 2 + 1
    return T1, F1, (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1


class PostLN:
    """A LayerNorm to run on a residual projection's output row in the same launch:
    g, b (its parameters), f32 (y1 stored fp32: a layer's final norm), nxt (optional: the
    parameters of a chained second norm, bf16 out).  After the call: y1, m1, r1 (+ y2, m2, r2)."""

    __slots__ = ("g", "b", "f32", "nxt", "y1", "m1", "r1", "y2", "m2", "r2")

    def __init__(self, ln, f32=False, nxt=None):
        self.g, self.b, self.f32, self.nxt = ln.g, ln.b, f32, nxt
        self.y1 = self.m1 = self.r1 = self.y2 = self.m2 = self.r2 = None


def norm_of(x, ln, adt, post=None):
    """(y, (mean, rstd)) of the norm `ln` of x: post's outputs when the residual projection that
    produced x ran it in its launch (res_proj), else the norm as its own launch."""
    if post is not None and post.y1 is not None:
        return post.y1, (post.m1, post.r1)
    y, _, m, r = ln_forward(x, ln.g, ln.b, adt)
    return y, (m, r)


def final_norm(x, post, adt):
    """A Conformer layer's final norm `post` of x (fp32 out), with post.nxt chained with the first
    norm of the layer above: ((y, (mean, rstd)), (z, (mean2, rstd2)) or None).  From the residual
    projection's launch when it ran them (res_proj), else one lasr_layernorm2_fwd launch for the
    pair, or the norm alone."""
    if post.y1 is not None:
        return (post.y1, (post.m1, post.r1)), (post.y2, (post.m2, post.r2)) if post.nxt is not None else None
    M, D = x.shape
    y, m, r = _ln_bufs(M, D, F32, x.device)
    if post.nxt is None:
        K.layernorm_fwd(x, post.g, post.b, LN_EPS, y, m, r)
        return (y, (m, r)), None
    z, m2, r2 = _ln_bufs(M, D, adt, x.device)
    K.layernorm2_fwd(x, post.g, post.b, post.nxt.g, post.nxt.b, LN_EPS, y, m, r, z, m2, r2)
    return (y, (m, r)), (z, (m2, r2))


def res_proj(x, W, bias, res, res_scale, p_res, s_res, post=None):
    """out = res + res_scale * drop(x W^T + bias) (fp32 residual stream); when `post` names
    the following LayerNorm and the row kernel takes the shape, the norm runs in the same
    launch and its outputs are set on `post` (post.y1 stays None otherwise)."""
    M, D = x.shape[0], W.shape[0]
    dev = x.device
    out = _e((M, D), F32, dev)
    kw = dict(bias=bias, res=res, res_scale=res_scale, drop_p=p_res, drop_seed=s_res)
    if post is not None:
        post.y1 = None
    row = post is not None and ROW_LN and K.row_ln_ok(x, W, D)
    if not row and not (post is not None and SPLITK_LN and post.nxt is None and x.dtype == torch.bfloat16
                        and W.shape[1] >= 1024):
        K.linear(x, W, out, **kw)
        return out
    post.y1, post.m1, post.r1 = _ln_bufs(M, D, F32 if post.f32 else x.dtype, dev)
    if not row:
        # the norm in the GEMM's split-K reduction launch (lasr_gemm_ln_fwd; two launches
        # when the plan does not split K)
        K.linear(x, W, out, ln_fwd=(post.g, post.b, LN_EPS, post.y1, post.m1, post.r1), **kw)
        return out
    if post.nxt is not None:
        post.y2, post.m2, post.r2 = _ln_bufs(M, D, x.dtype, dev)
        kw.update(g2=post.nxt.g, b2=post.nxt.b, y2=post.y2, mean2=post.m2, rstd2=post.r2)
    K.linear_res_ln(x, W, out, post.y1, post.m1, post.r1, post.g, post.b, LN_EPS, **kw)
    return out


class LnBwd:
    """The LayerNorm backward that consumes an input-gradient GEMM's output dln (the norm
    in front of a sub-block, liteasr/nets/conformer_layer.py:37-66), built from the norm's input
    x, its saved (mean, rstd), its weight and gradient namespaces and dx (fp32 out).  Fields: x,
    g (gamma), mean, rstd, dx, dgamma, dbeta, and optionally dres (fp32 residual gradient added),
    gb (+ bscale, bp, bseed: the preceding branch's gradient, layernorm_bwd's gb), chain (dx_ln)."""

    __slots__ = ("x", "g", "mean", "rstd", "dx", "dgamma", "dbeta", "dres", "gb", "bscale", "bp", "bseed", "chain")

    def __init__(self, x, st, w_ln, g_ln, dx, dres=None, gb=None, bscale=1.0, bp=0.0, bseed=0, chain=None):
        self.x, (self.mean, self.rstd), self.g, self.dx, self.dgamma, self.dbeta = x, st, w_ln.g, dx, g_ln.g, g_ln.b
        self.dres, self.gb, self.bscale, self.bp, self.bseed, self.chain = dres, gb, bscale, bp, bseed, chain


def dx_ln(dy, W, lnb):
    """dln = dy @ W ([M, K] x [K, D]); with `lnb` the LayerNorm backward of dln follows (one
    launch on the row kernel when it takes the shape) and None is returned, else dln.
    lnb.chain (an LnBwd on lnb.dx: the previous layer's final norm, ConformerLayerFn) runs
    right after it -- in the same launch as lnb's (lasr_layernorm2_bwd, lnb.dx never stored)
    when lnb is not on the row kernel."""
    M, D = dy.shape[0], W.shape[1]
    ch = lnb.chain if lnb is not None else None
    if lnb is not None and ROW_LN and K.row_ln_ok(dy, W, D) and lnb.x.dtype == F32 and lnb.dx.dtype == F32:
        K.linear_dx_ln_bwd(dy, W, lnb.x, lnb.g, lnb.mean, lnb.rstd, lnb.dx, lnb.dgamma, lnb.dbeta,
                           dres=lnb.dres, gb=lnb.gb, bscale=lnb.bscale, bp=lnb.bp, bseed=lnb.bseed)
        if ch is not None:
            ln_bwd_of(lnb.dx, ch)
        return None
    dln = _e((M, D), dy.dtype, dy.device)
    if ch is not None:
        assert lnb.gb is None and lnb.dres is not None and ch.dres is None and lnb.x.dtype == F32
        K.gemm(dy, W, dln)
        K.layernorm2_bwd(lnb.x, dln, lnb.dres, lnb.g, lnb.mean, lnb.rstd, lnb.dgamma, lnb.dbeta, ch.x, ch.g,
                         ch.mean, ch.rstd, ch.dx, ch.dgamma, ch.dbeta, gb2=ch.gb, bscale=ch.bscale, bp=ch.bp,
                         bseed=ch.bseed)
        return None
    if lnb is not None and SPLITK_LN and dy.dtype == torch.bfloat16 and W.shape[0] >= 1024:
        # the norm backward in the GEMM's split-K reduction launch (lasr_gemm_ln_bwd; two
        # launches when the plan does not split K)
        K.gemm(dy, W, dln, ln_bwd=lnb)
        return None
    K.gemm(dy, W, dln)
    if lnb is None:
        return dln
    ln_bwd_of(dln, lnb)
    return None


def ln_bwd_of(dln, lnb):
    """The LayerNorm backward `lnb` describes, on an already computed dln (the paths whose
    input-gradient GEMM is not the row kernel's: dx_ln does both in one launch)."""
    K.layernorm_bwd(lnb.x, dln, lnb.g, lnb.mean, lnb.rstd, lnb.dx, lnb.dgamma, lnb.dbeta, dres=lnb.dres,
                    gb=lnb.gb, bscale=lnb.bscale, bp=lnb.bp, bseed=lnb.bseed)


def after_norm_backward(enc, x, st, dh):
    """The encoder after_norm's backward, the tail of every heads node: its parameter gradients,
    its data-parallel unit reported, the residual stream's gradient (fp32) returned.  x, st: the
    norm's input and saved (mean, rstd); dh: fp32 gradient of its output."""
    we, ge = enc.after_norm_weights(), enc.after_norm_grads()
    dx = _e(x.shape, F32, x.device)
    K.layernorm_bwd(x, dh, we.g, *st, dx, ge.g, ge.b)
    enc.after_norm_ready()
    return dx


def ffn_forward(ln, ff, act, p_ff, s_ff, res, res_scale, p_res, s_res, post=None):
    """ff: the block's weights (W1, b1, W2, b2).  Returns (out, g, h).  g is the gate act'(u) *
    keep the backward needs, stored in the compute dtype by the fc1 epilogue (zout_mode 1):
    h = drop(act(u)) and g come out of the same launch, and the backward's dz GEMM multiplies by
    g (no recompute of u).  `post`: the LayerNorm after the residual add (res_proj)."""
    M, Fd = ln.shape[0], ff.W1.shape[0]
    dev, adt = ln.device, ln.dtype
    h = _e((M, Fd), adt, dev)
    g = _e((M, Fd), adt, dev)
    K.linear(ln, ff.W1, h, bias=ff.b1, act=act, zout=g, zout_mode=1, drop_p=p_ff, drop_seed=s_ff)
    out = res_proj(h, ff.W2, ff.b2, res, res_scale, p_res, s_res, post)
    return out, g, h


def ffn_backward(gb, ln, g, h, ff, gff, p_ff, lnb=None):
    """gb: gradient of the FFN output (after the residual-branch dropout/scale); g: the
    forward's stored gate act'(z) * keep; ff / gff: the block's weights and their gradients.
    Returns dln, or None when `lnb` (the norm in front of the FFN) consumed it (dx_ln)."""
    K.gemm(gb.t(), h, gff.W2, beta=1.0, split_k=0, rowsum=gff.b2, group=True)
    dz = _e((gb.shape[0], ff.W1.shape[0]), gb.dtype, gb.device)
    # dz = (gb W2) * scale * g: the dropout scale as alpha, the gate as aux
    K.gemm(gb, ff.W2, dz, alpha=K.dropout_scale(p_ff), aux=g, aux_act=ACT_GATE)
    K.gemm(dz.t(), ln, gff.W1, beta=1.0, split_k=0, rowsum=gff.b1, group=True)
    return dx_ln(dz, ff.W1, lnb)


def _heads(t, B, T, H, dk):
    """[B*T, H*dk] (row stride arbitrary) -> (B, H, T, dk) view."""
    return t.view(B, T, H, dk).permute(0, 2, 1, 3) if t.is_contiguous() else \
        t.unflatten(0, (B, T)).unflatten(2, (H, dk)).permute(0, 2, 1, 3)


def vocab_logits(x, W, b):
    """x W^T + b as [rows, V] padded rows (a view of [rows, roundup8(V)]) in x's dtype."""
    out = K.padded_rows(x.shape[0], W.shape[0], x.dtype, x.device)
    K.linear(x, W, out, bias=b)
    return out


# ============================================================ rel-pos MHSA ======
def fused_relattn(adt, dk, p_att):
    """The fused kernels (attn_flash.hip) cover bf16, d_k 32 or 64, no attention dropout
    (the my_U2 preset); other shapes take the materialised-score kernels."""
    return FUSED_RELATTN and adt == torch.bfloat16 and dk in (32, 64) and p_att == 0.0


def pos_projections(pos, Ws):
    """p_j = pos @ Wpos_j^T of every encoder layer in ONE batched GEMM (positional_encoding +
    attention.py:95 linear_pos; the table is the same for all layers): the layers' weights
    sit at a constant stride in the flat parameter store, so they form one strided batch.
    None when they do not (the layers then project their own)."""
    n = len(Ws)
    if n < 2 or not all(W.is_contiguous() for W in Ws):
        return None
    base = Ws[0].untyped_storage().data_ptr()
    if any(W.untyped_storage().data_ptr() != base for W in Ws):
        return None
    offs = [W.storage_offset() for W in Ws]
    st = offs[1] - offs[0]
    if st <= 0 or any(offs[j] - offs[0] != j * st for j in range(n)):
        return None
    dout, din = Ws[0].shape
    Wt = torch.as_strided(Ws[0], (n, din, dout), (st, 1, din), offs[0])  # W_j^T
    T = pos.shape[0]
    out = _e((n, T, dout), pos.dtype, pos.device)
    K.gemm(pos.unsqueeze(0).expand(n, T, din), Wt, out)
    return [out[j] for j in range(n)]


def _pos_heads(p, B, T, H, dk):
    """The positional projection p [T, H*dk] as a (B, H, T, dk) view, the same for every b."""
    return p.view(T, H, dk).permute(1, 0, 2).unsqueeze(0).expand(B, H, T, dk)


def relmha_forward(ln, pos, w, env, x_in, p_att, s_att, p_res, s_res, p=None, post=None):
    B, T, H = env.B, env.T, env.H
    d = ln.shape[1]
    dk = d // H
    dev, adt = ln.device, ln.dtype
    M = B * T
    scale = dk ** -0.5
    qkv = _e((M, 3 * d), adt, dev)
    K.linear(ln, w.Wqkv, qkv, bias=w.bqkv)
    if p is None:  # else precomputed for all layers at once (pos_projections)
        p = _e((T, d), adt, dev)
        K.linear(pos, w.Wpos, p)
    qu = _e((M, d), adt, dev)
    qv = _e((M, d), adt, dev)
    ctx = _e((M, d), adt, dev)
    P = Praw = stats = None
    if fused_relattn(adt, dk, p_att):
        # scores never materialised (attn_flash.hip); row stats kept for the backward; the
        # kernel forms qu / qv from q and the biases itself (lasr_relattn_fwd_qb)
        stats = _e((B * H * T * 2,), F32, dev)
        K.relattn_fwd_qb(qkv[:, :d], w.u, w.v, qu, qv, qkv[:, d:2 * d], qkv[:, 2 * d:], p, B, H, T, env.mask,
                         env.msb, env.msq, scale, stats, ctx)
    else:
        K.qbias_fwd(qkv, B, T, H, dk, w.u, w.v, qu, qv)
        ldS = ld_scores(T)
        Sac = _e((B, H, T, ldS), F32, dev)
        Sbd = _e((B, H, T, ldS), F32, dev)
        k4, v4 = _heads(qkv[:, d:2 * d], B, T, H, dk), _heads(qkv[:, 2 * d:], B, T, H, dk)
        K.gemm(_heads(qu, B, T, H, dk), k4.transpose(-1, -2), Sac[..., :T], alpha=scale)
        K.gemm(_heads(qv, B, T, H, dk), _pos_heads(p, B, T, H, dk).transpose(-1, -2), Sbd[..., :T], alpha=scale)
        P = _e((B, H, T, ldS), adt, dev)
        Praw = _e((B, H, T, ldS), adt, dev) if p_att > 0 else None
        K.attn_softmax_fwd(Sac, Sbd, B, H, T, T, ldS, env.mask, env.msb, env.msq, P, p_att, s_att, Praw)
        K.gemm(P[..., :T], v4, _heads(ctx, B, T, H, dk))
    out = res_proj(ctx, w.Wo, w.bo, x_in, 1.0, p_res, s_res, post)
    return out, SimpleNamespace(qkv=qkv, p=p, qu=qu, qv=qv, P=P, Praw=Praw, ctx=ctx, stats=stats)


def relmha_backward(gb, ln, pos, sv, w, g, env, p_att, s_att, lnb=None):
    B, T, H = env.B, env.T, env.H
    d = ln.shape[1]
    dk = d // H
    dev, adt = ln.device, ln.dtype
    M = B * T
    scale = dk ** -0.5
    ldS = ld_scores(T)
    K.gemm(gb.t(), sv.ctx, g.Wo, beta=1.0, split_k=0, rowsum=g.bo, group=True)
    dctx = _e((M, d), adt, dev)
    K.gemm(gb, w.Wo, dctx)
    dqkv = _e((M, 3 * d), adt, dev)
    dqu = _e((M, d), adt, dev)
    dqv = _e((M, d), adt, dev)
    dp = _e((T, d), adt, dev)
    p4 = _pos_heads(sv.p, B, T, H, dk)
    qb = (dqu, dqv, B, T, H, dk, dqkv, g.u, g.v)  # qbias_bwd: dq and the positional biases' gradients
    if sv.stats is not None:
        # fused recompute backward: dqu, dk, dv and the pre-shift bd gradient, head-major
        # ([H][B][T][ldS]) so the positional gradient is one K = B*T GEMM per head
        dBDh = _e((H, B, T, ldS), adt, dev)
        Dbuf = _e((B * H * T,), F32, dev)
        K.relattn_bwd(sv.qu, sv.qv, sv.qkv[:, d:2 * d], sv.qkv[:, 2 * d:], sv.p, B, H, T, env.mask,
                      env.msb, env.msq, scale, sv.stats, sv.ctx, dctx, Dbuf, dqu, dBDh, ldS,
                      dqkv[:, d:2 * d], dqkv[:, 2 * d:], dbd_head_major=True)
        K.gemm(dBDh.permute(1, 0, 2, 3)[..., :T], p4, _heads(dqv, B, T, H, dk), alpha=scale)
        # (qbias_bwd's blocks ride in this GEMM's split-K reduction launch: QBIAS_IN_REDUCE)
        qb_pending = not QBIAS_IN_REDUCE
        K.gemm(dBDh.view(H, B * T, ldS)[..., :T].transpose(-1, -2), sv.qv.view(M, H, dk).permute(1, 0, 2),
               dp.view(T, H, dk).permute(1, 0, 2), alpha=scale, split_k=0, qbias=None if qb_pending else qb)
    else:
        # materialised-score backward (fp32 build, attention dropout, other d_k)
        dBD = _e((B, H, T, ldS), adt, dev)
        dctx4 = _heads(dctx, B, T, H, dk)
        k4, v4 = _heads(sv.qkv[:, d:2 * d], B, T, H, dk), _heads(sv.qkv[:, 2 * d:], B, T, H, dk)
        dPd = _e((B, H, T, ldS), F32, dev)
        K.gemm(dctx4, v4.transpose(-1, -2), dPd[..., :T])
        K.gemm(sv.P[..., :T].transpose(-1, -2), dctx4, _heads(dqkv[:, 2 * d:], B, T, H, dk))
        dS = _e((B, H, T, ldS), adt, dev)
        K.attn_softmax_bwd(sv.Praw if sv.Praw is not None else sv.P, dPd, B, H, T, T, ldS, env.mask,
                           env.msb, env.msq, dS, p_att, s_att)
        K.relshift_bwd(dS.view(B * H, T, ldS), B * H, T, ldS, dBD)
        K.gemm(dS[..., :T], k4, _heads(dqu, B, T, H, dk), alpha=scale)
        K.gemm(dS[..., :T].transpose(-1, -2), _heads(sv.qu, B, T, H, dk), _heads(dqkv[:, d:2 * d], B, T, H, dk),
               alpha=scale)
        K.gemm(dBD[..., :T], p4, _heads(dqv, B, T, H, dk), alpha=scale)
        dpb = _e((B, H, T, dk), F32, dev)
        K.gemm(dBD[..., :T].transpose(-1, -2), _heads(sv.qv, B, T, H, dk), dpb, alpha=scale)
        K.reduce_batch(dpb, B, H, T, dk, dp)
        qb_pending = True
    if qb_pending:
        K.qbias_bwd(*qb)
    K.gemm(dp.t(), pos, g.Wpos, beta=1.0, split_k=0, group=True)
    K.gemm(dqkv.t(), ln, g.Wqkv, beta=1.0, split_k=0, rowsum=g.bqkv, group=True)
    return dx_ln(dqkv, w.Wqkv, lnb)


# ============================================================ plain MHA =========
def _fused_dec(adt, dk, p_att):
    return FUSED_DEC_ATTN and fused_relattn(adt, dk, p_att)


def mha_forward(ln, mem, w, B, Tq, Tk, H, mask, msb, msq, x_in, p_att, s_att, p_res, s_res, kv=None, post=None):
    """Decoder self (mem None) / source attention (liteasr/nets/attention.py:61-71).  kv: the
    memory's key/value projection [B*Tk, 2d] already computed (decoder_layers_fwd batches it
    over the layers); None computes it here.  post: the LayerNorm after the residual add, in
    the output projection's launch when the row kernel takes it (res_proj)."""
    d = ln.shape[1]
    dk = d // H
    dev, adt = ln.device, ln.dtype
    R = B * Tq
    scale = dk ** -0.5
    # the projections: q, k, v as column views of what the backward keeps
    qkv = qs = None
    if mem is None:
        qkv = _e((R, 3 * d), adt, dev)
        K.linear(ln, w.Wqkv, qkv, bias=w.bqkv)
        q, k, v, kv = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], None
    else:
        q = qs = _e((R, d), adt, dev)
        K.linear(ln, w.Wq, q, bias=w.bq)
        if kv is None:
            kv = _e((B * Tk, 2 * d), adt, dev)
            K.linear(mem, w.Wkv, kv, bias=w.bkv)
        k, v = kv[:, :d], kv[:, d:]
    ctx = _e((R, d), adt, dev)
    P = Praw = stats = None
    if _fused_dec(adt, dk, p_att):
        stats = _e((B * H * Tq * 2,), F32, dev)
        K.attn_fwd(q, k, v, B, H, Tq, Tk, mask, msb, msq, scale, stats, ctx)
    else:
        ldS = ld_scores(Tk)
        S = _e((B, H, Tq, ldS), F32, dev)
        K.gemm(_heads(q, B, Tq, H, dk), _heads(k, B, Tk, H, dk).transpose(-1, -2), S[..., :Tk], alpha=scale)
        P = _e((B, H, Tq, ldS), adt, dev)
        Praw = _e((B, H, Tq, ldS), adt, dev) if p_att > 0 else None
        K.attn_softmax_fwd(S, None, B, H, Tq, Tk, ldS, mask, msb, msq, P, p_att, s_att, Praw)
        K.gemm(P[..., :Tk], _heads(v, B, Tk, H, dk), _heads(ctx, B, Tq, H, dk))
    out = res_proj(ctx, w.Wo, w.bo, x_in, 1.0, p_res, s_res, post)
    return out, SimpleNamespace(qkv=qkv, q=qs, kv=kv, P=P, Praw=Praw, ctx=ctx, stats=stats)


def mha_backward(gb, ln, mem, sv, w, g, B, Tq, Tk, H, mask, msb, msq, p_att, s_att, dmem, dkv=None, lnb=None):
    """dkv: [B*Tk, 2d] destination of the key/value projection's gradient, whose weight /
    memory gradients the caller then computes (decoder_layers_bwd, batched over the layers);
    None computes them here (dmem accumulates).  lnb: the LayerNorm in front of the attention,
    whose backward the input-gradient GEMM runs (dx_ln; None is returned when it did)."""
    own_kv = dkv is None
    d = ln.shape[1]
    dk = d // H
    dev, adt = ln.device, ln.dtype
    R = B * Tq
    scale = dk ** -0.5
    K.gemm(gb.t(), sv.ctx, g.Wo, beta=1.0, split_k=0, rowsum=g.bo, group=True)
    dctx = _e((R, d), adt, dev)
    K.gemm(gb, w.Wo, dctx)
    # the core fills dq, dk, dv: column views of dqkv (self), or dq and dkv (source)
    if mem is None:
        dqkv = _e((R, 3 * d), adt, dev)
        q, k, v = sv.qkv[:, :d], sv.qkv[:, d:2 * d], sv.qkv[:, 2 * d:]
        dq, dkk, dv = dqkv[:, :d], dqkv[:, d:2 * d], dqkv[:, 2 * d:]
    else:
        dq = _e((R, d), adt, dev)
        if own_kv:
            dkv = _e((B * Tk, 2 * d), adt, dev)
        q, k, v = sv.q, sv.kv[:, :d], sv.kv[:, d:]
        dkk, dv = dkv[:, :d], dkv[:, d:]
    if sv.stats is not None:  # fused attention (mha_forward)
        Dbuf = _e((B * H * Tq,), F32, dev)
        K.attn_bwd(q, k, v, B, H, Tq, Tk, mask, msb, msq, scale, sv.stats, sv.ctx, dctx, Dbuf, dq, dkk, dv)
    else:
        ldS = ld_scores(Tk)
        dctx4 = _heads(dctx, B, Tq, H, dk)
        dPd = _e((B, H, Tq, ldS), F32, dev)
        K.gemm(dctx4, _heads(v, B, Tk, H, dk).transpose(-1, -2), dPd[..., :Tk])
        K.gemm(sv.P[..., :Tk].transpose(-1, -2), dctx4, _heads(dv, B, Tk, H, dk))
        dS = _e((B, H, Tq, ldS), adt, dev)
        K.attn_softmax_bwd(sv.Praw if sv.Praw is not None else sv.P, dPd, B, H, Tq, Tk, ldS, mask, msb,
                           msq, dS, p_att, s_att)
        K.gemm(dS[..., :Tk], _heads(k, B, Tk, H, dk), _heads(dq, B, Tq, H, dk), alpha=scale)
        K.gemm(dS[..., :Tk].transpose(-1, -2), _heads(q, B, Tq, H, dk), _heads(dkk, B, Tk, H, dk), alpha=scale)
    # the projections' weight gradients, then their input gradient (and the norm's backward)
    if mem is None:
        K.gemm(dqkv.t(), ln, g.Wqkv, beta=1.0, split_k=0, rowsum=g.bqkv, group=True)
        return dx_ln(dqkv, w.Wqkv, lnb)
    K.gemm(dq.t(), ln, g.Wq, beta=1.0, split_k=0, rowsum=g.bq, group=True)
    if own_kv:
        K.gemm(dkv.t(), mem, g.Wkv, beta=1.0, split_k=0, rowsum=g.bkv, group=True)
        K.gemm(dkv, w.Wkv, dmem, beta=1.0)
    return dx_ln(dq, w.Wq, lnb)


# ========================================================= conformer conv =======
def conv_forward(ln, w, env, x_in, p_res, s_res, training, post=None):
    B, T = env.B, env.T
    M, d = ln.shape
    dev, adt = ln.device, ln.dtype
    z1 = _e((M, 2 * d), adt, dev)
    K.linear(ln, w.Wpw1, z1, bias=w.bpw1)
    y = _e((M, d), adt, dev)
    nparts = K.dwconv_nparts(B, T)
    stats = _e(nparts * 3 * d, F32, dev)
    K.glu_dwconv_fwd(z1, B, T, d, w.kernel, w.wdw, w.bdw, y, stats)
    mean, rstd, scale, shift = (_e(d, F32, dev) for _ in range(4))
    K.bn_finalize(stats, nparts, d, 1e-5, 0.1, w.gamma, w.beta, w.rmean, w.rvar, w.nbt, mean, rstd,
                  scale, shift, 1 if training else 2)
    h3 = _e((M, d), adt, dev)
    K.bn_act_fwd(y, scale, shift, h3, act=w.act)
    out = res_proj(h3, w.Wpw2, w.bpw2, x_in, 1.0, p_res, s_res, post)
    return out, SimpleNamespace(z1=z1, y=y, mean=mean, rstd=rstd, scale=scale, shift=shift, h3=h3,
                                training=training)


def conv_backward(gb, ln, sv, w, g, env, lnb=None):
    B, T = env.B, env.T
    M, d = ln.shape
    dev, adt = ln.device, ln.dtype
    K.gemm(gb.t(), sv.h3, g.Wpw2, beta=1.0, split_k=0, rowsum=g.bpw2, group=True)
    dh3 = _e((M, d), adt, dev)
    K.gemm(gb, w.Wpw2, dh3)
    dz1 = _e((M, 2 * d), adt, dev)
    if BN_GLU_FUSED and d % 8 == 0:
        # the BN backward's dy computed inside the depthwise backward's window load (never stored)
        K.bn_act_glu_dwconv_bwd(sv.y, dh3, sv.scale, sv.shift, sv.mean, sv.rstd, w.gamma, g.gamma, g.beta, sv.z1,
                                B, T, d, w.kernel, w.wdw, dz1, g.wdw, g.bdw, batch_stats=sv.training, act=w.act)
    else:
        dy = _e((M, d), F32, dev)
        K.bn_act_bwd(sv.y, dh3, sv.scale, sv.shift, sv.mean, sv.rstd, w.gamma, g.gamma, g.beta, dy,
                     batch_stats=sv.training, act=w.act)
        K.glu_dwconv_bwd(sv.z1, dy, B, T, d, w.kernel, w.wdw, dz1, g.wdw, g.bdw)
    K.gemm(dz1.t(), ln, g.Wpw1, beta=1.0, split_k=0, rowsum=g.bpw1, group=True)
    return dx_ln(dz1, w.Wpw1, lnb)


def _conv2_implicit(adt, C):
    """conv2 on the implicit-GEMM instances (bf16 build, C % 128 == 0); the fp32 parity build
    and other widths take explicit im2col + the GEMM."""
    return adt == torch.bfloat16 and C % 128 == 0


# ============================================================ autograd nodes ====
@ranged
class EmbedConvFn(torch.autograd.Function):
    """Conv2DLayer's two convolutions (liteasr/nets/subsampling.py:42-46): y2 = relu(conv2(
    relu(conv1(x)))), channels-last, as [roundup32(M2 + 1), C] rows (the rows past M2 are the
    zero tail the implicit backward GEMMs read in dy2; EmbedOutFn's backward returns dy2 in
    that shape).  Its backward finishes conv2's and conv1's weight gradients and reports the
    data-parallel unit ``<embed>.conv``."""

    @staticmethod
    def forward(ctx, xs, anchor, mod, env):
        B, Tx, Fd = xs.shape
        w = mod.weights()
        C = w.C
        adt, dev = env.adt, xs.device
        T1, F1, T2, F2 = sub_dims(Tx, Fd)
        M2 = B * T2 * F2
        xs = xs.contiguous()
        y1 = _e((B, T1, F1, C), adt, dev)
        K.conv1_fwd(xs, w.W1, w.b1, y1)
        y2_full = _e((K.conv2_dy2_rows(M2), C), adt, dev)
        y2_full[M2:].zero_()  # the tail rows are part of the autograd output: defined (zero)
        y2 = y2_full[:M2]
        implicit = _conv2_implicit(adt, C)
        if implicit:  # conv2 as implicit GEMM: im2col(y1) is never materialised
            col = None
            K.conv2_fwd(y1, w.W2p, w.b2, y2)
        else:  # fp32 parity build: explicit im2col + GEMM
            col = _e((M2, 9 * C), adt, dev)
            K.im2col(y1, col)
            K.linear(col, w.W2p, y2, bias=w.b2, act=ACT_RELU)
        ctx.sv = SimpleNamespace(xs=xs, y1=y1, col=col, dims=(B, T1, F1, T2, F2, C), implicit=implicit)
        ctx.mod, ctx.env = mod, env
        return y2_full

    @staticmethod
    def backward(ctx, dy2_full):
        sv, mod = ctx.sv, ctx.mod
        B, T1, F1, T2, F2, C = sv.dims
        w, g = mod.weights(), mod.grads()
        M2 = B * T2 * F2
        dev = dy2_full.device
        # dW2 = dy2^T im2col(y1), implicit or against the stored columns
        dW2 = _e((C, 9 * C), F32, dev)
        if sv.implicit:
            K.conv2_dw(dy2_full, sv.y1, dW2, rowsum=g.b2)
        else:
            dy2 = dy2_full[:M2]
            K.gemm(dy2.t(), sv.col, dW2, split_k=0, rowsum=g.b2)
        K.permute_last2(dW2, C, C, 9, g.conv2_w, reverse=True, accumulate=True)
        if sv.implicit and K.conv2_dx_w1_ok(C):
            # dy1 = col2im(dy2 W2p) * relu'(y1) is consumed inside the data-gradient GEMM's
            # epilogue by conv1's weight gradient (never written or re-read)
            K.conv2_dx_w1(dy2_full, w.W2p, sv.y1, sv.xs, g.W1, g.b1)
        else:
            dy1 = torch.empty_like(sv.y1)
            if sv.implicit:
                K.conv2_dx(dy2_full, w.W2p, sv.y1, dy1)
            else:
                dcol = _e((M2, 9 * C), dy2.dtype, dev)
                K.gemm(dy2, w.W2p, dcol)
                K.col2im(dcol, sv.y1, dy1)
            K.conv1_bwd(sv.xs, dy1, g.W1, g.b1)
        mod.unit_ready("conv")
        return None, None, None, None


@ranged
class EmbedOutFn(torch.autograd.Function):
    """Conv2DLayer's output projection (subsampling.py:47-48) + RelativePositionalEncoding's
    x*sqrt(d) and dropout (positional_encoding.py:68-75).  The c-major flatten of the
    reference is folded into a column permutation of embed.out.weight (repacked working
    copy).  Its backward returns dy2 = (dx W_out) * relu'(y2) with the zero tail rows and
    reports the data-parallel unit ``<embed>.out`` before the convolutions' backward runs."""

    @staticmethod
    def forward(ctx, y2_full, anchor, mod, env):
        B, Tx, Fd = env.embed_in_shape
        w = mod.weights()
        C, d = w.C, w.d
        _, _, T2, F2 = sub_dims(Tx, Fd)
        dev = y2_full.device
        xl = _e((B * T2, d), F32, dev)
        y2f = y2_full[:B * T2 * F2].view(B * T2, F2 * C)
        K.linear(y2f, w.Woutp, xl, bias=w.bout)
        x0 = _e((B * T2, d), F32, dev)
        # relative PE: x * sqrt(d) (positional_encoding.py:68-75); absolute (use_rel False):
        # x * sqrt(d) + pe[t] (:49-56); dropout either way
        K.pe_fwd(xl, B * T2, T2, d, env.abs_pe, math.sqrt(d), x0, env.p_pos, env.seed + 1)
        ctx.sv = SimpleNamespace(y2_full=y2_full, dims=(B, T2, F2, C))
        ctx.mod, ctx.env = mod, env
        return x0

    @staticmethod
    def backward(ctx, dx0):
        sv, mod, env = ctx.sv, ctx.mod, ctx.env
        LayerLink.leftover(env.links)  # the first node below the stack: every hand-off was collected
        B, T2, F2, C = sv.dims
        w, g = mod.weights(), mod.grads()
        adt, dev = env.adt, dx0.device
        d = w.d
        M, M2 = B * T2, B * T2 * F2
        gb = _e((M, d), adt, dev)
        K.branch_grad(dx0.contiguous(), gb, math.sqrt(d), env.p_pos, env.seed + 1)
        y2f = sv.y2_full[:M2].view(M, F2 * C)
        dWo = _e((d, F2 * C), F32, dev)
        K.gemm(gb.t(), y2f, dWo, split_k=0, rowsum=g.bout)
        K.permute_last2(dWo, d, C, F2, g.out_w, reverse=True, accumulate=True)
        mod.unit_ready("out")
        # dy2 with its zero tail rows (the implicit GEMMs' K padding / out-of-range taps): one
        # buffer kept per subsampling module, its tail zeroed once when it is allocated (it is
        # produced here and consumed by EmbedConvFn.backward right after, in the same backward)
        key = (tuple(sv.y2_full.shape), adt, dev)
        if getattr(mod, "_dy2_key", None) != key:
            mod._dy2_buf = torch.zeros(sv.y2_full.shape, dtype=adt, device=dev)
            mod._dy2_key = key
        dy2_full = mod._dy2_buf
        K.gemm(gb, w.Woutp, dy2_full[:M2].view(M, F2 * C), aux=y2f, aux_act=ACT_RELU)
        return dy2_full, None, None, None


class EmbedFn:
    """The subsampling node (Conv2DLayer, subsampling.py:42-48, + the positional encoding's
    scale and dropout) as two autograd nodes, EmbedConvFn -> EmbedOutFn, so a segmented
    backward can launch the output projection's gradient bucket before the convolutions'
    backward runs (``cut``: the model's segment cut between them)."""

    @staticmethod
    def apply(xs, anchor, mod, env, cut=None):
        env.embed_in_shape = tuple(xs.shape)
        y2 = EmbedConvFn.apply(xs, mod.conv_anchor(), mod, env)
        if cut is not None:
            y2 = cut(y2)
        return EmbedOutFn.apply(y2, anchor, mod, env)


def enc_attn_forward(ln, pos, w, env, x_in, p_att, s_att, p_res, s_res, p=None, post=None):
    """An encoder layer's self-attention sub-block: relative-position attention
    (attention.py:120-154) when the layer has a positional projection, else the plain
    multi-head attention (:61-71) over the same key-padding / chunk mask (use_rel False)."""
    if w.Wpos is not None:
        return relmha_forward(ln, pos, w, env, x_in, p_att, s_att, p_res, s_res, p=p, post=post)
    if post is not None:
        post.y1 = None  # plain attention: the following norm runs on its own
    return mha_forward(ln, None, w, env.B, env.T, env.T, env.H, env.mask, env.msb, env.msq, x_in, p_att, s_att,
                       p_res, s_res)


def enc_attn_backward(gb, ln, pos, sv, w, g, env, p_att, s_att, lnb):
    if w.Wpos is not None:
        return relmha_backward(gb, ln, pos, sv, w, g, env, p_att, s_att, lnb=lnb)
    dln = mha_backward(gb, ln, None, sv, w, g, env.B, env.T, env.T, env.H, env.mask, env.msb, env.msq, p_att, s_att,
                       None)
    ln_bwd_of(dln, lnb)
    return None


@ranged
class ConformerLayerFn(torch.autograd.Function):
    """RelativeEncoderLayer.forward (liteasr/nets/conformer_layer.py:130-147), pre-norm."""

    @staticmethod
    def forward(ctx, x0, pos, anchor, layer, env):
        w = layer.weights()
        s = layer.seed
        pd, pff, pat = layer_rates(env)
        adt = env.adt
        x0 = x0.contiguous()
        link = _link(env, layer)
        # (a) macaron FFN, scale 0.5; its norm may have come with the previous layer's final one
        # (prev: that norm's (x4, mf, rf), for the chained backward)
        pre = link.take_first_norm(x0) if link is not None else None
        if pre is not None:
            ln_a, ma, ra, prev = pre
            sa = (ma, ra)
        else:
            (ln_a, sa), prev = norm_of(x0, w.ln_a, adt), None
        # every residual projection runs the following norm in its epilogue when the row
        # kernel takes the shape (res_proj); norm_of covers the rest
        pb_ = PostLN(w.ln_b)
        x1, za, ha = ffn_forward(ln_a, w.ffm, w.act, pff, _seed(s, 1), x0, 0.5, pd, _seed(s, 2), post=pb_)
        # (b) relative-position MHSA
        ln_b, sb = norm_of(x1, w.ln_b, adt, pb_)
        pc_ = PostLN(w.ln_c)
        x2, svb = enc_attn_forward(ln_b, pos, w.att, env, x1, pat, _seed(s, 3), pd, _seed(s, 4),
                                   p=link.pos_p if link is not None else None, post=pc_)
        # (c) convolution module
        ln_c, sc = norm_of(x2, w.ln_c, adt, pc_)
        pd_ = PostLN(w.ln_d)
        x3, svc = conv_forward(ln_c, w.conv, env, x2, pd, _seed(s, 5), env.training, post=pd_)
        # (d) FFN, scale 0.5
        ln_d, sd = norm_of(x3, w.ln_d, adt, pd_)
        # final LN -> next layer's residual stream (fp32); with the first norm of the layer above
        # chained (FUSED_LN2): in fc2's epilogue, or in one lasr_layernorm2_fwd launch
        up = link.above if link is not None and FUSED_LN2 and adt == torch.bfloat16 else None
        pf_ = PostLN(w.ln_f, f32=True, nxt=up.layer.weights().ln_a if up is not None else None)
        x4, zd, hd = ffn_forward(ln_d, w.ff, w.act, pff, _seed(s, 6), x3, 0.5, pd, _seed(s, 7), post=pf_)
        (x5, sf), first = final_norm(x4, pf_, adt)
        if up is not None:
            up.give_first_norm(x5, first[0], *first[1], x4, *sf)
        if torch.is_grad_enabled() or anchor.requires_grad:
            ctx.sv = SimpleNamespace(x=(x0, x1, x2, x3, x4), ln=(ln_a, ln_b, ln_c, ln_d), st=(sa, sb, sc, sd, sf),
                                     za=za, ha=ha, zd=zd, hd=hd, svb=svb, svc=svc, pos=pos,
                                     p=(pd, pff, pat), prev=prev)
        ctx.layer, ctx.env, ctx.link = layer, env, link
        return x5

    @staticmethod
    def backward(ctx, dx5):
        sv, layer, env = ctx.sv, ctx.layer, ctx.env
        w, g = layer.weights(), layer.grads()
        s = layer.seed
        pd, pff, pat = sv.p
        x0, x1, x2, x3, x4 = sv.x
        ln_a, ln_b, ln_c, ln_d = sv.ln
        sa, sb, sc, sd, sf = sv.st
        dev, adt = dx5.device, env.adt
        M, d = x4.shape
        # parameter-gradient reductions of the whole layer finish in one launch at the end (or,
        # held, with the layers below it in the same backward segment)
        link = ctx.link
        with K.deferred_reductions(hold=_hold(link), on_done=layer.on_grads_ready):
            # the layer above may have run this final norm's backward with its own first norm's
            # (LN2_BWD_CHAIN): dx5 is then the very dx4 tensor it produced, and gb came with it
            gb = link.take_final_grad(dx5) if link is not None else None
            dx5 = dx5.contiguous()
            if gb is not None:
                dx4 = dx5
            else:
                # final LN; emits the (d)-branch gradient 0.5*drop(dx4)
                dx4 = _e((M, d), F32, dev)
                gb = _e((M, d), adt, dev)
                ln_bwd_of(dx5, LnBwd(x4, sf, w.ln_f, g.ln_f, dx4, gb=gb, bscale=0.5, bp=pd, bseed=_seed(s, 7)))
            # each sub-block's input-gradient GEMM runs its norm's backward in its epilogue
            # (dx_ln); the branch-gradient buffers are fresh: grouped dW GEMMs read them at the
            # end of the node
            dx3 = _e((M, d), F32, dev)
            gb3 = _e((M, d), adt, dev)
            ffn_backward(gb, ln_d, sv.zd, sv.hd, w.ff, g.ff, pff,
                         lnb=LnBwd(x3, sd, w.ln_d, g.ln_d, dx3, dres=dx4, gb=gb3, bp=pd, bseed=_seed(s, 5)))
            dx2 = _e((M, d), F32, dev)
            gb2 = _e((M, d), adt, dev)
            conv_backward(gb3, ln_c, sv.svc, w.conv, g.conv, env,
                          lnb=LnBwd(x2, sc, w.ln_c, g.ln_c, dx2, dres=dx3, gb=gb2, bp=pd, bseed=_seed(s, 4)))
            dx1 = _e((M, d), F32, dev)
            gb1 = _e((M, d), adt, dev)
            enc_attn_backward(gb2, ln_b, sv.pos, sv.svb, w.att, g.att, env, pat, _seed(s, 3),
                              lnb=LnBwd(x1, sb, w.ln_b, g.ln_b, dx1, dres=dx2, gb=gb1, bscale=0.5, bp=pd,
                                        bseed=_seed(s, 2)))
            dx0 = _e((M, d), F32, dev)
            lnb_a = LnBwd(x0, sa, w.ln_a, g.ln_a, dx0, dres=dx1)
            pv = sv.prev if LN2_BWD_CHAIN else None
            if pv is not None:
                # the layer below's final norm on dx0 in the same launch: it receives dx4 / gb
                below = link.below.layer
                dx4p, gbp = _e((M, d), F32, dev), _e((M, d), adt, dev)
                lnb_a.chain = LnBwd(pv[0], pv[1:], below.weights().ln_f, below.grads().ln_f, dx4p, gb=gbp,
                                    bscale=0.5, bp=pd, bseed=_seed(below.seed, 7))
            ffn_backward(gb1, ln_a, sv.za, sv.ha, w.ffm, g.ffm, pff, lnb=lnb_a)
            if pv is not None:
                # autograd carries dx4p to that layer's node in place of this layer's input gradient
                link.below.give_final_grad(dx4p, gbp)
                dx0 = dx4p
        ctx.sv = None
        return dx0, None, None, None, None


@ranged
class TransformerLayerFn(torch.autograd.Function):
    """Transformer encoder layer (enc_arch "transformer"; liteasr/nets/transformer_layer.py:
    EncoderLayer.forward :64-76 / RelativeEncoderLayer.forward :119-136), pre-norm:
    x1 = x0 + drop(MHA(LN_b(x0))), x2 = x1 + drop(FFN(LN_d(x1))) -- no macaron half-step,
    no convolution module, no final norm (the encoder's after_norm follows the stack)."""

    @staticmethod
    def forward(ctx, x0, pos, anchor, layer, env):
        w = layer.weights()
        s = layer.seed
        pd, pff, pat = layer_rates(env)
        adt = env.adt
        x0 = x0.contiguous()
        link = _link(env, layer)
        ln_b, sb = norm_of(x0, w.ln_b, adt)
        pd_ = PostLN(w.ln_d)
        x1, svb = enc_attn_forward(ln_b, pos, w.att, env, x0, pat, _seed(s, 3), pd, _seed(s, 4),
                                   p=link.pos_p if link is not None else None, post=pd_)
        ln_d, sd = norm_of(x1, w.ln_d, adt, pd_)
        x2, zd, hd = ffn_forward(ln_d, w.ff, w.act, pff, _seed(s, 6), x1, 1.0, pd, _seed(s, 7))
        if torch.is_grad_enabled() or anchor.requires_grad:
            ctx.sv = SimpleNamespace(x=(x0, x1), ln=(ln_b, ln_d), st=(sb, sd), zd=zd, hd=hd, svb=svb,
                                     pos=pos, p=(pd, pff, pat))
        ctx.layer, ctx.env, ctx.link = layer, env, link
        return x2

    @staticmethod
    def backward(ctx, dx2):
        sv, layer, env = ctx.sv, ctx.layer, ctx.env
        w, g = layer.weights(), layer.grads()
        s = layer.seed
        pd, pff, pat = sv.p
        x0, x1 = sv.x
        ln_b, ln_d = sv.ln
        sb, sd = sv.st
        dev, adt = dx2.device, env.adt
        M, d = x1.shape
        dx2 = dx2.contiguous()
        with K.deferred_reductions(hold=_hold(ctx.link), on_done=layer.on_grads_ready):
            gb = _e((M, d), adt, dev)
            K.branch_grad(dx2, gb, 1.0, pd, _seed(s, 7))
            dx1 = _e((M, d), F32, dev)
            gb1 = _e((M, d), adt, dev)
            ffn_backward(gb, ln_d, sv.zd, sv.hd, w.ff, g.ff, pff,
                         lnb=LnBwd(x1, sd, w.ln_d, g.ln_d, dx1, dres=dx2, gb=gb1, bp=pd, bseed=_seed(s, 4)))
            dx0 = _e((M, d), F32, dev)
            enc_attn_backward(gb1, ln_b, sv.pos, sv.svb, w.att, g.att, env, pat, _seed(s, 3),
                              lnb=LnBwd(x0, sb, w.ln_b, g.ln_b, dx0, dres=dx1))
        ctx.sv = None
        return dx0, None, None, None, None


def _rows2d(g, rows):
    """(…, V) logits gradient -> [rows, V] view with unit column stride (padded row stride
    kept); anything else is made contiguous."""
    g2 = g.reshape(rows, g.shape[-1])
    return g2 if g2.stride(1) == 1 else g2.contiguous()


def decoder_layers_fwd(dec, wd, y, h, B, L1, T, masks, p, adt, seed_shift=0):
    """Decoder layers + after_norm + linear_out (transformer_decoder.py:84-93,
    transformer_layer.py:179-221; also ParallelDecoder, parallel_decoder.py:54-66) on the
    fp32 input rows y [B*L1, d]; memory h [B*T, d] (compute dtype).  masks = (self mask,
    its batch stride, its query stride (0: key padding), memory key mask); p = dropout
    rates (residual, ffn, self-attn, src-attn: decoder_rates).  Returns (h_attn [B*L1, V] padded
    rows, saved state for decoder_layers_bwd)."""
    smask, smsb, smsq, mmask = masks
    pd, pff, pat, pca = p
    layers_sv = []
    # every layer's source attention projects the same memory: its keys / values for all
    # layers are one GEMM against the cross-layer [n_layer * 2d, d] matrix (decoder_kv_groups)
    kvm = _e((B * T, len(wd.layers) * 2 * wd.d), adt, y.device)
    K.linear(h, wd.kv_all.W, kvm, bias=wd.kv_all.b)
    def post_ln(ln):  # the norm after a residual projection, in its launch (res_proj)
        return PostLN(ln) if DEC_ROW_LN else None

    nxt = None  # (l1, (m1, r1)) of the next layer, formed in this layer's fc2 launch
    for i, lw in enumerate(wd.layers):
        s = dec.dec_layers[i].seed + seed_shift
        l1, s1 = nxt if nxt is not None else norm_of(y, lw.ln1, adt)
        p2 = post_ln(lw.ln2)
        y1, sa = mha_forward(l1, None, lw.sa, B, L1, L1, wd.H, smask, smsb, smsq, y, pat, _seed(s, 1), pd,
                             _seed(s, 2), post=p2)
        l2, s2 = norm_of(y1, lw.ln2, adt, p2)
        p3 = post_ln(lw.ln3)
        y2, ca = mha_forward(l2, h, lw.ca, B, L1, T, wd.H, mmask, T, 0, y1, pca, _seed(s, 3), pd, _seed(s, 4),
                             kv=kvm[:, 2 * wd.d * i: 2 * wd.d * (i + 1)], post=p3)
        l3, s3 = norm_of(y2, lw.ln3, adt, p3)
        # the next norm (the next layer's first, or after_norm) after the FFN's residual add
        ln_n = wd.layers[i + 1].ln1 if i + 1 < len(wd.layers) else wd.ln_f
        p4 = PostLN(ln_n)
        y3, z, hh = ffn_forward(l3, lw.ff, ACT_RELU, pff, _seed(s, 5), y2, 1.0, pd, _seed(s, 6), post=p4)
        nxt = norm_of(y3, ln_n, adt, p4)
        layers_sv.append(SimpleNamespace(y=(y, y1, y2), ln=(l1, l2, l3), st=(s1, s2, s3), sa=sa, ca=ca, z=z, hh=hh))
        y = y3
    yf, sf = nxt if nxt is not None else norm_of(y, wd.ln_f, adt)
    return vocab_logits(yf, wd.Wout, wd.bout), SimpleNamespace(layers=layers_sv, yL=y, yf=yf, sf=sf, p=p, masks=masks, seed_shift=seed_shift)


def decoder_layers_bwd(g_attn, sv, dec, wd, gd, h, B, L1, T, dh, adt):
    """Backward of decoder_layers_fwd: parameter gradients into gd, the memory gradient
    accumulated into dh [B*T, d] fp32; returns the gradient of the input rows (fp32)."""
    smask, smsb, smsq, mmask = sv.masks
    pd, pff, pat, pca = sv.p
    dev = g_attn.device
    R, d = B * L1, wd.d
    K.gemm(g_attn.t(), sv.yf, gd.Wout, beta=1.0, split_k=0, rowsum=gd.bout)
    dyf = _e((R, d), adt, dev)
    K.gemm(g_attn, wd.Wout, dyf)
    dy = _e((R, d), F32, dev)
    nl = len(wd.layers)
    # the FFN branch gradient of each layer (its residual dropout's backward, seed 6 of the
    # layer) comes out of the LayerNorm backward that produces the layer's output gradient:
    # the final norm's for the top layer, the next layer's first norm's below (no separate
    # branch_grad launch; same product per element)
    ffn_seed = lambda i: _seed(dec.dec_layers[i].seed + sv.seed_shift, 6)  # noqa: E731
    fused_gb = DEC_GB_IN_LN
    gb_next = _e((R, d), adt, dev) if fused_gb else None
    ln_bwd_of(dyf, LnBwd(sv.yL, sv.sf, wd.ln_f, gd.ln_f, dy, gb=gb_next, bp=pd, bseed=ffn_seed(nl - 1)))
    dkvm = _e((B * T, nl * 2 * d), adt, dev)  # the batched memory K/V's gradient
    for i in range(nl - 1, -1, -1):
        lw, lg, ls = wd.layers[i], gd.layers[i], sv.layers[i]
        s = dec.dec_layers[i].seed + sv.seed_shift
        y0, y1, y2 = ls.y
        l1, l2, l3 = ls.ln
        s1, s2, s3 = ls.st
        # fresh gb per branch: the grouped dW GEMMs read it at the end of the node
        gb = gb_next
        if not fused_gb:  # the separate branch-gradient launch (kept for the bit-identity test)
            gb = _e((R, d), adt, dev)
            K.branch_grad(dy, gb, 1.0, pd, ffn_seed(i))
        dy2 = _e((R, d), F32, dev)
        gb3 = _e((R, d), adt, dev)
        ffn_backward(gb, l3, ls.z, ls.hh, lw.ff, lg.ff, pff,
                     lnb=LnBwd(y2, s3, lw.ln3, lg.ln3, dy2, dres=dy, gb=gb3, bp=pd, bseed=_seed(s, 4)))
        # the norms in front of the two attentions run in their input-gradient GEMMs (dx_ln) on
        # the row kernel, else (None returned: not consumed) as their own launch
        dy1 = _e((R, d), F32, dev)
        gb1 = _e((R, d), adt, dev)
        lnb2 = LnBwd(y1, s2, lw.ln2, lg.ln2, dy1, dres=dy2, gb=gb1, bp=pd, bseed=_seed(s, 2))
        dln = mha_backward(gb3, l2, h, ls.ca, lw.ca, lg.ca, B, L1, T, wd.H, mmask, T, 0, pca, _seed(s, 3), dh,
                           dkv=dkvm[:, 2 * d * i: 2 * d * (i + 1)], lnb=lnb2 if DEC_ROW_LN else None)
        if dln is not None:
            ln_bwd_of(dln, lnb2)
        dy0 = _e((R, d), F32, dev)
        gb_next = _e((R, d), adt, dev) if i > 0 and fused_gb else None
        lnb1 = LnBwd(y0, s1, lw.ln1, lg.ln1, dy0, dres=dy1, gb=gb_next, bp=pd if gb_next is not None else 0.0,
                     bseed=ffn_seed(i - 1) if gb_next is not None else 0)
        dln = mha_backward(gb1, l1, None, ls.sa, lw.sa, lg.sa, B, L1, L1, wd.H, smask, smsb, smsq, pat,
                           _seed(s, 1), None, lnb=lnb1 if DEC_ROW_LN else None)
        if dln is not None:
            ln_bwd_of(dln, lnb1)
        dy = dy0
    K.gemm(dkvm.t(), h, gd.kv_all.W, beta=1.0, split_k=0, rowsum=gd.kv_all.b, group=True)
    K.gemm(dkvm, wd.kv_all.W, dh, beta=1.0)
    return dy


@ranged
class HeadsFn(torch.autograd.Function):
    """Encoder after_norm (transformer_encoder.py:126), CTC head with its always-on
    input dropout (ctc.py:28-30) and the full Transformer decoder
    (transformer_decoder.py:70-93, transformer_layer.py:179-221)."""

    @staticmethod
    def forward(ctx, x, anchor, model, env):
        dev, adt = x.device, env.adt
        enc, dec = model.encoder, model.decoder
        B, T, L1 = env.B, env.T, env.L1
        R = B * L1
        tr = env.training
        x = x.contiguous()
        we = enc.after_norm_weights()
        h, hd, me, re = ln_forward(x, we.g, we.b, adt, y2=True, p2=env.p_ctc, seed2=env.seed + 2)
        wc = model.ctc.weights()
        h_ctc = vocab_logits(hd, wc.W, wc.b)
        # ---- decoder
        wd = dec.weights()
        d = wd.d
        y = _e((R, d), F32, dev)
        K.embed_pe_fwd(env.ys_in, L1, wd.E, wd.pe, math.sqrt(d), y, env.p_dec_pos if tr else 0.0,
                       env.seed + 3)
        masks = (env.dec_mask, env.dec_mask.stride(0), env.dec_mask.stride(1), env.mask_k)
        h_attn, dsv = decoder_layers_fwd(dec, wd, y, h, B, L1, T, masks, decoder_rates(dec, tr), adt)
        ctx.sv = SimpleNamespace(x=x, h=h, hd=hd, st=(me, re), dec=dsv)
        ctx.model, ctx.env = model, env
        return h_attn, h_ctc

    @staticmethod
    def backward(ctx, g_attn, g_ctc):
        sv, model, env = ctx.sv, ctx.model, ctx.env
        enc, dec = model.encoder, model.decoder
        dev, adt = sv.x.device, env.adt
        B, T, L1 = env.B, env.T, env.L1
        M, R = B * T, B * L1
        d_enc = sv.x.shape[1]
        dh = _e((M, d_enc), F32, dev)  # accumulated gradient of h_enc
        # ---- CTC head
        wc, gc = model.ctc.weights(), model.ctc.grads()
        if g_ctc is not None:
            g_ctc = _rows2d(g_ctc, M)
            K.gemm(g_ctc.t(), sv.hd, gc.W, beta=1.0, split_k=0, rowsum=gc.b)
            dhd = _e((M, d_enc), F32, dev)
            K.gemm(g_ctc, wc.W, dhd)
            K.branch_grad(dhd, dh, 1.0, env.p_ctc, env.seed + 2)
        else:
            K.fill(dh, 0.0)
        model.ctc.on_grads_ready()
        # ---- decoder
        wd, gd = dec.weights(), dec.grads()
        d = wd.d
        with K.deferred_reductions():  # decoder parameter-gradient reductions: one launch
            if g_attn is not None:
                dy = decoder_layers_bwd(_rows2d(g_attn, R), sv.dec, dec, wd, gd, sv.h, B, L1, T, dh, adt)
                K.embed_bwd(env.ys_in, dy, math.sqrt(d), gd.E, env.p_dec_pos if env.training else 0.0,
                            env.seed + 3)
        dec.on_grads_ready()
        dx = after_norm_backward(enc, sv.x, sv.st, dh)
        ctx.sv = None
        return dx, None, None, None


@ranged
class EncoderOutFn(torch.autograd.Function):
    """Encoder after_norm (transformer_encoder.py:126) as its own autograd node, for heads
    other than U2's HeadsFn (encoder reuse, SURVEY §8 f4: Transducer / Paraformer heads
    consume `self.encoder(xs, mask)`, transducer.py:128, paraformer.py:96).  Returns the
    fp32 encoder output; backward writes the after_norm parameter gradients and hands
    dx to the conformer layers' fused backward."""

    @staticmethod
    def forward(ctx, x, anchor, model, adt):
        x = x.contiguous()
        we = model.encoder.after_norm_weights()
        h, mean, rstd = _ln_bufs(*x.shape, F32, x.device)
        K.layernorm_fwd(x, we.g, we.b, LN_EPS, h, mean, rstd)
        ctx.sv = (x, (mean, rstd))
        ctx.model = model
        return h

    @staticmethod
    def backward(ctx, dh):
        x, st = ctx.sv
        dx = after_norm_backward(ctx.model.encoder, x, st, dh.float().contiguous())
        ctx.sv = None
        return dx, None, None, None
