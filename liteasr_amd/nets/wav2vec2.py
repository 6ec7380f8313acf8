"""wav2vec 2.0 on the HIP kernels: parameter containers that mirror the reference's modules
(liteasr/nets/wav2vec2_convolution.py, gumbel_vector_quantizer.py, transformer_encoder.py:130-193)
and the fused forward / backward stages built on csrc/w2v.hip and the GEMM.

Stages (each a plain forward / backward pair over tensors, so tests drive them one by one):
  ext_layer_*   Conv1d -> Fp32LayerNorm -> GELU of the feature extractor, channels-last.  Layers
                >= 1 are GEMMs over a strided, overlapping view of the activation (row t = the
                k C contiguous elements from row s t): no im2col buffer.
  posconv_*     grouped positional convolution through the same kind of view on a group-major,
                time-padded copy; GELU + residual fused in the unpack kernel.
  W2VFrontFn    extractor, layer_norm, linear_input, mask embedding, positional convolution,
                embed_norm, dropout, and the (B, T') -> (T', B) hand-off to the encoder layers.
  W2VHeadFn     masked-row gathers, linear_final, weight_proj + Gumbel quantizer +
                linear_quantizer, contrastive logits and the cross-entropy.

As everywhere in nets/functional.py, weight gradients accumulate straight into the flat fp32
gradient buffer; autograd only carries activations' gradients between the nodes.
"""

from __future__ import annotations

from types import SimpleNamespace

import torch
import torch.nn as nn

from .. import kernels as K
from .functional import LN_EPS, _seed
from .modules import LayerNorm, MultiHeadAttention, PositionwiseFeedForward, TransformerEncoderLayer, _Bound

F32 = torch.float32
EXT_LN_EPS = 1e-5  # Fp32LayerNorm keeps nn.LayerNorm's default (liteasr/nets/layer_norm.py:32-34)
POS_KERNEL, POS_GROUPS = 128, 16  # hard-coded in the reference (transformer_encoder.py:147-149)


def _e(shape, dtype, dev):
    return torch.empty(shape, dtype=dtype, device=dev)


# ============================================================ parameter containers ===
class ConvolutionBlock(nn.Module):
    """wav2vec2_convolution.py:9-32.  For n_in > 1 the weight parameter is kept (n_out, k, n_in)
    -- the GEMM's [N][K] operand over channels-last rows -- after the reference's draws on the
    (n_out, n_in, k) tensor; Wav2Vec2.state_dict() presents the reference's shape."""

    def __init__(self, n_in, n_out, kernel, stride, conv_bias=False, dropout_rate=0.0):
        super().__init__()
        self.conv = nn.Conv1d(n_in, n_out, kernel, stride, bias=conv_bias)
        self.dropout = nn.Dropout(p=dropout_rate)
        self.layer_norm = nn.LayerNorm(n_out, elementwise_affine=True)
        self.gelu = nn.GELU()
        nn.init.kaiming_normal_(self.conv.weight)
        self.kernel, self.stride, self.n_in, self.n_out = kernel, stride, n_in, n_out
        if n_in > 1:
            self.conv.weight = nn.Parameter(self.conv.weight.detach().permute(0, 2, 1).contiguous())


class Convolution(nn.Module):
    """wav2vec2_convolution.py:35-84."""

    def __init__(self, conv_layers, conv_bias=False, dropout_rate=0.0):
        super().__init__()
        in_d = 1
        self.conv_layers = nn.ModuleList()
        for dim, kernel, stride in conv_layers:
            self.conv_layers.append(ConvolutionBlock(in_d, dim, kernel, stride, conv_bias=conv_bias,
                                                     dropout_rate=dropout_rate))
            in_d = dim

    def out_frames(self, n):
        for blk in self.conv_layers:
            n = (n - blk.kernel) // blk.stride + 1
        return n


class GumbelVectorQuantizer(nn.Module):
    """gumbel_vector_quantizer.py:11-62; the temperature never decays (curr_temp stays at
    temp[0], as in the reference's forward)."""

    def __init__(self, dim, num_vars, temp, groups, vq_dim, combine_groups=False):
        super().__init__()
        assert not combine_groups, "the model builds the quantizer with combine_groups=False"
        assert vq_dim % groups == 0, f"dim {vq_dim} must be divisible by {groups} for concatenation"
        self.groups, self.num_vars, self.input_dim, self.var_dim = groups, num_vars, dim, vq_dim // groups
        self.vars = nn.Parameter(torch.FloatTensor(1, groups * num_vars, self.var_dim))
        nn.init.uniform_(self.vars)
        self.weight_proj = nn.Linear(dim, groups * num_vars)
        nn.init.normal_(self.weight_proj.weight, mean=0, std=1)
        nn.init.zeros_(self.weight_proj.bias)
        if isinstance(temp, str):
            import ast

            temp = ast.literal_eval(temp)
        assert len(temp) == 3, f"{temp}, {len(temp)}"
        self.max_temp, self.min_temp, self.temp_decay = temp
        self.curr_temp = self.max_temp


class Wav2Vec2TansformerEncoder(_Bound):
    """transformer_encoder.py:130-173 (the reference's spelling)."""

    def __init__(self, i_dim, h_dim, ff_dim, n_head, n_layer, dropout_rate, attn_dropout_rate, ff_dropout_rate):
        super().__init__()
        self.dropout_rate = dropout_rate
        self.embed = nn.Conv1d(i_dim, i_dim, kernel_size=POS_KERNEL, padding=POS_KERNEL // 2, groups=POS_GROUPS)
        self.gelu = nn.GELU()
        self.embed_norm = LayerNorm(i_dim)
        self.enc_layers = nn.ModuleList([
            TransformerEncoderLayer(
                size=i_dim,
                self_attn=MultiHeadAttention(n_head, h_dim, attn_dropout_rate),
                feed_forward=PositionwiseFeedForward(h_dim, ff_dim, dropout_rate=ff_dropout_rate),
                dropout_rate=dropout_rate,
            ) for _ in range(n_layer)
        ])
        self.h_dim, self.n_head = h_dim, n_head
        self.rates = SimpleNamespace(drop=dropout_rate, att=attn_dropout_rate, ff=ff_dropout_rate)


# ================================================================ extractor layer ===
def _overlap(a, k, s):
    """(B, T_out, k C) view of a contiguous (B, T_in, C): row t starts at row s t."""
    B, Tin, C = a.shape
    assert a.is_contiguous()
    return torch.as_strided(a, (B, (Tin - k) // s + 1, k * C), (Tin * C, s * C, 1), a.storage_offset())


def _bexp(m, *lead):
    return m.expand(*lead, *m.shape[-2:])


def ext_layer_fwd(a, W, bias, gamma, beta, k, s, adt):
    """a: waveform (B, T_in) fp32 (layer 0, W (C, k) fp32) or activation (B, T_in, C_in) in the
    compute dtype (W (C, k C_in) compute dtype).  Returns (y (B, T_out, C) compute dtype, saved)."""
    dev = a.device
    C = W.shape[0]
    if a.dim() == 2:
        B, Tin = a.shape
        Tout = (Tin - k) // s + 1
        u = _e((B, Tout, C), F32, dev)
        K.w2v_conv0_fwd(a, W, bias, k, s, u)
    else:
        A = _overlap(a, k, s)
        B, Tout = A.shape[0], A.shape[1]
        u = _e((B, Tout, C), F32, dev)
        K.gemm(A, _bexp(W.t(), B), u, bias=bias)
    y = _e((B, Tout, C), adt, dev)
    mean, rstd = _e(B * Tout, F32, dev), _e(B * Tout, F32, dev)
    K.w2v_ln_act_fwd(u, gamma, beta, EXT_LN_EPS, 1, y, mean, rstd)
    return y, (a, u, mean, rstd)


def ext_layer_bwd(dy, sv, W, gamma, beta, k, s, adt, gW, gbias, ggamma, gbeta):
    """dy (B, T_out, C) fp32.  Accumulates the parameter gradients; returns da (B, T_in, C_in)
    fp32, or None for layer 0 (no gradient reaches the waveform)."""
    a, u, mean, rstd = sv
    dev = dy.device
    B, Tout, C = u.shape
    du = _e(u.shape, adt, dev)
    K.w2v_ln_act_bwd(u, dy, gamma, beta, mean, rstd, 1, du, ggamma, gbeta)
    if gbias is not None:
        K.colsum(du.view(-1, C), gbias)
    if a.dim() == 2:
        K.w2v_conv0_dw(a, du, k, s, gW)
        return None
    A = _overlap(a, k, s)
    for b in range(B):  # fixed batch order
        K.gemm(du[b].t(), A[b], gW, beta=1.0)
    dcol = _e(A.shape, adt, dev)
    K.gemm(du, _bexp(W, B), dcol)
    da = _e(a.shape, F32, dev)
    K.w2v_col2im1d(dcol, a.shape[1], a.shape[2], k, s, da)
    return da


# ======================================================== positional convolution ===
def _pos_view(xg, T, k):
    G, B, Tp, cg = xg.shape
    return torch.as_strided(xg, (G, B, T, k * cg), (B * Tp * cg, Tp * cg, cg, 1), xg.storage_offset())


def posconv_fwd(x, W, bias, adt, k=POS_KERNEL, G=POS_GROUPS):
    """x (B, T, d) fp32, W (d, d / G, k) fp32 (the reference's Conv1d layout), bias (d,):
    x + GELU(conv(x)[:, :T]) (transformer_encoder.py:176-179), fp32."""
    B, T, d = x.shape
    cg = d // G
    dev = x.device
    Tp = T + k
    xg = _e((G, B, Tp, cg), adt, dev)
    K.w2v_group_pack(x, G, k // 2, xg)
    Wk = W.view(G, cg, cg, k).permute(0, 1, 3, 2).contiguous().to(adt).view(G, 1, cg, k * cg)  # [g][o][(j, i)]
    yg = _e((G, B, T, cg), F32, dev)
    K.gemm(_pos_view(xg, T, k), _bexp(Wk.transpose(-1, -2), G, B), yg)
    out = _e((B, T, d), F32, dev)
    K.w2v_group_unpack(yg, bias, 1, x, out)
    return out, (xg, yg)


def posconv_bwd(dout, sv, W, bias, adt, gW, gbias, k=POS_KERNEL, G=POS_GROUPS):
    """dout (B, T, d) fp32 -> dx (B, T, d) fp32 (residual included); gW (d, d / G, k), gbias +=."""
    xg, yg = sv
    B, T, d = dout.shape
    cg = d // G
    dev = dout.device
    Tp = T + k
    front = k - 1 - k // 2
    dyg = _e((G, B, Tp, cg), adt, dev)
    K.w2v_group_pack(dout, G, front, dyg, yg=yg, bias=bias)
    K.w2v_group_colsum(dyg, gbias)
    gk = torch.zeros(G, cg, k * cg, dtype=F32, device=dev)
    A = _pos_view(xg, T, k)
    dY = dyg[:, :, front:front + T]
    for b in range(B):  # fixed batch order
        K.gemm(dY[:, b].transpose(-1, -2), A[:, b], gk, beta=1.0)
    gW.view(G, cg, cg, k).add_(gk.view(G, cg, k, cg).permute(0, 1, 3, 2))
    # dx is the same convolution of dY with the taps reversed and (o, i) exchanged
    Wf = W.view(G, cg, cg, k).flip(-1).permute(0, 3, 1, 2).contiguous().to(adt).view(G, 1, k * cg, cg)
    dxg = _e((G, B, T, cg), F32, dev)
    K.gemm(_pos_view(dyg, T, k), _bexp(Wf, G, B), dxg)
    dx = _e((B, T, d), F32, dev)
    K.w2v_group_unpack(dxg, None, 0, dout, dx)
    return dx


# ==================================================================== helpers ===
def _linear_bwd(dy32, x, W, gW, gb, adt, need_dx=True):
    """y = x W^T + b: gW += dy^T x, gb += colsum(dy); returns dx fp32 (or None)."""
    dy = dy32 if dy32.dtype == adt else _e(dy32.shape, adt, dy32.device)
    if dy is not dy32:
        K.cast(dy32, dy)
    K.gemm(dy.t(), x, gW, beta=1.0)
    K.colsum(dy32, gb)
    if not need_dx:
        return None
    dx = _e((dy.shape[0], W.shape[1]), F32, dy.device)
    K.gemm(dy, W, dx)
    return dx


def _drop(x, p, seed):
    """x -> dropout(x) with the library's counter hash (the same call regenerates the mask in
    the backward)."""
    if p <= 0.0:
        return x
    y = torch.empty_like(x)
    K.branch_grad(x, y, 1.0, p, seed)
    return y


# ====================================================================== front ===
class W2VFrontFn(torch.autograd.Function):
    """wav2vec2.py:272-285 and transformer_encoder.py:175-188: source (B, S) fp32 ->
    (x (T' B, d) fp32 in (T', B) order for the encoder layers, feats (B T', C) fp32 = the
    unmasked features)."""

    @staticmethod
    def forward(ctx, source, anchor, model, st):
        w = model.front_weights()
        adt, dev, tr = st.adt, source.device, st.training
        a = source.contiguous().float()
        saved = []
        for lw in w.ext:
            a, sv = ext_layer_fwd(a, lw.W, lw.b, lw.g, lw.beta, lw.k, lw.s, adt)
            saved.append(sv)
        B, T, C = a.shape
        feats = _e((B * T, C), F32, dev)
        fm, fr = _e(B * T, F32, dev), _e(B * T, F32, dev)
        K.w2v_ln_act_fwd(a, w.ln.g, w.ln.b, LN_EPS, 0, feats, fm, fr)
        d = w.d
        if w.Wi is not None:
            fa = feats if adt == F32 else _e((B * T, C), adt, dev)
            if fa is not feats:
                K.cast(feats, fa)
            h = _e((B * T, d), F32, dev)
            K.linear(fa, w.Wi, h, bias=w.bi)
        else:
            fa, h = None, feats.clone()
        h = _drop(h, st.p_in if tr else 0.0, _seed(st.seed, 1))
        h3 = h.view(B, T, d)
        if st.midx is not None:
            K.w2v_mask_fwd(h3, st.midx, w.mask_emb)
        xr, svp = posconv_fwd(h3, w.Wpos, w.bpos, adt)
        y = _e((B * T, d), F32, dev)
        ym, yr = _e(B * T, F32, dev), _e(B * T, F32, dev)
        K.layernorm_fwd(xr.view(B * T, d), w.en.g, w.en.b, LN_EPS, y, ym, yr)
        y = _drop(y, st.p_drop if tr else 0.0, _seed(st.seed, 2))
        x = y.view(B, T, d).transpose(0, 1).contiguous().view(T * B, d)
        ctx.sv = SimpleNamespace(ext=saved, a=a, fm=fm, fr=fr, fa=fa, svp=svp, xr=xr, ym=ym, yr=yr, B=B, T=T)
        ctx.model, ctx.st = model, st
        return x, feats

    @staticmethod
    def backward(ctx, dx, dfeats):
        sv, model, st = ctx.sv, ctx.model, ctx.st
        w, g = model.front_weights(), model.front_grads()
        adt, dev, tr = st.adt, dx.device, st.training
        B, T, d = sv.B, sv.T, w.d
        dy = dx.reshape(T, B, d).transpose(0, 1).contiguous().view(B * T, d)
        dy = _drop(dy, st.p_drop if tr else 0.0, _seed(st.seed, 2))
        dxr = _e((B * T, d), F32, dev)
        K.layernorm_bwd(sv.xr.view(B * T, d), dy, w.en.g, sv.ym, sv.yr, dxr, g.en.g, g.en.b)
        dh = posconv_bwd(dxr.view(B, T, d), sv.svp, w.Wpos, w.bpos, adt, g.Wpos, g.bpos)
        if st.midx is not None:
            K.w2v_mask_bwd(dh, st.midx, g.mask_emb)
        dh = _drop(dh.view(B * T, d), st.p_in if tr else 0.0, _seed(st.seed, 1))
        if w.Wi is not None:
            df = _linear_bwd(dh, sv.fa, w.Wi, g.Wi, g.bi, adt)
        else:
            df = dh
        if dfeats is not None:
            df = df + dfeats.reshape(B * T, -1)
        da = _e(sv.a.shape, F32, dev)
        K.w2v_ln_act_bwd(sv.a, df, w.ln.g, w.ln.b, sv.fm, sv.fr, 0, da, g.ln.g, g.ln.b)
        for lw, lg, s in zip(reversed(w.ext), reversed(g.ext), reversed(sv.ext)):
            da = ext_layer_bwd(da, s, lw.W, lw.g, lw.beta, lw.k, lw.s, adt, lg.W, lg.b, lg.g, lg.beta)
        ctx.sv = None
        return None, None, None, None


# ======================================================================= head ===
class W2VHeadFn(torch.autograd.Function):
    """wav2vec2.py:289-315 + the cross-entropy of criterions/wav2vec_loss.py: x (T' B, d) fp32
    (the encoder layers' output, (T', B) order), feats (B T', C) fp32 -> (logits (M B, N + 1),
    loss ()).  Gradients flow from the loss; the logits are an output for inspection only."""

    @staticmethod
    def forward(ctx, x, feats, anchor, model, st):
        w = model.head_weights()
        adt, dev, tr = st.adt, x.device, st.training
        B, T, M, N = st.B, st.T, st.midx.shape[1], st.N
        d, C = x.shape[1], feats.shape[1]
        xe = _e((B, M, d), adt, dev)
        K.w2v_gather_rows(x.contiguous().view(T, B, d), st.midx, xe, time_major=True)
        Fd = w.Wf.shape[0]
        xf = _e((B * M, Fd), F32, dev)
        K.linear(xe.view(B * M, d), w.Wf, xf, bias=w.bf)
        ym = _e((B, M, C), adt, dev)
        K.w2v_gather_rows(feats.contiguous().view(B, T, C), st.midx, ym)
        ym = _drop(ym, st.p_feat if tr else 0.0, _seed(st.seed, 3)).view(B * M, C)
        G, V = w.G, w.V
        lg = _e((B * M, G * V), F32, dev)
        K.linear(ym, w.Wp, lg, bias=w.bp)
        q = _e((B * M, G * w.vars.shape[-1]), adt, dev)
        codes = _e((B * M, G), torch.int32, dev)
        K.w2v_gumbel_fwd(lg, G, w.vars, w.tau, not tr, q, codes, noise=st.noise, seed=_seed(st.seed, 4))
        yq = _e((B * M, Fd), F32, dev)
        K.linear(q, w.Wq, yq, bias=w.bq)
        logits = _e((M * B, N + 1), F32, dev)
        lse, row_loss = _e(B * M, F32, dev), _e(B * M, F32, dev)
        loss = _e((), F32, dev)
        K.w2v_contrast_fwd(xf.view(B, M, Fd), yq.view(B, M, Fd), st.neg, codes, N, w.temp, logits, lse, row_loss, loss)
        ctx.sv = SimpleNamespace(xe=xe, xf=xf, ym=ym, lg=lg, q=q, codes=codes, yq=yq, lse=lse, C=C, d=d)
        ctx.model, ctx.st = model, st
        ctx.mark_non_differentiable(logits)
        st.codes = codes
        return logits, loss

    @staticmethod
    def backward(ctx, _dlogits, dloss):
        sv, model, st = ctx.sv, ctx.model, ctx.st
        w, g = model.head_weights(), model.head_grads()
        adt, dev, tr = st.adt, dloss.device, st.training
        B, T, M, N = st.B, st.T, st.midx.shape[1], st.N
        Fd, G = w.Wf.shape[0], w.G
        dxf, dyq = _e((B * M, Fd), F32, dev), _e((B * M, Fd), F32, dev)
        K.w2v_contrast_bwd(sv.xf.view(B, M, Fd), sv.yq.view(B, M, Fd), st.neg, sv.codes, N, w.temp, sv.lse,
                           dloss.contiguous().float(), dxf, dyq)
        # encoder side
        dxe = _linear_bwd(dxf, sv.xe.view(B * M, sv.d), w.Wf, g.Wf, g.bf, adt)
        dx = torch.zeros(T, B, sv.d, dtype=F32, device=dev)
        K.w2v_scatter_rows(dxe, st.midx, dx, time_major=True)
        # quantizer side
        dq = _linear_bwd(dyq, sv.q, w.Wq, g.Wq, g.bq, adt)
        dlg = _e(sv.lg.shape, F32, dev)
        K.w2v_gumbel_bwd(sv.lg, G, w.vars, w.tau, not tr, dq, sv.codes, dlg, g.vars, noise=st.noise,
                         seed=_seed(st.seed, 4))
        dym = _linear_bwd(dlg, sv.ym, w.Wp, g.Wp, g.bp, adt)
        dym = _drop(dym, st.p_feat if tr else 0.0, _seed(st.seed, 3))
        dfeats = torch.zeros(B, T, sv.C, dtype=F32, device=dev)
        K.w2v_scatter_rows(dym, st.midx, dfeats)
        ctx.sv = None
        return dx.view(T * B, sv.d), dfeats.view(B * T, sv.C), None, None, None
