"""Node-level (teacher-forced) parity of the bf16 build at BASELINE config 2's real shapes
(B 32, T 1000 -> T' 249, d 256, 4 heads, ff 2048, V 4233): each fused autograd node of the
training step -- the subsampling (EmbedFn), one Conformer layer (ConformerLayerFn), one
decoder layer with after_norm + linear_out -- is fed the SAME inputs and upstream gradient
on the GPU and in the bf16-emulating oracle (oracle/u2_bf16.py, float64 with the bf16
build's roundings, itself pinned to the fp64 oracle by tests/test_oracle_golden.py).

Why per node: through a whole model the bf16 build is chaotic at the 1e-3 level -- every
fp32-vs-fp64 difference flips a few bf16 roundings per layer, and the flips (2^-9 relative
each) propagate and compound through 12 + 6 layers, so a whole-model bar cannot be tighter
than ~5e-2 whichever oracle is used (tests/test_model_gpu.py, DESIGN.md §2 measurements).
Feeding each node the same inputs removes the compounding: what remains is one node's
fp32 accumulation order and the rare rounding-boundary straddle, and the bar is 1e-2 of
each tensor's max for EVERY output, input gradient and parameter gradient (ReLU-gated
ones included: the decoder's ReLU FFN backward is driven on the oracle side by the gate the
kernel stored, and that gate is checked against the oracle's own relu'(u) everywhere a
pre-activation is not within accumulation error of zero).

Tensors whose exact gradient is zero (linear_k.bias: softmax is invariant to a per-row
constant; depthwise_conv.bias: BatchNorm removes it) carry only rounding noise in a bf16
pipeline; they are held to 1e-2 of the node's largest gradient instead."""

import math
import os
import sys
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import u2_bf16 as E  # noqa: E402
from oracle import u2_oracle as O  # noqa: E402

BAR = 1e-2
NOISE = ("linear_k.bias", "depthwise_conv.bias")
B, TX, L = 32, 1000, 40


def _model(cfg, seed, chunk=0):
    from liteasr_amd.models.u2 import U2, U2Config
    from liteasr_amd.utils.cfg import resolve_self

    c = U2Config(input_dim=80, vocab_size=cfg["vocab_size"], enc_dim=cfg["enc_dim"], enc_ff_dim=cfg["enc_ff"],
                 enc_attn_heads=cfg["enc_heads"], enc_layers=cfg["enc_layers"], dec_dim=cfg["dec_dim"],
                 dec_ff_dim=cfg["dec_ff"], dec_attn_heads=cfg["dec_heads"], dec_layers=cfg["dec_layers"],
                 dropout_rate=0.0, compute_dtype="bf16", chunk_size=chunk)
    resolve_self(c)
    params = {k: (v.bfloat16().float() if v.is_floating_point() else v)
              for k, v in O.init_params(cfg, seed=seed).items()}
    m = U2(c)
    m.load_state_dict({**params, **O.init_buffers(cfg)}, strict=False)
    return m.cuda().train(), params


def _env(model, seed, shape=(B, TX, L)):
    """The kernel env of a step on a config-2 batch (masks, rates, seeds), from one no-grad
    encoder pass; chained norms / batched position projections off for standalone calls."""
    xs, xlens, ys, ylens = O.synthetic_batch(*shape, model.ctc.ctc_lo.weight.shape[0], seed=seed)
    xs = xs.bfloat16().float()
    with torch.no_grad():
        _, prep, env = model._run_encoder(xs.cuda(), xlens.cuda(), ys.cuda(), ylens.cuda())
    env.links = None
    return env, prep, (xs, xlens, ys, ylens)


def _errs(pairs, gmax):
    out = {}
    for k, (a, b) in pairs.items():
        a, b = a.detach().double().cpu(), b.detach().double().cpu()
        noise = k.endswith(NOISE)
        den = gmax if noise else max(b.abs().max().item(), 1e-3 * gmax)
        out[k] = (a - b).abs().max().item() / den
    return out


def _check(errs, bar=BAR):
    worst = max((v, k) for k, v in errs.items())
    assert worst[0] < bar, (worst, sorted(((v, k) for k, v in errs.items()), reverse=True)[:6])


def _leaf(params, prefix):
    return {k: v.double().clone().requires_grad_() for k, v in params.items()
            if k.startswith(prefix) and v.is_floating_point()}


def test_conformer_layer_node_config2():
    """RelativeEncoderLayer (liteasr/nets/conformer_layer.py:130-147) at B 32 x T' 249."""
    _conformer_node(O.default_cfg(enc_layers=1, dec_layers=1), chunk=0, seed=31)


def test_conformer_layer_node_config4():
    """The same node at BASELINE config 4's layer shape: d 512, 16 heads (d_k 32), ff 2048, the
    dynamic-chunk streaming mask at chunk 16 (liteasr/utils/mask.py:30-90 triangle_mask with
    stage 16, OR the key padding), B 32 x T' 249 (liteasr/nets/attention.py:120-154 with the
    query-dependent mask staged per block pair in attn_flash.hip)."""
    cfg = O.default_cfg(enc_dim=512, enc_heads=16, enc_ff=2048, enc_layers=1, dec_dim=512, dec_heads=16,
                        dec_ff=2048, dec_layers=1)
    _conformer_node(cfg, chunk=16, seed=61)


def _conformer_node(cfg, chunk, seed):
    from liteasr_amd import kernels as K
    from liteasr_amd.nets import functional as FN

    model, params = _model(cfg, seed=seed, chunk=chunk)
    env, prep, _ = _env(model, seed=seed + 1)
    T, d = prep.T, cfg["enc_dim"]
    g = torch.Generator().manual_seed(seed + 2)
    x = torch.randn(B * T, d, generator=g)
    dy = torch.randn(B * T, d, generator=g)
    enc = model.encoder
    pos = torch.empty(T, d, dtype=torch.bfloat16, device="cuda")
    K.pe_fwd(None, T, T, d, enc.pe.table(T), 1.0, pos, 0.0, 0)
    layer = enc.enc_layers[0]
    model.store.ensure_grad().zero_()
    xd = x.cuda().requires_grad_()
    y = FN.ConformerLayerFn.apply(xd, pos, layer.final_norm.weight, layer, env)
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    got = {n: p.grad for n, p in model.named_parameters() if n.startswith("encoder.enc_layers.0.")}
    # oracle, same inputs
    pre = "encoder.enc_layers.0"
    leaf = _leaf(params, pre + ".")
    x64 = x.double().requires_grad_()
    mask = prep.enc_mask.bool().cpu()[:, None, :]
    if chunk > 0:
        assert prep.chunk_mask is not None
        mask = mask | O.triangle_mask(T, stage=chunk)[None]
    bn = {k: v.double() if v.is_floating_point() else v.clone() for k, v in O.init_buffers(cfg).items()}
    y64 = E.conformer_layer(x64.view(B, T, d), pos.double().cpu(), mask, leaf, pre, cfg["enc_heads"], bn, True)
    y64.backward(dy.double().view(B, T, d))
    gmax = max(v.grad.abs().max().item() for v in leaf.values())
    pairs = {k: (got[k], leaf[k].grad) for k in leaf}
    errs = _errs(pairs, gmax)
    errs["out"] = (y.detach().double().cpu().view(B, T, d) - y64.detach()).abs().max().item() / y64.abs().max().item()
    errs["dx"] = (xd.grad.double().cpu() - x64.grad).abs().max().item() / x64.grad.abs().max().item()
    _check(errs)


def test_subsampling_node_config2():
    """Conv2DLayer + x * sqrt(d) (liteasr/nets/subsampling.py:42-48, positional_encoding.py:
    68-75) at B 32 x T 1000 x 80: both ReLU-gated convs included."""
    from liteasr_amd.nets import functional as FN

    cfg = O.default_cfg(enc_layers=1, dec_layers=1)
    model, params = _model(cfg, seed=41)
    env, prep, (xs, _, _, _) = _env(model, seed=42)
    T, d = prep.T, cfg["enc_dim"]
    dy = torch.randn(B * T, d, generator=torch.Generator().manual_seed(43))
    enc = model.encoder
    model.store.ensure_grad().zero_()
    enc.embed.repack(model.compute_dtype)
    x0 = FN.EmbedFn.apply(xs.cuda(), enc.embed.out.weight, enc.embed, env)
    x0.backward(dy.cuda())
    torch.cuda.synchronize()
    got = {n: p.grad for n, p in model.named_parameters() if n.startswith("encoder.embed.")}
    leaf = _leaf(params, "encoder.embed.")
    x64 = math.sqrt(d) * E.G(E.subsample(xs.double(), leaf, "encoder.embed"))
    x64.backward(dy.double().view(B, T, d))
    gmax = max(v.grad.abs().max().item() for v in leaf.values())
    errs = _errs({k: (got[k], leaf[k].grad) for k in leaf}, gmax)
    errs["out"] = (x0.detach().double().cpu().view(B, T, d) - x64.detach()).abs().max().item() / x64.abs().max().item()
    _check(errs)


@pytest.mark.parametrize("shape,nsplit", [((B, TX, L), 1), ((8, 4000, 150), 4)], ids=["config2", "long"])
def test_decoder_layer_node(shape, nsplit):
    """One DecoderLayer (liteasr/nets/transformer_layer.py:179-221: self / source attention,
    ReLU FFN) + after_norm + linear_out (transformer_decoder.py:91-93), V 4233, the memory
    gradient included: config 2 (B 32 x (L+1) 41 rows over a T' 249 memory) and the long
    config (B 8 x (L+1) 151 rows over a T' 999 memory), where the source attention runs with
    its keys split 4 ways (lasr_attn_split_count) and combined by the second launch."""
    from liteasr_amd import kernels as K
    from liteasr_amd.nets import functional as FN

    cfg = O.default_cfg(enc_layers=1, dec_layers=1)
    model, params = _model(cfg, seed=51)
    env, prep, _ = _env(model, seed=52, shape=shape)
    B = shape[0]
    T, d, L1 = prep.T, cfg["dec_dim"], prep.L + 1
    assert K.attn_split(B, cfg["dec_heads"], L1, T, None) == nsplit, (B, L1, T)
    V = cfg["vocab_size"]
    g = torch.Generator().manual_seed(53)
    y_in = torch.randn(B * L1, d, generator=g)
    mem = torch.randn(B * T, d, generator=g).bfloat16()
    dlog = (torch.randn(B * L1, V, generator=g) * 1e-2).bfloat16()
    dec = model.decoder
    model.store.ensure_grad().zero_()
    wd, gd = dec.weights(), dec.grads()
    masks = (prep.dec_mask, prep.dec_mask.stride(0), prep.dec_mask.stride(1), prep.enc_mask)
    memd = mem.cuda()
    h_attn, sv = FN.decoder_layers_fwd(dec, wd, y_in.cuda(), memd, B, L1, T, masks, (0.0, 0.0, 0.0, 0.0),
                                       torch.bfloat16)
    dmem = torch.zeros(B * T, d, device="cuda")
    dyd = FN.decoder_layers_bwd(dlog.cuda(), sv, dec, wd, gd, memd, B, L1, T, dmem, torch.bfloat16)
    torch.cuda.synchronize()
    got = {n: p.grad for n, p in model.named_parameters() if n.startswith("decoder.")}
    # oracle: the same layer, after_norm and linear_out on the same rows / memory
    leaf = _leaf(params, "decoder.")
    n = "decoder.dec_layers.0"
    y64 = y_in.double().view(B, L1, d).requires_grad_()
    m64 = mem.double().view(B, T, d).requires_grad_()
    smask = prep.dec_mask.bool().cpu()
    mm = prep.enc_mask.bool().cpu()[:, None, :]
    H = cfg["dec_heads"]
    y = y64 + E.G(E.mha(E.RG(E.layer_norm(y64, leaf, n + ".self_attn_norm")), None, smask, leaf, n + ".self_attn", H))
    y = y + E.G(E.mha(E.RG(E.layer_norm(y, leaf, n + ".src_attn_norm")), m64, mm, leaf, n + ".src_attn", H))
    # the ReLU gate the kernel stored (act'(u), bf16 0/1) drives the oracle's FFN backward;
    # the gate itself must equal the oracle's relu'(u) wherever |u| exceeds 2e-3 of the
    # largest pre-activation: u reaches the two sides through bf16-rounded LayerNorm /
    # attention outputs whose rare rounding straddles move it by ~1e-3 (measured: flips only
    # at |u| <= 0.0045 of max |u| = 5.2)
    gate = sv.layers[0].z.double().cpu().view(B, L1, -1)
    pre = []
    y = y + E.G(E.ffn(E.RG(E.layer_norm(y, leaf, n + ".feed_forward_norm")), leaf, n + ".feed_forward", "relu",
                      gate=gate, pre=pre))
    u = pre[0]
    flip = (gate > 0) != (u > 0)
    assert (u[flip].abs() <= 2e-3 * u.abs().max()).all(), u[flip].abs().max()
    out = E.RG(E.linear(E.RG(E.layer_norm(y, leaf, "decoder.after_norm")), leaf, "decoder.linear_out"))
    out.backward(dlog.double().view(B, L1, V))
    gmax = max(v.grad.abs().max().item() for v in leaf.values() if v.grad is not None)
    errs = _errs({k: (got[k], leaf[k].grad) for k in leaf if leaf[k].grad is not None}, gmax)
    errs["h_attn"] = (h_attn.double().cpu().view(B, L1, V) - out.detach()).abs().max().item() / out.abs().max().item()
    errs["dy_in"] = (dyd.double().cpu().view(B, L1, d) - y64.grad).abs().max().item() / y64.grad.abs().max().item()
    errs["dmem"] = (dmem.double().cpu().view(B, T, d) - m64.grad).abs().max().item() / m64.grad.abs().max().item()
    _check(errs)
