"""wav2vec 2.0 forward in plain torch fp64, one function per device kernel (csrc/w2v.hip), written
from the model's definition: what the GPU tests compare the kernels against, and -- composed by
``model_forward`` -- what tests/test_wav2vec2_cpu.py checks against the reference's own run
(tests/golden/wav2vec2.npz).  Gradients come from torch autograd over these functions.

Activations are channels-last (B, T, C); weights are in the reference's ``state_dict`` layout.
"""

import math

import torch

F64 = torch.float64
EXT_EPS, LN_EPS, COS_EPS = 1e-5, 1e-12, 1e-8


def gelu(u):
    return 0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0)))


def layer_norm(x, g, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g + b


def conv_rows(x, W, bias, k, s):
    """Conv1d without padding over channels-last rows: x (B, T_in, C_in), W (C_out, C_in, k)."""
    win = x.unfold(1, k, s)  # (B, T_out, C_in, k)
    y = torch.einsum("btik,oik->bto", win, W)
    return y if bias is None else y + bias


def ext_layer(x, W, bias, g, b, k, s):
    """Conv1d -> LayerNorm over channels (eps 1e-5) -> exact GELU."""
    return gelu(layer_norm(conv_rows(x, W, bias, k, s), g, b, EXT_EPS))


def posconv(x, W, bias, k=128, groups=16):
    """x + GELU(grouped conv, padding k / 2, last frame dropped); x (B, T, d), W (d, d / groups, k)."""
    B, T, d = x.shape
    cg = d // groups
    xp = torch.nn.functional.pad(x, (0, 0, k // 2, k // 2))
    win = xp.unfold(1, k, 1)[:, :T]  # (B, T, d, k)
    win = win.reshape(B, T, groups, cg, k)
    y = torch.einsum("btgik,goik->btgo", win, W.view(groups, cg, cg, k)).reshape(B, T, d) + bias
    return x + gelu(y)


def mask_rows(x, mask, emb):
    """Rows where mask (B, T) is set become emb."""
    return torch.where(mask.unsqueeze(-1), emb.expand_as(x), x)


def gather_masked(x, mask):
    B = x.shape[0]
    return x[mask].view(B, -1, x.shape[-1])


def quantize(logits, vars_, G, tau, noise=None, train=True):
    """logits (R, G V), vars_ (G V, vd), noise (R G, V) or None.  Returns (out (R, G vd), codes
    (R, G), margin (R, G): relative gap between the two largest scores).  Train: argmax of
    (logit + noise) / tau with the straight-through gradient of its softmax; eval: argmax of the
    logits, no gradient to them."""
    R = logits.shape[0]
    V = logits.shape[1] // G
    z = logits.view(R * G, V)
    if train:
        z = (z + noise.view(R * G, V)) / tau
    top = z.detach().topk(2, dim=-1).values
    margin = ((top[:, 0] - top[:, 1]) / top.abs().max(-1).values.clamp_min(1e-30)).view(R, G)
    codes = z.argmax(-1)
    hard = torch.zeros_like(z).scatter_(-1, codes.view(-1, 1), 1.0)
    if train:
        soft = torch.softmax(z, -1)
        hard = hard + (soft - soft.detach())
    out = torch.einsum("rgv,gvd->rgd", hard.view(R, G, V), vars_.view(G, V, -1)).reshape(R, -1)
    return out, codes.view(R, G), margin


def contrast(x, y, neg, codes, temp):
    """x, y (B, M, D); neg (B, M N) rows of y.view(B M, D); codes (B M, G).  Returns (logits
    (M B, N + 1), loss): cosine similarity / temp, -inf where a negative's codes equal the
    positive's in every group, mean cross-entropy against column 0."""
    B, M, D = x.shape
    N = neg.shape[1] // M
    yf = y.reshape(B * M, D)
    tg = torch.cat([y.unsqueeze(2), yf[neg.reshape(-1)].view(B, M, N, D)], dim=2)  # (B, M, N + 1, D)
    nx = x.norm(dim=-1).clamp_min(COS_EPS).unsqueeze(-1)
    nt = tg.norm(dim=-1).clamp_min(COS_EPS)
    lg = (x.unsqueeze(2) * tg).sum(-1) / (nx * nt) / temp
    cf = codes.view(B * M, -1)
    same = (cf[neg.reshape(-1)].view(B, M, N, -1) == cf.view(B, M, 1, -1)).all(-1)
    lg = torch.cat([lg[..., :1], lg[..., 1:].masked_fill(same, float("-inf"))], dim=-1)
    logits = lg.transpose(0, 1).reshape(M * B, N + 1)
    loss = (torch.logsumexp(logits, -1) - logits[:, 0]).mean()
    return logits, loss


def encoder_layer(x, sd, p, H):
    """Pre-norm Transformer layer over x (batch, time, d): x + MHA(LN(x)), then x + FFN(LN(x)),
    ReLU, norms with eps 1e-12, no mask."""
    Bt, Tt, d = x.shape
    dk = d // H
    h = layer_norm(x, sd[p + "self_attn_norm.weight"], sd[p + "self_attn_norm.bias"], LN_EPS)
    lin = lambda n, v: v @ sd[p + n + ".weight"].t() + sd[p + n + ".bias"]  # noqa: E731
    q = lin("self_attn.linear_q", h).view(Bt, Tt, H, dk).transpose(1, 2)
    k = lin("self_attn.linear_k", h).view(Bt, Tt, H, dk).transpose(1, 2)
    v = lin("self_attn.linear_v", h).view(Bt, Tt, H, dk).transpose(1, 2)
    att = torch.softmax(q @ k.transpose(-1, -2) * dk ** -0.5, -1) @ v
    x = x + lin("self_attn.linear_o", att.transpose(1, 2).reshape(Bt, Tt, d))
    h = layer_norm(x, sd[p + "feed_forward_norm.weight"], sd[p + "feed_forward_norm.bias"], LN_EPS)
    return x + lin("feed_forward.fc2", torch.relu(lin("feed_forward.fc1", h)))


def model_forward(sd, cfg, source, mask, neg, noise=None, train=True):
    """The whole model on fp64 tensors: sd the reference-layout state dict, cfg a dict with
    layers [(C, k, s)], heads, groups, tau, logit_temp; dropout 0.  Returns (logits, loss, codes)."""
    x = source.unsqueeze(-1)
    for i, (C, k, s) in enumerate(cfg["layers"]):
        p = f"feature_extractor.conv_layers.{i}."
        x = ext_layer(x, sd[p + "conv.weight"], sd.get(p + "conv.bias"), sd[p + "layer_norm.weight"],
                      sd[p + "layer_norm.bias"], k, s)
    feats = layer_norm(x, sd["layer_norm.weight"], sd["layer_norm.bias"], LN_EPS)
    h = feats @ sd["linear_input.weight"].t() + sd["linear_input.bias"] if "linear_input.weight" in sd else feats
    h = mask_rows(h, mask, sd["mask_emb"])
    h = posconv(h, sd["encoder.embed.weight"], sd["encoder.embed.bias"])
    h = layer_norm(h, sd["encoder.embed_norm.weight"], sd["encoder.embed_norm.bias"], LN_EPS)
    h = h.transpose(0, 1)  # the layers then treat T' as the batch and B as time
    n_layer = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("encoder.enc_layers."))
    for i in range(n_layer):
        h = encoder_layer(h, sd, f"encoder.enc_layers.{i}.", cfg["heads"])
    h = h.transpose(0, 1)
    xm = gather_masked(h, mask) @ sd["linear_final.weight"].t() + sd["linear_final.bias"]
    B, M = xm.shape[0], xm.shape[1]
    ym = gather_masked(feats, mask).reshape(B * M, -1)
    lg = ym @ sd["quantizer.weight_proj.weight"].t() + sd["quantizer.weight_proj.bias"]
    G = cfg["groups"]
    q, codes, _ = quantize(lg, sd["quantizer.vars"][0], G, cfg["tau"], noise, train)
    yq = (q @ sd["linear_quantizer.weight"].t() + sd["linear_quantizer.bias"]).view(B, M, -1)
    logits, loss = contrast(xm, yq, neg, codes, cfg["logit_temp"])
    return logits, loss, codes
