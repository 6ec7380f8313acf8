"""Inputs shared by the wav2vec 2.0 CPU and GPU tests: the golden fixture, the tiny model's config
and the quantizer / contrastive-head cases (seeded fp32 tensors, built once)."""

import functools
import os

import numpy as np
import torch

import wav2vec2_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
LAYERS = [(32, 10, 5), (32, 3, 2), (32, 3, 2), (32, 2, 2)]
REF_CFG = {"layers": LAYERS, "heads": 4, "groups": 2, "tau": 2.0, "logit_temp": 0.1}
SEED_W = 42
TIE = 1e-5  # rows whose two best scores are closer than this (relative) may be left out


@functools.lru_cache(None)
def golden():
    return dict(np.load(os.path.join(HERE, "golden", "wav2vec2.npz")))


def model_config(compute_dtype="fp32"):
    from liteasr_amd.models.wav2vec2 import Wav2Vec2Config

    return Wav2Vec2Config(encoder_layers=2, encoder_embed_dim=64, encoder_ffn_embed_dim=128,
                          encoder_attention_heads=4, dropout=0.0, final_dim=32, latent_vars=16, latent_groups=2,
                          num_negatives=10, conv_feature_layers="[(32, 10, 5)] + [(32, 3, 2)] * 2 + [(32, 2, 2)]",
                          compute_dtype=compute_dtype)


def golden_state(dtype=torch.float32):
    g = golden()
    return {str(k): torch.from_numpy(g["w." + str(k)]).to(dtype) for k in g["names"]}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# (G, V, vd): a small codebook and one that is no power of two and wider than a 256-thread block
QUANT_CASES = {"v16": (2, 16, 16, 101), "v320": (2, 320, 24, 102)}
QUANT_ROWS, QUANT_TAU = 297, 2.0


@functools.lru_cache(None)
def quant_case(name):
    """(logits (R, G V), noise (R G, V), vars (G V, vd), dout (R, G vd)) fp32."""
    G, V, vd, seed = QUANT_CASES[name]
    g = _gen(seed)
    logits = torch.randn(QUANT_ROWS, G * V, generator=g) * 2.0
    noise = -torch.empty(QUANT_ROWS * G, V).exponential_(generator=g).log()
    vars_ = torch.rand(G * V, vd, generator=g)
    dout = torch.randn(QUANT_ROWS, G * vd, generator=g)
    return logits, noise, vars_, dout


# (N, D, M, B, V): V 2 with 2 groups = 4 code pairs, so many negatives equal their positive
HEAD_CASES = {"n10": (10, 32, 7, 3, 2, 201), "n100": (100, 48, 23, 2, 2, 202)}


@functools.lru_cache(None)
def head_case(name):
    """(x, y (B, M, D) fp32, neg (B, M N) int64, codes (B M, 2) int64, temp).  Row (b 0, m 0) has
    every negative equal to its positive: all its negatives point at rows given its codes."""
    N, D, M, B, V, seed = HEAD_CASES[name]
    g = _gen(seed)
    x = torch.randn(B, M, D, generator=g)
    y = torch.randn(B, M, D, generator=g)
    codes = torch.randint(0, V, (B * M, 2), generator=g)
    own = torch.arange(M).unsqueeze(-1).expand(-1, N).flatten()
    neg = torch.randint(0, M - 1, (B, M * N), generator=g)
    neg[neg >= own] += 1
    for b in range(1, B):
        neg[b] += b * M
    codes[1] = codes[0]
    codes[2] = codes[0]
    neg[0, :N] = torch.tensor([1, 2] * N)[:N]
    return x, y, neg, codes, 0.1


def rel_max(a, b, scale=None):
    """max |a - b| / max |b| over the finite entries (the positions of -inf must agree); `scale`
    replaces max |b|."""
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    fin = torch.isfinite(b)
    assert torch.equal(torch.isfinite(a), fin), "non-finite positions differ"
    if not fin.any():
        return 0.0
    den = b[fin].abs().max().clamp_min(1e-30) if scale is None else scale
    return float((a[fin] - b[fin]).abs().max() / den)


def grad_errors(grads, ref):
    """{key: rel_max} of gradients against ``ref`` (key -> array).  A key projection's bias has
    no gradient in exact arithmetic (a constant added to every key's score leaves the softmax
    unchanged), so both sides hold rounding residue there; it is measured on the scale of the
    same layer's query-bias gradient, the same sums without the cancellation."""
    out = {}
    for k, v in grads.items():
        scale = None
        if k.endswith("linear_k.bias"):
            scale = float(np.abs(np.asarray(ref[k.replace("linear_k", "linear_q")], dtype=np.float64)).max())
        out[k] = rel_max(v, np.asarray(ref[k]), scale)
    return out


@functools.lru_cache(None)
def ref_run(run):
    """The fp64 restatement on the fixture's inputs of ``run`` ("eval" / "train"): (logits, loss,
    codes, {parameter: gradient} for train)."""
    g = golden()
    sd = {k: v.clone().requires_grad_(run == "train") for k, v in golden_state(torch.float64).items()}
    mask = torch.from_numpy(g[run + ".mask"])
    neg = torch.from_numpy(g[run + ".neg"]).long()
    noise = torch.from_numpy(g["train.noise"]).double() if run == "train" else None
    logits, loss, codes = R.model_forward(sd, REF_CFG, torch.from_numpy(g["source"]).double(), mask, neg, noise,
                                          train=run == "train")
    grads = {}
    if run == "train":
        loss.backward()
        grads = {k: v.grad for k, v in sd.items()}
    return logits.detach(), loss.detach(), codes, grads
