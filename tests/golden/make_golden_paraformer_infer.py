"""Generate tests/golden/paraformer_infer.npz by running the *reference's* own Paraformer
(liteasr/models/paraformer.py, imported through refshim) on the CPU in its inference mode.
Data only; the tests and the GPU box read the .npz.

    python tests/golden/make_golden_paraformer_infer.py [--scan N]

The model is the tiny Paraformer of make_golden.py gen_paraformer (d 64, 2 encoder / 1
decoder layers, V 20, F 40) with its seed-42 weights read from paraformer.npz (``init.*``;
not stored again).  A random-init predictor gives alpha ~ 0.5 (a token every other frame), so
``predictor.lin.bias`` is set per case (stored as ``lin_bias``): with -1.0 the token rate is
speech-like (one token per 4-6 subsampled frames).

Single-utterance cases go through ``model.inference(x)`` (paraformer.py:124-129).  Batch
cases go through the reference's modules composed as its ``forward`` composes them, the
predictor in its inference branch:
    h = encoder(xs, padding_mask(xlens)); h_cif, sum_alpha = predictor(h, get_pred_len(xlens), None)
    ids = argmax(decoder(h_cif, memory=h, memory_mask=padding_mask(xlens)))
with row b trimmed to its first ulens[b] ids.

Per case ``c<i>.``:
  kind ("single" / "batch"), seed, lin_bias
  xs [B, T, 40], xlens [B]
  h_enc [B, T', 64], z [B, T'] (predictor logits), alpha [B, T'] (masked), sum_alpha [B],
  ulens [B], h_cif [B, max ulens, 64], logits [B, max ulens, 20], ids [B, max ulens]
  fired [B, T'] (frames whose new_alpha >= beta)
  margin_round   min_b |frac(sum_alpha_b) - 0.5|
  margin_fire    min_{b,t} |new_alpha - beta| (inf where ulen = 0: beta = +inf)
  margin_logit   min over the kept tokens of (top1 - top2) (inf without tokens)

A case is kept only if
  margin_round >= 10 * MAX_DSUM, margin_fire >= 10 * MAX_DALPHA * T', margin_logit >= 10 * MAX_DLOGIT
(T': the fire decision compares a running sum of up to T' alphas).  The three constants bound
the fp32 device build's error against the values recorded here; --scan N prints, per shape,
the seed with the largest worst ratio margin / requirement (ties: the next-worst ratio).
"""

import argparse
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import refshim  # noqa: E402

refshim.install()

from liteasr.models.paraformer import Paraformer  # noqa: E402
from liteasr.utils.mask import padding_mask  # noqa: E402

# Bounds on |fp32 device build - recorded value| over all cases.  Measured on MI355X by
# tests/test_paraformer_infer_gpu.py test_inference_matches_reference (it prints them), maxima
# over the six cases: |delta sum_alpha| 1.91e-6 (a sum of up to 74 alphas near 18: 16 ulp),
# |delta alpha| 8.94e-8 (1.5 ulp of a value below 1: the sigmoid of a logit that differs in its
# last bits), |delta logit| 3.65e-6.  The constants are those maxima with a factor of two or
# more to spare.  (The search started from the fp32 bars of tests/test_paraformer_gpu.py:
# 1e-5 of sum_alpha, hence 1e-5 per alpha, and 2e-4 of max for the logits; at those no case
# can pass, because the last token's fire margin is ulen * 1e-4 by construction of beta.)
MAX_DSUM = 4e-6    # |delta sum_alpha|
MAX_DALPHA = 2e-7  # |delta alpha|, per frame
MAX_DLOGIT = 1e-5  # |delta decoder logit|

LIN_BIAS = -1.0
# (kind, xlens, seed); the T = 7 utterance has no token, every other case at least one
# (seeds: --scan 300)
CASES = [("single", [7], 92), ("single", [11], 24), ("single", [64], 235), ("single", [300], 119),
         ("batch", [120, 113, 97], 212), ("batch", [160, 160, 131, 90], 171)]


def build():
    cfg = types.SimpleNamespace(dropout_rate=0.0, use_rel=True, input_dim=40, enc_dim=64, enc_ff_dim=128,
                                enc_attn_heads=4, enc_dropout_rate=0.0, enc_pos_dropout_rate=0.0,
                                enc_attn_dropout_rate=0.0, enc_ff_dropout_rate=0.0, enc_layers=2,
                                activation="swish", sample_ratio=0.75, vocab_size=20, dec_dim=64, dec_ff_dim=128,
                                dec_attn_heads=4, dec_dropout_rate=0.0, dec_self_attn_dropout_rate=0.0,
                                dec_src_attn_dropout_rate=0.0, dec_ff_dropout_rate=0.0, dec_layers=1,
                                pos_dropout_rate=0.0)
    torch.manual_seed(42)
    model = Paraformer(cfg)
    d = np.load(os.path.join(HERE, "paraformer.npz"))
    init = {k[5:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("init.")}
    missing, unexpected = model.load_state_dict(init, strict=False)
    assert not unexpected and all(k.endswith("pe.pe") or k == "pe.pe" for k in missing), (missing, unexpected)
    with torch.no_grad():
        model.predictor.lin.bias.fill_(LIN_BIAS)
    model.eval()
    return model


def run(model, kind, xlens, seed):
    B, Tx = len(xlens), max(xlens)
    xl = torch.tensor(xlens)
    g = torch.Generator().manual_seed(1000 + seed)
    xs = torch.randn(B, Tx, 40, generator=g).masked_fill(padding_mask(xl).unsqueeze(-1), 0.0)
    rec = {}
    pred, dec = model.predictor, model.decoder
    pred_fwd, dec_fwd = pred.forward, dec.forward

    def pred_hook(h, xlens_=None, ylens_=None):
        rec["h_enc"] = h.detach().clone()
        z = pred.lin(pred.relu(pred.conv(h.transpose(1, 2))).transpose(1, 2)).squeeze(-1)
        a = pred.sigmoid(z)
        if xlens_ is not None:
            a = a.masked_fill(padding_mask(xlens_), 0)
        rec["z"], rec["alpha"] = z.detach().clone(), a.detach().clone()
        out = pred_fwd(h, xlens_, ylens_)
        rec["h_cif"], rec["sum_alpha"] = out[0].detach().clone(), out[1].detach().clone()
        return out

    def dec_hook(*a, **k):
        rec["logits"] = dec_fwd(*a, **k)
        return rec["logits"]

    pred.forward, dec.forward = pred_hook, dec_hook
    try:
        with torch.no_grad():
            if kind == "single":
                ids = model.inference(xs)
                ids = torch.tensor(ids, dtype=torch.int64).view(1, -1)
            else:
                mask = padding_mask(xl)
                h = model.encoder(xs, mask)
                h_cif, _ = model.predictor(h, model.get_pred_len(xl), None)
                ids = torch.argmax(model.decoder(h_cif, memory=h, memory_mask=mask), dim=-1)
    finally:
        del pred.forward, dec.forward
    alpha, sum_alpha = rec["alpha"], rec["sum_alpha"]
    assert torch.equal(alpha.sum(-1), sum_alpha)
    ulens = torch.round(sum_alpha).int()
    L = int(ulens.max())
    assert rec["h_cif"].shape[1] == L and ids.shape == (B, L)
    # the fire decisions, with the reference's own float32 expressions (predictor.py:53, 73-85)
    beta = sum_alpha / ulens - 1e-4
    Tp = alpha.shape[1]
    prev = torch.zeros(B)
    fired = torch.zeros(B, Tp, dtype=torch.bool)
    margin_fire = np.inf
    for t in range(Tp):
        new = prev + alpha[:, t]
        f = new >= beta
        margin_fire = min(margin_fire, float((new - beta).abs().min()))
        fired[:, t] = f
        prev = torch.where(f, new - beta, new)
    frac = sum_alpha.double() - torch.floor(sum_alpha.double())
    margin_round = float((frac - 0.5).abs().min())
    margin_logit = np.inf
    logits = rec["logits"].detach()
    for b in range(B):
        for u in range(int(ulens[b])):
            top = torch.topk(logits[b, u], 2).values
            margin_logit = min(margin_logit, float(top[0] - top[1]))
    return dict(kind=np.array(kind), seed=np.array(seed), lin_bias=np.array(LIN_BIAS, dtype=np.float32), xs=xs,
                xlens=xl, h_enc=rec["h_enc"], z=rec["z"], alpha=alpha, sum_alpha=sum_alpha, ulens=ulens,
                h_cif=rec["h_cif"], logits=logits, ids=ids, fired=fired, margin_round=np.array(margin_round),
                margin_fire=np.array(margin_fire), margin_logit=np.array(margin_logit))


def needed(c):
    Tp = c["alpha"].shape[1]
    return 10 * MAX_DSUM, 10 * MAX_DALPHA * Tp, 10 * MAX_DLOGIT


def ratios(c):
    """margin / requirement of the three rules, worst first (seeds compare by this list: the
    fire margin of the last token is ulen * 1e-4 whatever the seed, so ties are common)."""
    return sorted(float(c[k]) / n for k, n in zip(("margin_round", "margin_fire", "margin_logit"), needed(c)))


def ratio(c):
    return ratios(c)[0]


def scan(n):
    model = build()
    for kind, xlens, _ in CASES:
        best = None
        for seed in range(n):
            c = run(model, kind, xlens, seed)
            ul = c["ulens"].tolist()
            ok = min(ul) < max(ul) if kind == "batch" else (max(ul) > 0 or max(xlens) == 7)
            if ok and (best is None or ratios(c) > best[1]):
                best = (seed, ratios(c), ul, [float(c[k]) for k in ("margin_round", "margin_fire", "margin_logit")])
        print(f"{kind} {xlens}: seed, margin / requirement worst first, ulens, margins (round, fire, logit) = {best}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scan", type=int, default=0, help="scan this many seeds per shape and print the best")
    a = ap.parse_args()
    torch.set_num_threads(4)
    if a.scan:
        return scan(a.scan)
    model = build()
    arrs = {"n_cases": np.array(len(CASES))}
    short = False
    for i, (kind, xlens, seed) in enumerate(CASES):
        c = run(model, kind, xlens, seed)
        for k, n in zip(("margin_round", "margin_fire", "margin_logit"), needed(c)):
            assert float(c[k]) >= n, (kind, xlens, seed, k, float(c[k]), n)
        ul = c["ulens"].tolist()
        short |= kind == "batch" and min(ul) < max(ul)
        print(f"case {i}: {kind} xlens {xlens} seed {seed} ulens {ul} ids {c['ids'].tolist()} margins "
              f"round {float(c['margin_round']):.3g} fire {float(c['margin_fire']):.3g} "
              f"logit {float(c['margin_logit']):.3g} (worst ratio {ratio(c):.3g})")
        arrs.update({f"c{i}.{k}": (v.detach().numpy() if torch.is_tensor(v) else v) for k, v in c.items()})
    assert short, "no batch case has an utterance with ulen < L"
    path = os.path.join(HERE, "paraformer_infer.npz")
    np.savez_compressed(path, **arrs)
    print("wrote paraformer_infer.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
