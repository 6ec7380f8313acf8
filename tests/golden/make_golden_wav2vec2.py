"""Generate tests/golden/wav2vec2.npz by running the *reference's* own wav2vec 2.0 model
(liteasr/models/wav2vec2.py, imported through refshim) and its criterion's cross-entropy on the
CPU.  Data only; the tests read the .npz and never the reference.

    python tests/golden/make_golden_wav2vec2.py

Config: conv layers [(32, 10, 5)] + [(32, 3, 2)] * 2 + [(32, 2, 2)], d 64, ff 128, 4 heads, 2
layers, final_dim 32, 16 codes x 2 groups, 10 negatives, dropout 0; B 3 x 4000 samples (799 ->
399 -> 199 -> 99 frames).  The weights are drawn in fp32 under torch.manual_seed(SEED_W); the
model then runs in float64 (its own ``.float()`` casts in the extractor norms, the quantizer and
the cosine similarity stay as they are), so what is recorded carries no accumulated fp32 error.

Stored:
  names, w.<key>        state_dict keys in order and the fp32 weights
  source                the (3, 4000) waveform
  eval.* / train.*      seeds (np, torch), mask (B, T'), neg (B, M N), codes (B M, G), logits,
                        loss; train also noise (B M G, V) and g.<key>, every parameter's gradient
Both runs draw the mask from ``np.random`` and the negatives from torch's generator under the
stored seeds.  The train run replaces ``F.gumbel_softmax`` by a recording stand-in: it draws the
Gumbel noise itself (own generator) and saves it, applies the same formula, and returns an
*exactly* one-hot value with the straight-through gradient (the reference's selected entry is
(1 - p) + p, which can be one ulp off 1 and makes its float ``negs == pos`` compare depend on
rounding; the product compares code indices).  Asserted here: in both runs the -inf logits are
exactly the (n, b, m) whose codes equal the positive's, the eval run has at least one, and every
(row, group) separates its two best scores by more than 1e-4 relative.
"""

import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import refshim  # noqa: E402

refshim.install()

import liteasr.models.wav2vec2 as RM  # noqa: E402
import liteasr.nets.gumbel_vector_quantizer as RQ  # noqa: E402

SEED_W, SEED_X, SEED_NOISE = 42, 5, 13
RUNS = {"eval": (7, 11), "train": (8, 12)}  # (np seed, torch seed)
LAYERS = "[(32, 10, 5)] + [(32, 3, 2)] * 2 + [(32, 2, 2)]"
MIN_MARGIN = 1e-4


def config():
    return types.SimpleNamespace(
        encoder_layers=2, encoder_embed_dim=64, encoder_ffn_embed_dim=128, encoder_attention_heads=4, dropout=0.0,
        attention_dropout=0.0, activation_dropout=0.0, encoder_layerdrop=0.0, dropout_input=0.0, dropout_features=0.0,
        final_dim=32, layer_norm_first=False, conv_feature_layers=LAYERS, conv_bias=False, logit_temp=0.1,
        quantize_targets=True, quantize_input=False, same_quantizer=False, target_glu=False, feature_grad_mult=1.0,
        latent_vars=16, latent_groups=2, latent_dim=0, mask_length=10, mask_prob=0.65, mask_other=0,
        no_mask_overlap=False, mask_min_space=1, num_negatives=10, negatives_from_everywhere=False,
        cross_sample_negatives=0, codebook_negatives=0, conv_pos=128, conv_pos_groups=16,
        latent_temp=(2, 0.5, 0.999995))


def main():
    cfg = config()
    torch.manual_seed(SEED_W)
    model = RM.Wav2Vec2(cfg)
    out = {"names": np.array(list(model.state_dict().keys()))}
    for k, v in model.state_dict().items():
        out["w." + k] = v.detach().numpy().copy()
    model = model.double()
    source = torch.randn(3, 4000, generator=torch.Generator().manual_seed(SEED_X))
    out["source"] = source.numpy()

    rec = {}
    real_mask = RM.span_mask

    def mask_spy(**kw):
        rec["mask"] = real_mask(**kw)
        return rec["mask"]

    RM.span_mask = mask_spy
    real_neg = model.sample_negatives

    def neg_spy(sample_source, num_mask):
        negs, idx = real_neg(sample_source=sample_source, num_mask=num_mask)
        rec["neg"] = idx.clone()
        return negs, idx

    model.sample_negatives = neg_spy
    gen = torch.Generator().manual_seed(SEED_NOISE)

    def gumbel_standin(logits, tau=1, hard=False, eps=1e-10, dim=-1):
        g = -torch.empty_like(logits).exponential_(generator=gen).log()
        rec["noise"] = g.detach().clone()
        rec["scores"] = ((logits + g) / tau).detach().clone()
        y = ((logits + g) / tau).softmax(dim)
        one = torch.zeros_like(logits).scatter_(dim, y.max(dim, keepdim=True)[1], 1.0)
        return one + (y - y.detach())

    RQ.F = types.SimpleNamespace(gumbel_softmax=gumbel_standin)
    proj = model.quantizer.weight_proj
    proj.register_forward_hook(lambda m, i, o: rec.__setitem__("proj", o.detach().clone()))

    for run, (s_np, s_t) in RUNS.items():
        train = run == "train"
        model.train(train)
        model.zero_grad()
        np.random.seed(s_np)
        torch.manual_seed(s_t)
        logits = model(source.double())
        loss = torch.nn.CrossEntropyLoss()(logits, model.get_target(logits, None))
        mask, neg = rec["mask"], rec["neg"]
        B, M, N, G = 3, int(mask[0].sum()), cfg.num_negatives, cfg.latent_groups
        scores = rec["scores"] if train else rec["proj"].view(B * M * G, -1).float()
        codes = scores.argmax(-1).view(B * M, G)
        top = scores.topk(2, -1).values
        margin = (top[:, 0] - top[:, 1]) / top.abs().max(-1).values
        assert float(margin.min()) > MIN_MARGIN, (run, float(margin.min()))
        # float equality (the reference's mask) == code equality (the product's), as a set
        same = (codes[neg.view(-1)].view(B, M, N, G) == codes.view(B, M, 1, G)).all(-1)  # (B, M, N)
        ninf = torch.isinf(logits.view(M, B, N + 1)[:, :, 1:]).permute(1, 0, 2)
        assert torch.equal(same, ninf), run
        assert not torch.isinf(logits[:, 0]).any()
        if not train:
            assert int(same.sum()) >= 1
        print(f"{run}: M {M}, loss {loss.item():.6f}, -inf logits {int(same.sum())}, min margin {float(margin.min()):.2e}")
        out[run + ".seeds"] = np.array([s_np, s_t])
        out[run + ".mask"] = mask.numpy()
        out[run + ".neg"] = neg.numpy().astype(np.int32)
        out[run + ".codes"] = codes.numpy().astype(np.int32)
        out[run + ".logits"] = logits.detach().numpy()
        out[run + ".loss"] = np.float64(loss.item())
        if train:
            out["train.noise"] = rec["noise"].numpy()
            loss.backward()
            for k, p in model.named_parameters():
                assert p.grad is not None, k
                out["g." + k] = p.grad.numpy().astype(np.float32)
    path = os.path.join(HERE, "wav2vec2.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
