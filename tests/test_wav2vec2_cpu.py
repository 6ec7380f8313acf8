"""wav2vec 2.0 host side, no GPU: registry and presets, state_dict layout and initialisation, the
host-drawn mask and negatives against the reference's draws, the CPU refusal, and the fp64
restatement (tests/wav2vec2_ref.py) against the reference's own run (tests/golden/wav2vec2.npz,
written by tests/golden/make_golden_wav2vec2.py)."""

import numpy as np
import pytest
import torch

import wav2vec2_cases as C
import wav2vec2_ref as R

# restatement vs the reference's run: both CPU torch; max |difference| / max |reference| per tensor
REF_TOL = 1e-6


def test_registry_and_presets():
    from liteasr_amd.config.compose import compose
    from liteasr_amd.criterions import CRITERION_REGISTRY
    from liteasr_amd.models import MODEL_REGISTRY

    assert "wav2vec2" in MODEL_REGISTRY and "wav2vec" in CRITERION_REGISTRY
    cfg = compose(overrides=["task=asr_kaldi", "model=wav2vec2_base", "criterion=wav2vec", "optimizer=noam_d256"])
    m = cfg.model
    assert m.name == "wav2vec2" and cfg.criterion.name == "wav2vec" and cfg.criterion.infonce is False
    assert (m.encoder_layers, m.encoder_embed_dim, m.encoder_ffn_embed_dim, m.encoder_attention_heads) == \
        (12, 768, 3072, 12)
    assert (m.final_dim, m.latent_vars, m.latent_groups, m.num_negatives, m.compute_dtype) == (256, 320, 2, 100, "bf16")
    assert list(m.latent_temp) == [2, 0.5, 0.999995] and m.conv_pos == 128 and m.negatives_from_everywhere is False


def test_state_dict_matches_reference_and_seeded_init():
    from liteasr_amd.models.wav2vec2 import Wav2Vec2

    g = C.golden()
    torch.manual_seed(C.SEED_W)
    model = Wav2Vec2(C.model_config())
    sd = model.state_dict()
    assert list(sd) == [str(k) for k in g["names"]]
    for k, v in sd.items():
        assert tuple(v.shape) == g["w." + k].shape, k
        assert np.array_equal(v.numpy(), g["w." + k]), k  # same seed, same draws, same weights
    # loading the reference layout and presenting it again is the identity
    model.load_state_dict(C.golden_state())
    for k, v in model.state_dict().items():
        assert np.array_equal(v.numpy(), g["w." + k]), k
    # extractor layers >= 1 live (C_out, k, C_in) in the flat store
    assert tuple(model.feature_extractor.conv_layers[1].conv.weight.shape) == (32, 3, 32)


@pytest.mark.parametrize("run", ["eval", "train"])
def test_host_draws_reproduce_reference(run):
    from liteasr_amd.utils.mask import negative_indices, span_mask

    g = C.golden()
    s_np, s_t = (int(v) for v in g[run + ".seeds"])
    np.random.seed(s_np)
    torch.manual_seed(s_t)
    mask = span_mask(batch=3, frame=99, prob=0.65, length=10, policy="static", no_overlap=False, min_mask_num=2,
                     min_interval=1)
    assert np.array_equal(mask.numpy(), g[run + ".mask"])
    M = int(mask[0].sum())
    neg = negative_indices(3, M, 10)
    assert np.array_equal(neg.numpy(), g[run + ".neg"])


def test_span_mask_no_overlap_keeps_spans_apart():
    from liteasr_amd.utils.mask import span_mask

    np.random.seed(3)
    mask = span_mask(batch=4, frame=200, prob=0.5, length=5, no_overlap=True, min_mask_num=2, min_interval=2)
    assert mask.shape == (4, 200) and len({int(r.sum()) for r in mask}) == 1 and int(mask[0].sum()) > 0


def test_cpu_batch_is_refused():
    from liteasr_amd.criterions.wav2vec_loss import Wav2Vec2Loss, Wav2Vec2LossConfig
    from liteasr_amd.models.wav2vec2 import Wav2Vec2

    model = Wav2Vec2(C.model_config())
    with pytest.raises(RuntimeError, match="HIP device only"):
        Wav2Vec2Loss(Wav2Vec2LossConfig())(model, torch.zeros(2, 4000), None, None, None)


def test_negatives_from_everywhere_is_refused():
    from liteasr_amd.models.wav2vec2 import Wav2Vec2

    cfg = C.model_config()
    cfg.negatives_from_everywhere = True
    with pytest.raises(NotImplementedError, match="negatives_from_everywhere"):
        Wav2Vec2(cfg)(torch.zeros(2, 4000))


@pytest.mark.parametrize("run", ["eval", "train"])
def test_restatement_reproduces_reference(run):
    g = C.golden()
    logits, loss, codes, grads = C.ref_run(run)
    assert np.array_equal(codes.numpy(), g[run + ".codes"])
    assert np.array_equal(torch.isinf(logits).numpy(), np.isinf(g[run + ".logits"]))
    assert int(np.isinf(g[run + ".logits"]).sum()) >= 1
    errs = {"logits": C.rel_max(logits, g[run + ".logits"]),
            "loss": abs(float(loss) - float(g[run + ".loss"])) / abs(float(g[run + ".loss"]))}
    errs.update(C.grad_errors(grads, {k: g["g." + k] for k in grads}))
    worst = max(errs, key=errs.get)
    print(f"{run}: worst {worst} {errs[worst]:.3e}")
    assert errs[worst] <= REF_TOL, {k: v for k, v in errs.items() if v > REF_TOL}
    if run == "train":
        assert set(grads) == {str(k) for k in g["names"]} and all(float(v.abs().max()) > 0 for v in grads.values())


@pytest.mark.parametrize("name", sorted(C.QUANT_CASES))
def test_quantizer_cases_have_few_near_ties(name):
    """The GPU quantizer test may leave out rows whose two best scores are within 1e-5 relative;
    its inputs leave out at most 1 % of the rows (here: in the restatement)."""
    logits, noise, vars_, _ = C.quant_case(name)
    G = C.QUANT_CASES[name][0]
    for train in (True, False):
        _, _, margin = R.quantize(logits.double(), vars_.double(), G, C.QUANT_TAU, noise.double(), train)
        assert float((margin < C.TIE).any(-1).float().mean()) <= 0.01


@pytest.mark.parametrize("name", sorted(C.HEAD_CASES))
def test_head_cases_mask_a_whole_row(name):
    x, y, neg, codes, temp = C.head_case(name)
    logits, loss = R.contrast(x.double(), y.double(), neg, codes, temp)
    N, _, M, B = C.HEAD_CASES[name][:4]
    row = logits.view(M, B, N + 1)[0, 0]
    assert torch.isinf(row[1:]).all() and torch.isfinite(row[0]) and torch.isfinite(loss)
    assert 0 < int(torch.isinf(logits).sum()) < logits.numel() - M * B
