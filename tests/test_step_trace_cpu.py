"""Host-only launch trace of whole steps: every model family's forward + backward (and the
inference entry points) runs on CPU tensors with ``_native.call`` replaced by a recorder, the way
tools/step_census.py does it (the host planner ``lasr_gemm_plan`` and the ``lasr_dropout*`` host
functions really run; the library is loaded for them only).  Each recorded call is its name plus
its normalised arguments: integers and floats by value, every field of a struct argument (each
element of the ``lasr_gemm_dw_group`` / ``lasr_reduce_multi`` arrays included), every pointer as
(null or not, address mod 16) -- the mod-16 bit selects vector paths; pointer identity is not
recorded, so the Python around the launches may allocate in another order, but it may not launch
in another order or with other geometry.

The expected traces are tests/golden/step_trace/<scenario>.txt, one line per call (name, short
hash of the normalised arguments), written once from the tree before nets/functional.py was split
(``python tests/test_step_trace_cpu.py --write`` writes the files that do not exist yet and never
overwrites one).  No GPU, no conftest support."""

import ctypes as C
import hashlib
import importlib
import os
import random
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "step_trace")

SWITCHES = ("ROW_LN", "DEC_ROW_LN", "SPLITK_LN", "QBIAS_IN_REDUCE", "LN2_BWD_CHAIN", "BN_GLU_FUSED", "LAYER_RED_HOLD",
            "FUSED_RELATTN", "BATCH_POS_PROJ", "FUSED_LN2", "FUSED_DEC_ATTN", "DEC_GB_IN_LN")
V = 50  # vocabulary of the reduced models


# ------------------------------------------------------------------- recorder ---
def _ptr(v):
    v = getattr(v, "value", v)
    return "-" if not v else f"p{int(v) % 16}"


def _struct(s, N):
    out = []
    for name, ty in s._fields_:
        v = getattr(s, name)
        if ty is N._p:
            v = _ptr(v)
        elif issubclass(ty, C.Array):
            v = tuple(_ptr(x) for x in v)
        out.append((name, v))
    return tuple(out)


def _normalise(name, a, N):
    sig = N.SIGNATURES[name]
    assert len(sig) == len(a), f"{name}: {len(a)} arguments for {len(sig)}"
    out = []
    for i, (ty, v) in enumerate(zip(sig, a)):
        if ty is N._p:
            out.append(_ptr(v))
        elif issubclass(ty, C._Pointer):  # one struct by reference, or an array of a[i + 1] of them
            structs = [v._obj] if hasattr(v, "_obj") else [v[j] for j in range(a[i + 1])]
            out.append(tuple(_struct(s, N) for s in structs))
        elif ty is N._f:
            out.append(C.c_float(v).value)
        else:
            out.append(int(v))
    return tuple(out)


def _zero(p, nbytes):
    if p:
        C.memset(p, 0, nbytes)


# Kernel outputs that host code reads back get a fixed value, so that no trace depends on
# uninitialised memory (the scenarios that need one say so).
def _fix_topk(a):
    """lasr_logsoftmax_topk: values, ids and gathered log-probs all 0."""
    rows, k = a[2], a[5]
    _zero(a[7], rows * k * 4)
    _zero(a[8], rows * k * 4)
    _zero(a[9], rows * 4)


def _fix_cif_infer(a):
    """lasr_cif_infer: utterance b fires 4 + b tokens (sum_alpha and count 0)."""
    s = a[0]._obj
    (C.c_int32 * s.B).from_address(s.ulen)[:] = [4 + b for b in range(s.B)]
    _zero(s.sum_alpha, 4 * s.B)
    _zero(s.count, 4 * s.B)


_FIXED = {"lasr_logsoftmax_topk": _fix_topk, "lasr_cif_infer": _fix_cif_infer}


class Recorder:
    def __init__(self, mp):
        from liteasr_amd import _native as N
        from liteasr_amd import kernels as K
        from liteasr_amd.models import _fused

        N.load()
        real = N.call
        self.calls = []

        def call(name, *a):
            if name == "lasr_gemm_plan" or name.startswith("lasr_dropout"):
                return real(name, *a)
            self.calls.append((name, _normalise(name, a, N)))
            if name in _FIXED:
                _FIXED[name](a)
            return 0

        mp.setattr(N, "call", call)
        mp.setattr(K, "stream", lambda: 0)
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
        mp.setattr(_fused, "_require_hip", lambda model, xs: None)
        for mod in ("paraformer", "wav2vec2"):  # (they bind the check by name)
            m = importlib.import_module("liteasr_amd.models." + mod)
            if hasattr(m, "_require_hip"):
                mp.setattr(m, "_require_hip", lambda model, xs: None)
        # process-wide state a trace must not inherit from the scenario before it
        mp.setattr(K, "WS", type(K.WS)())
        mp.setattr(K, "_DEFER", type(K._DEFER)())
        mp.setattr(K, "_PUSHED", {"lasr_gemm_dw_group_order": K.DW_GROUP_LPT,
                                  "lasr_gemm_narrow_tiles": K.GEMM_NARROW_TILES})
        torch.manual_seed(0)
        random.seed(0)
        np.random.seed(0)

    def lines(self):
        return [f"{n} {hashlib.sha1(repr(a).encode()).hexdigest()[:12]}" for n, a in self.calls]


def _sym(name):
    """A node or function of nets/functional.py, wherever the tree keeps it."""
    for mod in ("functional", "decode", "paraformer", "transducer", "losses"):
        try:
            m = importlib.import_module("liteasr_amd.nets." + mod)
        except ImportError:
            continue
        if hasattr(m, name):
            return getattr(m, name)
    raise AttributeError(name)


# --------------------------------------------------------------------- models ---
def _u2(dtype="bf16", **kw):
    """The smallest U2 that opens the gates bench.py's `small` opens: d 256, 4 heads (d_k 64),
    256 conv channels, FFN 2048 (the split-K LayerNorm fusions want K >= 1024), 2 + 1 layers; the
    my_U2 preset's rates (attention dropout 0, every other rate 0.1)."""
    from liteasr_amd.models.u2 import U2, U2Config
    from liteasr_amd.utils.cfg import resolve_self

    c = U2Config(input_dim=80, vocab_size=V, enc_dim=256, enc_ff_dim=2048, enc_attn_heads=4, enc_layers=2,
                 dec_dim=256, dec_ff_dim=2048, dec_attn_heads=4, dec_layers=1, dropout_rate=0.1,
                 compute_dtype=dtype, **kw)
    resolve_self(c)
    c.enc_attn_dropout_rate = c.dec_self_attn_dropout_rate = c.dec_src_attn_dropout_rate = 0.0
    return U2(c).train()


def _batch(B=2, T=163, L=6, F=80):
    """163 frames subsample to 40."""
    from liteasr_amd.utils.synthetic import synthetic_batch

    return list(synthetic_batch(B, T, L, V, F_=F, seed=1234))


def _hybrid(w=0.3):
    from liteasr_amd.criterions.hybrid_ctc_attn import HybridCTCLoss, HybridCTCLossConfig

    return HybridCTCLoss(HybridCTCLossConfig(vocab_size=V, smoothing=0.1, ctc_weight=w))


def _train_step(model, crit, batch):
    crit(model, *batch).backward()


# ------------------------------------------------------------------ scenarios ---
def u2_small(mp):
    """bench.py's own small config, model and batch: one bf16 hybrid CTC/attention step."""
    import bench
    from liteasr_amd.criterions.hybrid_ctc_attn import HybridCTCLoss, HybridCTCLossConfig

    cfgd = bench.CONFIGS["small"]
    dev = torch.device("cpu")
    model = bench.build(cfgd, "bf16", 0.1, dev)
    crit = HybridCTCLoss(HybridCTCLossConfig(vocab_size=bench.V, smoothing=0.1, ctc_weight=cfgd["w"]))
    _train_step(model, crit, bench.synthetic(cfgd, 0, dev))


def u2_reduced(mp):
    _train_step(_u2(), _hybrid(), _batch())


def _switch_off(name):
    def run(mp):
        from liteasr_amd.nets import functional as FN

        assert getattr(FN, name) is True
        mp.setattr(FN, name, False)
        _train_step(_u2(), _hybrid(), _batch())

    run.__doc__ = f"The reduced model with functional.{name} off."
    return run


def u2_fp32(mp):
    """The fp32 build: materialised attention, explicit im2col, no row kernel."""
    _train_step(_u2("fp32"), _hybrid(), _batch())


def u2_chunk(mp):
    """A fixed chunk mask (query-dependent encoder mask)."""
    _train_step(_u2(chunk_size=8), _hybrid(), _batch())


def u2_segmented(mp):
    """The backward in three pieces (graph_step's way): cuts inside the subsampling and between
    the two encoder layers."""
    model, crit = _u2(), _hybrid()
    with model.segmented((-1, 1)) as pairs:
        loss = crit(model, *_batch())
    chain = sorted(pairs, key=lambda p: p[0], reverse=True)
    assert [p[0] for p in chain] == [1, -1]
    (g,) = torch.autograd.grad(loss, [chain[0][2]])
    (g,) = torch.autograd.grad(chain[0][1], [chain[1][2]], grad_outputs=g)
    torch.autograd.backward(chain[1][1], g)


def u2_eval(mp):
    model = _u2().eval()
    with torch.no_grad():
        _hybrid()(model, *_batch())


def u2_transformer_abs(mp):
    """Transformer encoder layers with absolute positions: TransformerLayerFn, the abs_pe branch
    of EmbedOutFn, plain attention in the encoder."""
    _train_step(_u2(enc_arch="transformer", use_rel=False), _hybrid(), _batch())


def paraformer_train(mp):
    """Reads back the first decoder pass's top-1 ids (the glancing sampler runs on the host): the
    recorder makes them all 0.  The sampler draws from the module-level `random`, seeded."""
    from liteasr_amd.criterions.paraformer_loss import ParaformerLoss, ParaformerLossConfig

    _train_step(_paraformer().train(), ParaformerLoss(ParaformerLossConfig(vocab_size=V)), _batch())


def _paraformer():
    from liteasr_amd.models.paraformer import Paraformer, ParaformerConfig
    from liteasr_amd.utils.cfg import resolve_self

    c = ParaformerConfig(input_dim=80, vocab_size=V, enc_dim=256, enc_ff_dim=2048, enc_attn_heads=4, enc_layers=2,
                         dec_dim=256, dec_ff_dim=2048, dec_attn_heads=4, dec_layers=1, dropout_rate=0.1)
    resolve_self(c)
    c.enc_attn_dropout_rate = c.dec_self_attn_dropout_rate = 0.0
    return Paraformer(c)


def transducer_train(mp):
    """The model's default encoder: Transformer layers with relative positions, ReLU."""
    from liteasr_amd.criterions.rnnt import RNNTLoss, RNNTLossConfig
    from liteasr_amd.models.transducer import Transducer, TransducerConfig
    from liteasr_amd.utils.cfg import resolve_self

    c = TransducerConfig(input_dim=80, vocab_size=V, enc_dim=256, enc_ff_dim=2048, enc_attn_heads=4, enc_layers=2,
                         dec_dim=64, dec_units=128, dec_layers=2, joint_dim=64, dropout_rate=0.1)
    resolve_self(c)
    c.enc_attn_dropout_rate = 0.0
    _train_step(Transducer(c).train(), RNNTLoss(RNNTLossConfig()), _batch())


def wav2vec2_train(mp):
    """One pretraining step (the mask is drawn from np.random, the negatives from torch's CPU
    generator, both seeded); attention dropout 0.1: the materialised attention with dropout."""
    from liteasr_amd.criterions.wav2vec_loss import Wav2Vec2Loss, Wav2Vec2LossConfig
    from liteasr_amd.models.wav2vec2 import Wav2Vec2, Wav2Vec2Config

    c = Wav2Vec2Config(encoder_layers=2, encoder_embed_dim=128, encoder_ffn_embed_dim=256, encoder_attention_heads=4,
                       dropout=0.1, final_dim=32, latent_vars=16, latent_groups=2, num_negatives=10,
                       conv_feature_layers="[(32, 10, 5)] + [(32, 3, 2)] * 2 + [(32, 2, 2)]")
    model = Wav2Vec2(c).train()
    src = torch.randn(2, 4000)
    Wav2Vec2Loss(Wav2Vec2LossConfig())(model, src, None, None, None).backward()


def u2_inference(mp):
    """encoder_out (through decoding._encode_eager: decoding.encode itself insists on a HIP
    tensor before anything is launched), ctc_logits, decoder_logits on a rescoring batch and two
    DecoderStepCache steps, the second with a beam selection.  Nothing is read back."""
    from liteasr_amd import decoding as D

    model = _u2().eval()
    beam, L = 3, 4
    with torch.no_grad():
        x = _batch(B=1)[0]
        h, T = D._encode_eager(model, x)
        _sym("ctc_logits")(h, model)
        ys = torch.randint(1, V - 1, (beam, L))
        prep = model._prep_targets(ys, torch.full((beam,), L, dtype=torch.int64), beam, 4 * T + 3)
        mem = h.view(1, T, -1).expand(beam, T, h.shape[1]).reshape(beam * T, h.shape[1])
        _sym("decoder_logits")(model, mem, prep.ys_in, prep.dec_mask, D._mem_mask(beam, T, h.device), beam, L + 1, T)
        cache = _sym("DecoderStepCache")(model, h, beam, T, T + 1)
        ids = torch.full((beam,), model.sos, dtype=torch.int32)
        cache.step(ids, 1)
        cache.step(ids, 2, torch.tensor([1, 0, 0]))


def paraformer_inference(mp):
    """Paraformer.inference_batch: the encoder, EncoderOutFn, paraformer_decode.  The token
    counts `ulen` size the decoder pass on the host and the top-1 ids are copied down: the recorder
    writes ulen = (4, 5) and ids 0."""
    model = _paraformer().eval()
    xs, xlens, _, _ = _batch()
    out = model.inference_batch(xs, xlens)
    assert [len(o) for o in out] == [4, 5]


SCENARIOS = {f.__name__: f for f in (u2_small, u2_reduced, u2_fp32, u2_chunk, u2_segmented, u2_eval,
                                     u2_transformer_abs, paraformer_train, transducer_train, wav2vec2_train,
                                     u2_inference, paraformer_inference)}
SCENARIOS.update({"off_" + s: _switch_off(s) for s in SWITCHES})


def record(name, mp):
    rec = Recorder(mp)
    SCENARIOS[name](mp)
    return rec


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_step_trace(name, monkeypatch):
    rec = record(name, monkeypatch)
    got = rec.lines()
    with open(os.path.join(GOLDEN, name + ".txt")) as f:
        want = f.read().split("\n")[:-1]
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            pytest.fail(f"{name}: call {i} differs: expected `{w}`, got `{g}`\n  {rec.calls[i]}")
    if len(got) != len(want):
        i = min(len(got), len(want))
        extra = rec.calls[i] if len(got) > len(want) else want[i]
        pytest.fail(f"{name}: {len(got)} calls for {len(want)} expected; the first one beyond the shorter: {extra}")


def test_switch_off_traces_differ_from_the_default():
    """Every switch changes the launch sequence of the reduced model (or its scenario pins nothing)."""
    def read(n):
        with open(os.path.join(GOLDEN, n + ".txt")) as f:
            return f.read()

    base = read("u2_reduced")
    same = [s for s in SWITCHES if read("off_" + s) == base]
    assert not same, same


if __name__ == "__main__":
    assert sys.argv[1:] == ["--write"], "usage: test_step_trace_cpu.py --write"
    os.makedirs(GOLDEN, exist_ok=True)
    for scen in SCENARIOS:
        path = os.path.join(GOLDEN, scen + ".txt")
        if os.path.exists(path):
            print(f"{scen}: kept")
            continue
        with pytest.MonkeyPatch.context() as mpatch:
            lines = record(scen, mpatch).lines()
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
        print(f"{scen}: {len(lines)} calls")
