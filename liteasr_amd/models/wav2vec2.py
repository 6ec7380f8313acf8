"""wav2vec 2.0 pretraining model (liteasr/models/wav2vec2.py) on the HIP kernels.

Same config schema, registry name ("wav2vec2"), ``state_dict()`` keys / shapes, construction
order and initialisation as the reference: ``model(source (B, S)) -> logits (M B, N + 1)``,
with the ``wav2vec`` criterion (criterions/wav2vec_loss.py) on top.  ``source`` is the fp32
waveform, or the 16-bit PCM batch of the pretraining collator (int16: converted on the device by
``lasr_pcm_to_float``, sample / 32768, before anything else).  The path: feature
extractor (layer 0 a direct kernel, the others GEMMs over a strided view), layer_norm,
linear_input, mask embedding, grouped positional convolution, embed_norm, the pre-norm
Transformer layers of nets/functional.py driven with batch = T' and time = B (the reference
transposes to (T', B, C) before calling batch-first layers, transformer_encoder.py:188-190, and
that is what is reproduced), then the fused head (nets/wav2vec2.py).

Drawn on the host, call for call like the reference (utils/mask.py): the span mask from
``np.random`` and the negative indices from torch's CPU generator; each is one small
host-to-device copy per step.  The Gumbel noise comes from the library's counter hash on the
device; ``gumbel_noise`` (a (B M G, V) fp32 tensor, or None) overrides it for tests.

Reference behaviour kept as it is: the positional convolution ignores ``conv_pos`` /
``conv_pos_groups`` (128 / 16), ``avg_probs`` is not produced, the temperature never decays,
there is no feature penalty, and ``encoder_layerdrop``, ``mask_channel_*``, ``quantize_input``,
``quantize_targets``, ``same_quantizer``, ``target_glu``, ``feature_grad_mult``,
``cross_sample_negatives``, ``codebook_negatives`` and ``layer_norm_first`` are schema fields
the forward never reads.  Extension: ``compute_dtype`` ("bf16" default, "fp32" parity build).
"""

from __future__ import annotations

import ast
from dataclasses import dataclass, field
from types import SimpleNamespace
from typing import Optional, Tuple

import torch
import torch.nn as nn

from .. import kernels as K
from ..config import LiteasrDataclass
from ..nets import functional as FN
from ..nets import wav2vec2 as WN
from ..nets.modules import LayerNorm, _Bound
from ..utils.mask import negative_indices, span_mask
from ..utils.param_store import FlatParams
from . import LiteasrModel, register_model
from ._fused import _require_hip


@dataclass
class Wav2Vec2Config(LiteasrDataclass):
    name: Optional[str] = field(default="wav2vec2")
    encoder_layers: int = field(default=12)
    encoder_embed_dim: int = field(default=768)
    encoder_ffn_embed_dim: int = field(default=3072)
    encoder_attention_heads: int = field(default=12)
    dropout: float = field(default=0.1)
    attention_dropout: float = field(default=0.1)
    activation_dropout: float = field(default=0.0)
    encoder_layerdrop: float = field(default=0.0)
    dropout_input: float = field(default=0.0)
    dropout_features: float = field(default=0.0)
    final_dim: int = field(default=0)
    layer_norm_first: bool = field(default=False)
    conv_feature_layers: str = field(default="[(512, 10, 5)] + [(512, 3, 2)] * 4 + [(512,2,2)] + [(512,2,2)]")
    conv_bias: bool = field(default=False)
    logit_temp: float = field(default=0.1)
    quantize_targets: bool = field(default=True)
    quantize_input: bool = field(default=False)
    same_quantizer: bool = field(default=False)
    target_glu: bool = field(default=False)
    feature_grad_mult: float = field(default=1.0)
    latent_vars: int = field(default=320)
    latent_groups: int = field(default=2)
    latent_dim: int = field(default=0)
    mask_length: int = field(default=10)
    mask_prob: float = field(default=0.65)
    mask_other: float = field(default=0)
    no_mask_overlap: bool = field(default=False)
    mask_min_space: int = field(default=1)
    mask_channel_length: int = field(default=10)
    mask_channel_prob: float = field(default=0.0)
    mask_channel_other: float = field(default=0)
    no_mask_channel_overlap: bool = field(default=False)
    mask_channel_min_space: int = field(default=1)
    num_negatives: int = field(default=100)
    negatives_from_everywhere: bool = field(default=False)
    cross_sample_negatives: int = field(default=0)
    codebook_negatives: int = field(default=0)
    conv_pos: int = field(default=128)
    conv_pos_groups: int = field(default=16)
    latent_temp: Tuple[float, float, float] = field(default=(2, 0.5, 0.999995))
    # liteasr_amd extension
    compute_dtype: str = field(default="bf16")


def _conv_layers(spec):
    """The layer list the reference gets by eval() of the config string (wav2vec2.py:224): a sum
    of literal lists, each optionally repeated; parsed without evaluating arbitrary code."""

    def ev(n):
        if isinstance(n, ast.BinOp) and isinstance(n.op, ast.Add):
            return ev(n.left) + ev(n.right)
        if isinstance(n, ast.BinOp) and isinstance(n.op, ast.Mult):
            a, b = ev(n.left), ev(n.right)
            return a * b
        return ast.literal_eval(n)

    layers = ev(ast.parse(str(spec), mode="eval").body) if isinstance(spec, str) else spec
    return [tuple(int(v) for v in l) for l in layers]


@register_model("wav2vec2", dataclass=Wav2Vec2Config)
class Wav2Vec2(LiteasrModel):
    def __init__(self, cfg: Wav2Vec2Config, task=None):
        super().__init__()
        self.cfg = cfg
        g = lambda k, d=None: getattr(cfg, k, d)  # noqa: E731
        layers = _conv_layers(g("conv_feature_layers"))
        d = int(g("encoder_embed_dim"))
        self.embed = layers[-1][0]
        self.feature_extractor = WN.Convolution(conv_layers=layers, conv_bias=bool(g("conv_bias", False)))
        self.linear_input = nn.Linear(self.embed, d) if self.embed != d else None
        self.dropout_input = nn.Dropout(float(g("dropout_input", 0.0)))
        self.dropout_features = nn.Dropout(float(g("dropout_features", 0.0)))
        final_dim = int(g("final_dim", 0)) if int(g("final_dim", 0)) > 0 else d
        vq_dim = int(g("latent_dim", 0)) if int(g("latent_dim", 0)) > 0 else final_dim
        self.quantizer = WN.GumbelVectorQuantizer(dim=self.embed, num_vars=int(g("latent_vars")),
                                                  temp=tuple(g("latent_temp")) if not isinstance(g("latent_temp"), str)
                                                  else g("latent_temp"), groups=int(g("latent_groups")),
                                                  combine_groups=False, vq_dim=vq_dim)
        self.linear_quantizer = nn.Linear(vq_dim, final_dim)
        self.mask_emb = nn.Parameter(torch.FloatTensor(d).uniform_())
        rate = float(g("dropout", 0.1))
        self.encoder = WN.Wav2Vec2TansformerEncoder(i_dim=d, h_dim=d, ff_dim=int(g("encoder_ffn_embed_dim")),
                                                    n_head=int(g("encoder_attention_heads")),
                                                    n_layer=int(g("encoder_layers")), dropout_rate=rate,
                                                    attn_dropout_rate=rate, ff_dropout_rate=rate)
        self.layer_norm = LayerNorm(self.embed)
        self.linear_final = nn.Linear(d, final_dim)
        cd = str(g("compute_dtype", "bf16")).lower()
        self.compute_dtype = torch.float32 if cd in ("fp32", "float32", "float") else torch.bfloat16
        self.gumbel_noise = None  # test hook: (B M G, V) fp32 noise in place of the device draw
        self.last = None
        self._finalize()

    # ------------------------------------------------------------ flat params
    def _finalize(self):
        groups = []
        for name, mod in self.named_modules():
            if isinstance(mod, _Bound):
                mod._pfx = name
        for i, layer in enumerate(self.encoder.enc_layers):
            groups += layer.flat_groups()
            layer.seed = 1000 + 16 * i
        self.store = FlatParams(self, groups, self.compute_dtype)
        for mod in self.modules():
            if isinstance(mod, _Bound):
                mod._store = self.store
        self.register_buffer("_drop_ctr", torch.zeros(1, dtype=torch.int64), persistent=False)
        self._seed_base = 77
        # extractor weights of layers >= 1 live (C_out, k, C_in); state_dict speaks (C_out, C_in, k)
        self._kc_keys = [f"feature_extractor.conv_layers.{i}.conv.weight"
                         for i, b in enumerate(self.feature_extractor.conv_layers) if b.n_in > 1]
        self._register_state_dict_hook(Wav2Vec2._present_reference_layout)
        self._register_load_state_dict_pre_hook(self._accept_reference_layout)

    @staticmethod
    def _present_reference_layout(module, sd, prefix, local_metadata):
        for k in module._kc_keys:
            if prefix + k in sd:
                sd[prefix + k] = sd[prefix + k].permute(0, 2, 1).contiguous()
        return sd

    def _accept_reference_layout(self, sd, prefix, *unused):
        for k in self._kc_keys:
            if prefix + k in sd:
                sd[prefix + k] = sd[prefix + k].permute(0, 2, 1).contiguous()

    def _apply(self, fn, recurse=True):
        """Device / dtype moves act on the flat buffers; parameters stay views."""
        self.store.apply(fn)
        for mod in self.modules():
            for k, b in mod._buffers.items():
                if b is not None:
                    mod._buffers[k] = fn(b)
        return self

    def flat_parameters(self):
        return self.store

    # ------------------------------------------------------------ operand views
    def _views(self, grad):
        st = self.store
        p = st.grad_view if grad else st.view          # fp32 masters / their gradients
        w = st.grad_view if grad else st.work_view     # GEMM operands (compute dtype)
        has = lambda n: n in st.offsets  # noqa: E731
        return st, p, w, has

    def _front(self, grad):
        st, p, w, has = self._views(grad)
        ext = []
        for i, blk in enumerate(self.feature_extractor.conv_layers):
            n = f"feature_extractor.conv_layers.{i}."
            W = (p if blk.n_in == 1 else w)(n + "conv.weight").view(blk.n_out, -1)
            ext.append(SimpleNamespace(W=W, b=p(n + "conv.bias") if has(n + "conv.bias") else None,
                                       g=p(n + "layer_norm.weight"), beta=p(n + "layer_norm.bias"),
                                       k=blk.kernel, s=blk.stride))
        lin = self.linear_input is not None
        return SimpleNamespace(
            ext=ext, d=self.encoder.h_dim, ln=SimpleNamespace(g=p("layer_norm.weight"), b=p("layer_norm.bias")),
            Wi=w("linear_input.weight") if lin else None, bi=p("linear_input.bias") if lin else None,
            mask_emb=p("mask_emb"), Wpos=p("encoder.embed.weight"), bpos=p("encoder.embed.bias"),
            en=SimpleNamespace(g=p("encoder.embed_norm.weight"), b=p("encoder.embed_norm.bias")))

    def _head(self, grad):
        st, p, w, has = self._views(grad)
        q = self.quantizer
        return SimpleNamespace(
            Wf=w("linear_final.weight"), bf=p("linear_final.bias"), Wp=w("quantizer.weight_proj.weight"),
            bp=p("quantizer.weight_proj.bias"), vars=p("quantizer.vars").view(q.groups * q.num_vars, q.var_dim),
            Wq=w("linear_quantizer.weight"), bq=p("linear_quantizer.bias"), G=q.groups, V=q.num_vars,
            tau=float(q.curr_temp), temp=float(getattr(self.cfg, "logit_temp", 0.1)))

    def front_weights(self):
        return self._front(False)

    def front_grads(self):
        return self._front(True)

    def head_weights(self):
        return self._head(False)

    def head_grads(self):
        return self._head(True)

    # ------------------------------------------------------------------ forward
    def draw_mask(self, batch, frame):
        """wav2vec2.py:319-331 (host, np.random)."""
        c = self.cfg
        return span_mask(batch=batch, frame=frame, prob=float(c.mask_prob), length=int(c.mask_length),
                         policy="static", no_overlap=bool(c.no_mask_overlap), min_mask_num=2,
                         min_interval=int(c.mask_min_space))

    def forward(self, source):
        """wav2vec2.py:271-317: logits (M B, N + 1); the cross-entropy against class 0 is kept in
        ``self.last.loss`` for the criterion."""
        c = self.cfg
        if bool(getattr(c, "negatives_from_everywhere", False)):
            raise NotImplementedError("wav2vec2: negatives_from_everywhere=True is not built on the HIP path "
                                      "(negatives are sampled from the masked targets)")
        if not float(c.mask_prob) > 0:
            raise NotImplementedError("wav2vec2: mask_prob must be > 0 (the reference's forward needs the mask)")
        _require_hip(self, source)
        if source.dtype == torch.int16:  # 16-bit PCM as the pretraining collator delivers it
            source = K.pcm_to_float(source.contiguous())
        dev = source.device
        B = source.shape[0]
        T = self.feature_extractor.out_frames(source.shape[1])
        if T < 2:
            raise ValueError(f"wav2vec2: {source.shape[1]} samples give {T} frames")
        mask = self.draw_mask(B, T)
        M = int(mask[0].sum())
        N = int(c.num_negatives)
        if M < 2:
            raise ValueError(f"wav2vec2: {M} masked frames per utterance; negatives need at least 2")
        midx_h = mask.nonzero()[:, 1].view(B, M).to(torch.int32)
        neg_h = negative_indices(B, M, N)
        assert int(neg_h.min()) >= 0 and int(neg_h.max()) < B * M
        tr = self.training
        rate = self.encoder.dropout_rate
        st = SimpleNamespace(
            adt=self.compute_dtype, training=tr, seed=self._seed_base, B=B, T=T, N=N,
            midx=midx_h.to(dev), neg=neg_h.to(torch.int32).to(dev), noise=self.gumbel_noise,
            p_in=self.dropout_input.p, p_feat=self.dropout_features.p, p_drop=rate, codes=None)
        K.set_dropout_counter(self._drop_ctr)
        K.counter_add(self._drop_ctr, 1)
        self.store.working()
        if torch.is_grad_enabled():
            self.store.ensure_grad()
        x, feats = WN.W2VFrontFn.apply(source, self.mask_emb, self, st)
        enc = self.encoder
        # the layers see batch = T', time = B (transformer_encoder.py:188-190), no mask, no positions
        env = SimpleNamespace(B=T, T=B, H=enc.n_head, adt=self.compute_dtype, training=tr, p_drop=rate, p_ff=rate,
                              p_att=rate, mask=None, msb=0, msq=0, seed=self._seed_base, links=None)
        for layer in enc.enc_layers:
            x = FN.TransformerLayerFn.apply(x, None, layer.feed_forward_norm.weight, layer, env)
        logits, loss = WN.W2VHeadFn.apply(x, feats, self.linear_final.weight, self, st)
        self.last = SimpleNamespace(loss=loss, mask=mask, midx=midx_h, neg=neg_h, codes=st.codes, M=M)
        return logits

    def get_target(self, ys, ylens):
        """wav2vec2.py:382-384: ``ys`` is the logits tensor; class 0 is the positive."""
        return ys.new_zeros(ys.size(0), dtype=torch.long)

    @classmethod
    def build_model(cls, cfg: Wav2Vec2Config, task=None):
        return cls(cfg, task)
