"""wav2vec 2.0 loss (liteasr/criterions/wav2vec_loss.py:21-37): the mean cross-entropy of the
contrastive logits against class 0.  The model's fused head computes it with the logits
(csrc/w2v.hip lasr_w2v_contrast_fwd), so the criterion calls ``model(xs)`` and returns it."""

from dataclasses import dataclass, field
from typing import Optional

from ..config import LiteasrDataclass
from . import LiteasrLoss, register_criterion


@dataclass
class Wav2Vec2LossConfig(LiteasrDataclass):
    name: Optional[str] = field(default="wav2vec")
    infonce: bool = field(default=False)


@register_criterion("wav2vec", dataclass=Wav2Vec2LossConfig)
class Wav2Vec2Loss(LiteasrLoss):
    def __init__(self, cfg: Wav2Vec2LossConfig, task=None):
        super().__init__(cfg)

    @classmethod
    def build_criterion(cls, cfg, task):
        return cls(cfg, task)

    def __call__(self, model, xs, xlens=None, ys=None, ylens=None):
        logits = model(xs)
        inner = getattr(model, "module", model)  # a data-parallel wrapper keeps the model in .module
        assert inner.get_target(logits, xlens).shape[0] == logits.shape[0]
        return inner.last.loss
