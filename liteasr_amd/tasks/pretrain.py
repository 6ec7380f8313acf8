"""Pretraining task (liteasr/tasks/pretrain.py:20-51): raw-waveform datasets from wav.scp data
directories for the wav2vec 2.0 model; no vocabulary, no transcripts."""

import logging
import os
from dataclasses import dataclass, field
from pathlib import Path

from ..config import MISSING, LiteasrDataclass
from ..dataset import RawAudioFileDataset
from . import LiteasrTask, register_task

logger = logging.getLogger(__name__)


@dataclass
class PreTrainConfig(LiteasrDataclass):
    train: str = field(default=MISSING)
    valid: str = field(default=MISSING)
    save_dir: str = field(default="ckpts")
    # liteasr_amd extension: batches travel to the GPU as 16-bit PCM (False: the reference's
    # float32 collation)
    raw_pcm: bool = field(default=True)


@register_task("pretrain", dataclass=PreTrainConfig)
class PreTrainTask(LiteasrTask):
    def __init__(self, cfg: PreTrainConfig):
        super().__init__(cfg)
        self.save_dir = cfg.save_dir
        Path(self.save_dir).mkdir(parents=True, exist_ok=True)

    def load_dataset(self, split: str, data_cfg: str, dataset_cfg=None, postprocess_cfg=None,
                     memory_save: bool = False):
        assert split in ["train", "valid"]
        logger.info("loading {} data from {}".format(split, data_cfg))
        self.datasets[split] = RawAudioFileDataset(data_cfg, dataset_cfg, postprocess_cfg,
                                                   raw_pcm=bool(getattr(self.cfg, "raw_pcm", True)))

    def save_model(self, model_name: str, model):
        model.save(os.sep.join((self.save_dir, model_name)))
