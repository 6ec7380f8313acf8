"""ASR task (liteasr/tasks/asr.py:23-98): vocabulary, feature datasets, model saving.

Data directories with feats.scp are read as the reference reads them.  A directory with wav.scp
and no feats.scp is raw audio: the task's front end (``task.frontend``: Kaldi fbank with
``num_mel_bins`` filters and optional global CMVN statistics, liteasr_amd/utils/frontend.py)
computes the features on the device, in the trainer and in ``inference``.  Every other Kaldi
fbank option is fixed at the value documented there; ``dither`` other than 0 is refused.
``task.frontend.speed_perturb`` (a list of speed factors) applies to the train split of a raw-audio
directory only: valid and test splits, ``inference`` and feats.scp directories ignore it.  So does
``task.frontend.noise`` (a list of noise directories: additive noise mixed in on the device, at
SNRs drawn per utterance; the ``noise_*`` keys beside it) and ``task.frontend.rir`` (a list of
directories of room impulse responses: reverberation convolved on the device; ``rir_prob``,
``rir_seed`` and ``rir_max_mb`` beside it)."""

import inspect
import logging
import os
from dataclasses import dataclass, field
from pathlib import Path
from typing import List, Optional, Union

import torch

from ..config import MISSING, LiteasrDataclass
from ..dataclass.vocab import Vocab
from ..dataset import AudioFileDataset
from ..utils.frontend import (FRAME_SHIFT, SAMPLE_RATE, Fbank, NoiseSpec, RirSpec, check_noise_options,
                              check_rir_options, num_frames, speed_ratios)
from . import LiteasrTask, register_task

logger = logging.getLogger(__name__)


@dataclass
class FrontendConfig(LiteasrDataclass):
    """liteasr_amd extension: the device front end of raw-audio (wav.scp) data directories."""

    num_mel_bins: int = field(default=80)
    cmvn: Optional[str] = field(default=None)  # Kaldi global CMVN statistics, 2 x (num_mel_bins + 1)
    dither: float = field(default=0.0)  # only 0 is supported
    # speed factors of the train split, e.g. [0.9, 1.0, 1.1]: one copy of every utterance per factor,
    # resampled on the device in front of the fbank kernel (None: off)
    speed_perturb: Optional[List[float]] = field(default=None)
    # additive noise of the train split, mixed on the device in front of the fbank kernel: wav.scp
    # directories of 16 kHz 16-bit mono recordings, kept resident in HBM (None: off)
    noise: Optional[List[str]] = field(default=None)
    noise_prob: float = field(default=0.5)  # probability that an utterance is augmented
    # SNR range in dB and range of the number of sources: one pair for all directories, or one per directory
    noise_snr: List[float] = field(default_factory=lambda: [0.0, 15.0])
    noise_sources: List[int] = field(default_factory=lambda: [1, 1])  # each value in 1..8
    noise_seed: int = field(default=0)  # seed of the augmentation generator
    noise_max_mb: int = field(default=2048)  # cap on the resident bank
    # room reverberation of the train split, convolved on the device between the resampler and the
    # mixer: wav.scp directories of 16 kHz 16-bit mono impulse responses of at most 65536 samples,
    # kept resident in HBM (None: off)
    rir: Optional[List[str]] = field(default=None)
    rir_prob: float = field(default=0.5)  # probability that an utterance is reverberated
    rir_seed: int = field(default=0)  # seed of the generator of the reverberation draws
    rir_max_mb: int = field(default=512)  # cap on the resident bank


@dataclass
class ASRConfig(LiteasrDataclass):
    vocab: str = field(default=MISSING)
    train: str = field(default=MISSING)
    valid: str = field(default=MISSING)
    test: List[str] = field(default_factory=list)
    delimiter: Optional[str] = field(default=None)
    save_dir: str = field(default="ckpts")
    frontend: FrontendConfig = field(default_factory=FrontendConfig)


def _frontend_get(cfg):
    fe = cfg.get("frontend") if isinstance(cfg, dict) else getattr(cfg, "frontend", None)
    if fe is None:
        return lambda k, d=None: d
    return fe.get if isinstance(fe, dict) else lambda k, d=None: getattr(fe, k, d)


def _noise_of(get) -> Optional[NoiseSpec]:
    """``frontend.noise*`` as a checked NoiseSpec, None with the option off; the other keys are
    checked either way."""
    def val(key, default):
        v = get(key, None)
        return default if v is None else v

    opts = dict(prob=val("noise_prob", 0.5), snr=list(val("noise_snr", [0.0, 15.0])),
                sources=list(val("noise_sources", [1, 1])), seed=val("noise_seed", 0), max_mb=val("noise_max_mb", 2048))
    dirs = get("noise", None)
    if not dirs:
        check_noise_options(**opts)
        return None
    return NoiseSpec([dirs] if isinstance(dirs, str) else list(dirs), **opts)


def _rir_of(get) -> Optional[RirSpec]:
    """``frontend.rir*`` as a checked RirSpec, None with the option off; the other keys are checked
    either way."""
    def val(key, default):
        v = get(key, None)
        return default if v is None else v

    opts = dict(prob=val("rir_prob", 0.5), seed=val("rir_seed", 0), max_mb=val("rir_max_mb", 512))
    dirs = get("rir", None)
    if not dirs:
        check_rir_options(**opts)
        return None
    return RirSpec([dirs] if isinstance(dirs, str) else list(dirs), **opts)


def _frontend_of(cfg) -> Fbank:
    get = _frontend_get(cfg)
    return Fbank(num_mel_bins=get("num_mel_bins", 80), cmvn=get("cmvn", None), dither=float(get("dither", 0.0) or 0.0),
                 noise=_noise_of(get), rir=_rir_of(get))


@register_task("asr", dataclass=ASRConfig)
class ASRTask(LiteasrTask):
    def __init__(self, cfg: ASRConfig):
        super().__init__(cfg)
        self.vocab = Vocab(cfg.vocab)
        self.save_dir = cfg.save_dir
        Path(self.save_dir).mkdir(parents=True, exist_ok=True)
        self.vocab_size = len(self.vocab)
        self.feat_dim = 0
        self.frontend = _frontend_of(cfg)
        sp = _frontend_get(cfg)("speed_perturb", None)
        self.speed_perturb = [float(s) for s in sp] if sp else None
        speed_ratios(self.speed_perturb)  # a factor the resampler does not take is refused here
        self.noise = self.frontend.noise.spec if self.frontend.noise is not None else None
        self.rir = self.frontend.reverb.spec if self.frontend.reverb is not None else None

    def load_dataset(self, split: str, data_dir: Union[str, list], dataset_cfg=None, postprocess_cfg=None,
                     memory_save: bool = False):
        assert split in ["train", "valid", "test"]

        def one(d):
            logger.info("loading {} data from {}".format(split, d))
            return AudioFileDataset(split=split, data_dir=d, delimiter=self.cfg.delimiter, dataset_cfg=dataset_cfg,
                                    postprocess_cfg=postprocess_cfg, vocab=self.vocab, keep_raw=split == "test",
                                    memory_save=memory_save, num_mel_bins=self.frontend.num_mel_bins,
                                    speed_perturb=self.speed_perturb if split == "train" else None,
                                    noise=self.noise if split == "train" else None,
                                    rir=self.rir if split == "train" else None)

        if isinstance(data_dir, str):
            self.datasets[split] = one(data_dir)
            self.feat_dim = self.datasets[split].feat_dim
        elif isinstance(data_dir, (list, tuple)):
            self.datasets[split] = [one(d) for d in data_dir]
            self.feat_dim = self.datasets[split][0].feat_dim
        else:
            raise TypeError("data_dir with type {} cannot be parsed".format(type(data_dir)))

    def inference(self, x, model, encoder_graph=None):
        """encoder_graph (None: the model's default) is handed to models whose ``inference``
        takes it: whether this utterance's frame count is worth an encoder graph capture.
        ``x``: (1, T, F) features, or (1, n) int16 PCM of a raw-audio utterance on the device, which
        goes through the task's front end first (every sample of it is used)."""
        if x.dtype == torch.int16:
            frames = num_frames(x.shape[-1])
            x = self.frontend(x, torch.full((x.shape[0],), frames, dtype=torch.int32, device=x.device),
                              max_frames=frames)
        if encoder_graph is None or "encoder_graph" not in inspect.signature(model.inference).parameters:
            ids = model.inference(x)
        else:
            ids = model.inference(x, encoder_graph=bool(encoder_graph))
        tokens = self.vocab.lookupi(ids, convert=True)
        return "".join(tokens) if self.cfg.delimiter is None else self.cfg.delimiter.join(tokens)

    def inference_batch(self, xs, xlens, model):
        """One string per row through ``model.inference_batch`` (U2, Paraformer).  ``xs``: (B, T, F)
        features zero-padded past ``xlens`` frames, or (B, S) int16 PCM zero-padded past ``xlens``
        samples, which goes through the task's front end with per-row frame counts first."""
        if xs.dtype == torch.int16:
            frames = [num_frames(int(n)) for n in xlens]
            xs = self.frontend(xs, torch.tensor(frames, dtype=torch.int32, device=xs.device), max_frames=max(frames))
            xlens = frames
        out = []
        for ids in model.inference_batch(xs, xlens):
            tokens = self.vocab.lookupi(list(ids), convert=True)
            out.append("".join(tokens) if self.cfg.delimiter is None else self.cfg.delimiter.join(tokens))
        return out

    def align(self, xs, xlens, ys, ylens, model):
        """Token timestamps through ``model.align`` (U2: CTC forced alignment on the device).  ``xs``
        / ``xlens`` as ``inference_batch`` takes them (features, or int16 PCM that goes through the
        task's front end first); ``ys`` (B, L) token ids padded with -1, ``ylens`` tokens each.

        Returns per row ``([(token, start_s, dur_s)], score)``, or ``(None, -inf)`` for a row that
        cannot be aligned.  Times count encoder frames from the start of the utterance: start_s =
        first * step and dur_s = (end - first) * step with step = frame shift of the front end
        (10 ms) x the model's ``frame_subsampling`` (4) = 0.04 s; the window length and the
        receptive field of the subsampling convolutions are not added."""
        if not hasattr(model, "align"):
            raise TypeError(f"{type(model).__name__} has no align (forced alignment needs a CTC head: U2)")
        if xs.dtype == torch.int16:
            frames = [num_frames(int(n)) for n in xlens]
            xs = self.frontend(xs, torch.tensor(frames, dtype=torch.int32, device=xs.device), max_frames=max(frames))
            xlens = frames
        step = FRAME_SHIFT / SAMPLE_RATE * model.frame_subsampling
        ylens = [int(n) for n in ylens]
        out = []
        for b, rec in enumerate(model.align(xs, xlens, ys, ylens)):
            if rec is None:
                out.append((None, float("-inf")))
                continue
            tokens = self.vocab.lookupi([int(i) for i in ys[b, :ylens[b]].tolist()], convert=True)
            out.append(([(tok, first * step, (end - first) * step) for tok, (first, end) in zip(tokens, rec["spans"])],
                        rec["score"]))
        return out

    def save_model(self, model_name: str, model):
        model.save(os.sep.join((self.save_dir, model_name)))
