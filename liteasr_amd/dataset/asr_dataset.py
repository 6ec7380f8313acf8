"""Feature dataset with length-sorted minibatches (liteasr/dataset/asr_dataset.py:24-155).

Behaviour kept from the reference: utterances are read from feats.scp / utt2num_frames /
text in file order; ``batchify`` sorts indices by frame count (descending, stable) and
groups them with SeqBatch/FrameBatch; ``dataset[i]`` is the i-th minibatch (a list of
Audio records); ``collator`` pads xs with 0 and ys with -1 and returns int64 lengths.

MI355X-side difference: the collator decodes the whole minibatch with one native call
(lasr_ark_read_padded) straight into the padded float32 batch instead of loading and
padding utterance by utterance.  With a device-capable postprocess (SpecAugment) the
collator only draws the augmentation plan and returns it as a fifth element; the trainer
applies it to the batch on the GPU.  (The reference's ``memory_save`` pickle dump of
batches is not carried over: it serialises Python objects to disk and is not on the step
path.)

Raw audio (a directory with wav.scp and no feats.scp; the reference has no such path for
task=asr): every record keeps its sample window and is batched by its fbank frame count
``1 + (n - 400) // 160``, so the SeqBatch / FrameBatch budgets mean frames as they do for
feats.scp; utterances below 400 samples (no frame) are dropped with one logged count;
``feat_dim`` is the front end's ``num_mel_bins``.  The collator reads the minibatch with one
native call (lasr_wav_read_batch) into a zero-padded int16 (B, Smax) tensor and returns it with
the frame counts; the trainer turns it into features on the GPU (liteasr_amd/utils/frontend.py)
before the SpecAugment plan, drawn here from the frame counts as for features, is applied.

Speed perturbation (``speed_perturb``, the train split of a raw-audio directory only) is Kaldi's
static copy: for each factor in the listed order, every utterance in file order, as one
SpeedWavAudio whose ``xlen`` is the frame count of its ceil(q n / p) resampled samples, so the
length sort, the batch budgets and the SpecAugment plan see what the model will; a copy left
without a frame is dropped and counted like a short utterance.  The collator still reads the
source samples with one native call and appends a ResamplePlan (source and resampled counts and
the ratio of every row); the resampling itself runs on the device (liteasr_amd/utils/frontend.py).

Additive noise (``noise``, a NoiseSpec; the train split of a raw-audio directory only) is drawn per
step: the dataset holds the bank's index only (offset, length and directory of every noise
recording, from the WAV headers), and the collator draws per row, from a generator of the
dataset's own, whether it is augmented, a directory, the number of sources and per source a
recording, a start and an SNR, and appends them as a NoisePlan, the batch's last element.  The
mixing runs on the device, on the resampled samples when both options are on.

Room reverberation (``rir``, a RirSpec; the train split of a raw-audio directory only) is drawn per
step in the same way, from a generator of its own: the dataset holds the RIR bank's index only, the
collator draws per utterance whether it is reverberated, a directory and an RIR, and appends a
ReverbPlan after the ResamplePlan and before the NoisePlan.
"""

import logging
import os
from typing import List, Optional

import numpy as np
import torch

from ..dataclass.audio_data import Audio, SpeedWavAudio, WavAudio
from ..dataclass.sheet import AudioSheet, TextSheet
from ..utils import wavio
from ..utils.batchify import FrameBatch, SeqBatch
from ..utils.frontend import (ResamplePlan, draw_noise_plan, draw_reverb_plan, num_frames, resampled_samples,
                              speed_ratios, used_samples)
from ..utils.kaldiio import read_padded
from ..utils.transform import PostProcess
from .liteasr_dataset import LiteasrDataset

logger = logging.getLogger(__name__)


class AudioFileDataset(LiteasrDataset):
    def __init__(self, split: str, data_dir: str, delimiter: Optional[str], dataset_cfg, postprocess_cfg, vocab,
                 keep_raw=False, memory_save=False, num_mel_bins: int = 80, speed_perturb=None, noise=None,
                 rir=None):
        super().__init__()
        if memory_save:
            raise NotImplementedError("memory_save (pickled batch dumps) is not supported")
        self.split = split
        self.data: List[Audio] = []
        self.uttids: List[str] = []  # the utterance id of self.data[i] (the records do not carry it)
        self.batchify_policy = None
        self.postprocess = None
        if postprocess_cfg is not None:
            self.set_postprocess(postprocess_cfg)
        audios = AudioSheet(data_dir)
        texts = TextSheet(data_dir, vocab=vocab, delimiter=delimiter)
        assert len(audios) == len(texts)
        self.wav = audios.scp.endswith("wav.scp")  # raw audio: features come from the device front end
        self.speed = speed_ratios(speed_perturb) if split == "train" else None  # [(p, q)] or None
        if self.speed is not None and not self.wav:
            logger.info("{}: speed_perturb is ignored for a feats.scp directory".format(data_dir))
            self.speed = None
        self.speed_table = list(dict.fromkeys(self.speed)) if self.speed is not None else None  # the distinct ratios
        self.noise = noise if split == "train" else None  # a NoiseSpec or None
        if self.noise is not None and not self.wav:
            logger.info("{}: noise is ignored for a feats.scp directory".format(data_dir))
            self.noise = None
        # where every noise recording lies in the bank (never the samples: workers stay light)
        self.noise_index = self.noise.index() if self.noise is not None else None
        self._noise_rng = None  # (pid, Generator), made in the process that collates
        self.rir = rir if split == "train" else None  # a RirSpec or None
        if self.rir is not None and not self.wav:
            logger.info("{}: rir is ignored for a feats.scp directory".format(data_dir))
            self.rir = None
        self.rir_index = self.rir.index() if self.rir is not None else None  # never the samples
        self._rir_rng = None  # (pid, Generator), as for the noise
        short = 0
        records = list(zip(audios, texts))
        for ratio in self.speed if self.speed is not None else [None]:
            for (uttid, fd, start, shape), (uttid_t, ids, text) in records:
                assert uttid_t == uttid
                if not self.wav:
                    self.data.append(Audio(fd, start, shape, ids, text if keep_raw else None))
                    self.uttids.append(uttid)
                elif ratio is not None:
                    p, q = ratio
                    samples = resampled_samples(shape, p, q)
                    if num_frames(samples) == 0:
                        short += 1
                    else:
                        self.data.append(SpeedWavAudio(fd, start, shape, ids, text if keep_raw else None,
                                                       num_frames(samples), (p, q), samples))
                        self.uttids.append(uttid)
                elif num_frames(shape) == 0:
                    short += 1
                else:
                    self.data.append(WavAudio(fd, start, shape, ids, text if keep_raw else None, num_frames(shape)))
                    self.uttids.append(uttid)
        if short:
            logger.warning("{}: dropped {} utterance(s) shorter than one 25 ms frame".format(data_dir, short))
        self.feat_dim = int(num_mel_bins) if self.wav else self.data[0].x.shape[-1]
        if dataset_cfg is not None:
            self.batchify(dataset_cfg)

    def batchify(self, dataset_cfg):
        if dataset_cfg.batch_count == "seq":
            policy = SeqBatch
        elif dataset_cfg.batch_count == "frame":
            policy = FrameBatch
        else:
            logger.error(f"unsupport strategy {dataset_cfg.batch_count}")
            raise ValueError
        self.batchify_policy = policy(dataset_cfg)
        order = sorted(range(len(self.data)), key=lambda i: self.data[i].xlen, reverse=True)
        self.batchify_policy.batchify(order, self.data)

    def set_postprocess(self, postprocess_cfg):
        self.postprocess = PostProcess(postprocess_cfg)

    @property
    def train(self):
        return self.split == "train"

    def collator(self, samples: List[List[Audio]]):
        batch = samples[0]
        B = len(batch)
        xlens = torch.tensor([s.xlen for s in batch], dtype=torch.long)
        ylens = torch.tensor([s.ylen for s in batch], dtype=torch.long)
        post = self.postprocess if (self.train and self.postprocess is not None and len(self.postprocess)) else None
        plan = rplan = vplan = nplan = None
        if post is not None and post.device_capable:
            # draw the augmentation here (same RNG order as the reference's per-utterance
            # calls); the pixels are produced on the GPU by the trainer (apply_batch)
            plan = post.plan_batch(xlens.tolist(), self.feat_dim)
            post = None
        if self.wav:
            if post is not None:
                raise NotImplementedError("raw-audio batches take device-side postprocessing only (spec_aug)")
            xs = self._collate_pcm(batch)
            if self.speed is not None:
                rplan = self._resample_plan(batch)
            ns = [s.samples if isinstance(s, SpeedWavAudio) else s.shape for s in batch]
            if self.rir is not None:
                vplan = draw_reverb_plan(self._rir_generator(), self.rir, self.rir_index, ns)
            if self.noise is not None:
                nplan = draw_noise_plan(self._noise_generator(), self.noise, self.noise_index, ns)
        elif post is None and all(s.start is None for s in batch):
            tmax = int(xlens.max()) if B else 0
            xs = torch.empty(B, tmax, self.feat_dim, dtype=torch.float32)
            _, lens = read_padded([s.fd for s in batch], tmax, self.feat_dim, out=xs.numpy())
            if not np.array_equal(lens, xlens.numpy()):
                raise ValueError("feature frame counts disagree with utt2num_frames")
        else:
            xs = [post(s.x) if post is not None else s.x for s in batch]
            xs = torch.nn.utils.rnn.pad_sequence(xs, batch_first=True, padding_value=0)
        lmax = int(ylens.max()) if B else 0
        ys = torch.full((B, lmax), -1, dtype=torch.long)
        for i, s in enumerate(batch):
            if s.ylen:
                ys[i, : s.ylen] = torch.tensor(s.tokenids, dtype=torch.long)
        out = (xs, xlens, ys, ylens) if plan is None else (xs, xlens, ys, ylens, plan)
        out = out if rplan is None else out + (rplan,)
        out = out if vplan is None else out + (vplan,)
        return out if nplan is None else out + (nplan,)

    def _noise_generator(self):
        """The dataset's own generator for the noise draws, seeded from ``noise_seed`` and torch's
        initial seed of the collating process (a DataLoader worker's follows the loader's per-epoch
        base seed).  Python's, numpy's and torch's global streams are not touched."""
        pid = os.getpid()
        if self._noise_rng is None or self._noise_rng[0] != pid:
            self._noise_rng = (pid, np.random.default_rng([self.noise.seed, torch.initial_seed() % (1 << 63)]))
        return self._noise_rng[1]

    def _rir_generator(self):
        """The dataset's own generator for the reverberation draws, made like the noise's from
        ``rir_seed``; the trailing 1 keeps the two streams apart at equal seeds."""
        pid = os.getpid()
        if self._rir_rng is None or self._rir_rng[0] != pid:
            self._rir_rng = (pid, np.random.default_rng([self.rir.seed, torch.initial_seed() % (1 << 63), 1]))
        return self._rir_rng[1]

    def __getstate__(self):
        state = dict(self.__dict__)
        state["_noise_rng"] = state["_rir_rng"] = None  # a worker makes its own
        return state

    def _resample_plan(self, batch: List[SpeedWavAudio]) -> ResamplePlan:
        rows = torch.tensor([[s.shape, s.samples, self.speed_table.index(s.ratio)] for s in batch],
                            dtype=torch.int32).reshape(len(batch), 3)
        return ResamplePlan(rows, self.speed_table, max((s.samples for s in batch), default=0))

    @staticmethod
    def _collate_pcm(batch: List[WavAudio]):
        """int16 (B, Smax), Smax the longest sample count; zero past every utterance's own samples."""
        B = len(batch)
        smax = max((s.shape for s in batch), default=0)
        xs = torch.empty(B, smax, dtype=torch.int16)
        arr = xs.numpy()
        _, got = wavio.read_batch([s.fd for s in batch], [s.start for s in batch], smax, out=arr)
        for i, s in enumerate(batch):
            need = s.shape if isinstance(s, SpeedWavAudio) else used_samples(s.frames)  # resampling reads all
            if got[i] < need:
                raise ValueError("{}: {} samples from {} on disk, {} frames need {}".format(
                    s.fd, int(got[i]), s.start, s.frames, need))
            arr[i, s.shape:] = 0  # a segment's window may run on into the recording
        return xs

    def __getitem__(self, index):
        if self.batchify_policy is not None:
            return [self.data[i] for i in self.batchify_policy[index]]
        return self.data[index]

    def __len__(self):
        return len(self.batchify_policy) if self.batchify_policy is not None else len(self.data)
