"""Raw-waveform dataset of the pretraining task (liteasr/dataset/pretrain_dataset.py:16-70).

Behaviour kept from the reference: records come from AudioSheet (wav.scp, with or without
segments) in file order; ``batchify`` sorts indices by length (descending, stable) and groups
them with Wav2VecBatch; ``dataset[i]`` is the i-th minibatch (a list of Audio records);
``collator`` crops every utterance to S = min(shortest length of the minibatch, 250000)
samples and returns ``(xs, None, None, None)``.

MI355X-side difference: with ``raw_pcm`` the collator reads the minibatch's windows with one
native call (lasr_wav_read_batch) into an int16 (B, S) tensor, which goes to HBM as it is, at
half the bytes of float32, and is converted by ``lasr_pcm_to_float`` inside
``Wav2Vec2.forward``.  With ``raw_pcm=False`` it returns the reference's float32 tensor
(``pad_sequence`` of the cropped ``Audio.x``); the two are equal bit for bit after the
conversion.  Where the reference would silently return a batch narrower than S (no utterance
has S samples on disk: segments that end beyond their recording), this raises.
"""

import logging
from typing import List

import torch

from ..dataclass.audio_data import Audio
from ..dataclass.sheet import AudioSheet
from ..utils import wavio
from ..utils.batchify import Wav2VecBatch
from .liteasr_dataset import LiteasrDataset

logger = logging.getLogger(__name__)

MAX_CROP = 250000  # pretrain_dataset.py:53 ("should be configurable" there too)


class RawAudioFileDataset(LiteasrDataset):
    def __init__(self, data_cfg: str, dataset_cfg, postprocess_cfg, raw_pcm: bool = True) -> None:
        super().__init__()
        self.data: List[Audio] = []
        self.batchify_policy = None
        self.raw_pcm = bool(raw_pcm)
        for uttid, fd, start, shape in AudioSheet(data_cfg):
            self.data.append(Audio(fd, start, shape, None, None))
            if len(self.data) % 10000 == 0:
                logger.info("number of loaded data: {}".format(len(self.data)))
        if len(self.data) % 10000 != 0:
            logger.info("number of loaded data: {}".format(len(self.data)))
        self.batchify(dataset_cfg)
        self.set_postprocess(postprocess_cfg)

    def batchify(self, dataset_cfg):
        self.batchify_policy = Wav2VecBatch(dataset_cfg)
        order = sorted(range(len(self.data)), key=lambda i: self.data[i].xlen, reverse=True)
        self.batchify_policy.batchify(order, self.data)

    def set_postprocess(self, postprocess_cfg):
        pass

    def collator(self, samples: List[List[Audio]]):
        batch = samples[0]
        S = min(batch[-1].xlen, MAX_CROP)
        if self.raw_pcm:
            xs = torch.empty(len(batch), S, dtype=torch.int16)
            _, got = wavio.read_batch([s.fd for s in batch], [s.start for s in batch], S, out=xs.numpy())
            widest = int(got.max())
        else:
            xs = torch.nn.utils.rnn.pad_sequence([s.x[:S] for s in batch], batch_first=True)
            widest = xs.shape[1]
        if widest < S:
            raise ValueError("no utterance of the minibatch has its {} samples on disk (at most {}): {}".format(
                S, widest, ", ".join(sorted({s.fd for s in batch}))))
        return xs, None, None, None

    def __getitem__(self, index: int):
        if self.batchify_policy is None:
            return self.data[index]
        return [self.data[i] for i in self.batchify_policy[index]]

    def __len__(self):
        return len(self.data) if self.batchify_policy is None else len(self.batchify_policy)
