"""Per-utterance record of a dataset (the Audio record of liteasr/dataclass/audio_data.py).

Holds where the utterance's input lives, its length and its token ids.  A feature entry
(``start`` None) has ``fd`` a Kaldi "ark:offset" path and ``shape`` frames; a raw-waveform
entry (from wav.scp / segments, the pretraining path) has ``fd`` a WAV file, ``start`` its
first sample and ``shape`` samples.  Both are decoded lazily by the native readers.
Positional construction order (fd, start, shape, tokenids, text) is the reference's.
"""

from typing import Optional, Tuple

import torch

from ..utils import wavio
from ..utils.kaldiio import load_mat


class Audio(object):
    __slots__ = ("fd", "start", "shape", "tokenids", "text")

    def __init__(self, fd: str, start: Optional[int], shape: int, tokenids: Optional[Tuple[int]],
                 text: Optional[str]):
        self.fd, self.start, self.shape, self.tokenids, self.text = fd, start, shape, tokenids, text

    def __repr__(self):
        return f"Audio(fd={self.fd!r}, start={self.start}, shape={self.shape}, ylen={self.ylen})"

    def __eq__(self, other):
        return isinstance(other, Audio) and all(getattr(self, k) == getattr(other, k) for k in self.__slots__)

    @property
    def x(self) -> torch.Tensor:
        if self.start is not None:
            # samples[start : start + xlen] of soundfile's PCM_16 decode (int16 / 32768, exact in
            # float32), audio_data.py:30-33; a window past the end of the file comes back shorter
            pcm, got = wavio.read(self.fd, self.start, max(self.xlen, 0))
            return torch.from_numpy(pcm[:got].astype("float32") / 32768.0)
        return torch.from_numpy(load_mat(self.fd))

    @property
    def xlen(self) -> int:
        return self.shape

    @property
    def y(self):
        return None if self.tokenids is None else torch.tensor(self.tokenids)

    @property
    def ylen(self) -> int:
        return 0 if self.tokenids is None else len(self.tokenids)


class WavAudio(Audio):
    """An utterance of task=asr read from wav.scp: the record keeps its sample window (``start``,
    ``shape`` samples) and its length for batching, ``xlen``, is the frame count of the fbank
    front end.  ``x`` is the window as stored, 16-bit PCM: the features are computed on the
    device (liteasr_amd/utils/frontend.py)."""

    __slots__ = ("frames",)

    def __init__(self, fd, start, shape, tokenids, text, frames: int):
        super().__init__(fd, start, shape, tokenids, text)
        self.frames = frames

    def __repr__(self):
        return (f"WavAudio(fd={self.fd!r}, start={self.start}, shape={self.shape}, frames={self.frames}, "
                f"ylen={self.ylen})")

    def __eq__(self, other):
        return isinstance(other, WavAudio) and all(getattr(self, k) == getattr(other, k)
                                                   for k in Audio.__slots__ + WavAudio.__slots__)

    @property
    def x(self) -> torch.Tensor:
        pcm, got = wavio.read(self.fd, self.start, self.shape)
        if got < self.shape:
            raise ValueError(f"{self.fd}: {got} of the utterance's {self.shape} samples are on disk")
        return torch.from_numpy(pcm)

    @property
    def xlen(self) -> int:
        return self.frames


class SpeedWavAudio(WavAudio):
    """A speed-perturbed copy of a wav.scp utterance (task.frontend.speed_perturb): ``shape`` is
    the source window's samples as stored, ``ratio`` the speed factor as a reduced fraction
    (p, q), ``samples`` = ceil(q shape / p) what the device resampler makes of it and ``frames``
    (``xlen``) the frame count of those.  ``x`` is the source window, unperturbed."""

    __slots__ = ("ratio", "samples")

    def __init__(self, fd, start, shape, tokenids, text, frames: int, ratio: Tuple[int, int], samples: int):
        super().__init__(fd, start, shape, tokenids, text, frames)
        self.ratio, self.samples = tuple(ratio), samples

    def __repr__(self):
        return (f"SpeedWavAudio(fd={self.fd!r}, start={self.start}, shape={self.shape}, ratio={self.ratio}, "
                f"samples={self.samples}, frames={self.frames}, ylen={self.ylen})")

    def __eq__(self, other):
        return isinstance(other, SpeedWavAudio) and all(
            getattr(self, k) == getattr(other, k)
            for k in Audio.__slots__ + WavAudio.__slots__ + SpeedWavAudio.__slots__)
