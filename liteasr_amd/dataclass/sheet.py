"""Kaldi data-directory sheets (liteasr/dataclass/sheet.py:19-123): AudioSheet over feats.scp +
utt2num_frames (features, taken first when present) or wav.scp with or without segments (raw
waveforms, the pretraining path), and TextSheet over text; iterated line by line.

AudioSheet yields (uttid, where, start, length): a feature entry has start None and its frame
count; a segment has its first sample round(start * 16000) and the reference's length
end - start - 1 (sheet.py:75-77); a whole recording has start 0 and its sample count, which
comes from the WAV header (lasr_wav_probe) where the reference decodes the file to count."""

import os
from typing import Optional

from ..utils import wavio
from .vocab import Vocab


def _lines(path: Optional[str]) -> int:
    if path is None:
        return 0
    n = 0
    with open(path, "r") as f:
        for n, _ in enumerate(f, 1):
            pass
    return n


class AudioSheet(object):
    def __init__(self, data_dir):
        files = os.listdir(data_dir)
        if "feats.scp" in files:
            self.scp = f"{data_dir}/feats.scp"
            assert "utt2num_frames" in files
            self.shape = f"{data_dir}/utt2num_frames"
            self.segments = None
            self.lines = _lines(self.scp)
        elif "wav.scp" in files:
            self.scp = f"{data_dir}/wav.scp"
            self.segments = f"{data_dir}/segments" if "segments" in files else None
            self.lines = max(_lines(self.scp), _lines(self.segments))
        else:
            raise FileNotFoundError(f"wav.scp not found in {data_dir}")

    def __iter__(self):
        if self.scp.endswith("feats.scp"):
            return self._features()
        return self._segments() if self.segments is not None else self._recordings()

    @staticmethod
    def _wav_entries(fscp):
        for line in fscp:
            entry = line.strip().split(None, 1)
            if len(entry) != 2:
                raise ValueError(f"Invalid line is found:\n>   {line}")
            if entry[1].rstrip().endswith("|"):
                raise NotImplementedError(f"wav.scp pipe input is not supported: {entry[1]}")
            yield entry

    def _segments(self):
        with open(self.segments, "r") as fseg, open(self.scp, "r") as fscp:
            fds = dict(self._wav_entries(fscp))
            for line in fseg:
                entry = line.strip().split()
                if len(entry) != 4:
                    raise ValueError(f"Invalid line is found:\n>   {line}")
                uttid, wavid, start, end = entry
                start = round(float(start) * 16000)
                end = round(float(end) * 16000)
                yield uttid, fds[wavid], start, end - start - 1

    def _recordings(self):
        with open(self.scp, "r") as fscp:
            for wavid, wavfd in self._wav_entries(fscp):
                yield wavid, wavfd, 0, wavio.probe(wavfd).frames

    def _features(self):
        with open(self.scp, "r") as fscp, open(self.shape, "r") as fshp:
            while True:
                a, b = fscp.readline(), fshp.readline()
                if not a or not b:
                    break
                e1, e2 = a.strip().split(None, 1), b.strip().split(None, 1)
                if len(e1) != 2 or len(e2) != 2:
                    raise ValueError(f"Invalid line found:\n>\t{a}\n>\t{b}")
                assert e1[0] == e2[0]
                yield e1[0], e1[1], None, int(e2[1])

    def __len__(self):
        return self.lines


class TextSheet(object):
    def __init__(self, data_dir, vocab: Vocab, delimiter: Optional[str] = None):
        self.text = f"{data_dir}/text"
        self.vocab = vocab
        self.delimiter = delimiter
        self.lines = _lines(self.text)

    def __iter__(self):
        with open(self.text, "r") as f:
            for line in f:
                uttid, text = line.strip().split(maxsplit=1)
                tokens = text.split(self.delimiter)
                # delimiter None: the text is one token string looked up character-wise
                ids = self.vocab.lookup(tokens[0]) if self.delimiter is None else self.vocab.lookup(tokens)
                yield uttid, ids, text

    def __len__(self):
        return self.lines
