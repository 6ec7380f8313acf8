"""WAV input of the pretraining path, through the native reader ``libliteasr_io.so``
(include/liteasr_io.h, the ``lasr_wav_*`` entries; csrc/io/wav_io.cpp).

The reference reads waveforms with ``soundfile.read`` (liteasr/dataclass/sheet.py:89,
audio_data.py:31): float64, one whole file per call.  Here samples stay as stored, 16-bit PCM:
``probe`` answers a file's length from its header, ``read`` returns one window and
``read_batch`` fills an int16 [n, count] array (a view of a pinned torch buffer in the collator)
with the same window of n files on a few host threads.  ``sample / 32768`` is the value
``soundfile.read`` gives for PCM_16; the division is exact in float32.  Only 16-bit mono PCM is
accepted; anything else raises ``IOError`` naming the file.
"""

from __future__ import annotations

import ctypes as C
from collections import namedtuple
from typing import Optional, Sequence

import numpy as np

from . import kaldiio as _kio

WavInfo = namedtuple("WavInfo", "rate channels bits frames data_offset")

_BOUND = False


def lib():
    global _BOUND
    L = _kio.lib()
    if not _BOUND:
        i64p, ip = C.POINTER(C.c_int64), C.POINTER(C.c_int)
        L.lasr_wav_probe.argtypes = [C.c_char_p, ip, ip, ip, i64p, i64p]
        L.lasr_wav_read_i16.argtypes = [C.c_char_p, C.c_int64, C.c_int64, C.c_void_p, i64p]
        L.lasr_wav_read_batch.argtypes = [C.c_int, C.POINTER(C.c_char_p), i64p, C.c_int64, C.c_void_p, i64p, C.c_int]
        _BOUND = True
    return L


def probe(path: str) -> WavInfo:
    """(rate, channels, bits, frames, data_offset) from the header; no sample is read."""
    r, c, b, n, o = C.c_int(), C.c_int(), C.c_int(), C.c_int64(), C.c_int64()
    _kio._check(lib().lasr_wav_probe(path.encode(), C.byref(r), C.byref(c), C.byref(b), C.byref(n), C.byref(o)))
    return WavInfo(r.value, c.value, b.value, n.value, o.value)


def read(path: str, start: int = 0, count: Optional[int] = None):
    """Samples [start, start + count) as (int16 [count], got): what lies past the end of the
    data is zero and ``got`` says how many samples were there.  count None: to the end."""
    if count is None:
        count = max(probe(path).frames - start, 0)
    out = np.empty(count, dtype=np.int16)
    got = C.c_int64()
    _kio._check(lib().lasr_wav_read_i16(path.encode(), start, count, out.ctypes.data_as(C.c_void_p), C.byref(got)))
    return out, got.value


def read_into(path: str, out: np.ndarray, start: int = 0) -> int:
    """Samples [start, start + len(out)) into ``out`` (int16, C-contiguous; a slice of a pinned
    buffer, say); returns how many were there, the rest is zero."""
    assert out.dtype == np.int16 and out.ndim == 1 and out.flags.c_contiguous
    got = C.c_int64()
    _kio._check(lib().lasr_wav_read_i16(path.encode(), start, out.shape[0], out.ctypes.data_as(C.c_void_p),
                                        C.byref(got)))
    return got.value


def read_batch(paths: Sequence[str], starts: Sequence[int], count: int, out: Optional[np.ndarray] = None,
               nthreads: int = 0):
    """The window [starts[i], starts[i] + count) of every file into an int16 [n, count] array
    (``out``: C-contiguous, e.g. the numpy view of a torch buffer).  Returns (array, got int64[n])."""
    n = len(paths)
    assert len(starts) == n
    if out is None:
        out = np.empty((n, count), dtype=np.int16)
    assert out.dtype == np.int16 and out.flags.c_contiguous and out.shape == (n, count)
    got = np.zeros(n, dtype=np.int64)
    parr = (C.c_char_p * max(n, 1))(*[p.encode() for p in paths])
    sarr = (C.c_int64 * max(n, 1))(*[int(s) for s in starts])
    _kio._check(lib().lasr_wav_read_batch(n, parr, sarr, count, out.ctypes.data_as(C.c_void_p),
                                          got.ctypes.data_as(C.POINTER(C.c_int64)), nthreads))
    return out, got
