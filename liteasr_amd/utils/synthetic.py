"""Synthetic fbank batches for throughput runs (SURVEY.md §8(d) input recipe).

xs ~ N(0, 1) of shape (B, T, F) zeroed past each length, xlens ~ U[0.95 T, T] with
xlens[0] = T (the collator's descending sort puts the longest utterance first,
liteasr/dataset/asr_dataset.py:107-110), ys ~ U{1 .. V-2} (never blank 0 nor sos/eos
V-1) padded with -1, ylens ~ U[L/2, L] with ylens[0] = L.  Drawn on the host from one
seeded torch.Generator, in that order, so every rank/run gets reproducible inputs.
"""

from __future__ import annotations

import torch


def synthetic_batch(B: int, T: int, L: int, V: int, F_: int = 80, seed: int = 0):
    gen = torch.Generator().manual_seed(seed)
    xlens = torch.randint(int(0.95 * T), T + 1, (B,), generator=gen)
    xlens[0] = T
    xs = torch.randn(B, T, F_, generator=gen)
    frame = torch.arange(T)
    xs[frame[None, :] >= xlens[:, None]] = 0.0
    ylens = torch.randint(max(1, L // 2), L + 1, (B,), generator=gen)
    ylens[0] = L
    ys = torch.randint(1, V - 1, (B, L), generator=gen)
    ys[torch.arange(L)[None, :] >= ylens[:, None]] = -1
    return xs, xlens, ys, ylens


# ---- synthetic raw-audio data directories (tests, tools/fbank_bench.py, tools/compute_cmvn.py) ----
def write_wav(path: str, pcm) -> None:
    """``pcm`` (int16 samples) as a 16 kHz, 16-bit mono WAV file."""
    import wave

    import numpy as np

    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(np.ascontiguousarray(pcm, dtype="<i2").tobytes())


def synthetic_wave(n: int, rng):
    """n int16 samples: two tones under a slow envelope plus noise, at a speech-like level."""
    import numpy as np

    t = np.arange(n) / 16000.0
    f0, f1 = rng.uniform(90, 400), rng.uniform(500, 3000)
    env = 0.6 + 0.4 * np.sin(2 * np.pi * rng.uniform(1.0, 4.0) * t)
    x = env * (0.30 * np.sin(2 * np.pi * f0 * t) + 0.15 * np.sin(2 * np.pi * f1 * t + 1.0))
    x = x + 0.05 * rng.standard_normal(n)
    return np.clip(np.round(x * 32768), -32768, 32767).astype(np.int16)


def synthetic_wav_dir(root: str, lengths, seed: int = 0, tokens: str = "abcdefgh", lines: int = 0) -> str:
    """A Kaldi data directory ``root`` of raw audio: one seeded WAV file per entry of ``lengths``
    (samples), wav.scp, text (a short seeded token string per utterance, looked up character-wise)
    and vocab.txt (``tokens`` and ``<unk>``).  With ``lines`` above len(lengths) wav.scp and text go
    on to that many entries, cycling over the files.  Returns ``root``."""
    import os

    import numpy as np

    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "wav"), exist_ok=True)
    with open(os.path.join(root, "vocab.txt"), "w") as f:
        for i, tok in enumerate(list(tokens) + ["<unk>"], start=1):
            f.write(f"{tok} {i}\n")
    paths, texts = [], []
    for i, n in enumerate(lengths):
        paths.append(os.path.join(root, "wav", f"utt{i:04d}.wav"))
        write_wav(paths[-1], synthetic_wave(int(n), rng))
        texts.append("".join(rng.choice(list(tokens), size=int(rng.integers(2, 7)))))
    with open(os.path.join(root, "wav.scp"), "w") as scp, open(os.path.join(root, "text"), "w") as txt:
        for j in range(max(len(paths), int(lines))):
            scp.write(f"utt{j:04d} {paths[j % len(paths)]}\n")
            txt.write(f"utt{j:04d} {texts[j % len(paths)]}\n")
    return root


def synthetic_rir_dir(root: str, lengths, seed: int = 0) -> str:
    """A wav.scp directory ``root`` of synthetic room impulse responses, one per entry of ``lengths``
    (samples): Gaussian noise under an exponential decay (60 dB over the recording, at a tenth of
    the direct path's level) with one unit direct-path peak, 32767, within the first 20 samples.
    Returns ``root``."""
    import os

    import numpy as np

    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "wav"), exist_ok=True)
    with open(os.path.join(root, "wav.scp"), "w") as scp:
        for i, n in enumerate(lengths):
            n = int(n)
            h = 0.1 * rng.standard_normal(n) * 10.0 ** (-3.0 * np.arange(n) / max(n, 1))
            h[int(rng.integers(min(n, 20)))] = 1.0
            path = os.path.join(root, "wav", f"rir{i:04d}.wav")
            write_wav(path, np.clip(np.round(h * 32767), -32767, 32767).astype(np.int16))
            scp.write(f"rir{i:04d} {path}\n")
    return root
