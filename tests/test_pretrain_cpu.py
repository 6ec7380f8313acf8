"""The pretraining data path without a GPU: the native WAV reader against the standard library's
``wave`` module and hand-built headers, then AudioSheet, Wav2VecBatch, RawAudioFileDataset and
its collator against what the reference's own classes produced (tests/golden/pretrain.npz, made
by tests/golden/make_golden_pretrain.py), the 250000-sample crop, config composition, the CLI's
help and the I/O library's exported symbols."""

import os
import re
import struct
import subprocess
import wave

import numpy as np
import pytest
import torch

import pretrain_cases as C
from liteasr_amd.config.compose import compose
from liteasr_amd.dataclass.audio_data import Audio
from liteasr_amd.dataclass.sheet import AudioSheet
from liteasr_amd.dataset import RawAudioFileDataset
from liteasr_amd.utils import wavio
from liteasr_amd.utils.batchify import Wav2VecBatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pcm(n, seed):
    pcm = np.random.default_rng(seed).integers(-32768, 32768, size=n).astype("<i2")
    pcm[:3] = (-32768, 32767, 0)[:n]
    return pcm


def _write(path, pcm, rate=16000):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(pcm.tobytes())
    return str(path)


def _wave_window(path, start, count):
    """(zero-padded int16 [count], got) through wave.readframes."""
    with wave.open(path, "rb") as w:
        n = w.getnframes()
        if start < n:
            w.setpos(start)
            got = np.frombuffer(w.readframes(min(count, n - start)), dtype="<i2")
        else:
            got = np.zeros(0, dtype="<i2")
    out = np.zeros(count, dtype=np.int16)
    out[:len(got)] = got
    return out, len(got)


# ------------------------------------------------------------------ reader vs wave ---
@pytest.mark.parametrize("n", [1, 777, 16000])
def test_reader_matches_wave(tmp_path, n):
    p = _write(tmp_path / "a.wav", _pcm(n, n), rate=8000 if n == 777 else 16000)
    info = wavio.probe(p)
    with wave.open(p, "rb") as w:
        assert (info.rate, info.channels, info.bits, info.frames) == (w.getframerate(), 1, 16, w.getnframes())
    assert info.data_offset == 44
    windows = [(0, n), (0, n + 9), (n // 2, n), (n - 1, 5), (n, 4), (n + 3, 2), (3, 0), (0, 1), (n // 3, n // 3)]
    for start, count in windows:
        out, got = wavio.read(p, start, count)
        ref, ref_got = _wave_window(p, start, count)
        assert out.dtype == np.int16 and got == ref_got and np.array_equal(out, ref), (start, count)
    whole, got = wavio.read(p)
    assert got == n and np.array_equal(whole, _wave_window(p, 0, n)[0])
    assert wavio.read(p, n)[0].shape == (0,)


# --------------------------------------------------------------- hand-built headers ---
def _chunk(cid, body, size=None):
    return cid + struct.pack("<I", len(body) if size is None else size) + body + (b"\0" if len(body) & 1 else b"")


def _fmt(tag=1, ch=1, rate=16000, bits=16, extensible=False, sub=1):
    body = struct.pack("<HHIIHH", 0xFFFE if extensible else tag, ch, rate, rate * ch * bits // 8, ch * bits // 8, bits)
    if extensible:
        body += struct.pack("<HHIH", 22, bits, 4, sub) + bytes.fromhex("000000001000800000aa00389b71")
    return _chunk(b"fmt ", body)


def _riff(*chunks):
    body = b"WAVE" + b"".join(chunks)
    return b"RIFF" + struct.pack("<I", len(body)) + body


SAMPLES = _pcm(301, 5)
DATA = SAMPLES.tobytes()

ACCEPTED = {
    "extensible": _riff(_fmt(extensible=True), _chunk(b"data", DATA)),
    "list_before_data": _riff(_chunk(b"LIST", b"x" * 26), _fmt(), _chunk(b"fact", b"\0" * 4), _chunk(b"data", DATA)),
    "odd_chunk_with_pad": _riff(_fmt(), _chunk(b"junk", b"j" * 7), _chunk(b"data", DATA)),
    "size_ffffffff": _riff(_fmt(), _chunk(b"data", DATA, 0xFFFFFFFF)),
    "size_zero": _riff(_fmt(), _chunk(b"data", DATA, 0)),
    "size_beyond_file": _riff(_fmt(), _chunk(b"data", DATA, 100000)),
}
REFUSED = {
    "eight_bit": (_riff(_fmt(bits=8), _chunk(b"data", DATA)), "8-bit"),
    "stereo": (_riff(_fmt(ch=2), _chunk(b"data", DATA)), "2 channels"),
    "ieee_float": (_riff(_fmt(tag=3, bits=32), _chunk(b"data", DATA)), "float"),
    "extensible_float": (_riff(_fmt(extensible=True, sub=3), _chunk(b"data", DATA)), "float"),
    "twenty_bytes": (_riff(_fmt(), _chunk(b"data", DATA))[:20], "truncated"),
    "not_riff": (b"A" * 200, "not a RIFF/WAVE"),
    "no_data_chunk": (_riff(_fmt(), _chunk(b"LIST", b"x" * 10)), "no data chunk"),
}


@pytest.mark.parametrize("name", sorted(ACCEPTED))
def test_accepted_headers(tmp_path, name):
    p = str(tmp_path / (name + ".wav"))
    open(p, "wb").write(ACCEPTED[name])
    info = wavio.probe(p)
    assert (info.rate, info.channels, info.bits, info.frames) == (16000, 1, 16, 301)
    assert ACCEPTED[name][info.data_offset:info.data_offset + 602] == DATA
    out, got = wavio.read(p, 0, 310)
    assert got == 301 and np.array_equal(out[:301], SAMPLES) and not out[301:].any()
    out, got = wavio.read(p, 300, 2)
    assert got == 1 and out.tolist() == [int(SAMPLES[300]), 0]


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refused_headers_name_the_file(tmp_path, name):
    p = str(tmp_path / (name + ".wav"))
    blob, why = REFUSED[name]
    open(p, "wb").write(blob)
    for call in (lambda: wavio.probe(p), lambda: wavio.read(p, 0, 4), lambda: wavio.read_batch([p], [0], 4)):
        with pytest.raises(IOError) as e:
            call()
        assert p in str(e.value) and why in str(e.value), str(e.value)


def test_missing_file_is_an_error(tmp_path):
    p = str(tmp_path / "nothing.wav")
    with pytest.raises(IOError, match="nothing.wav"):
        wavio.probe(p)


# ----------------------------------------------------------------------- batched read ---
@pytest.mark.parametrize("threads", [1, 4])
def test_read_batch_unequal_lengths(tmp_path, threads):
    lens = [500, 37, 1200, 1, 800, 64]
    paths = [_write(tmp_path / f"f{i}.wav", _pcm(n, 100 + i)) for i, n in enumerate(lens)]
    starts = [0, 5, 1000, 0, 799, 70]
    count = 300
    buf = torch.full((len(lens), count), 77, dtype=torch.int16)
    out, got = wavio.read_batch(paths, starts, count, out=buf.numpy(), nthreads=threads)
    for i, (p, s) in enumerate(zip(paths, starts)):
        ref, ref_got = _wave_window(p, s, count)
        assert got[i] == ref_got and np.array_equal(buf[i].numpy(), ref), i
    assert got.tolist() == [300, 32, 200, 1, 1, 0]
    out0, got0 = wavio.read_batch(paths, starts, 0, nthreads=threads)
    assert out0.shape == (6, 0) and not got0.any()
    with pytest.raises(IOError, match="gone.wav"):
        wavio.read_batch(paths + [str(tmp_path / "gone.wav")], starts + [0], count, nthreads=threads)


# ------------------------------------------------------------------------------ golden ---
@pytest.mark.parametrize("form", ["seg", "whole"])
def test_sheet_order_batches_and_collation_match_reference(tmp_path, form):
    g = C.golden()
    d = C.data_dir(tmp_path, form)
    sheet = AudioSheet(d)
    rows = list(sheet)
    assert len(sheet) == len(rows) == len(g[form + ".uttid"])
    assert [r[0] for r in rows] == g[form + ".uttid"].tolist()
    assert [os.path.basename(r[1]) for r in rows] == g[form + ".wav"].tolist()
    assert [r[2] for r in rows] == g[form + ".start"].tolist()
    assert [r[3] for r in rows] == g[form + ".shape"].tolist()

    pcm = RawAudioFileDataset(d, C.small_cfg(), None)
    flt = RawAudioFileDataset(d, C.small_cfg(), None, raw_pcm=False)
    assert pcm.raw_pcm is True and pcm.batchify_policy.max_batch_frame == C.SMALL_BUDGET
    order = sorted(range(len(pcm.data)), key=lambda i: pcm.data[i].xlen, reverse=True)
    assert order == g[form + ".order"].tolist()
    batches = C.golden_batches(form)
    assert [list(b) for b in pcm.batchify_policy.data] == batches == [list(b) for b in flt.batchify_policy.data]
    assert len(pcm) == len(batches) >= 3
    for i in range(len(batches)):
        assert pcm[i] == [pcm.data[j] for j in batches[i]]
        ref = g[f"{form}.xs.{i}"]
        xf, a, b, c = flt.collator([flt[i]])
        assert a is None and b is None and c is None
        assert xf.dtype == torch.float32 and np.array_equal(xf.numpy(), ref), (form, i)
        xi, a, b, c = pcm.collator([pcm[i]])
        assert a is None and b is None and c is None
        assert xi.dtype == torch.int16 and xi.shape == ref.shape and xi.is_contiguous()
        assert np.array_equal(xi.numpy().astype(np.float32) * np.float32(2.0 ** -15), ref), (form, i)


def test_synthetic_policy_matches_reference():
    g = C.golden()
    recs = [Audio("none", 0, int(n), None, None) for n in g["syn.len"]]
    order = sorted(range(len(recs)), key=lambda i: recs[i].xlen, reverse=True)
    assert order == g["syn.order"].tolist()
    pol = Wav2VecBatch(None)
    assert pol.max_batch_frame == 1400000 and pol.min_frame == 250000
    pol.batchify(order, recs)
    assert [list(b) for b in pol.data] == C.golden_batches("syn")
    assert len(pol) >= 4 and any(min(recs[i].xlen for i in b) > 250000 for b in pol.data)
    # the optional extension field, as an attribute and as a mapping key
    assert Wav2VecBatch({"max_batch_frame": 99}).max_batch_frame == 99
    assert Wav2VecBatch({"batch_size": 3}).max_batch_frame == 1400000


def test_audio_x_is_the_float_window(tmp_path):
    pcm = _pcm(100, 3)
    p = _write(tmp_path / "a.wav", pcm)
    x = Audio(p, 10, 50, None, None).x
    assert x.dtype == torch.float32 and np.array_equal(x.numpy(), pcm[10:60].astype(np.float64) / 32768)
    assert Audio(p, 90, 50, None, None).x.shape == (10,)  # a slice past the end is shorter, as in the reference


def test_crop_at_250000(tmp_path):
    d = tmp_path / "long"
    d.mkdir()
    n = 250003
    pcm = _pcm(n, 9)
    long_wav = _write(d / "long.wav", pcm)
    short = _write(d / "longer.wav", _pcm(n + 40, 10))
    (d / "wav.scp").write_text(f"a {long_wav}\nb {short}\n")
    for raw in (True, False):
        ds = RawAudioFileDataset(str(d), None, None, raw_pcm=raw)
        assert len(ds) == 1 and [a.xlen for a in ds[0]] == [n + 40, n]
        xs = ds.collator([ds[0]])[0]
        assert xs.shape == (2, 250000)
        row = xs[1].numpy() if raw else np.round(xs[1].numpy().astype(np.float64) * 32768).astype(np.int16)
        assert np.array_equal(row, pcm[:250000])


def test_batch_with_no_full_utterance_raises(tmp_path):
    d = tmp_path / "short"
    d.mkdir()
    w = _write(d / "r.wav", _pcm(1000, 1))
    (d / "wav.scp").write_text(f"r {w}\n")
    (d / "segments").write_text("u0 r 0.05 0.2\nu1 r 0.04 0.3\n")  # both end beyond the 1000 samples
    for raw in (True, False):
        ds = RawAudioFileDataset(str(d), None, None, raw_pcm=raw)
        with pytest.raises(ValueError, match="r.wav"):
            ds.collator([ds[0]])


def test_sheet_errors_and_feats_priority(tmp_path):
    from cfgtree import data_dir

    feats = data_dir(tmp_path)
    (feats / "wav.scp").write_text("x /nowhere.wav\n")
    rows = list(AudioSheet(str(feats)))
    assert rows and all(r[2] is None and ":" in r[1] for r in rows)  # the feature branch: ark:offset, no start

    d = tmp_path / "bad"
    d.mkdir()
    (d / "wav.scp").write_text("onlyid\n")
    with pytest.raises(ValueError, match="Invalid line is found"):
        list(AudioSheet(str(d)))
    (d / "wav.scp").write_text("a sox a.flac -t wav - |\n")
    with pytest.raises(NotImplementedError, match="pipe"):
        list(AudioSheet(str(d)))
    (d / "wav.scp").write_text("a /x/a.wav\n")
    (d / "segments").write_text("u0 a 0.0\n")
    with pytest.raises(ValueError, match="Invalid line is found"):
        list(AudioSheet(str(d)))
    (tmp_path / "empty").mkdir()
    with pytest.raises(FileNotFoundError):
        AudioSheet(str(tmp_path / "empty"))


# ---------------------------------------------------------------------- config and CLI ---
def test_pretrain_task_composes_and_builds(tmp_path, monkeypatch):
    for task in ("pretrain", "pretrain_wav"):
        cfg = compose(overrides=[f"task={task}", "model=wav2vec2_base", "criterion=wav2vec", "optimizer=noam_d256"])
        assert cfg.task.name == "pretrain" and cfg.task.train == "???" and cfg.task.save_dir == "ckpts"
        assert cfg.task.raw_pcm is True and cfg.model.name == "wav2vec2"
    from liteasr_amd import tasks

    d = C.data_dir(tmp_path, "whole")
    monkeypatch.chdir(tmp_path)
    cfg = compose(overrides=["task=pretrain_wav", f"task.train={d}", f"task.valid={d}", "model=wav2vec2_base",
                             "criterion=wav2vec", "optimizer=noam_d256", "+dataset.max_batch_frame=20000"])
    task = tasks.setup_task(cfg.task)
    assert type(task).__name__ == "PreTrainTask" and os.path.isdir(tmp_path / "ckpts")
    task.load_dataset("train", cfg.task.train, cfg.dataset, cfg.postprocess, False)
    ds = task.dataset("train")
    assert isinstance(ds, RawAudioFileDataset) and ds.raw_pcm and [len(b) for b in ds.batchify_policy.data] == [1, 2, 4]


def test_train_help_names_pretrain(capsys):
    from liteasr_amd import train as T

    with pytest.raises(SystemExit):
        T.parse_args(["--help"])
    out = capsys.readouterr().out
    line = [ln for ln in out.splitlines() if ln.strip().startswith("task:")]
    names = re.split(r"[,\s]+", line[0].split(":", 1)[1].strip())
    assert "pretrain" in names and "pretrain_wav" in names and "asr" in names, line


# --------------------------------------------------------------------------------- ABI ---
def test_io_header_symbols_exported():
    hdr = os.path.join(ROOT, "include", "liteasr_io.h")
    so = os.path.join(ROOT, "liteasr_amd", "lib", "libliteasr_io.so")
    if not os.path.exists(so):
        subprocess.run(["make", "-C", ROOT, so], check=True, capture_output=True)
    src = re.sub(r"/\*.*?\*/", "", open(hdr).read(), flags=re.S)
    declared = set(re.findall(r"\b(lasr_[a-z0-9_]+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert {"lasr_wav_probe", "lasr_wav_read_i16", "lasr_wav_read_batch", "lasr_ark_read_padded"} <= declared
    assert declared <= exported, declared - exported
