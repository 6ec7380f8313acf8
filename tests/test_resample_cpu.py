"""Speed perturbation of task=asr on raw audio, the host side: the kernel's host-built tap tables
agree with the float64 restatement of the transform (tests/resample_ref.py), speed factors parse
to reduced fractions or are refused, and AudioFileDataset over a wav.scp directory holds Kaldi's
static copies (one record per utterance and factor, batched by the resampled frame counts) while a
dataset without ``speed_perturb`` is, record for record and batch for batch, what it was."""

import logging
import os
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import resample_cases as C
import resample_ref as R

LENGTHS = [16000, 399, 8000, 400, 12345, 200, 559, 560, 19999]
SPEEDS = [0.9, 1.0, 1.1]


def _dcfg(**kw):
    base = dict(batch_count="seq", batch_size=3, max_len_in=100000, max_len_out=1000, max_frame_num=100000,
                min_batch_size=1, sort_by="input")
    base.update(kw)
    return SimpleNamespace(**base)


@pytest.fixture(scope="module")
def wav_dir(tmp_path_factory):
    from liteasr_amd.utils.synthetic import synthetic_wav_dir

    return synthetic_wav_dir(str(tmp_path_factory.mktemp("resample") / "train"), LENGTHS, seed=3)


def _dataset(d, split="train", workflow=(), dcfg=None, **kw):
    from liteasr_amd.config import PostProcessConfig
    from liteasr_amd.dataclass.vocab import Vocab
    from liteasr_amd.dataset import AudioFileDataset

    return AudioFileDataset(split, d, None, dcfg or _dcfg(), PostProcessConfig(workflow=list(workflow)),
                            Vocab(os.path.join(d, "vocab.txt")), **kw)


# ------------------------------------------------------------------------------ the tables ---
def _apply_tables(x, row, taps):
    """The polyphase form in float64: output j q + i = sum_k x[j p - width + k] tap[i][k]."""
    p, q, width, off = (int(v) for v in row)
    nt = 2 * width + p
    tap = taps[off:off + q * nt].reshape(q, nt)
    M = R.num_samples(len(x), p, q)
    m = np.arange(M)
    padded = np.concatenate([np.zeros(width), np.asarray(x, dtype=np.float64), np.zeros(width + 2 * p)])
    idx = ((m // q) * p)[:, None] + np.arange(nt)[None, :]  # input j p - width + k sits at padded[j p + k]
    return (padded[idx] * tap[m % q]).sum(axis=1)


def test_tables_match_ref():
    from liteasr_amd.kernels import resample_tables

    ratios = [(9, 10), (11, 10), (4, 5), (5, 4)]
    table, taps = resample_tables(ratios, dtype=np.float64)
    assert table.dtype == np.int32 and table.shape == (4, 4) and taps.dtype == np.float64
    assert [tuple(r[:3]) for r in table.tolist()] == [(9, 10, 7), (11, 10, 7), (4, 5, 7), (5, 4, 8)]
    sizes = [q * (2 * w + p) for p, q, w, _ in table.tolist()]
    assert sizes[:2] == [10 * 23, 10 * 25] and table[:, 3].tolist() == [0] + list(np.cumsum(sizes)[:-1])
    assert taps.shape == (sum(sizes),)
    x = C.signal("noise_full")[:4000]
    for row, (p, q) in zip(table, ratios):
        err = np.abs(_apply_tables(x, row, taps) - C.reference("noise_full", 4000, (p, q))).max()
        print(f"tables {p}/{q}: {err:.3e} LSB")
        assert err <= 1e-7
    # the kernel's own are these rounded to float32, laid out the same
    t32, f32 = resample_tables(ratios)
    assert f32.dtype == np.float32 and np.array_equal(t32, table) and np.array_equal(f32, taps.astype(np.float32))
    # 1/1 is a copy: no width, one tap
    one, tap = resample_tables([(1, 1)])
    assert one.tolist() == [[1, 1, 0, 0]] and tap.tolist() == [1.0]
    for bad in ([], [(3, 1)], [(1, 3)], [(33, 32)], [(2, 2)], [(0, 1)]):
        with pytest.raises(ValueError):
            resample_tables(bad)


def test_ref_is_a_copy_at_unit_speed_and_counts_samples():
    x = C.signal("noise_full")[:1000]
    assert np.array_equal(R.quantise(R.resample(x, 1, 1)), x)
    for n, (p, q), m in ((400, (11, 10), 364), (400, (9, 10), 445), (0, (9, 10), 0), (1, (11, 10), 1), (9, (9, 10), 10)):
        assert R.num_samples(n, p, q) == m == R.resample(np.zeros(n, np.int16), p, q).shape[0]
    assert R.quantise([0.5, 1.5, -0.5, 40000.0, -40000.0, 32767.5, -32768.5]).tolist() == [
        0, 2, 0, 32767, -32768, 32767, -32768]
    # a constant comes out scaled by the filter's DC gain, which is 1 to a few 1e-3 away from the edges
    y = R.resample(np.full(2000, 1000, np.int16), 9, 10)
    assert np.abs(y[100:-100] - 1000).max() < 5


def test_reference_stays_within_the_excused_cap():
    """What tests/resample_cases.py asserts as a script, on the chosen inputs."""
    for s in C.SIGNALS:
        for pq in C.RATIOS:
            assert C.figures(s, pq)[2] <= C.EXCUSED_CAP


def test_factor_parsing():
    from liteasr_amd.kernels import resample_ratio
    from liteasr_amd.utils.frontend import resampled_samples, speed_ratios

    assert resample_ratio(0.9) == (9, 10) and resample_ratio(1.0) == (1, 1) and resample_ratio(1.1) == (11, 10)
    assert resample_ratio("0.8") == (4, 5) and resample_ratio(2) == (2, 1) and resample_ratio(0.5) == (1, 2)
    for bad in (3.0, 0.3, 0.123):
        with pytest.raises(ValueError, match=str(bad)):
            resample_ratio(bad)
    assert speed_ratios(None) is None and speed_ratios([]) is None
    assert speed_ratios(SPEEDS) == [(9, 10), (1, 1), (11, 10)]
    with pytest.raises(ValueError, match="0.123"):
        speed_ratios([0.9, 0.123])
    for n in (0, 1, 9, 10, 400, 16000):
        for p, q in C.RATIOS:
            assert resampled_samples(n, p, q) == R.num_samples(n, p, q)


# ------------------------------------------------------------------------------ the dataset ---
def test_dataset_holds_static_copies(wav_dir, caplog):
    from liteasr_amd.dataclass.audio_data import SpeedWavAudio
    from liteasr_amd.utils.frontend import ResamplePlan, num_frames

    dcfg = _dcfg(batch_count="frame", max_frame_in=250, max_frame_out=0, max_frame_inout=0)
    with caplog.at_level(logging.WARNING):
        ds = _dataset(wav_dir, dcfg=dcfg, speed_perturb=SPEEDS)
    want = []
    for p, q in [(9, 10), (1, 1), (11, 10)]:
        for n in LENGTHS:
            m = R.num_samples(n, p, q)
            if num_frames(m):
                want.append((n, (p, q), m, num_frames(m)))
    # 200 samples hold no frame at any speed, 399 only at 0.9 (444 samples), 400 none at 1.1 (364): 6 dropped
    dropped = 3 * len(LENGTHS) - len(want)
    assert dropped == 6 and (399, (9, 10), 444, 1) in want and (400, (9, 10), 445, 1) in want
    assert not any(w[:2] == (400, (11, 10)) for w in want)
    assert any(f"dropped {dropped} utterance" in r.getMessage() for r in caplog.records)
    assert all(type(a) is SpeedWavAudio for a in ds.data)
    assert [(a.shape, a.ratio, a.samples, a.xlen) for a in ds.data] == want
    assert all(a.xlen == a.frames == num_frames(-(-a.ratio[1] * a.shape // a.ratio[0])) for a in ds.data)
    # sorted by the perturbed frame counts, and every batch within the frame budget on them
    flat = [a.xlen for i in range(len(ds)) for a in ds[i]]
    assert flat == sorted(flat, reverse=True) and len(flat) == len(want) and len(ds) > 3
    for i in range(len(ds)):
        assert len(ds[i]) * max(a.xlen for a in ds[i]) <= 250 or len(ds[i]) == 1
    assert any(len({a.ratio for a in ds[i]}) > 1 for i in range(len(ds)))  # the speeds interleave
    # the collator: the source samples as before, and the plan as the last element
    from liteasr_amd.utils import wavio

    for i in range(len(ds)):
        batch = ds[i]
        out = ds.collator([batch])
        assert len(out) == 5 and isinstance(out[4], ResamplePlan)
        xs, xlens, ys, ylens, plan = out
        assert xs.dtype == torch.int16 and xs.shape == (len(batch), max(a.shape for a in batch))
        assert xlens.tolist() == [a.xlen for a in batch]
        assert plan.rows.dtype == torch.int32 and plan.rows.shape == (len(batch), 3)
        assert plan.ratios == ((9, 10), (1, 1), (11, 10)) and plan.max_out == max(a.samples for a in batch)
        assert plan.rows.tolist() == [[a.shape, a.samples, plan.ratios.index(a.ratio)] for a in batch]
        for j, a in enumerate(batch):
            pcm, got = wavio.read(a.fd, 0, a.shape)
            assert got == a.shape and np.array_equal(xs[j, :a.shape].numpy(), pcm) and (xs[j, a.shape:] == 0).all()
    # with SpecAugment the plan of the masks is drawn from the perturbed frame counts
    aug = _dataset(wav_dir, dcfg=dcfg, workflow=("spec_aug",), speed_perturb=SPEEDS)
    random.seed(4)
    np.random.seed(4)
    out = aug.collator([aug[0]])
    assert len(out) == 6 and isinstance(out[5], ResamplePlan) and out[0].dtype == torch.int16
    random.seed(4)
    np.random.seed(4)
    assert torch.equal(torch.as_tensor(out[4]), torch.as_tensor(aug.postprocess.plan_batch(out[1].tolist(), 80)))


def test_other_splits_and_feats_ignore_it(wav_dir, tmp_path, caplog):
    import shutil

    from liteasr_amd.utils.kaldiio import save_ark

    for split in ("valid", "test"):
        a, b = _dataset(wav_dir, split=split), _dataset(wav_dir, split=split, speed_perturb=SPEEDS)
        assert b.speed is None and a.data == b.data and len(a) == len(b)
        assert all(type(r).__name__ == "WavAudio" for r in b.data)
        for i in range(len(a)):
            ca, cb = a.collator([a[i]]), b.collator([b[i]])
            assert len(ca) == len(cb) == 4 and all(torch.equal(u, v) for u, v in zip(ca, cb))
    rng = np.random.default_rng(8)
    feats = {f"utt{i:04d}": rng.standard_normal((int(rng.integers(5, 40)), 13)).astype(np.float32)
             for i in range(len(LENGTHS))}
    d = str(tmp_path / "feats")
    os.makedirs(d)
    save_ark(os.path.join(d, "feats.ark"), feats, scp=os.path.join(d, "feats.scp"))
    with open(os.path.join(d, "utt2num_frames"), "w") as f:
        f.writelines(f"{k} {v.shape[0]}\n" for k, v in feats.items())
    for fn in ("text", "vocab.txt"):
        shutil.copy(os.path.join(wav_dir, fn), d)
    with caplog.at_level(logging.INFO):
        a, b = _dataset(d), _dataset(d, speed_perturb=SPEEDS)
    assert sum("speed_perturb is ignored" in r.getMessage() for r in caplog.records) == 1
    assert not b.wav and b.speed is None and a.data == b.data and len(b.data) == len(LENGTHS)
    assert all(torch.equal(u, v) for u, v in zip(a.collator([a[0]]), b.collator([b[0]])))


@pytest.mark.parametrize("workflow", [(), ("spec_aug",)])
def test_off_is_what_it_was(wav_dir, workflow):
    """speed_perturb=None: the records, the batches and what the collator delivers equal those of
    a dataset built without the argument, and are the plain raw-audio records and tuples."""
    a = _dataset(wav_dir, workflow=workflow)
    b = _dataset(wav_dir, workflow=workflow, speed_perturb=None)
    c = _dataset(wav_dir, workflow=workflow, speed_perturb=[])
    kept = [n for n in LENGTHS if n >= 400]
    for ds in (b, c):
        assert ds.speed is None and ds.data == a.data and [r.shape for r in ds.data] == kept
        assert all(type(r).__name__ == "WavAudio" for r in ds.data)
        assert [r.xlen for r in ds.data] == [1 + (n - 400) // 160 for n in kept]
        assert len(ds) == len(a) == 3
        for i in range(len(a)):
            assert ds[i] == a[i]
            random.seed(4)
            np.random.seed(4)
            ca = a.collator([a[i]])
            random.seed(4)
            np.random.seed(4)
            cb = ds.collator([ds[i]])
            assert type(cb) is tuple and len(ca) == len(cb) == (5 if workflow else 4)
            assert cb[0].dtype == torch.int16 and cb[0].shape == (len(a[i]), max(r.shape for r in a[i]))
            assert all(torch.equal(torch.as_tensor(u), torch.as_tensor(v)) for u, v in zip(ca, cb))
            assert [t.dtype for t in cb[:4]] == [torch.int16, torch.long, torch.long, torch.long]


def test_segments_window_is_an_utterance_of_its_own(tmp_path):
    from liteasr_amd.utils.synthetic import synthetic_wave, write_wav

    d = str(tmp_path)
    rec = synthetic_wave(20000, np.random.default_rng(0))
    write_wav(os.path.join(d, "rec.wav"), rec)
    open(os.path.join(d, "wav.scp"), "w").write(f"rec {d}/rec.wav\n")
    open(os.path.join(d, "segments"), "w").write("s0 rec 0.0 0.5\ns1 rec 0.25 0.3\ns2 rec 0.5 0.52\n")
    open(os.path.join(d, "text"), "w").write("s0 ab\ns1 ba\ns2 a\n")
    open(os.path.join(d, "vocab.txt"), "w").write("a 1\nb 2\n<unk> 3\n")
    ds = _dataset(d, speed_perturb=[1.1, 0.9])
    # s2 (319 samples) holds no frame at either speed; s1: 799 samples -> 727 and 888
    assert [(a.start, a.shape, a.ratio, a.samples, a.xlen) for a in ds.data] == [
        (0, 7999, (11, 10), 7272, 43), (4000, 799, (11, 10), 727, 3),
        (0, 7999, (9, 10), 8888, 54), (4000, 799, (9, 10), 888, 4)]
    xs, _, _, _, plan = ds.collator([[ds.data[1], ds.data[2]]])
    assert xs.shape == (2, 7999) and np.array_equal(xs[0, :799].numpy(), rec[4000:4799]) and (xs[0, 799:] == 0).all()
    assert plan.ratios == ((11, 10), (9, 10)) and plan.rows.tolist() == [[799, 727, 0], [7999, 8888, 1]]


def test_config_and_task(wav_dir, tmp_path):
    from liteasr_amd.config.compose import compose
    from liteasr_amd.tasks.asr import ASRConfig, ASRTask, FrontendConfig

    base = ["task=asr_wav", "model=conformer_tiny", "criterion=hybrid_ctc_w03", "optimizer=noam_d256"]
    cfg = compose(overrides=base)
    assert "speed_perturb" in cfg.task.frontend and cfg.task.frontend.speed_perturb is None
    cfg = compose(overrides=base + ["task.frontend.speed_perturb=[0.9,1.0,1.1]"])
    assert cfg.task.frontend.speed_perturb == SPEEDS
    assert FrontendConfig().speed_perturb is None
    vocab = os.path.join(wav_dir, "vocab.txt")

    def task(**fe):
        return ASRTask(ASRConfig(vocab=vocab, train=wav_dir, valid=wav_dir, save_dir=str(tmp_path / "c"),
                                 frontend=FrontendConfig(**fe)))

    with pytest.raises(ValueError, match="3.0"):
        task(speed_perturb=[0.9, 3.0])
    t = task(speed_perturb=SPEEDS)
    t.load_dataset("train", wav_dir, _dcfg(), None)
    t.load_dataset("valid", wav_dir, _dcfg(), None)
    kept = sum(n >= 400 for n in LENGTHS)
    assert len(t.dataset("train").data) == 3 * len(LENGTHS) - 6 and t.dataset("train").speed == [(9, 10), (1, 1), (11, 10)]
    assert len(t.dataset("valid").data) == kept and t.dataset("valid").speed is None
    off = task()
    off.load_dataset("train", wav_dir, _dcfg(), None)
    assert off.speed_perturb is None and off.dataset("train").speed is None
    assert off.dataset("train").data == t.dataset("valid").data
