"""task=asr on raw audio, the host side: the float64 restatement of Kaldi fbank (tests/fbank_ref.py)
checks itself, the kernel's host-built tables agree with it, AudioFileDataset over a wav.scp
directory batches by frame counts and collates int16 PCM, a directory with feats.scp is read as
before, and CMVN statistics round-trip through the project's Kaldi reader and writer."""

import os
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import fbank_ref as R

LENGTHS = [16000, 399, 8000, 400, 12345, 200, 559, 560, 19999]  # two of them hold no frame


def _dcfg(**kw):
    base = dict(batch_count="seq", batch_size=3, max_len_in=100000, max_len_out=1000, max_frame_num=100000,
                min_batch_size=1, sort_by="input")
    base.update(kw)
    return SimpleNamespace(**base)


@pytest.fixture(scope="module")
def wav_dir(tmp_path_factory):
    from liteasr_amd.utils.synthetic import synthetic_wav_dir

    return synthetic_wav_dir(str(tmp_path_factory.mktemp("fbank") / "train"), LENGTHS, seed=3)


def _dataset(d, split="train", workflow=(), **kw):
    from liteasr_amd.config import PostProcessConfig
    from liteasr_amd.dataclass.vocab import Vocab
    from liteasr_amd.dataset import AudioFileDataset

    return AudioFileDataset(split, d, None, _dcfg(), PostProcessConfig(workflow=list(workflow)),
                            Vocab(os.path.join(d, "vocab.txt")), **kw)


# ------------------------------------------------------------------ the reference itself ---
def test_ref_frame_counts():
    assert [R.num_frames(n) for n in (399, 400, 559, 560)] == [0, 1, 1, 2]
    from liteasr_amd.kernels import fbank_num_frames
    from liteasr_amd.utils.frontend import num_frames, used_samples

    for n in (0, 1, 399, 400, 401, 559, 560, 719, 720, 16000, 160400):
        assert num_frames(n) == fbank_num_frames(n) == R.num_frames(n)
        assert used_samples(num_frames(n)) <= n or num_frames(n) == 0
    assert R.fbank(np.zeros(399, np.int16)).shape == (0, 80)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_ref_floor_is_exact(dtype):
    """All-zero and constant input: the DC removal leaves nothing, every bin sits on the floor."""
    floor = np.log(np.dtype(dtype).type(R.FLT_EPSILON))
    for x in (np.zeros(1000, np.int16), np.full(1000, 1000, np.int16), np.full(400, -32768, np.int16)):
        y = R.fbank(x, 80, dtype)
        assert y.shape == (R.num_frames(len(x)), 80) and y.dtype == dtype
        assert (y == floor).all()
    assert np.float32(np.log(np.float64(R.FLT_EPSILON))) == R.LOG_EPS32


@pytest.mark.parametrize("F", [1, 23, 40, 80, 128])
def test_ref_mel_banks(F):
    W = R.mel_banks(F)
    assert W.shape == (F, 257) and (W >= 0).all() and (W <= 1).all()
    assert ((W > 0).sum(axis=0) <= 2).all()
    assert (W[:, 256] == 0).all() and (W[:, 0] == 0).all()
    assert (W.sum(axis=1) > 0).all() or F == 128  # at 128 bins the lowest triangles may hold no FFT bin
    assert W[:, 1:256].sum() > 0


@pytest.mark.parametrize("F", [1, 23, 80, 128])
def test_kernel_tables_match_ref(F):
    """The (run, rising weight, falling weight) form the kernel reads expands to the reference's
    mel matrix, and the window is the reference's, to float32 rounding."""
    from liteasr_amd.kernels import fbank_tables

    tab, seg = fbank_tables(F)
    assert tab.dtype == np.float32 and tab.shape == (2048,) and seg.dtype == np.int32 and seg.shape == (F + 2,)
    assert (np.diff(seg) >= 0).all() and seg[0] >= 1 and seg[-1] <= 256
    W = np.zeros((F, 256))
    for f in range(F):
        W[f, seg[f]:seg[f + 1]] += tab[1536:1792][seg[f]:seg[f + 1]]
        W[f, seg[f + 1]:seg[f + 2]] += tab[1792:2048][seg[f + 1]:seg[f + 2]]
    assert np.abs(W - R.mel_banks(F)[:, :256]).max() <= 2.0 ** -24
    assert np.abs(tab[:400] - R.povey_window()).max() <= 2.0 ** -24 and (tab[400:512] == 0).all()
    k = np.arange(256)
    for base, n in ((512, 256), (1024, 512)):
        w = tab[base:base + 512:2] + 1j * tab[base + 1:base + 512:2]
        assert np.abs(w - np.exp(-2j * np.pi * k / n)).max() <= 2.0 ** -23
    with pytest.raises(ValueError):
        fbank_tables(0)
    with pytest.raises(ValueError):
        fbank_tables(129)


# -------------------------------------------------------------------------- the data path ---
def test_wav_dataset_batches_by_frames(wav_dir):
    ds = _dataset(wav_dir)
    assert ds.wav and ds.feat_dim == 80
    kept = [n for n in LENGTHS if n >= 400]
    assert len(ds.data) == len(kept) == len(LENGTHS) - 2  # 399 and 200 samples: dropped
    assert [a.shape for a in ds.data] == kept and all(a.start == 0 for a in ds.data)
    assert [a.xlen for a in ds.data] == [1 + (n - 400) // 160 for n in kept]
    assert _dataset(wav_dir, num_mel_bins=40).feat_dim == 40
    flat = [a.xlen for i in range(len(ds)) for a in ds[i]]
    assert flat == sorted(flat, reverse=True) and len(ds) == 3
    from liteasr_amd.utils import wavio

    for i in range(len(ds)):
        batch = ds[i]
        xs, xlens, ys, ylens = ds.collator([batch])
        smax = max(a.shape for a in batch)
        assert xs.dtype == torch.int16 and xs.shape == (len(batch), smax) and xs.is_contiguous()
        assert xlens.dtype == torch.long and xlens.tolist() == [a.xlen for a in batch]
        assert ylens.tolist() == [a.ylen for a in batch] and ys.shape == (len(batch), int(ylens.max()))
        for j, a in enumerate(batch):
            pcm, got = wavio.read(a.fd, 0, a.shape)
            assert got == a.shape and np.array_equal(xs[j, :a.shape].numpy(), pcm)
            assert (xs[j, a.shape:] == 0).all()
            assert a.x.dtype == torch.int16 and np.array_equal(a.x.numpy(), pcm)
    assert any((ds.collator([ds[i]])[0] != 0).any() for i in range(len(ds)))


def test_wav_dataset_spec_augment_plan_from_frames(wav_dir):
    """Training with spec_aug: the collator adds the plan, drawn from frame counts and feat_dim."""
    ds = _dataset(wav_dir, workflow=("spec_aug",))
    random.seed(4)
    np.random.seed(4)
    out = ds.collator([ds[0]])
    assert len(out) == 5 and out[0].dtype == torch.int16
    random.seed(4)
    np.random.seed(4)
    plan = ds.postprocess.plan_batch(out[1].tolist(), 80)
    assert torch.equal(torch.as_tensor(out[4]), torch.as_tensor(plan))
    assert len(_dataset(wav_dir, split="valid", workflow=("spec_aug",)).collator([ds[0]])) == 4


def test_segments_window_is_zero_padded(tmp_path):
    """With segments a shorter utterance's row must not run on into its recording."""
    from liteasr_amd.utils.synthetic import synthetic_wave, write_wav

    d = str(tmp_path)
    rec = synthetic_wave(20000, np.random.default_rng(0))
    write_wav(os.path.join(d, "rec.wav"), rec)
    open(os.path.join(d, "wav.scp"), "w").write(f"rec {d}/rec.wav\n")
    open(os.path.join(d, "segments"), "w").write("s0 rec 0.0 0.5\ns1 rec 0.25 0.3\ns2 rec 0.5 0.52\n")
    open(os.path.join(d, "text"), "w").write("s0 ab\ns1 ba\ns2 a\n")
    open(os.path.join(d, "vocab.txt"), "w").write("a 1\nb 2\n<unk> 3\n")
    ds = _dataset(d)
    assert [(a.start, a.shape, a.xlen) for a in ds.data] == [(0, 7999, 48), (4000, 799, 3)]  # s2: 319 samples
    xs, xlens, _, _ = ds.collator([ds[0]])
    assert xs.shape == (2, 7999) and xlens.tolist() == [48, 3]
    assert np.array_equal(xs[0].numpy(), rec[:7999]) and np.array_equal(xs[1, :799].numpy(), rec[4000:4799])
    assert (xs[1, 799:] == 0).all()


def test_dither_is_refused(wav_dir, tmp_path):
    from liteasr_amd.tasks.asr import ASRConfig, ASRTask, FrontendConfig
    from liteasr_amd.utils.frontend import Fbank

    with pytest.raises(NotImplementedError):
        Fbank(dither=0.1)
    vocab = os.path.join(wav_dir, "vocab.txt")
    with pytest.raises(NotImplementedError):
        ASRTask(ASRConfig(vocab=vocab, train=wav_dir, valid=wav_dir, save_dir=str(tmp_path / "c"),
                          frontend=FrontendConfig(dither=0.1)))
    task = ASRTask(ASRConfig(vocab=vocab, train=wav_dir, valid=wav_dir, save_dir=str(tmp_path / "c"),
                             frontend=FrontendConfig(num_mel_bins=40)))
    task.load_dataset("train", wav_dir, _dcfg(), None)
    assert task.feat_dim == 40 and task.dataset("train").wav
    from liteasr_amd.config.compose import compose

    cfg = compose(overrides=["task=asr_wav", "model=conformer_tiny", "criterion=hybrid_ctc_w03", "optimizer=noam_d256"])
    assert dict(cfg.task.frontend)["num_mel_bins"] == 80 and cfg.task.frontend.cmvn is None
    assert cfg.task.frontend.dither == 0.0 and cfg.task.name == "asr"


def test_feats_scp_keeps_priority(wav_dir, tmp_path):
    """A directory with feats.scp and wav.scp is the feats.scp directory, bit for bit."""
    import shutil

    from liteasr_amd.utils.kaldiio import save_ark

    rng = np.random.default_rng(8)
    n = len(LENGTHS)
    feats = {f"utt{i:04d}": rng.standard_normal((int(rng.integers(5, 40)), 13)).astype(np.float32) for i in range(n)}
    dirs = []
    for name in ("plain", "both"):
        d = str(tmp_path / name)
        os.makedirs(d)
        save_ark(os.path.join(d, "feats.ark"), feats, scp=os.path.join(d, "feats.scp"))
        with open(os.path.join(d, "utt2num_frames"), "w") as f:
            for k, v in feats.items():
                f.write(f"{k} {v.shape[0]}\n")
        for fn in ("text", "vocab.txt"):
            shutil.copy(os.path.join(wav_dir, fn), d)
        dirs.append(d)
    shutil.copy(os.path.join(wav_dir, "wav.scp"), dirs[1])
    a, b = _dataset(dirs[0]), _dataset(dirs[1])
    assert not a.wav and not b.wav and a.feat_dim == b.feat_dim == 13 and len(a) == len(b) == 3
    assert type(b.data[0]).__name__ == "Audio" and len(b.data) == n
    for i in range(len(a)):
        assert [(r.start, r.shape, r.tokenids) for r in a[i]] == [(r.start, r.shape, r.tokenids) for r in b[i]]
        ca, cb = a.collator([a[i]]), b.collator([b[i]])
        assert len(ca) == len(cb) == 4 and ca[0].dtype == torch.float32
        assert all(torch.equal(u, v) for u, v in zip(ca, cb))
        for j, r in enumerate(a[i]):
            assert torch.equal(ca[0][j, :r.shape], r.x) and r.x.shape == (r.shape, 13)
    assert sum(r.shape for i in range(len(a)) for r in a[i]) == sum(v.shape[0] for v in feats.values())


# ---------------------------------------------------------------------------------- CMVN ---
@pytest.mark.parametrize("binary", [True, False])
def test_cmvn_stats_round_trip(tmp_path, binary):
    from liteasr_amd.utils.frontend import Fbank, cmvn_from_stats, read_cmvn_stats, write_cmvn_stats

    rng = np.random.default_rng(5)
    F, count = 80, 12345.0
    x = rng.standard_normal((int(count), F)) * rng.uniform(0.5, 3.0, F) + rng.uniform(-4, 12, F)
    stats = np.zeros((2, F + 1))
    stats[0, :F], stats[0, F], stats[1, :F] = x.sum(0), count, (x * x).sum(0)
    p = str(tmp_path / "cmvn.stats")
    write_cmvn_stats(p, stats, binary=binary)
    assert (open(p, "rb").read(2) == b"\0B") == binary
    back = read_cmvn_stats(p)
    assert back.dtype == np.float64 and np.array_equal(back, stats)
    mean, istd = cmvn_from_stats(back)
    assert np.allclose(mean, x.mean(0), rtol=1e-12, atol=1e-12) and np.allclose(istd, 1 / x.std(0), rtol=1e-9)
    rm, ri = R.cmvn_from_stats(stats)
    assert np.array_equal(mean, rm) and np.array_equal(istd, ri)
    fe = Fbank(80, cmvn=p)
    assert np.array_equal(fe.cmvn[0], mean.astype(np.float32)) and np.array_equal(fe.cmvn[1], istd.astype(np.float32))
    with pytest.raises(ValueError):
        Fbank(40, cmvn=p)
    # a constant bin: the variance floor keeps istd finite
    stats[1, 3] = stats[0, 3] ** 2 / count
    assert np.isfinite(cmvn_from_stats(stats)[1][3])
