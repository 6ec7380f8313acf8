"""Room reverberation of task=asr on raw audio, the host side: the restatement's own identities and
its excused share (tests/reverb_ref.py, tests/reverb_cases.py), the host tables of the kernel, the
configuration keys and their refusals, the RIR index and bank, and AudioFileDataset over a wav.scp
directory with ``rir``: a ReverbPlan drawn from a generator of its own, after a ResamplePlan and
before a NoisePlan, while the noise and SpecAugment draws are what they were without it."""

import logging
import os
import pickle
import random
import wave
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import reverb_cases as C
import reverb_ref as R

LENGTHS = [16000, 399, 8000, 400, 12345, 200, 559, 560, 19999]
RIR_A, RIR_B = [3000, 1, 4100], [500, 65536]


def _dcfg(**kw):
    base = dict(batch_count="seq", batch_size=3, max_len_in=100000, max_len_out=1000, max_frame_num=100000,
                min_batch_size=1, sort_by="input")
    base.update(kw)
    return SimpleNamespace(**base)


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    from liteasr_amd.utils.synthetic import synthetic_rir_dir, synthetic_wav_dir

    root = tmp_path_factory.mktemp("reverb")
    return SimpleNamespace(train=synthetic_wav_dir(str(root / "train"), LENGTHS, seed=3),
                           a=synthetic_rir_dir(str(root / "rir_a"), RIR_A, seed=31),
                           b=synthetic_rir_dir(str(root / "rir_b"), RIR_B, seed=32),
                           noise=synthetic_wav_dir(str(root / "noise"), [5000, 777, 24000], seed=21), root=str(root))


def _spec(dirs, **kw):
    from liteasr_amd.utils.frontend import RirSpec

    return RirSpec([dirs.a, dirs.b], **kw)


def _dataset(d, split="train", workflow=(), dcfg=None, **kw):
    from liteasr_amd.config import PostProcessConfig
    from liteasr_amd.dataclass.vocab import Vocab
    from liteasr_amd.dataset import AudioFileDataset

    return AudioFileDataset(split, d, None, dcfg or _dcfg(), PostProcessConfig(workflow=list(workflow)),
                            Vocab(os.path.join(d, "vocab.txt")), **kw)


# ------------------------------------------------------------------------ the restatement ---
def test_ref_identities():
    x = C.signal("gauss")[:4000]
    for amp in (1, 12345, 700, 32767):  # a delta of any amplitude returns x exactly
        y, g = R.reverb(x, np.asarray([amp], dtype=np.int16), 0)
        assert np.array_equal(R.quantise(y), x) and g == np.float32(32768.0 / abs(amp))
    for p, L in ((0, 5), (123, 300), (299, 300)):  # a delta at index p with peak p is the identity
        h = np.zeros(L, dtype=np.int16)
        h[p] = 20000
        assert R.peak(h) == p
        for method in ("float64", "direct32", "overlap_save32"):
            y, _ = R.reverb(x, h, p, method=method, block=C.BLOCK)
            assert np.array_equal(R.quantise(y), x), (p, method)
    assert R.peak(np.asarray([3, 9, -20, 9, 1])) == 1  # the first index of the largest sample
    # the shift and the cut: c[m] = sum_k h[k] x[m + p - k]
    h, p = np.asarray([1000, -3000, 32767, 500], dtype=np.int16), 2
    c = R.convolve(x[:50], h, p)
    for m in (0, 1, 25, 48, 49):
        want = sum(int(h[k]) * int(x[m + p - k]) for k in range(4) if 0 <= m + p - k < 50) / 32768.0
        assert abs(c[m] - want) <= 1e-9
    # output power equals input power, up to the float32 rounding of the gain
    for i in (2, 6, 7):
        y, g = R.reverb(x, *C.rir(i))
        assert y.shape == x.shape and abs(float((y ** 2).sum()) / R.energy(x) - 1.0) <= 3e-7
        assert g == np.float32(R.exact_gain(x, *C.rir(i)))
        for method in ("direct32", "overlap_save32"):  # the float32 restatements say the same
            y32, _ = R.reverb(x, *C.rir(i), method=method, block=C.BLOCK)
            assert y32.dtype == np.float32 and np.abs(y32 - y).max() <= 0.05
    zero = np.zeros(100, dtype=np.int16)
    assert not R.reverb(zero, *C.rir(6))[0].any() and R.reverb(zero, *C.rir(6))[1] == 0.0
    assert R.reverb(x[:0], *C.rir(6))[0].shape == (0,)
    assert R.quantise([0.5, 1.5, -0.5, 40000.0, -40000.0, 32767.5, -32768.5]).tolist() == [
        0, 2, 0, 32767, -32768, 32767, -32768]


def test_cases_cover_the_edges():
    from liteasr_amd import kernels as K

    P = C.BLOCK
    assert P == K.REVERB_BLOCK
    assert [L for L, _, _ in C.RIR_SPECS[:8]] == [1, 2, 257, P - 1, P, P + 1, 4000, 2 * P + 1000]
    peaks = {(p == 0, p == L - 1) for L, p, _ in C.RIR_SPECS if L > 1}
    assert peaks == {(True, False), (False, True), (False, False)}  # at 0, at L - 1 and inside
    flat, table = C.bank()
    assert flat.shape[0] == int(table[:, 1].sum()) and all(R.peak(C.rir(i)[0]) == C.rir(i)[1] for i in range(len(table)))
    for name in C.SIGNALS:
        rows = C.rows(name)
        assert {n for n, _, _ in rows} >= set(C.LENGTHS)
        assert all(rows[r][1] != rows[r + 1][1] for r in range(len(rows) - 2))  # neighbours differ
        assert sum(i < 0 for _, i, _ in rows[:-1]) * 4 == len(rows) - 1  # one row in four carries none
    assert {i for _, i, _ in C.rows("gauss")} == set(range(len(C.RIR_SPECS))) | {-1}
    for name in C.SATURATING:
        q = R.quantise(np.concatenate([C.reference(name, r)[0] for r in range(len(C.rows(name)))]))
        assert (q == 32767).any() and (q == -32768).any()


def test_reference_stays_within_the_excused_cap():
    """What tests/reverb_cases.py asserts as a script, on the chosen inputs."""
    for s in C.SIGNALS:
        for L in C.taps(s):
            loss, _, near, _ = C.figures(s, L)
            assert near <= C.EXCUSED_CAP and loss > 0
        assert 0 < C.gain_deviation(s) < 1e-6


def test_reverb_plan_and_tables_layout():
    from liteasr_amd import kernels as K

    rows = K.reverb_plan([100, 0, 7], [2, -1, 0])
    assert rows.dtype == np.int32 and rows.tolist() == [[100, 2], [0, -1], [7, 0]]
    assert K.reverb_plan([], []).shape == (0, 2)
    with pytest.raises(ValueError):
        K.reverb_plan([1, 2], [0])
    tab = K.reverb_tables()
    n = 2 * K.REVERB_BLOCK
    assert tab.dtype == np.float32 and tab.shape == (2 * n,)
    w = np.exp(-2j * np.pi * np.arange(n) / n)
    assert np.array_equal(tab[0::2], w.real.astype(np.float32)) and np.array_equal(tab[1::2], w.imag.astype(np.float32))
    assert tab[:2].tolist() == [1.0, 0.0] and tab[n] == -1.0


# ------------------------------------------------------------------ configuration and bank ---
def test_config_defaults_and_overrides():
    from liteasr_amd.config.compose import compose
    from liteasr_amd.tasks.asr import FrontendConfig

    base = ["task=asr_wav", "model=conformer_tiny", "criterion=hybrid_ctc_w03", "optimizer=noam_d256"]
    fe = compose(overrides=base).task.frontend
    assert fe.rir is None and fe.rir_prob == 0.5 and fe.rir_seed == 0 and fe.rir_max_mb == 512
    fe = compose(overrides=base + ["task.frontend.rir=[rirs/simulated,rirs/real]", "task.frontend.rir_prob=0.7",
                                   "task.frontend.rir_seed=9", "task.frontend.rir_max_mb=64"]).task.frontend
    assert list(fe.rir) == ["rirs/simulated", "rirs/real"] and fe.rir_prob == 0.7
    assert fe.rir_seed == 9 and fe.rir_max_mb == 64
    d = FrontendConfig()
    assert (d.rir, d.rir_prob, d.rir_seed, d.rir_max_mb) == (None, 0.5, 0, 512)


def test_task_refuses_bad_values(dirs, tmp_path):
    from liteasr_amd.tasks.asr import ASRConfig, ASRTask, FrontendConfig
    from liteasr_amd.utils.frontend import Reverberator

    vocab = os.path.join(dirs.train, "vocab.txt")

    def task(**fe):
        return ASRTask(ASRConfig(vocab=vocab, train=dirs.train, valid=dirs.train, save_dir=str(tmp_path / "c"),
                                 frontend=FrontendConfig(**fe)))

    two = [dirs.a, dirs.b]
    for bad in (dict(rir_prob=-0.1), dict(rir_prob=1.5), dict(rir_prob=float("nan")), dict(rir_seed=-1),
                dict(rir_seed=1.5), dict(rir_max_mb=-1), dict(rir_max_mb=0.5)):
        with pytest.raises(ValueError, match="frontend.rir_"):
            task(rir=two, **bad)
        with pytest.raises(ValueError, match="frontend.rir_"):
            task(**bad)  # refused with the option off as well
    off = task()
    assert off.frontend.reverb is None and off.rir is None
    on = task(rir=two, rir_prob=0.25, rir_seed=6)
    assert isinstance(on.frontend.reverb, Reverberator) and on.rir is on.frontend.reverb.spec
    assert (on.rir.prob, on.rir.seed, on.rir.max_mb, on.rir.dirs) == (0.25, 6, 512, two)
    on.load_dataset("train", dirs.train, _dcfg(), None)
    on.load_dataset("valid", dirs.train, _dcfg(), None)
    assert on.dataset("train").rir is on.rir and on.dataset("valid").rir is None
    assert on.dataset("train").rir_index is on.frontend.reverb.index
    assert task(rir=dirs.a).rir.dirs == [dirs.a]  # a single directory as a string


def _write(path, rate=16000, channels=1, width=2, frames=100, value=0):
    with wave.open(path, "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes(bytes([value]) * (frames * channels * width))


def test_index_bank_and_their_refusals(dirs, tmp_path):
    from liteasr_amd.utils import wavio
    from liteasr_amd.utils.frontend import NoiseIndex, Reverberator, RirSpec

    spec = _spec(dirs)
    idx = spec.index()
    assert idx is spec.index() and isinstance(idx, NoiseIndex)
    assert idx.lengths.tolist() == RIR_A + RIR_B and idx.total == sum(RIR_A + RIR_B)
    assert [b.tolist() for b in idx.by_dir] == [[0, 1, 2], [3, 4]]
    assert len(pickle.dumps(idx.lengths)) + len(pickle.dumps(idx.offsets)) < 1000  # no sample in it
    bank, table = Reverberator(spec).read_bank()
    assert bank.dtype == torch.int16 and bank.shape == (idx.total,)
    assert table.dtype == torch.int64 and table.shape == (5, 3)
    assert table[:, 0].tolist() == idx.offsets.tolist() and table[:, 1].tolist() == idx.lengths.tolist()
    for path, (o, n, p) in zip(idx.paths, table.tolist()):
        h = wavio.read(path)[0]
        assert np.array_equal(bank[o:o + n].numpy(), h)
        assert p == int(np.argmax(h)) and h[p] == 32767 and p < 20  # synthetic_rir_dir: one unit direct-path peak
    # the cap names the total and leaves nothing out
    with pytest.raises(ValueError, match=f"{idx.total} samples.*rir_max_mb = 0"):
        RirSpec([dirs.a, dirs.b], max_mb=0).index()
    assert RirSpec([dirs.a, dirs.b], max_mb=1).index().total == idx.total
    # anything that is not 16 kHz 16-bit mono, an empty or too long recording, an empty or missing directory
    for name, kw, match in (("rate", dict(rate=8000), "x.wav"), ("stereo", dict(channels=2), "x.wav"),
                            ("bits", dict(width=1), "x.wav"), ("empty", dict(frames=0), "x.wav"),
                            ("long", dict(frames=65537, value=1), "x.wav holds 65537 samples, at most 65536")):
        d = tmp_path / name
        d.mkdir()
        _write(str(d / "x.wav"), **kw)
        (d / "wav.scp").write_text(f"x {d}/x.wav\n")
        with pytest.raises((ValueError, IOError), match=match):
            RirSpec([dirs.a, str(d)]).index()
    d = tmp_path / "nothing"
    d.mkdir()
    (d / "wav.scp").write_text("")
    with pytest.raises(ValueError, match="frontend.rir: .*lists no recording"):
        RirSpec([str(d)]).index()
    with pytest.raises(FileNotFoundError):
        RirSpec([str(tmp_path / "absent")]).index()
    with pytest.raises(ValueError, match="no directory"):
        RirSpec([])
    # an all-zero recording passes the index (no sample is read for it) and is refused when the bank is read
    d = tmp_path / "silent"
    d.mkdir()
    _write(str(d / "x.wav"), frames=300)
    (d / "wav.scp").write_text(f"x {d}/x.wav\n")
    silent = RirSpec([dirs.a, str(d)])
    assert silent.index().total == sum(RIR_A) + 300
    with pytest.raises(ValueError, match="x.wav holds 300 samples, all zero"):
        Reverberator(silent).read_bank()


# ------------------------------------------------------------------------------ the dataset ---
class _Counting(object):
    """A Generator that counts what is drawn from it."""

    def __init__(self, seed):
        self.rng, self.randoms, self.integers_ = np.random.default_rng(seed), 0, 0

    def random(self):
        self.randoms += 1
        return self.rng.random()

    def integers(self, *a, **kw):
        self.integers_ += 1
        return self.rng.integers(*a, **kw)


def test_draw_order():
    """One uniform number per row; a directory and a recording only for a reverberated row."""
    from liteasr_amd.utils.frontend import ReverbPlan, draw_reverb_plan

    index = SimpleNamespace(by_dir=[np.arange(0, 3), np.arange(3, 5)])
    ns = [100 + i for i in range(40)]
    for prob in (0.0, 0.3, 1.0):
        spec = SimpleNamespace(prob=prob, dirs=["a", "b"])
        rng = _Counting(5)
        plan = draw_reverb_plan(rng, spec, index, ns)
        assert isinstance(plan, ReverbPlan) and plan.rows.dtype == torch.int32 and plan.rows.shape == (40, 2)
        assert plan.rows[:, 0].tolist() == ns
        hit = int((plan.rows[:, 1] >= 0).sum())
        assert rng.randoms == 40 and rng.integers_ == 2 * hit
        assert hit == {0.0: 0, 1.0: 40}.get(prob, hit) and (prob != 0.3 or 0 < hit < 40)
        assert ((plan.rows[:, 1] >= -1) & (plan.rows[:, 1] < 5)).all()
        # the same stream, drawn by hand
        ref, want = np.random.default_rng(5), []
        for _ in ns:
            if ref.random() < prob:
                d = int(ref.integers(2))
                want.append(int(index.by_dir[d][int(ref.integers(len(index.by_dir[d])))]))
            else:
                want.append(-1)
        assert plan.rows[:, 1].tolist() == want


def _states():
    return random.getstate(), np.random.get_state()[1].tobytes(), np.random.get_state()[2], torch.get_rng_state()


def test_plan_is_drawn_from_a_generator_of_its_own(dirs):
    from liteasr_amd.utils.frontend import NoisePlan, NoiseSpec, ResamplePlan, ReverbPlan

    spec = _spec(dirs, prob=0.6, seed=4)
    idx = spec.index()
    torch.manual_seed(123)
    ds = _dataset(dirs.train, rir=spec)
    assert ds.rir is spec and ds.rir_index is idx and all(type(r).__name__ == "WavAudio" for r in ds.data)
    before = _states()
    outs = [ds.collator([ds[i]]) for i in range(len(ds))]
    after = _states()
    assert before[0] == after[0] and before[1:3] == after[1:3] and torch.equal(before[3], after[3])
    used = set()
    for i, out in enumerate(outs):
        assert len(out) == 5 and isinstance(out[4], ReverbPlan) and out[0].dtype == torch.int16
        rows = out[4].rows
        assert rows.dtype == torch.int32 and rows.shape == (len(ds[i]), 2)
        assert rows[:, 0].tolist() == [r.shape for r in ds[i]]
        assert ((rows[:, 1] >= -1) & (rows[:, 1] < len(idx.paths))).all()
        used |= set(rows[:, 1].tolist())
    assert -1 in used and len(used) > 2

    def plans(seed, torch_seed):
        torch.manual_seed(torch_seed)
        d2 = _dataset(dirs.train, rir=_spec(dirs, prob=0.6, seed=seed))
        return [d2.collator([d2[i]])[-1] for i in range(len(d2))]

    def same(a, b):
        return all(torch.equal(u.rows, v.rows) for u, v in zip(a, b))

    ref = [o[4] for o in outs]
    assert same(plans(4, 123), ref) and not same(plans(5, 123), ref) and not same(plans(4, 124), ref)
    # a copy sent to another process starts its own generator
    ds2 = pickle.loads(pickle.dumps(ds))
    assert ds2._rir_rng is None and ds._rir_rng is not None and ds2.rir_index.total == idx.total
    # Resample, Reverb, Noise, in this order; the noise and SpecAugment draws do not change when rir
    # is switched on, and the ReverbPlan counts the resampled samples
    dcfg = _dcfg(batch_size=4)
    kw = dict(workflow=("spec_aug",), dcfg=dcfg, speed_perturb=[0.9, 1.0, 1.1])
    torch.manual_seed(77)
    plain = _dataset(dirs.train, noise=NoiseSpec([dirs.noise], prob=0.8, seed=2), **kw)
    both = _dataset(dirs.train, noise=NoiseSpec([dirs.noise], prob=0.8, seed=2), rir=spec, **kw)
    for i in range(len(plain)):
        random.seed(4)
        np.random.seed(4)
        a = plain.collator([plain[i]])
        random.seed(4)
        np.random.seed(4)
        b = both.collator([both[i]])
        assert len(a) == 7 and len(b) == 8
        assert [type(p) for p in b[5:]] == [ResamplePlan, ReverbPlan, NoisePlan] and isinstance(a[6], NoisePlan)
        assert all(torch.equal(torch.as_tensor(u), torch.as_tensor(v)) for u, v in zip(a[:5], b[:5]))
        assert torch.equal(a[5].rows, b[5].rows) and b[6].rows[:, 0].tolist() == b[5].rows[:, 1].tolist()
        assert torch.equal(a[6].rows, b[7].rows) and torch.equal(a[6].sources, b[7].sources)
    # equal seeds: the two streams still differ
    torch.manual_seed(5)
    ds3 = _dataset(dirs.train, rir=_spec(dirs, prob=0.5, seed=0), noise=NoiseSpec([dirs.noise], prob=0.5, seed=0))
    ds3.collator([ds3[0]])
    assert ds3._rir_rng[1].random() != ds3._noise_rng[1].random()


def test_probability_bounds(dirs):
    never = _dataset(dirs.train, rir=_spec(dirs, prob=0.0))
    always = _dataset(dirs.train, rir=_spec(dirs, prob=1.0))
    for i in range(len(never)):
        assert (never.collator([never[i]])[-1].rows[:, 1] == -1).all()
        assert (always.collator([always[i]])[-1].rows[:, 1] >= 0).all()


def test_other_splits_and_feats_ignore_it(dirs, tmp_path, caplog):
    import shutil

    from liteasr_amd.utils.kaldiio import save_ark

    spec = _spec(dirs)
    for split in ("valid", "test"):
        a, b = _dataset(dirs.train, split=split), _dataset(dirs.train, split=split, rir=spec)
        assert b.rir is None and b.rir_index is None and a.data == b.data and len(a) == len(b)
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
        shutil.copy(os.path.join(dirs.train, fn), d)
    with caplog.at_level(logging.INFO):
        a, b = _dataset(d), _dataset(d, rir=spec)
    assert sum("rir is ignored" in r.getMessage() for r in caplog.records) == 1
    assert not b.wav and b.rir is None and a.data == b.data
    assert all(torch.equal(u, v) for u, v in zip(a.collator([a[0]]), b.collator([b[0]])))


@pytest.mark.parametrize("workflow", [(), ("spec_aug",)])
def test_off_is_what_it_was(dirs, workflow):
    """rir=None: the records, the batches and what the collator delivers equal those of a dataset
    built without the argument, and nothing is drawn."""
    a = _dataset(dirs.train, workflow=workflow)
    b = _dataset(dirs.train, workflow=workflow, rir=None)
    assert b.rir is None and b.rir_index is None and b.data == a.data and len(a) == len(b) == 3
    for i in range(len(a)):
        assert b[i] == a[i]
        random.seed(4)
        np.random.seed(4)
        ca = a.collator([a[i]])
        random.seed(4)
        np.random.seed(4)
        cb = b.collator([b[i]])
        assert type(cb) is tuple and len(ca) == len(cb) == (5 if workflow else 4)
        assert all(torch.equal(torch.as_tensor(u), torch.as_tensor(v)) for u, v in zip(ca, cb))
    assert b._rir_rng is None


def test_features_refuses_a_plan_it_cannot_use():
    """A ReverbPlan without task.frontend.rir, or on a feature batch, is a TypeError."""
    from liteasr_amd.trainer import Trainer
    from liteasr_amd.utils.frontend import ReverbPlan

    plan = ReverbPlan(torch.tensor([[400, 0]], dtype=torch.int32))
    tr = SimpleNamespace(device=torch.device("cpu"), task=SimpleNamespace(frontend=SimpleNamespace(reverb=None, noise=None)))
    pcm = (torch.zeros(1, 400, dtype=torch.int16), torch.tensor([1]), torch.zeros(1, 1, dtype=torch.long),
           torch.tensor([1]))
    with pytest.raises(TypeError, match="a ReverbPlan needs task.frontend.rir"):
        Trainer._features(tr, pcm + (plan,))
    feats = (torch.zeros(1, 5, 80), torch.tensor([5]), torch.zeros(1, 1, dtype=torch.long), torch.tensor([1]))
    with pytest.raises(TypeError, match="raw-audio batches only"):
        Trainer._features(tr, feats + (plan,))
