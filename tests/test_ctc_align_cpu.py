"""The yardstick of the CTC alignment kernel, held to account without a GPU: the float32
restatement (tests/ctc_align_ref.py) against float64 and against brute force, the structure of its
output, and the host side of the feature (the workspace formula, ``inference.align_dir``, which
models have ``align``, the dataset's utterance ids)."""

import os
from types import SimpleNamespace

import numpy as np
import pytest

import ctc_align_cases as C
import ctc_align_ref as R

SEEDS = 6
GROUPS = ["task=asr_kaldi", "model=conformer_small", "criterion=hybrid_ctc_w03", "optimizer=noam_d256"]


@pytest.fixture(scope="module")
def cases():
    """(T, L, seed) -> (lp, y, float32 result, float64 result), computed once."""
    out = {}
    for T, L in C.SHAPES:
        for seed in range(2 if T * (2 * L + 1) > 100000 else SEEDS):
            lp, y = C.make_case(T, L, seed)
            out[(T, L, seed)] = (lp, y, R.align_row(lp, y, T, np.float32), R.align_row(lp, y, T, np.float64))
    return out


def test_float32_and_float64_agree(cases):
    feas = same = 0
    for (T, L, seed), (lp, y, r32, r64) in cases.items():
        ok = C.feasible(T, y)
        assert (r32[1] is not None) == ok and (r64[1] is not None) == ok, (T, L, seed)
        if not ok:
            assert r32[0] == -np.inf and r64[0] == -np.inf
            continue
        feas += 1
        same += int(np.array_equal(r32[1], r64[1]))
        s32, s64 = float(r32[0]), float(r64[0])
        assert np.isfinite(s32) and abs(s32 - s64) <= T * 2.0 ** -24 * abs(s64) * 4, (T, L, seed, s32, s64)
    assert feas >= 40 and same >= 0.9 * feas, (same, feas)


def test_cases_cover_what_they_claim(cases):
    assert all(cases[(5, 5, s)][2][1] is None for s in range(SEEDS))  # the repeat makes 5 frames too few
    exact = [s for s in range(SEEDS) if C.repeats(cases[(5, 4, s)][1]) == 1]
    assert exact and all(np.isfinite(cases[(5, 4, s)][2][0]) for s in exact)  # T = L + repeats: finite
    assert all(cases[(64, 0, s)][2][1].tolist() == [0] * 64 for s in range(SEEDS))
    for s in range(SEEDS):  # an empty target sums the blank log-probs left to right in fp32
        lp = cases[(64, 0, s)][0]
        acc = np.float32(lp[0, 0])
        for t in range(1, 64):
            acc = np.float32(acc + lp[t, 0])
        assert cases[(64, 0, s)][2][0] == acc


def test_structure_of_the_path(cases):
    for (T, L, seed), (lp, y, (score, states, spans), _) in cases.items():
        if states is None:
            continue
        S = 2 * L + 1
        ext, skip = R.extended(y), R.skip_allowed(y)
        assert states[0] in (0, 1) and states[-1] in (S - 1, S - 2) or S == 1 and (states == 0).all()
        steps = np.diff(states)
        assert ((steps >= 0) & (steps <= 2)).all()
        for t in np.nonzero(steps == 2)[0]:
            assert skip[states[t + 1]]
        # collapsing the path (merge repeats, drop blanks) gives the target
        labels = ext[states]
        keep = np.concatenate([[True], states[1:] != states[:-1]])
        collapsed = [int(v) for v, k in zip(labels, keep) if k and v != 0]
        assert collapsed == [int(v) for v in y]
        # the score is the sum of the emissions along the path (to rounding)
        col = np.where(states & 1, 1 + states // 2, 0)
        total = float(np.sum(lp[np.arange(T), col].astype(np.float64)))
        assert abs(float(score) - total) <= T * 2.0 ** -24 * abs(total) * 4
        # spans tile the odd states: token i holds exactly the frames [first, end)
        assert spans.shape == (L, 2)
        for i, (first, end) in enumerate(spans):
            assert 0 <= first < end <= T and (states[first:end] == 2 * i + 1).all()
            assert int(np.sum(states == 2 * i + 1)) == end - first
        if L:
            assert (spans[1:, 0] >= spans[:-1, 1]).all()


@pytest.mark.parametrize("T,L", [(6, 2), (7, 3)])
def test_viterbi_score_is_the_brute_force_maximum(T, L):
    for seed in range(8):
        lp, y = C.make_case(T, L, seed)
        if L == 2:
            y[1] = y[0]  # the recipe plants its repeat from L = 3 on
            lp[:, 2] = lp[:, 1]
        best = R.brute_force_best(lp, y, T)
        s64, states, _ = R.align_row(lp, y, T, np.float64)
        assert states is not None and abs(float(s64) - best) <= 1e-12 * abs(best)
        s32 = float(R.align_row(lp, y, T, np.float32)[0])
        assert abs(s32 - best) <= T * 2.0 ** -24 * abs(best) * 4


def test_workspace_formula_matches_the_library():
    from liteasr_amd import _native as N
    from liteasr_amd import kernels as K

    lib = N.load()
    seen = set()
    for B in (0, 1, 3):
        for T in (0, 1, 16, 17, 250, 480, 481, 600, 993, 4000):
            for Lmax in (0, 1, 100, 127, 255, 256, 511, 512):
                need = K.ctc_align_workspace(B, T, Lmax)  # asserts the two agree
                assert need == lib.lasr_ctc_align_workspace(B, T, Lmax)
                if B == 0:
                    assert need == 0
                seen.add(need > 0)
    assert seen == {True, False}
    assert K.ctc_align_workspace(1, *C.LDS_EDGE_IN) == 0 and K.ctc_align_workspace(1, *C.LDS_EDGE_OUT) > 0
    assert K.ctc_align_workspace(2, 600, 256) == 2 * 38 * 513 * 4
    # just inside: the score vectors and the move words fill at most 64 KB
    T, L = C.LDS_EDGE_IN
    assert 4 * (2 * L + 1) * (2 + -(-T // 16)) <= 65536 < 4 * (2 * L + 1) * (2 + -(-(T + 1) // 16))


def test_align_dir_composes():
    from liteasr_amd.config.compose import compose

    cfg = compose(overrides=GROUPS, job_name="align")
    assert cfg.inference.align_dir == "align" and cfg.inference.batch_size == 1
    assert cfg.hydra.job_logging.handlers.file.filename == "align.log"
    cfg = compose(overrides=GROUPS + ["inference.align_dir=/x/ali", "inference.batch_size=8"], job_name="align")
    assert cfg.inference.align_dir == "/x/ali" and cfg.inference.batch_size == 8


def test_only_u2_aligns():
    from liteasr_amd.models.paraformer import Paraformer
    from liteasr_amd.models.transducer import Transducer
    from liteasr_amd.models.u2 import U2

    assert callable(getattr(U2, "align", None)) and U2.frame_subsampling == 4
    assert not hasattr(Paraformer, "align") and not hasattr(Transducer, "align")


def test_align_refuses_a_model_without_a_ctc_head(tmp_path, monkeypatch):
    """before any data is read: task.test names a directory that does not exist"""
    from liteasr_amd import align as A
    from liteasr_amd.config.compose import ConfigError

    from cfgtree import user_tree

    conf, data = user_tree(tmp_path)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ConfigError, match="no align"):
        A.main(["-cd", str(conf), f"task.test=[{tmp_path / 'nowhere'}]", "inference.ckpt_name=1", "model.name=transducer"])


def _dataset(d, split, **kw):
    from liteasr_amd.config import PostProcessConfig
    from liteasr_amd.dataclass.vocab import Vocab
    from liteasr_amd.dataset import AudioFileDataset

    dcfg = SimpleNamespace(batch_count="seq", batch_size=3, max_len_in=100000, max_len_out=1000, max_frame_num=100000,
                           min_batch_size=1, sort_by="input")
    return AudioFileDataset(split, d, None, dcfg, PostProcessConfig(workflow=[]), Vocab(os.path.join(d, "vocab.txt")),
                            **kw)


def _ids(path):
    return [ln.split()[0] for ln in open(path).read().splitlines() if ln.strip()]


def test_dataset_keeps_uttids_feats(tmp_path):
    from cfgtree import data_dir

    d = str(data_dir(tmp_path))
    ds = _dataset(d, "test", keep_raw=True)
    ids = _ids(os.path.join(d, "text"))
    assert ds.uttids == ids and len(ds.uttids) == len(ds.data) == 16
    texts = dict(ln.split(maxsplit=1) for ln in open(os.path.join(d, "text")).read().splitlines())
    assert [rec.text for rec in ds.data] == [texts[u] for u in ds.uttids]


def test_dataset_keeps_uttids_wav_and_speed_perturb(tmp_path):
    from liteasr_amd.utils.synthetic import synthetic_wav_dir

    lengths = [16000, 399, 8000, 400, 12345, 200]  # two are shorter than one frame and are dropped
    d = synthetic_wav_dir(str(tmp_path / "wav"), lengths, seed=3)
    ids = _ids(os.path.join(d, "wav.scp"))
    kept = [u for u, n in zip(ids, lengths) if n >= 400]
    ds = _dataset(d, "test", keep_raw=True)
    assert ds.uttids == kept and len(ds.data) == len(kept)
    sp = _dataset(d, "train", speed_perturb=[0.9, 1.0, 1.1])
    assert len(sp.uttids) == len(sp.data) > len(kept)
    by_shape = {}
    for u, rec in zip(ds.uttids, ds.data):
        by_shape[u] = rec.shape
    for u, rec in zip(sp.uttids, sp.data):  # every copy carries the id of its source utterance
        assert rec.shape == dict(zip(ids, lengths))[u]
    assert [u for u, rec in zip(sp.uttids, sp.data) if rec.ratio == (1, 1)] == kept
    # test and valid splits ignore speed_perturb
    assert _dataset(d, "test", speed_perturb=[0.9, 1.0]).uttids == kept
