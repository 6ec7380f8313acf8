"""``lasr_ctc_align`` on the GPU against the float32 restatement (tests/ctc_align_ref.py), bit for
bit: states, spans and the score's bits, the -1s past ``ilen`` / ``tlen``, untouched guard
elements, the tie rule, row independence, the existing loss kernel as an upper bound, and the
argument checks.  Then the layers above it: ``decoding.ctc_align`` on a tiny fp32 U2,
``ASRTask.align`` from int16 PCM, and ``python -m liteasr_amd.align``.

The restatement is the yardstick because every step is a max of fp32 values and one fp32 add:
nothing in it can be rounded differently on the device.  tests/test_ctc_align_cpu.py holds the
restatement itself to float64 and to brute force."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ctc_align_cases as C
import ctc_align_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
GUARD = 7
SENT_I, SENT_F = -77777, 12345.0

SMALL = [(8, 3), (5, 5), (12, 4), (5, 4), (62, 20), (64, 0), (1, 1), (1, 0), (0, 0), (0, 2)]
GROUPS = {
    "lds": SMALL + [(250, 100)],
    "spill": [(600, 256)] + SMALL,
    "edge_in": [C.LDS_EDGE_IN] + SMALL,
    "edge_out": [C.LDS_EDGE_OUT] + SMALL,
}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _launch(lp, targets, ilen, tlen, ws_bytes=None, null=None, expect_rc=0):
    """lasr_ctc_align on host arrays with sentinel-filled, guarded outputs; returns the numpy
    outputs (guards checked) and the status."""
    from liteasr_amd import _native as N
    from liteasr_amd import kernels as K

    B, T, L1 = lp.shape
    Lmax = L1 - 1
    bufs = {"states": torch.full((2 * GUARD + B * T,), SENT_I, dtype=torch.int32, device=DEV),
            "spans": torch.full((2 * GUARD + B * Lmax * 2,), SENT_I, dtype=torch.int32, device=DEV),
            "score": torch.full((2 * GUARD + B,), SENT_F, dtype=torch.float32, device=DEV)}
    need = N.load().lasr_ctc_align_workspace(B, T, Lmax)
    ws = torch.empty(max(need, 4) // 4, dtype=torch.int32, device=DEV)
    d = [_dev(x) for x in (targets, ilen, tlen, lp)]
    ptrs = {k: (None if k == null else v[GUARD:].data_ptr()) for k, v in bufs.items()}
    rc = N.load().lasr_ctc_align(B, T, Lmax, K.ptr(d[0]) if Lmax else None, K.ptr(d[1]), K.ptr(d[2]), K.ptr(d[3]),
                                 ws.data_ptr(), need if ws_bytes is None else ws_bytes, ptrs["states"],
                                 ptrs["spans"], ptrs["score"], K.stream())
    torch.cuda.synchronize()
    assert rc == expect_rc
    out = {k: v.cpu().numpy() for k, v in bufs.items()}
    for k, v in out.items():
        sent = SENT_F if k == "score" else SENT_I
        assert (v[:GUARD] == sent).all() and (v[len(v) - GUARD:] == sent).all(), f"{k}: guard overwritten"
    return (out["states"][GUARD:-GUARD].reshape(B, T), out["spans"][GUARD:-GUARD].reshape(B, Lmax, 2),
            out["score"][GUARD:-GUARD]), rc


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _assert_equal(got, want, what=""):
    for name, g, w in zip(("states", "spans"), got[:2], want[:2]):
        assert g.dtype == np.int32 and np.array_equal(g, w), f"{what}{name} differ"
    assert np.array_equal(_bits(got[2]), _bits(want[2])), f"{what}score bits differ: {got[2]} vs {want[2]}"


@pytest.fixture(scope="module")
def batches():
    """per group: the padded batch and the float32 restatement of it (made once, never changed)."""
    out = {}
    for i, (name, shapes) in enumerate(GROUPS.items()):
        batch = C.make_batch(shapes, seed=100 * i)
        out[name] = (shapes, batch, R.align_batch(*batch, dtype=np.float32))
    return out


@pytest.mark.parametrize("group", list(GROUPS))
def test_kernel_equals_float32_restatement(batches, group):
    from liteasr_amd import kernels as K

    shapes, (lp, targets, ilen, tlen), want = batches[group]
    B, T, L1 = lp.shape
    spilled = K.ctc_align_workspace(B, T, L1 - 1) > 0
    assert spilled == (group in ("spill", "edge_out"))
    got, _ = _launch(lp, targets, ilen, tlen)
    _assert_equal(got, want, f"{group}: ")
    states, spans, score = got
    for b, (Tb, Lb) in enumerate(shapes):
        assert (states[b, Tb:] == -1).all() and (spans[b, Lb:] == -1).all()
        ok = C.feasible(Tb, targets[b, :Lb]) and Tb > 0
        if Tb == 0:
            assert score[b] == (0.0 if Lb == 0 else -np.inf)
        assert np.isfinite(score[b]) == (ok or (Tb == 0 and Lb == 0))
        if ok:
            assert (states[b, :Tb] >= 0).all() and (spans[b, :Lb] >= 0).all()
        else:
            assert (states[b] == -1).all() and (spans[b] == -1).all()
    # the wrapper (own outputs, workspace from K.WS) gives the same
    st, sp, sc = K.ctc_align(_dev(lp), _dev(targets), _dev(ilen), _dev(tlen))
    _assert_equal((st.cpu().numpy(), sp.cpu().numpy(), sc.cpu().numpy()), want, f"{group} (wrapper): ")


def test_exactly_feasible_is_finite(batches):
    shapes, (lp, targets, ilen, tlen), want = batches["lds"]
    b = shapes.index((5, 4))
    y = targets[b, :4]
    assert C.repeats(y) == 1  # the planted repeat only: T = 5 = L + repeats
    assert np.isfinite(want[2][b]) and (want[0][b, :5] >= 0).all()


@pytest.mark.parametrize("T,L", [(10, 3), (9, 4)])
def test_uniform_logits_all_paths_tie(T, L):
    y = np.array([[5, 5, 7, 9][:L]], dtype=np.int32)
    lp = np.full((1, T, L + 1), np.float32(-np.log(50.0)), dtype=np.float32)
    ilen, tlen = np.array([T], dtype=np.int32), np.array([L], dtype=np.int32)
    got, _ = _launch(lp, y, ilen, tlen)
    _assert_equal(got, R.align_batch(lp, y, ilen, tlen), "ties: ")
    assert np.isfinite(got[2][0])


def test_planted_path_comes_back():
    T, L = 16, 4
    y = np.array([[3, 3, 8, 2]], dtype=np.int32)
    path = np.array([0, 1, 1, 2, 3, 3, 3, 4, 4, 5, 6, 6, 7, 7, 8, 8], dtype=np.int32)
    lp = np.full((1, T, L + 1), -20.0, dtype=np.float32)
    for t, s in enumerate(path):
        lp[0, t, (1 + s // 2) if s & 1 else 0] = -0.01
    ilen, tlen = np.array([T], dtype=np.int32), np.array([L], dtype=np.int32)
    (states, spans, score), _ = _launch(lp, y, ilen, tlen)
    assert np.array_equal(states[0], path)
    assert spans[0].tolist() == [[1, 3], [4, 7], [9, 10], [12, 14]]
    _assert_equal((states, spans, score), R.align_batch(lp, y, ilen, tlen), "planted: ")


def test_rows_are_independent():
    shapes = [(62, 20), (40, 7), (5, 5), (64, 0), (33, 12)]
    lp, targets, ilen, tlen = C.make_batch(shapes, seed=900)
    full, _ = _launch(lp, targets, ilen, tlen)
    lp2, targets2, _, _ = C.make_batch(shapes, seed=950)
    for b in range(len(shapes)):
        alone, _ = _launch(lp[b:b + 1], targets[b:b + 1], ilen[b:b + 1], tlen[b:b + 1])
        mixed_lp, mixed_tg = lp2.copy(), targets2.copy()
        mixed_lp[b], mixed_tg[b] = lp[b], targets[b]
        mixed, _ = _launch(mixed_lp, mixed_tg, ilen, tlen)
        for f, a, m in zip(full, alone, mixed):
            assert f[b].tobytes() == a[0].tobytes() == m[b].tobytes()


def test_score_is_bounded_by_the_loss_kernel():
    from liteasr_amd import kernels as K

    shapes = [(8, 3), (5, 5), (12, 4), (5, 4), (62, 20), (250, 100), (64, 0), (1, 1), (1, 0)]
    B, T, Lmax = len(shapes), 250, 100
    logits = np.zeros((B, T, C.V), dtype=np.float32)
    targets = np.zeros((B, Lmax), dtype=np.int32)
    for b, (Tb, Lb) in enumerate(shapes):
        x, y = C.make_logits(Tb, Lb, 300 + b)
        logits[b, :Tb], targets[b, :Lb] = x, y
    ilen = _dev(np.array([t for t, _ in shapes], dtype=np.int32))
    tlen = _dev(np.array([l for _, l in shapes], dtype=np.int32))
    lg, tg = _dev(logits), _dev(targets)
    lse = torch.empty(B * T, dtype=torch.float32, device=DEV)
    lp = torch.empty(B, T, Lmax + 1, dtype=torch.float32, device=DEV)
    alpha = torch.empty(B, T, 2 * Lmax + 1, dtype=torch.float32, device=DEV)
    nll = torch.empty(B, dtype=torch.float32, device=DEV)
    K.ctc_fwd(lg, tg, ilen, tlen, lse, lp, alpha, nll)
    states, spans, score = K.ctc_align(lp, tg, ilen, tlen)
    nll, score = nll.cpu().numpy().astype(np.float64), score.cpu().numpy().astype(np.float64)
    _assert_equal((states.cpu().numpy(), spans.cpu().numpy(), score),
                  R.align_batch(lp.cpu().numpy(), targets, ilen.cpu().numpy(), tlen.cpu().numpy()), "device lp: ")
    for b, (Tb, Lb) in enumerate(shapes):
        print(f"row {b} (T={Tb}, L={Lb}): score {score[b]:.6f}  -nll {-nll[b]:.6f}")
        assert (score[b] == -np.inf) == (nll[b] == np.inf)
        if np.isfinite(nll[b]):
            assert score[b] <= -nll[b] + Tb * 2.0 ** -24 * abs(nll[b]) * 4


def test_argument_checks_leave_outputs_untouched():
    from liteasr_amd import _native as N

    def untouched(out):
        return all((o == (SENT_F if o.dtype == np.float32 else SENT_I)).all() for o in out)

    # one lattice state per thread: 2 Lmax + 1 <= 1024
    lp = np.zeros((1, 4, 513), dtype=np.float32)
    one = np.array([2], dtype=np.int32)
    out, _ = _launch(lp, np.ones((1, 512), dtype=np.int32), one + 2, one, expect_rc=-1)
    assert untouched(out) and b"Lmax" in N.load().lasr_last_error()
    # a spill shape with a workspace one byte short
    lp, targets, ilen, tlen = C.make_batch([(600, 256)], seed=7)
    need = N.load().lasr_ctc_align_workspace(1, 600, 256)
    assert need > 0
    out, _ = _launch(lp, targets, ilen, tlen, ws_bytes=need - 1, expect_rc=-1)
    assert untouched(out) and b"workspace" in N.load().lasr_last_error()
    # null outputs
    lp, targets, ilen, tlen = C.make_batch([(8, 3)], seed=8)
    for null in ("states", "spans", "score"):
        out, _ = _launch(lp, targets, ilen, tlen, null=null, expect_rc=-1)
        assert untouched(out)


# ------------------------------------------------------------------ the layers above the kernel ---
V_MODEL = 30


@pytest.fixture(scope="module")
def tiny():
    """A tiny fp32 U2 in eval mode and a padded batch: B = 4, mixed frame counts, T = 120."""
    from liteasr_amd.models.u2 import U2, U2Config
    from liteasr_amd.utils.cfg import resolve_self

    c = U2Config(input_dim=80, vocab_size=V_MODEL, enc_dim=64, enc_ff_dim=128, enc_layers=2, dec_dim=64,
                 dec_ff_dim=128, dec_layers=1, dropout_rate=0.0, compute_dtype="fp32")
    resolve_self(c)
    torch.manual_seed(11)
    model = U2(c).to(DEV).eval()
    rng = np.random.default_rng(5)
    xlens = [120, 87, 120, 33]
    ylens = [9, 6, 0, 12]  # 33 frames subsample to 7: 12 tokens do not fit
    xs = np.zeros((4, 120, 80), dtype=np.float32)
    ys = np.full((4, 12), -1, dtype=np.int64)
    for b in range(4):
        xs[b, :xlens[b]] = rng.standard_normal((xlens[b], 80)).astype(np.float32)
        ys[b, :ylens[b]] = rng.integers(1, V_MODEL - 1, ylens[b])
    ys[0, 1] = ys[0, 0]
    return model, torch.from_numpy(xs).to(DEV), xlens, torch.from_numpy(ys).to(DEV), ylens


def _first_stage(model, xs, xlens, ys, ylens):
    """lp as K.ctc_fwd(..., alpha=None) makes it from the model and the batch, and what it read."""
    from liteasr_amd import kernels as K
    from liteasr_amd.nets import decode as DN

    B = xs.shape[0]
    with torch.no_grad():
        xe, prep, _ = model._run_encoder(xs, torch.tensor(xlens, device=DEV), ys, torch.tensor(ylens, device=DEV))
        h = DN.encoder_out(xe, model, model.compute_dtype)
        hc = DN.ctc_logits(h, model).view(B, prep.T, -1)
        lse = torch.empty(B * prep.T, dtype=torch.float32, device=DEV)
        lp = torch.empty(B, prep.T, prep.L + 1, dtype=torch.float32, device=DEV)
        K.ctc_fwd(hc, prep.tgt_ctc, prep.pred_len, prep.ylen, lse, lp, None, None)
    return lp.cpu().numpy(), prep.tgt_ctc.cpu().numpy(), prep.pred_len.cpu().numpy(), prep.ylen.cpu().numpy()


def _assert_record(rec, want, b, Tb, Lb):
    states, spans, score = want
    if not np.isfinite(score[b]):
        assert rec is None
        return
    assert rec["states"] == states[b, :Tb].tolist() and len(rec["states"]) == Tb
    assert rec["spans"] == [tuple(p) for p in spans[b, :Lb].tolist()]
    assert np.float32(rec["score"]) == score[b]


def test_decoding_ctc_align_equals_restatement_on_the_models_lp(tiny):
    from liteasr_amd import decoding as D

    model, xs, xlens, ys, ylens = tiny
    lp, targets, pred_len, ylen = _first_stage(model, xs, xlens, ys, ylens)
    assert pred_len.tolist() == [((n - 1) // 2 - 1) // 2 for n in xlens] and ylen.tolist() == ylens
    want = R.align_batch(lp, targets, pred_len, ylen)
    trace = {}
    recs = D.ctc_align(model, xs, xlens, ys, ylens, trace=trace)
    assert np.array_equal(trace["lp"].cpu().numpy(), lp)
    assert len(recs) == 4 and recs[3] is None and all(r is not None for r in recs[:3])
    for b in range(4):
        _assert_record(recs[b], want, b, int(pred_len[b]), ylens[b])
    assert recs[2]["spans"] == [] and set(recs[2]["states"]) == {0}
    assert model.align(xs, xlens, ys, ylens) == recs


def test_full_length_row_equals_the_utterance_alone(tiny):
    from liteasr_amd import decoding as D

    model, xs, xlens, ys, ylens = tiny
    recs = D.ctc_align(model, xs, xlens, ys, ylens)
    for b in (0, 2):
        assert xlens[b] == xs.shape[1]
        alone = D.ctc_align(model, xs[b:b + 1], [xlens[b]], ys[b:b + 1, :max(ylens[b], 1)], [ylens[b]])[0]
        print(f"row {b}: score in the batch {recs[b]['score']!r}, alone {alone['score']!r}")
        assert alone == recs[b]


def test_one_device_to_host_copy(tiny, monkeypatch):
    from liteasr_amd import decoding as D

    model, xs, xlens, ys, ylens = tiny
    D.ctc_align(model, xs, xlens, ys, ylens)  # warm: workspace growth, lazy tables
    count = {"n": 0}
    for name in ("cpu", "tolist", "item", "numpy", "__bool__", "__int__", "__float__"):
        inner = getattr(torch.Tensor, name)

        def counted(self, *a, _inner=inner, **k):
            if self.is_cuda:
                count["n"] += 1
            return _inner(self, *a, **k)

        monkeypatch.setattr(torch.Tensor, name, counted)
    inner_copy = torch.Tensor.copy_

    def counted_copy(self, src, *a, **k):
        if not self.is_cuda and torch.is_tensor(src) and src.is_cuda:
            count["n"] += 1
        return inner_copy(self, src, *a, **k)

    monkeypatch.setattr(torch.Tensor, "copy_", counted_copy)
    trace = {}
    recs = D.ctc_align(model, xs, xlens, ys, ylens, trace=trace)
    monkeypatch.undo()
    assert count["n"] == 1 and trace["d2h"] == 1 and recs[0] is not None


def _task(tmp_path):
    from liteasr_amd.tasks.asr import ASRConfig, ASRTask

    vocab = tmp_path / "vocab.txt"
    vocab.write_text("".join(f"t{k} {k}\n" for k in range(1, V_MODEL - 1)))  # 0 blank, V - 1 sos / eos
    task = ASRTask(ASRConfig(vocab=str(vocab), train="", valid="", save_dir=str(tmp_path / "ckpts")))
    assert task.vocab_size == V_MODEL
    return task


def test_task_align_from_pcm_equals_features(tiny, tmp_path):
    from liteasr_amd.utils.frontend import num_frames

    model, _, _, ys, ylens = tiny
    task = _task(tmp_path)
    rng = np.random.default_rng(9)
    samples = [19440, 14000, 19440, 5600]
    pcm = np.zeros((4, max(samples)), dtype=np.int16)
    for b, n in enumerate(samples):
        pcm[b, :n] = rng.integers(-8000, 8000, n)
    pcm = torch.from_numpy(pcm).to(DEV)
    frames = [num_frames(n) for n in samples]
    assert frames == [120, 86, 120, 33]
    feats = task.frontend(pcm, torch.tensor(frames, dtype=torch.int32, device=DEV), max_frames=max(frames))
    from_pcm = task.align(pcm, samples, ys, ylens, model)
    from_feats = task.align(feats, frames, ys, ylens, model)
    assert from_pcm == from_feats and from_pcm[3] == (None, float("-inf"))
    recs = model.align(feats, frames, ys, ylens)
    for b in range(3):
        tokens, score = from_pcm[b]
        assert score == recs[b]["score"] and len(tokens) == ylens[b]
        assert [t for t, _, _ in tokens] == [f"t{int(i)}" for i in ys[b, :ylens[b]].tolist()]
        for (_, start, dur), (first, end) in zip(tokens, recs[b]["spans"]):
            assert start == pytest.approx(0.04 * first, abs=1e-9) and dur == pytest.approx(0.04 * (end - first), abs=1e-9)
    with pytest.raises(TypeError, match="no align"):
        task.align(feats, frames, ys, ylens, object())


# ------------------------------------------------------------------------------------- CLI ---
N_UTT = 6


def _read(path):
    return [ln.split() for ln in open(path).read().splitlines()]


def test_cli(tmp_path, monkeypatch):
    from cfgtree import user_tree
    from liteasr_amd import infer as I
    from liteasr_amd import tasks
    from liteasr_amd.config.compose import compose

    conf, data = user_tree(tmp_path, compute_dtype="fp32")
    for fn in ("feats.scp", "text", "utt2num_frames"):
        lines = (data / fn).read_text().splitlines()[:N_UTT]
        (data / fn).write_text("\n".join(lines) + "\n")
    run_dir = tmp_path / "runs" / "asr_U2"
    (run_dir / "ckpts").mkdir(parents=True)
    monkeypatch.chdir(run_dir)
    ovr = [f"task.test=[{data}]", "inference.ckpt_name=1"]
    cfg = compose(str(conf), "config", ovr, job_name="align")
    task = tasks.setup_task(cfg.task)
    task.load_dataset("test", task.cfg.test, None, cfg.postprocess)
    torch.manual_seed(3)
    torch.save(task.build_model(cfg.model).state_dict(), run_dir / "ckpts" / "model.ep.1.pt")
    ds = task.dataset("test")[0]
    ids = [ln.split()[0] for ln in (data / "text").read_text().splitlines()]
    texts = [ds[i].text for i in range(N_UTT)]
    assert ds.uttids == ids and len(ds) == N_UTT
    xlens = [ds[i].xlen for i in range(N_UTT)]
    fits = [((n - 1) // 2 - 1) // 2 >= len(t) + C.repeats(list(t)) for n, t in zip(xlens, texts)]
    assert not all(fits) and sum(fits) >= 4  # the fixture has a transcript longer than its frames
    whole = [u for u, t, f in zip(ids, texts, fits)
             if f and "<unk>" not in task.vocab.lookup(ds[ids.index(u)].tokenids, convert=True)]
    assert len(whole) >= 3  # utterances whose joined tokens must be the transcript itself
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    runs = {}
    for bs in (4, 1):
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "liteasr_amd.align", "-cd", str(conf)]
                           + ovr + [f"inference.batch_size={bs}"], cwd=tmp_path, env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        runs[bs] = (_read(run_dir / "align" / "data.ctm"), _read(run_dir / "align" / "data.scores"))
    for bs, (ctm, scores) in runs.items():
        assert [s[0] for s in scores] == ids and all(len(s) == 3 for s in scores)
        assert [s[1] == "-inf" for s in scores] == [not f for f in fits]
        assert all(len(c) == 5 and c[1] == "1" for c in ctm)
        assert [u for u in dict.fromkeys(c[0] for c in ctm)] == [u for u, f in zip(ids, fits) if f]  # dataset order
        for u, text, f in zip(ids, texts, fits):
            mine = [c for c in ctm if c[0] == u]
            if not f:
                assert not mine
                continue
            # the transcript as the vocabulary spells it (the fixture's vocabulary has no "z": <unk>)
            spelled = list(task.vocab.lookupi(ds[ids.index(u)].tokenids, convert=True))
            assert [c[4] for c in mine] == spelled and len(mine) == len(text)
            assert "".join(c[4] for c in mine) == text or "<unk>" in spelled
            starts = [float(c[2]) for c in mine]
            assert starts == sorted(starts) and all(float(c[3]) > 0 for c in mine)
    # batch_size 1: the same tokens per utterance; the same times for each group's longest row
    (ctm4, _), (ctm1, _) = runs[4], runs[1]
    assert [(c[0], c[4]) for c in ctm4] == [(c[0], c[4]) for c in ctm1]
    for group in I.batch_plan(xlens, 4):
        longest = ids[max(group, key=lambda i: xlens[i])]
        assert [c for c in ctm4 if c[0] == longest] == [c for c in ctm1 if c[0] == longest]
