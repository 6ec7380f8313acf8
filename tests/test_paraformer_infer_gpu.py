"""Paraformer one-pass decoding on the GPU (lasr_cif_infer in csrc/cif.hip,
Paraformer.inference / inference_batch) -- liteasr/models/paraformer.py:124-129,
nets/paraformer/predictor.py:41-118 with ``ylens=None``.

* lasr_cif_infer against the host restatement (tests/paraformer_infer_ref.py): token counts,
  fire frames and output rows exact; values bit-equal wherever numpy's float32 sigmoid agrees
  with the device's to the bit, otherwise within 2e-6 of max;
* lasr_cif_infer against the scan kernel lasr_cif_fwd run with ylen = the device's ulen: every
  output bit-identical (this pins the parallel decomposition);
* the fp32 build against the reference's own run (tests/golden/paraformer_infer.npz): ulens
  and ids exact.  That is sound because the fixture's margins dominate the arithmetic error:
  test_inference_matches_reference prints max |delta sum_alpha|, |delta alpha|, |delta logit|
  per case (the generator's MAX_DSUM / MAX_DALPHA / MAX_DLOGIT bound them) and asserts each
  within a tenth of the case's margin;
* inference_batch against the training path's no-grad first pass at the same shapes (bf16 and
  fp32: the same kernels, so the ids agree exactly), single = batch of one, stable replays,
  ASRTask.inference."""

import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from paraformer_infer_ref import cif_infer_ref  # noqa: E402
from test_paraformer_infer_cpu import N_CASES, _tiny, load_case, pred_len  # noqa: E402

DEV = "cuda"
GOLD_INIT = os.path.join(ROOT, "tests", "golden", "paraformer.npz")
# (B, T', D): the smallest shapes at which each mechanism can break (one frame; two frames;
# ragged batch below one wave of frames; T' > 64: the alpha pass and the planning chunks cross
# 64 lanes; T' > 128 with the widest rows)
SHAPES = [(1, 1, 64), (1, 2, 64), (3, 15, 128), (4, 74, 256), (2, 130, 512)]
PLEN = {(1, 1, 64): [1], (1, 2, 64): [2], (3, 15, 128): [15, 0, 9], (4, 74, 256): [74, 60, 0, 33],
        (2, 130, 512): [130, 97]}


@functools.lru_cache(maxsize=None)
def _synthetic(B, T, D):
    """z, plen, h (numpy) and the float32 restatement's results, computed once per shape.
    (1, 1, 64) has ulen = 0; (3, 15, 128) and (4, 74, 256) lead utterance 0 with zero h rows up
    to its first fire frame (a fired state that is exactly zero)."""
    g = torch.Generator().manual_seed(100 * B + T)
    z = (torch.randn(B, T, generator=g) - 0.5).numpy()
    h = torch.randn(B, T, D, generator=g).numpy()
    plen = np.array(PLEN[(B, T, D)], dtype=np.int32)
    if (B, T, D) == (1, 1, 64):
        z[:] = -3.0
    if (B, T, D) == (1, 2, 64):
        z[:] = np.array([[0.5, 0.8]], dtype=np.float32)
    ref = cif_infer_ref(z, plen, h)
    if T in (15, 74):
        first = int(np.flatnonzero(ref[2][0])[0])  # the fire frames do not depend on h
        h[0, :first + 1] = 0.0
        ref = cif_infer_ref(z, plen, h)
        assert ref[3][0, first] == -1 and ref[2][0, first]
    return z, plen, h, ref


def _run_infer(z, plen, h):
    from liteasr_amd import kernels as K

    B, T, D = h.shape
    zd = torch.from_numpy(z).reshape(B * T, 1).contiguous().to(DEV)
    hd = torch.from_numpy(h).contiguous().to(DEV)
    pl = torch.from_numpy(plen).int().to(DEV)
    st = K.cif_infer(zd, pl, hd)
    torch.cuda.synchronize()
    return st, zd, pl, hd


@pytest.mark.parametrize("B,T,D", SHAPES)
def test_cif_infer_matches_restatement(B, T, D):
    z, plen, h, (s, ulen, fired, row, out, ex) = _synthetic(B, T, D)
    st, _, _, _ = _run_infer(z, plen, h)
    assert st.ulen.cpu().tolist() == ulen.tolist()
    assert st.count.cpu().tolist() == ex.count.tolist()
    assert np.array_equal(st.fired.view(B, T).cpu().numpy().astype(bool), fired), "fire frames differ"
    assert np.array_equal(st.row.view(B, T).cpu().numpy(), row), "output rows differ"
    if (B, T, D) == (1, 1, 64):
        assert ulen.tolist() == [0]
    alpha = st.alpha.view(B, T).cpu().numpy()
    got_s, got_out = st.sum_alpha.cpu().numpy(), st.out.cpu().numpy()
    assert got_out.shape == (B, T, D)
    scale = max(np.abs(out).max(), 1e-30)
    for b in range(B):
        assert np.abs(alpha[b] - ex.alpha[b]).max() <= 2e-7  # a few ulp of a value <= 1
        if np.array_equal(alpha[b].view(np.int32), ex.alpha[b].view(np.int32)):
            assert got_s[b].view(np.int32) == s[b].view(np.int32), (b, got_s[b], s[b])
            assert np.array_equal(got_out[b].view(np.int32), out[b].view(np.int32)), b
        else:
            assert abs(got_s[b] - s[b]) <= 2e-6 * max(1.0, abs(s[b]))
            assert np.abs(got_out[b] - out[b]).max() <= 2e-6 * scale
        assert not got_out[b, ex.count[b]:].any()


@pytest.mark.parametrize("B,T,D", SHAPES)
def test_cif_infer_bit_identical_to_scan_kernel(B, T, D):
    """The scan kernel with ylen = the device's ulen and U = max ulen computes the same
    function one frame after the other: every output agrees to the bit.  (The scan kernel
    needs U >= 1 and reports -1 for a row at or past U.)"""
    from liteasr_amd import kernels as K

    z, plen, h, _ = _synthetic(B, T, D)
    st, zd, pl, hd = _run_infer(z, plen, h)
    ulen = st.ulen.cpu()
    U = max(1, int(ulen.max()))
    f = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=DEV)  # noqa: E731
    sc = SimpleNamespace(alpha=f(B * T), acc=f(B * T), fired=f(B * T, dt=torch.uint8), row=f(B * T, dt=torch.int32),
                         sum_alpha=f(B), mae=f(B), out=f(B, U, D))
    K.cif_fwd(zd, pl, st.ulen, hd, B, T, U, sc)
    torch.cuda.synchronize()
    assert torch.equal(st.sum_alpha, sc.sum_alpha)
    assert torch.equal(st.alpha, sc.alpha)
    assert torch.equal(st.acc, sc.acc)
    assert torch.equal(st.fired, sc.fired)
    assert torch.equal(torch.where(st.row >= U, torch.full_like(st.row, -1), st.row), sc.row)
    assert torch.equal(st.out[:, :U].contiguous().view(torch.int32), sc.out.view(torch.int32))
    assert not st.out[:, U:].any() or int(st.count.max()) > U


@functools.lru_cache(maxsize=None)
def _model(dtype):
    z = np.load(GOLD_INIT)
    m = _tiny(dtype)
    init = {k[5:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("init.")}
    missing, unexpected = m.load_state_dict(init, strict=False)
    assert not unexpected and all(k.endswith("pe.pe") or k == "pe.pe" for k in missing), (missing, unexpected)
    with torch.no_grad():
        m.predictor.lin.bias.fill_(float(load_case(0)["lin_bias"]))
    return m.cuda().eval()


def _deltas(model, c, B):
    """max |delta sum_alpha|, |delta alpha|, |delta logit| of the last decode against case c."""
    ld = model.last_decode
    Tp = c["alpha"].shape[1]
    dsum = float(np.abs(ld.cif.sum_alpha.cpu().numpy() - c["sum_alpha"]).max())
    dalpha = float(np.abs(ld.cif.alpha.view(B, Tp).cpu().numpy() - c["alpha"]).max())
    L = int(c["ulens"].max())
    dlogit = 0.0
    if L:
        got = ld.logits.float().cpu().numpy().reshape(B, L, -1)
        dlogit = float(np.abs(got - c["logits"]).max())
    return dsum, dalpha, dlogit


@pytest.mark.parametrize("i", range(N_CASES))
def test_inference_matches_reference(i):
    """Measured on MI355X (fp32 build), maxima over the six cases: |d sum_alpha| 1.91e-6,
    |d alpha| 8.94e-8, |d logit| 3.65e-6; the generator's constants (tests/golden/
    make_golden_paraformer_infer.py: 4e-6, 2e-7, 1e-5) bound them.  The alpha error is scaled by
    T' as in the generator's rule: the fire decision compares a running sum of up to T' alphas."""
    c = load_case(i)
    model = _model("fp32")
    B = c["xs"].shape[0]
    Tp = c["alpha"].shape[1]
    xs = torch.from_numpy(c["xs"]).to(DEV)
    want = [c["ids"][b, :int(c["ulens"][b])].tolist() for b in range(B)]
    runs = [("inference_batch", lambda: model.inference_batch(xs, c["xlens"].tolist()))]
    if str(c["kind"]) == "single":
        runs.insert(0, ("inference", lambda: [model.inference(xs)]))
    for name, run in runs:
        got = run()
        dsum, dalpha, dlogit = _deltas(model, c, B)
        print(f"case {i} {name}: max |d sum_alpha| {dsum:.3g} |d alpha| {dalpha:.3g} |d logit| {dlogit:.3g} "
              f"(margins round {float(c['margin_round']):.3g} fire {float(c['margin_fire']):.3g} "
              f"logit {float(c['margin_logit']):.3g}, T' {Tp})")
        assert model.last_decode.ulens == c["ulens"].tolist()
        assert got == want
        assert dsum <= float(c["margin_round"]) / 10
        assert dalpha * Tp <= float(c["margin_fire"]) / 10
        assert dlogit <= float(c["margin_logit"]) / 10


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("i", [j for j in range(N_CASES) if str(load_case(j)["kind"]) == "batch"])
def test_inference_equals_training_first_pass(i, dtype):
    """Eval-mode forward with ylens = the decoded ulens runs the same kernels at the same
    shapes in its no-grad first pass: its argmax equals inference_batch exactly."""
    c = load_case(i)
    model = _model(dtype)
    xs = torch.from_numpy(c["xs"]).to(DEV)
    xlens = torch.from_numpy(c["xlens"]).to(DEV)
    ids = model.inference_batch(xs, xlens)
    ulens = model.last_decode.ulens
    if dtype == "fp32":
        assert ulens == c["ulens"].tolist()
    L = max(ulens)
    assert L > 0
    ylens = torch.tensor(ulens, device=DEV)
    ys = torch.ones(len(ulens), L, dtype=torch.int64, device=DEV)
    ys = ys.masked_fill(torch.arange(L, device=DEV)[None, :] >= ylens[:, None], -1)  # padded as a batch is
    model(xs, xlens, ys, ylens)
    ys_hat = model.last_glance.ys_hat
    for b, u in enumerate(ulens):
        assert ys_hat[b, :u].tolist() == ids[b], b


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_inference_single_equals_batch_of_one(dtype):
    """inference(x) == inference_batch(x, [T])[0]; replays of the captured encoder are stable,
    also with another utterance of the same shape in between (one graph per shape)."""
    model = _model(dtype)
    for i in range(N_CASES):
        c = load_case(i)
        if str(c["kind"]) != "single":
            continue
        x = torch.from_numpy(c["xs"]).to(DEV)
        T = x.shape[1]
        first = model.inference(x)
        assert isinstance(first, list) and all(isinstance(t, int) for t in first)
        other = model.inference(torch.flip(x, dims=[1]).contiguous())
        assert isinstance(other, list)
        assert model.inference(x) == first and model.inference(x) == first
        assert len(model._encode_graphs) == 1
        assert model.inference_batch(x, [T]) == [first]
        assert model.inference_batch(x, torch.tensor([T])) == [first]
    with pytest.raises(ValueError):
        model.inference(torch.zeros(1, 6, 40, device=DEV))  # T' = 0
    with pytest.raises(ValueError):
        model.inference(torch.zeros(2, 64, 40, device=DEV))  # one utterance only


def test_task_inference_paraformer(tmp_path):
    from liteasr_amd.tasks.asr import ASRConfig, ASRTask

    vocab = tmp_path / "vocab.txt"
    vocab.write_text("".join(f"t{k} {k}\n" for k in range(1, 19)))  # ids 1..18; 0 blank, 19 sos/eos
    task = ASRTask(ASRConfig(vocab=str(vocab), train="", valid="", save_dir=str(tmp_path / "ckpts")))
    assert task.vocab_size == 20
    model = _model("fp32")
    for i in range(N_CASES):
        c = load_case(i)
        if str(c["kind"]) != "single":
            continue
        ids = c["ids"][0].tolist()
        want = "".join("" if k in (0, 19) else f"t{k}" for k in ids)
        assert task.inference(torch.from_numpy(c["xs"]).to(DEV), model) == want


def test_cif_infer_rejects_other_widths():
    from liteasr_amd import kernels as K
    from liteasr_amd._native import NativeError

    for D in (96, 1024):
        with pytest.raises(NativeError, match="lasr_cif_infer"):
            K.cif_infer(torch.zeros(4, device=DEV), torch.full((1,), 4, dtype=torch.int32, device=DEV),
                        torch.zeros(1, 4, D, device=DEV))
