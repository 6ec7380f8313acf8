"""Attention rescoring kept on the device (csrc/rescore.hip, decoding.attention_rescore_device)
against the host path that U2.inference runs, and the evaluation CLI on the GPU --
liteasr/models/u2.py:218-317, liteasr/infer.py.

* the search kernel against the native host search (libliteasr_decode.so) on identical
  candidates: n and the token lists equal in order, double scores within 1e-9, the overflow
  word set exactly when a kept hypothesis is longer than Lcap (the Lcap 64 -> 128 -> 256
  re-runs included), and the tie rule on a frame without any libm call, bit for bit.
  Token equality is a fair demand: over all these cases the smallest gap between rank 10 and
  rank 11 of a frame or between adjacent final scores is 6.9e-5 (seed 1; 2.3e-3 on the golden
  arrays), far above last-bit differences of the device's fp64 exp / log;
* the decoder inputs (ys_in, decoder mask, gather index, memory mask) against what the host
  path builds through _prep_targets;
* the pick against decoding.pick_best (an exact tie: the earlier wins; n = 5);
* end to end on the golden tiny model against the reference's own run, the host path's
  gathered log-probs, state hygiene across utterances and a weight update, bf16;
* ``python -m liteasr_amd.infer`` as a child process.
"""

import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import decode_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = os.path.join(ROOT, "tests", "golden", "decode.npz")
RANDOM_CASES = [(0, 60, 30, 1.0), (1, 80, 12, 0.2), (2, 40, 50, 4.0), (3, 1, 5, 1.0), (4, 120, 8, 0.05),
                (5, 249, 4233, 0.15), (7, 7, 30, 0.2), (10, 64, 30, 0.5), (11, 65, 30, 0.5), (13, 129, 40, 0.3),
                (14, 16, 4233, 0.2)]
CASES = [("gold", u) for u in range(3)] + [("rand",) + c for c in RANDOM_CASES]


def _topk(logp, k):
    v = np.empty((logp.shape[0], k), np.float32)
    i = np.empty((logp.shape[0], k), np.int32)
    for t in range(logp.shape[0]):
        v[t], i[t] = R.topk_desc(logp[t], k)
    return v, i


_CAND = {}


def _candidates(case):
    """(vals, idx) of a case, computed once."""
    if case not in _CAND:
        if case[0] == "gold":
            logp = np.load(GOLD)[f"u{case[1]}.ctc_logp"]
        else:
            _, seed, T, V, temp = case
            rng = np.random.default_rng(seed)
            x = (rng.standard_normal((T, V)) / temp).astype(np.float32)
            logp = (x - np.log(np.exp(x.astype(np.float64)).sum(-1, keepdims=True))).astype(np.float32)
        _CAND[case] = _topk(logp, min(10, logp.shape[1]))
    return _CAND[case]


def _tcap(T):
    c = 64
    while c < T:
        c *= 2
    return c


def _search(vals, idx, Lcap, blank=0):
    """One launch of the search kernel at (Tcap(T), Lcap): (result block words, arena, Tcap)."""
    from liteasr_amd import decoding as D
    from liteasr_amd import kernels as K

    T, k = vals.shape
    Tcap = _tcap(T)
    v = torch.zeros(Tcap, k, dtype=torch.float32)
    i = torch.zeros(Tcap, k, dtype=torch.int32)
    v[:T], i[:T] = torch.from_numpy(vals), torch.from_numpy(idx)
    arena = torch.zeros(K.rescore_workspace(Tcap, Lcap), dtype=torch.uint8, device="cuda")
    tp = torch.tensor([T], dtype=torch.int32, device="cuda")
    K.rescore_search(arena, Tcap, Lcap, v.cuda(), i.cuda(), tp, blank)
    torch.cuda.synchronize()
    head = arena[: 4 * D.rescore_layout(Tcap, Lcap)["head_words"]].cpu().numpy().view(np.int32)
    return head, arena, Tcap


def _search_with_reruns(vals, idx, longest):
    """The Lcap 64 -> ... doubling of attention_rescore_device, checking the overflow word at
    every step; returns the final (head, arena, Tcap, Lcap)."""
    Lcap = 64
    while True:
        head, arena, Tcap = _search(vals, idx, Lcap)
        assert head[0] in (0, 1), head[0]
        assert bool(head[0] & 1) == (longest > Lcap), (Lcap, longest, head[0])
        if not head[0]:
            return head, arena, Tcap, Lcap
        assert Lcap < Tcap
        Lcap *= 2


# --------------------------------------------------------------------------- 1. search
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c[:2]))
def test_search_kernel_matches_native_host_search(case):
    from liteasr_amd import decoding as D

    vals, idx = _candidates(case)
    ref = D.prefix_beam_search(vals, idx, beam=10)
    longest = max(len(t) for t, _ in ref)
    head, _, Tcap, Lcap = _search_with_reruns(vals, idx, longest)
    got = D.rescore_nbest(head, Lcap)
    dmax = max(abs(a[1] - b[1]) for a, b in zip(got, ref)) if len(got) == len(ref) else float("nan")
    print(f"{case}: n {len(got)} longest {longest} Tcap {Tcap} Lcap {Lcap} max |dscore| {dmax:.3e}")
    assert head[1] == len(ref) and head[4] == vals.shape[0]
    assert [t for t, _ in got] == [t for t, _ in ref]
    assert dmax <= 1e-9
    if case == ("rand", 3, 1, 5, 1.0):
        assert len(ref) == 5 and vals.shape[1] == 5
    if case[:2] in (("rand", 1), ("rand", 4)):
        assert longest > 64 and Lcap == 128


def test_search_cases_sit_on_both_sides_of_the_tcap_boundaries():
    assert [_tcap(T) for T in (64, 65, 129, 1, 249)] == [64, 128, 256, 64, 256]


def test_search_tie_rule_without_libm():
    """One frame, V = 12, all log-probs equal: ranks come from the host loop's first-touch order
    alone, and every score is the candidate's float32 log-prob as a double, bit for bit."""
    from liteasr_amd import decoding as D

    logp = np.full((1, 12), np.float32(np.log(1.0 / 12)), np.float32)
    vals, idx = _topk(logp, 10)
    head, _, _ = _search(vals, idx, 64)
    got = D.rescore_nbest(head, 64)
    want = float(np.float32(np.log(1.0 / 12)))
    assert got == [([], want)] + [([t], want) for t in range(1, 10)]
    assert got == D.prefix_beam_search(vals, idx, beam=10)


def test_search_rejects_other_beams():
    from liteasr_amd import kernels as K
    from liteasr_amd._native import NativeError

    arena = torch.zeros(K.rescore_workspace(64, 64), dtype=torch.uint8, device="cuda")
    v = torch.zeros(64, 10, device="cuda")
    i = torch.zeros(64, 10, dtype=torch.int32, device="cuda")
    tp = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(NativeError, match="beam of 10"):
        K.rescore_search(arena, 64, 64, v, i, tp, 0, beam=4)
    # the wrappers hand raw pointers to the kernels: a host tensor is refused
    for bad in ((v.cpu(), i, tp), (v, i.cpu(), tp), (v, i, tp.cpu())):
        with pytest.raises(ValueError, match="same HIP device"):
            K.rescore_search(arena, 64, 64, *bad, 0)
    with pytest.raises(ValueError, match="same HIP device"):
        K.rescore_pick(arena, 64, 64, torch.zeros(650), 0.5)


# --------------------------------------------------------------------------- golden model
def _golden_model(dtype="fp32"):
    from liteasr_amd.models.u2 import U2, U2Config
    from liteasr_amd.utils.cfg import resolve_self

    d = np.load(GOLD)
    c = U2Config(input_dim=40, vocab_size=30, enc_dim=64, enc_ff_dim=256, enc_attn_heads=4, enc_layers=2,
                 dec_dim=64, dec_ff_dim=256, dec_attn_heads=4, dec_layers=1, compute_dtype=dtype)
    resolve_self(c)
    m = U2(c)
    sd = {k[5:]: torch.from_numpy(np.array(v)) for k, v in d.items() if k.startswith("init.")}
    m.load_state_dict(sd, strict=False)
    return m.cuda().eval(), d


@pytest.fixture(scope="module")
def golden():
    return _golden_model()


def _nbest_ref(d, u):
    lens, toks, sc = d[f"u{u}.nbest_len"], d[f"u{u}.nbest_tok"], d[f"u{u}.nbest_score"]
    out, o = [], 0
    for n, s in zip(lens, sc):
        out.append((toks[o:o + n].tolist(), float(s)))
        o += n
    return out


def _x(d, u):
    return torch.from_numpy(d[f"u{u}.x"]).unsqueeze(0).cuda()


def _host_path(model, x, monkeypatch):
    """(answer, n-best, gathered [n, Lmax + 1]) of the retained host path."""
    from liteasr_amd import decoding as D

    seen = {}
    inner = D.pick_best

    def recording(hyps, g, ctc_weight=0.5):
        seen["hyps"], seen["g"] = hyps, np.array(g)
        return inner(hyps, g, ctc_weight)

    monkeypatch.setattr(D, "pick_best", recording)
    with torch.no_grad():
        out = D.attention_rescore_host(model, x)
    monkeypatch.setattr(D, "pick_best", inner)
    return out, seen["hyps"], seen["g"]


# --------------------------------------------------------------------------- 2. prep
@pytest.mark.parametrize("case", [("gold", 0), ("rand", 3, 1, 5, 1.0), ("rand", 0, 60, 30, 1.0)],
                         ids=["gold0", "n5", "seed0"])
def test_prep_matches_host_inputs(golden, case):
    from liteasr_amd import decoding as D
    from liteasr_amd import kernels as K

    model, _ = golden
    vals, idx = _candidates(case)
    T = vals.shape[0]
    Lcap, L1 = 64, 65
    head, arena, Tcap = _search(vals, idx, Lcap)
    hyps = D.rescore_nbest(head, Lcap)
    n = len(hyps)
    assert hyps == [(t, pytest.approx(s, abs=1e-9)) for t, s in D.prefix_beam_search(vals, idx, beam=10)]
    ys_in = torch.full((10, L1), -7, dtype=torch.int32, device="cuda")
    dec_full = torch.full((10, L1, 80), 9, dtype=torch.uint8, device="cuda")  # 16-B aligned rows, as _prep's
    dec_mask = dec_full[:, :, :L1]
    gidx = torch.full((10 * L1,), -7, dtype=torch.int32, device="cuda")
    mem_mask = torch.full((10, Tcap), 9, dtype=torch.uint8, device="cuda")
    K.rescore_prep(arena, Tcap, Lcap, model.sos, model.eos, ys_in, dec_mask, gidx, mem_mask)
    torch.cuda.synchronize()
    # the host path's inputs (decoding.rescore)
    Lmax = max(1, max(len(t) for t, _ in hyps))
    ys = torch.full((n, Lmax), -1, dtype=torch.int64)
    for i, (t, _) in enumerate(hyps):
        ys[i, :len(t)] = torch.tensor(t, dtype=torch.int64)
    ylens = torch.tensor([len(t) for t, _ in hyps], dtype=torch.int64)
    prep = model._prep_targets(ys.cuda(), ylens.cuda(), n, 4 * T + 3)
    want_g = torch.full((n, Lmax + 1), -1, dtype=torch.int32)
    for i, (t, _) in enumerate(hyps):
        want_g[i, :len(t)] = torch.tensor(t, dtype=torch.int32)
        want_g[i, len(t)] = model.eos
    torch.cuda.synchronize()
    assert torch.equal(ys_in[:n, :Lmax + 1].cpu(), prep.ys_in.cpu())
    assert torch.equal(dec_mask[:n, :Lmax + 1, :Lmax + 1].cpu(), prep.dec_mask.cpu())
    g2 = gidx.view(10, L1).cpu()
    assert torch.equal(g2[:n, :Lmax + 1], want_g)
    # beyond the leading block: eos padding, masked keys, no gathers; rows >= n are empty
    assert (ys_in[:, 0] == model.sos).all() and (ys_in[:n, Lmax + 1:] == model.eos).all()
    assert (g2[:n, Lmax + 1:] == -1).all() and (g2[n:] == -1).all()
    assert (ys_in[n:, 1:] == model.eos).all()
    dm = dec_mask.cpu()
    for i in range(10):
        ln = len(hyps[i][0]) if i < n else 0
        q, c = torch.meshgrid(torch.arange(L1), torch.arange(L1), indexing="ij")
        assert torch.equal(dm[i], ((c >= ln + 1) | (c > q)).to(torch.uint8)), i
    assert (dec_full[:, :, L1:] == 1).all()  # the padding columns of the aligned rows are masked
    want_m = (torch.arange(Tcap) >= T).to(torch.uint8).expand(10, Tcap)
    assert torch.equal(mem_mask.cpu(), want_m)


# --------------------------------------------------------------------------- 3. pick
def _pick_case(seed, n):
    rng = np.random.default_rng(seed)
    V, eos = 12, 11
    hyps = [(rng.integers(1, V - 1, rng.integers(0, 7)).tolist(), float(rng.normal() * 3)) for _ in range(n)]
    L1 = max(len(t) for t, _ in hyps) + 1
    attn = np.log(rng.dirichlet(np.ones(V), size=(n, L1))).astype(np.float32)
    if seed == 2:  # two identical hypotheses that lead: the earlier one wins
        hyps[1] = (hyps[1][0], 40.0)
        hyps[3] = hyps[1]
        attn[3] = attn[1]
    g = np.full((n, L1), -np.inf, np.float32)
    for i, (t, _) in enumerate(hyps):
        for j, w in enumerate(t + [eos]):
            g[i, j] = attn[i, j, w]
    return hyps, g


@pytest.mark.parametrize("seed,n", [(0, 10), (1, 10), (2, 10), (3, 5)])
def test_pick_matches_pick_best(seed, n):
    from liteasr_amd import decoding as D
    from liteasr_amd import kernels as K

    hyps, g = _pick_case(seed, n)
    want = D.pick_best(hyps, g)
    if seed == 2:
        assert want == 1
    Tcap, Lcap, L1 = 64, 64, 65
    off = D.rescore_layout(Tcap, Lcap)
    head = np.zeros(off["head_words"], np.int32)
    head[1] = n
    head[8:8 + n] = [len(t) for t, _ in hyps]
    sc = np.full(10, -np.inf)
    sc[:n] = [s for _, s in hyps]
    head[20:40] = sc.view(np.int32)
    toks = head[off["toks"]:off["toks"] + 10 * Lcap].reshape(10, Lcap)
    for i, (t, _) in enumerate(hyps):
        toks[i, :len(t)] = t
    arena = torch.zeros(K.rescore_workspace(Tcap, Lcap), dtype=torch.uint8, device="cuda")
    arena[: head.nbytes] = torch.from_numpy(head.view(np.uint8)).cuda()
    gd = torch.full((10, L1), -float("inf"))
    gd[:n, :g.shape[1]] = torch.from_numpy(g)
    K.rescore_pick(arena, Tcap, Lcap, gd.cuda().view(-1), 0.5)
    torch.cuda.synchronize()
    out = arena[: head.nbytes].cpu().numpy().view(np.int32)
    assert out[2] == want
    assert out[3] == len(hyps[want][0])
    assert out[off["best"]:off["best"] + out[3]].tolist() == hyps[want][0]
    # the totals are pick_best's float32 sums, bit for bit
    f32 = np.float32
    for i, (t, s0) in enumerate(hyps):
        s = f32(0.0)
        for j in range(len(t) + 1):
            s = f32(s + g[i, j])
        s = f32(s + f32(s0 * 0.5))
        assert out[40 + i].view(np.float32) == s, i


# --------------------------------------------------------------------------- 4. end to end
def test_device_path_against_reference(golden, monkeypatch):
    from liteasr_amd import decoding as D

    model, d = golden
    for u in range(int(d["n_utt"])):
        x = _x(d, u)
        trace = {}
        with torch.no_grad():
            out = D.attention_rescore_device(model, x, trace=trace)
        assert list(out) == d[f"u{u}.rescore_best"].tolist(), u
        ref = _nbest_ref(d, u)
        assert [t for t, _ in trace["nbest"]] == [t for t, _ in ref], u
        assert np.allclose([s for _, s in trace["nbest"]], [s for _, s in ref], atol=1e-4, rtol=0)
        host_out, host_hyps, host_g = _host_path(model, x, monkeypatch)
        assert list(host_out) == list(out)
        assert [t for t, _ in host_hyps] == [t for t, _ in trace["nbest"]]
        assert trace["gathered"].shape == host_g.shape
        fin = np.isfinite(host_g)
        assert np.array_equal(fin, np.isfinite(trace["gathered"]))
        dg = np.abs(trace["gathered"][fin] - host_g[fin]).max()
        print(f"utt {u}: max |d gathered| device vs host {dg:.3e}")
        assert dg <= 1e-4
        assert list(model.inference(x)) == list(out)
        assert list(model.inference(x, encoder_graph=False)) == list(out)


# --------------------------------------------------------------------------- 5. hygiene
def test_state_hygiene_and_weight_update(monkeypatch):
    from liteasr_amd import decoding as D

    model, d = _golden_model()
    first = {}
    with torch.no_grad():
        for u in (0, 1, 2, 0, 2):
            trace = {}
            out = D.attention_rescore_device(model, _x(d, u), trace=trace)
            assert trace["caps"] == (64, 64)  # T' 29, 23, 15 share one bucket
            if u not in first:
                first[u] = (out, trace)
                continue
            out0, t0 = first[u]
            assert out == out0 and trace["best"] == t0["best"], u
            assert trace["nbest"] == t0["nbest"], u  # double scores compared with ==
            assert np.array_equal(trace["gathered"], t0["gathered"]), u
            assert np.array_equal(trace["totals"], t0["totals"]), u
        states = model._rescore_states
        s0 = states[(64, 64)]
        st = model.store
        ver = st.flat._version
        name = next(n for n in st.offsets if n.endswith("after_norm.weight"))
        st.view(name).add_(0.01)  # in place on a view of the flat buffer: bumps its version
        assert st.flat._version != ver
        x = _x(d, 1)
        out = D.attention_rescore_device(model, x)
        assert model._rescore_states[(64, 64)] is not s0
    host_out, _, _ = _host_path(model, x, monkeypatch)
    assert list(out) == list(host_out)


# --------------------------------------------------------------------------- 6. bf16
def test_bf16_device_path_against_host_path(monkeypatch):
    from liteasr_amd import decoding as D

    model, d = _golden_model("bf16")
    for u in range(int(d["n_utt"])):
        x = _x(d, u)
        trace = {}
        with torch.no_grad():
            D.attention_rescore_device(model, x, trace=trace)
        _, host_hyps, host_g = _host_path(model, x, monkeypatch)
        assert [t for t, _ in trace["nbest"]] == [t for t, _ in host_hyps], u
        fin = np.isfinite(host_g)
        assert np.array_equal(fin, np.isfinite(trace["gathered"]))
        dg = np.abs(trace["gathered"][fin] - host_g[fin]).max()
        big = np.abs(host_g[fin]).max()
        print(f"utt {u} bf16: max |d gathered| {dg:.3e}, largest magnitude {big:.3f}")
        assert dg <= 1e-2 * big


# --------------------------------------------------------------------------- 7. CLI
N_UTT = 5


def _cli_tree(tmp_path):
    """The loader fixture cut to its first utterances, the user config tree over it."""
    from cfgtree import user_tree

    conf, data = user_tree(tmp_path, compute_dtype="fp32")
    for fn in ("feats.scp", "text", "utt2num_frames"):
        lines = (data / fn).read_text().splitlines()[:N_UTT]
        (data / fn).write_text("\n".join(lines) + "\n")
    return conf, data


def _blocks(log):
    """(utterance blocks, error-rate lines) the infer logger wrote, in order."""
    utt = re.findall(r"\[INFO\]\[liteasr_amd\.infer\] - \n(\[[X ]\] .*\n\s*\d+ .*)\n", log)
    rate = re.findall(r"\[INFO\]\[liteasr_amd\.infer\] - (Error rate: .*)\n", log)
    return utt, rate


def test_cli_end_to_end(tmp_path, monkeypatch):
    from liteasr_amd import infer as I
    from liteasr_amd import tasks
    from liteasr_amd.config.compose import compose
    from liteasr_amd.utils.score import levenshtein

    conf, data = _cli_tree(tmp_path)
    run_dir = tmp_path / "runs" / "asr_U2"
    (run_dir / "ckpts").mkdir(parents=True)
    monkeypatch.chdir(run_dir)
    ovr = [f"task.test=[{data}]", "inference.ckpt_name=1"]
    cfg = compose(str(conf), "config", ovr, job_name="infer")
    task = tasks.setup_task(cfg.task)
    task.load_dataset("test", task.cfg.test, None, cfg.postprocess)
    torch.manual_seed(3)
    model = task.build_model(cfg.model)
    torch.save(model.state_dict(), run_dir / "ckpts" / "model.ep.1.pt")
    model = model.cuda().eval()
    ds = task.dataset("test")[0]
    assert len(ds) == N_UTT
    with torch.no_grad():
        hyps = [task.inference(ds[i].x.unsqueeze(0).cuda(), model) for i in range(len(ds))]
    refs = [ds[i].text for i in range(len(ds))]
    want_utt = [I.utt_line(r, h)[0][1:] for r, h in zip(refs, hyps)]
    errs = sum(levenshtein(r, h) for r, h in zip(refs, hyps))
    want_rate = "Error rate: {} / {} = {:.2%}".format(errs, sum(len(r) for r in refs),
                                                      errs / sum(len(r) for r in refs))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    logs = []
    for extra in ([], ["inference.model_avg=true", "inference.avg_num=1", "inference.avg_policy=null"]):
        log = run_dir / "infer.log"
        if log.exists():
            log.unlink()
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "liteasr_amd.infer", "-cd", str(conf)]
                           + ovr + extra, cwd=tmp_path, env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        utt, rate = _blocks(log.read_text())
        assert utt == want_utt, (utt, want_utt)
        assert rate == [want_rate]
        assert log.read_text().rstrip("\n").endswith(want_rate)
        logs.append((utt, rate))
    assert logs[0] == logs[1]
    shutil.rmtree(run_dir, ignore_errors=True)
