"""Batched attention rescoring on the device (the *_batch entries of csrc/rescore.hip,
decoding.attention_rescore_batch, U2.inference_batch, ``inference.batch_size``) --
liteasr/models/u2.py:218-317 per row, the modules composed as U2.forward composes them.

* the batched kernels against the single-utterance kernels (tests/test_rescore_device_gpu.py pins
  those to the host search and to the reference's own run): result heads byte for byte, the
  double scores included; overflow per row; prep / pick per row, the memory mask from mem_len;
* an equal-length batch against the reference's own run (tests/golden/decode.npz) and
  ``U2.inference``; a row does not see the content of the other rows (``==``);
* a ragged batch in stages, so that no stage demands token equality across precisions: encoder
  and CTC log-probs against the fp64 oracle, the device search against the native host search on
  the device's own candidates, the gathered attention log-probs against the fp64 oracle decoder
  under the encoder's key mask, the pick against decoding.pick_best;
* short batches, state hygiene, bf16, errors, the CLI as a child process.

One launch takes one k for all its rows, so the T = 1, V 5 case (k = 5, n = 5) cannot share a
launch at k = 10 with the V >= 30 cases: the B = 5 launch runs at k = 5 on the leading 5 of
every row's candidates (descending, so they are that row's top 5), and a second launch runs the
V >= 30 rows and the T' = 0 row at k = 10.  Both are compared with single launches at their k.
"""

import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_rescore_device_gpu import (N_UTT, _blocks, _candidates, _cli_tree, _golden_model, _host_path,  # noqa: E402
                                     _nbest_ref, _pick_case)

pytestmark = pytest.mark.gpu

C_T1, C_64, C_65, C_129 = ("rand", 3, 1, 5, 1.0), ("rand", 10, 64, 30, 0.5), ("rand", 11, 65, 30, 0.5), \
    ("rand", 13, 129, 40, 0.3)
C_LONG, C_T7, C_BIG = ("rand", 1, 80, 12, 0.2), ("rand", 7, 7, 30, 0.2), ("rand", 5, 249, 4233, 0.15)
EMPTY = None  # a row with T' = 0


def _rows(cases, k):
    """[(vals [T, k], idx [T, k])] of the cases, the leading k candidates; EMPTY: no frame."""
    out = []
    for c in cases:
        if c is EMPTY:
            out.append((np.zeros((0, k), np.float32), np.zeros((0, k), np.int32)))
        else:
            v, i = _candidates(c)
            out.append((np.ascontiguousarray(v[:, :k]), np.ascontiguousarray(i[:, :k])))
    return out


def _head_bytes(Tcap, Lcap):
    from liteasr_amd import decoding as D

    return 4 * D.rescore_layout(Tcap, Lcap)["head_words"]


def _search_batch(rows, Tcap, Lcap, blank=0):
    """One batched launch: (heads int32 [B, head_words], the batch arena)."""
    from liteasr_amd import kernels as K

    B, k = len(rows), rows[0][0].shape[1]
    v = torch.zeros(B * Tcap, k, dtype=torch.float32)
    i = torch.zeros(B * Tcap, k, dtype=torch.int32)
    for b, (rv, ri) in enumerate(rows):
        T = rv.shape[0]
        v[b * Tcap:b * Tcap + T], i[b * Tcap:b * Tcap + T] = torch.from_numpy(rv), torch.from_numpy(ri)
    tp = torch.tensor([r[0].shape[0] for r in rows], dtype=torch.int32, device="cuda")
    arena = torch.zeros(K.rescore_workspace_batch(B, Tcap, Lcap), dtype=torch.uint8, device="cuda")
    K.rescore_search_batch(arena, B, Tcap, Lcap, v.cuda(), i.cuda(), tp, blank)
    torch.cuda.synchronize()
    stride = K.rescore_workspace(Tcap, Lcap)
    heads = arena.view(B, stride)[:, :_head_bytes(Tcap, Lcap)].cpu().numpy().view(np.int32)
    return heads, arena


def _search_single(row, Tcap, Lcap, blank=0):
    """One single-utterance launch on the same candidates at the same (Tcap, Lcap)."""
    from liteasr_amd import kernels as K

    rv, ri = row
    T, k = rv.shape
    v = torch.zeros(Tcap, k, dtype=torch.float32)
    i = torch.zeros(Tcap, k, dtype=torch.int32)
    v[:T], i[:T] = torch.from_numpy(rv), torch.from_numpy(ri)
    arena = torch.zeros(K.rescore_workspace(Tcap, Lcap), dtype=torch.uint8, device="cuda")
    tp = torch.tensor([T], dtype=torch.int32, device="cuda")
    K.rescore_search(arena, Tcap, Lcap, v.cuda(), i.cuda(), tp, blank)
    torch.cuda.synchronize()
    return arena[:_head_bytes(Tcap, Lcap)].cpu().numpy().view(np.int32)


def _assert_rows_equal_singles(rows, Tcap, Lcap):
    heads, arena = _search_batch(rows, Tcap, Lcap)
    for b, row in enumerate(rows):
        want = _search_single(row, Tcap, Lcap)
        assert heads[b].tobytes() == want.tobytes(), b
    return heads, arena


# --------------------------------------------------------------------------- 1. search
def test_search_batch_of_five_equals_single_launches():
    from liteasr_amd import decoding as D

    rows = _rows([C_T1, C_64, EMPTY, C_65, C_129], 5)
    heads, _ = _assert_rows_equal_singles(rows, 256, 64)
    assert [int(h[0]) for h in heads] == [0, 0, 0, 0, 1]  # the 129 frames' longest hypothesis, 122, overflows Lcap 64
    heads, _ = _assert_rows_equal_singles(rows, 256, 256)
    assert not any(h[0] for h in heads)
    assert heads[0][1] == 5 and heads[0][4] == 1  # V 5, one frame: n = 5
    assert [int(h[4]) for h in heads] == [1, 64, 0, 65, 129]
    # the T' = 0 row: n = 1, the empty prefix with score log 1, no error
    assert heads[2][0] == 0 and heads[2][1] == 1 and D.rescore_nbest(heads[2], 256) == [([], 0.0)]
    assert heads[2][3] == 0
    # against the host search too, on the same candidates
    for b in (0, 1, 3, 4):
        ref = D.prefix_beam_search(*rows[b], beam=10)
        got = D.rescore_nbest(heads[b], 256)
        assert [t for t, _ in got] == [t for t, _ in ref], b
        assert max(abs(a[1] - r[1]) for a, r in zip(got, ref)) <= 1e-9


def test_search_batch_at_k10_equals_single_launches():
    rows = _rows([C_64, EMPTY, C_65, C_129], 10)
    _assert_rows_equal_singles(rows, 256, 64)
    heads, _ = _assert_rows_equal_singles(rows, 256, 256)
    assert not any(h[0] for h in heads)
    assert [int(h[1]) for h in heads] == [10, 1, 10, 10]


def test_search_batch_at_the_real_size():
    """Tcap 256, T' 249, V 4233 in row 1: the table capacity (65536 slots a row) and the row
    offsets at the size evaluation runs."""
    from liteasr_amd import decoding as D

    rows = _rows([C_129, C_BIG], 10)
    heads, _ = _assert_rows_equal_singles(rows, 256, 256)
    assert heads[1][0] == 0 and heads[1][4] == 249
    ref = D.prefix_beam_search(*rows[1], beam=10)
    assert [t for t, _ in D.rescore_nbest(heads[1], 256)] == [t for t, _ in ref]


# --------------------------------------------------------------------------- 2. overflow
def test_overflow_is_per_row():
    from liteasr_amd import decoding as D

    rows = _rows([C_T7, C_LONG, C_64, EMPTY], 10)
    assert max(len(t) for t, _ in D.prefix_beam_search(*rows[1], beam=10)) > 64
    heads, _ = _assert_rows_equal_singles(rows, 128, 64)
    assert [int(h[0]) for h in heads] == [0, 1, 0, 0]
    heads, _ = _assert_rows_equal_singles(rows, 128, 128)
    assert [int(h[0]) for h in heads] == [0, 0, 0, 0]
    for b in (0, 1, 2):
        ref = D.prefix_beam_search(*rows[b], beam=10)
        assert [t for t, _ in D.rescore_nbest(heads[b], 128)] == [t for t, _ in ref], b


# --------------------------------------------------------------------------- 3. prep and pick
def _prep_outputs(R, L1, Tcap):
    ys_in = torch.full((R, L1), -7, dtype=torch.int32, device="cuda")
    dec_full = torch.full((R, L1, (L1 + 15) // 16 * 16), 9, dtype=torch.uint8, device="cuda")
    gidx = torch.full((R * L1,), -7, dtype=torch.int32, device="cuda")
    mem_mask = torch.full((R, Tcap), 9, dtype=torch.uint8, device="cuda")
    return ys_in, dec_full, gidx, mem_mask


def test_prep_batch_equals_single_kernels_and_follows_mem_len():
    from liteasr_amd import kernels as K

    Tcap, Lcap, L1, sos = 64, 64, 65, 29
    rows = _rows([("gold", 0), C_T7, ("rand", 0, 60, 30, 1.0)], 10)
    B = len(rows)
    tps = [r[0].shape[0] for r in rows]
    _, arena = _search_batch(rows, Tcap, Lcap)
    stride = K.rescore_workspace(Tcap, Lcap)
    singles = []
    for b in range(B):
        one = arena[b * stride:(b + 1) * stride].clone()  # a row of the batch arena is a single arena
        out = _prep_outputs(10, L1, Tcap)
        K.rescore_prep(one, Tcap, Lcap, sos, sos, out[0], out[1][:, :, :L1], out[2], out[3])
        singles.append(out)
    torch.cuda.synchronize()
    for delta in ([0, 0, 0], [2, -3, 1]):
        mem_len = torch.tensor([t + e for t, e in zip(tps, delta)], dtype=torch.int32, device="cuda")
        ys_in, dec_full, gidx, mem_mask = _prep_outputs(10 * B, L1, Tcap)
        K.rescore_prep_batch(arena, B, Tcap, Lcap, sos, sos, ys_in, dec_full[:, :, :L1], gidx, mem_mask, mem_len)
        torch.cuda.synchronize()
        for b in range(B):
            s_ys, s_dec, s_g, s_mm = singles[b]
            r = slice(10 * b, 10 * b + 10)
            assert torch.equal(ys_in[r], s_ys), b
            assert torch.equal(dec_full[r], s_dec), b
            assert torch.equal(gidx.view(10 * B, L1)[r], s_g.view(10, L1)), b
            want = (torch.arange(Tcap) >= tps[b] + delta[b]).to(torch.uint8).expand(10, Tcap)
            assert torch.equal(mem_mask[r].cpu(), want), (b, delta)
            if delta[b] == 0:
                assert torch.equal(mem_mask[r], s_mm), b


def test_pick_batch_equals_single_kernel_tie_in_row_1():
    from liteasr_amd import decoding as D
    from liteasr_amd import kernels as K

    Tcap, Lcap, L1 = 64, 64, 65
    cases = [(0, 10), (2, 10), (3, 5)]  # seed 2: two identical leading hypotheses, the earlier wins
    B = len(cases)
    off = D.rescore_layout(Tcap, Lcap)
    stride = K.rescore_workspace(Tcap, Lcap)
    arena = torch.zeros(K.rescore_workspace_batch(B, Tcap, Lcap), dtype=torch.uint8, device="cuda")
    gd = torch.full((B, 10, L1), -float("inf"))
    wants = []
    for b, (seed, n) in enumerate(cases):
        hyps, g = _pick_case(seed, n)
        wants.append((hyps, D.pick_best(hyps, g)))
        head = np.zeros(off["head_words"], np.int32)
        head[1] = n
        head[8:8 + n] = [len(t) for t, _ in hyps]
        sc = np.full(10, -np.inf)
        sc[:n] = [s for _, s in hyps]
        head[20:40] = sc.view(np.int32)
        toks = head[off["toks"]:off["toks"] + 10 * Lcap].reshape(10, Lcap)
        for i, (t, _) in enumerate(hyps):
            toks[i, :len(t)] = t
        arena[b * stride:b * stride + head.nbytes] = torch.from_numpy(head.view(np.uint8)).cuda()
        gd[b, :n, :g.shape[1]] = torch.from_numpy(g)
    assert wants[1][1] == 1
    gd = gd.cuda()
    singles = []
    for b in range(B):
        one = arena[b * stride:(b + 1) * stride].clone()
        K.rescore_pick(one, Tcap, Lcap, gd[b].reshape(-1), 0.5)
        singles.append(one[:4 * off["head_words"]].cpu().numpy())
    K.rescore_pick_batch(arena, B, Tcap, Lcap, gd.view(-1), 0.5)
    torch.cuda.synchronize()
    heads = arena.view(B, stride)[:, :4 * off["head_words"]].cpu().numpy()
    for b, (hyps, want) in enumerate(wants):
        assert heads[b].tobytes() == singles[b].tobytes(), b
        out = heads[b].view(np.int32)
        assert out[2] == want and out[3] == len(hyps[want][0])
        assert out[off["best"]:off["best"] + out[3]].tolist() == hyps[want][0]


# --------------------------------------------------------------------------- golden model
@pytest.fixture(scope="module")
def golden():
    return _golden_model()


def _xu(d, u):
    return torch.from_numpy(d[f"u{u}.x"])


def _check_row_against_reference(d, u, out, trace, b):
    assert list(out[b]) == d[f"u{u}.rescore_best"].tolist(), u
    ref = _nbest_ref(d, u)
    assert [t for t, _ in trace["nbest"][b]] == [t for t, _ in ref], u
    dmax = max(abs(a[1] - r[1]) for a, r in zip(trace["nbest"][b], ref))
    print(f"utt {u} in row {b}: max |d n-best score| vs the reference {dmax:.3e}")
    assert dmax <= 1e-4


# --------------------------------------------------------------------------- 4. equal lengths
def test_equal_length_batch_against_reference(golden):
    from liteasr_amd import decoding as D

    model, d = golden
    for u in range(int(d["n_utt"])):
        x = _xu(d, u)
        T = x.shape[0]
        g = torch.Generator().manual_seed(40 + u)
        a, c = torch.randn(T, 40, generator=g), torch.randn(T, 40, generator=g)
        trace, swapped = {}, {}
        with torch.no_grad():
            out = D.attention_rescore_batch(model, torch.stack([a, x, c]).cuda(), [T] * 3, trace=trace)
            out2 = D.attention_rescore_batch(model, torch.stack([c, x, a]).cuda(), [T] * 3, trace=swapped)
            single = model.inference(x.unsqueeze(0).cuda())
        _check_row_against_reference(d, u, out, trace, 1)
        assert list(out[1]) == list(single)
        assert list(model.inference_batch(torch.stack([a, x, c]).cuda(), [T] * 3)[1]) == list(single)
        # row 1 does not see what the other rows hold
        assert out2[1] == out[1] and out2[0] == out[2] and out2[2] == out[0]
        assert swapped["nbest"][1] == trace["nbest"][1]  # double scores compared with ==
        assert np.array_equal(swapped["gathered"][1], trace["gathered"][1])
        assert np.array_equal(swapped["totals"][1], trace["totals"][1]) and swapped["best"][1] == trace["best"][1]


# --------------------------------------------------------------------------- 5. ragged batch
XLENS = (120, 97, 64)


def _ragged(d):
    xs = torch.zeros(3, 120, 40)
    for u, n in enumerate(XLENS):
        xs[u, :n] = _xu(d, u)
    return xs


def _oracle(d, dtype):
    """(cfg, params) of the fp64 / fp32 oracle with the golden model's weights."""
    from oracle import u2_oracle as O

    cfg = O.default_cfg(enc_dim=64, enc_heads=4, enc_ff=256, enc_layers=2, dec_dim=64, dec_heads=4, dec_ff=256,
                        dec_layers=1, vocab_size=30, input_dim=40)
    p = {k[5:]: torch.from_numpy(np.array(v)) for k, v in d.items() if k.startswith("init.")}
    p = {k: v.to(dtype) if v.is_floating_point() else v for k, v in p.items()}
    return cfg, p


def _oracle_encoder(d, dtype):
    """(h [3, T', d], key mask [3, T'] True = padding, CTC log-probs [3, T', V]) of the ragged batch."""
    from oracle import u2_oracle as O

    cfg, p = _oracle(d, dtype)
    with torch.no_grad():
        h, kmask = O.encoder(_ragged(d).to(dtype), torch.tensor(XLENS), p, cfg, p, False)
        logp = O.linear(h, p, "ctc.ctc_lo").log_softmax(-1)
    return h, kmask, logp


def _oracle_gathered(d, dtype, hyps, memory, mem_mask):
    """Attention log-probs of the hypotheses' tokens + eos, [n, Lmax + 1] (nan past the eos), from
    the oracle decoder over ``memory`` [T', d] under ``mem_mask`` [T'] (True = padding)."""
    from oracle import u2_oracle as O

    cfg, p = _oracle(d, dtype)
    n, eos = len(hyps), 29
    Lmax = max(1, max(len(t) for t, _ in hyps))
    ys = torch.full((n, Lmax), -1, dtype=torch.int64)
    for i, (t, _) in enumerate(hyps):
        ys[i, :len(t)] = torch.tensor(t, dtype=torch.int64)
    ylens = torch.tensor([len(t) for t, _ in hyps])
    ys_in, dec_mask, _ = O.decoder_io(ys, ylens, eos, eos)
    with torch.no_grad():
        logits = O.decoder(ys_in, dec_mask, memory.to(dtype)[None].expand(n, -1, -1), mem_mask[None].expand(n, -1), p,
                           cfg, False)
    lp = logits.log_softmax(-1)
    g = np.full((n, Lmax + 1), np.nan)
    for i, (t, _) in enumerate(hyps):
        for j, w in enumerate(t + [eos]):
            g[i, j] = float(lp[i, j, w])
    return g


def oracle_precision_maxima(d):
    """max |fp32 - fp64| of the oracle on the ragged batch: (encoder output, CTC log-probs on the
    searched frames, gathered attention log-probs of the reference's n-bests)."""
    h64, km, lp64 = _oracle_encoder(d, torch.float64)
    h32, _, lp32 = _oracle_encoder(d, torch.float32)
    dh = dl = dg = 0.0
    for b, n in enumerate(XLENS):
        pl = ((n - 1) // 2 - 1) // 2
        dh = max(dh, float((h32[b, :pl].double() - h64[b, :pl]).abs().max()))
        dl = max(dl, float((lp32[b, :pl].double() - lp64[b, :pl]).abs().max()))
        hyps = _nbest_ref(d, b)
        g64 = _oracle_gathered(d, torch.float64, hyps, h64[b], km[b])
        g32 = _oracle_gathered(d, torch.float32, hyps, h64[b], km[b])
        dg = max(dg, float(np.nanmax(np.abs(g32 - g64))))
    return dh, dl, dg


def test_ragged_batch_in_stages(golden):
    """Rows padded to 120 frames, xlens (120, 97, 64).  Row 0 is unpadded: the reference's answer.
    Rows 1 and 2 are the computation training sees, checked stage by stage; the 1e-4 bars of (a)
    and (c) are 10x the fp32-vs-fp64 spread of the oracle itself on these inputs (asserted
    <= 1e-5 below; observed on the CPU: encoder 1.3e-6, CTC log-probs 5.3e-6, gathered 2.8e-6),
    the margin the existing encoder bar gives."""
    from liteasr_amd import decoding as D

    model, d = golden
    dh, dl, dg = oracle_precision_maxima(d)
    print(f"oracle fp32 vs fp64: encoder {dh:.3e}, CTC log-probs {dl:.3e}, gathered {dg:.3e}")
    assert max(dh, dl, dg) <= 1e-5
    trace = {}
    with torch.no_grad():
        out = D.attention_rescore_batch(model, _ragged(d).cuda(), list(XLENS), trace=trace)
    _check_row_against_reference(d, 0, out, trace, 0)
    s = trace["state"]
    Bcap, Tcap, Lcap = trace["caps"]
    assert (Bcap, Tcap) == (3, 64)
    h64, km, lp64 = _oracle_encoder(d, torch.float64)
    vals, idx = (t.cpu().numpy() for t in s.keep)
    mem = s.mem.float().cpu()
    for b in (1, 2):
        pl = ((XLENS[b] - 1) // 2 - 1) // 2
        ml = min(-(-XLENS[b] // 4), h64.shape[1])
        assert int((~km[b]).sum()) == ml and ml > pl  # the memory mask is longer than the search
        # (a) encoder output and CTC log-probs (at the device's candidates) on the searched frames
        de = float((mem[b, :pl].double() - h64[b, :pl]).abs().max())
        v, i = vals[b * Tcap:b * Tcap + pl], idx[b * Tcap:b * Tcap + pl]
        dc = float(np.abs(v - np.take_along_axis(lp64[b, :pl].numpy(), i.astype(np.int64), 1)).max())
        # (b) the device search against the native host search on the device's own candidates
        ref = D.prefix_beam_search(v, i, beam=10)
        got = trace["nbest"][b]
        assert [t for t, _ in got] == [t for t, _ in ref], b
        ds = max(abs(a[1] - r[1]) for a, r in zip(got, ref))
        # (c) the gathered attention log-probs against the oracle decoder under the key mask
        g64 = _oracle_gathered(d, torch.float64, got, h64[b], km[b])
        gd = trace["gathered"][b]
        assert gd.shape == g64.shape
        fin = ~np.isnan(g64)
        assert np.isfinite(gd[fin]).all() and np.isneginf(gd[~fin]).all()
        dgat = float(np.abs(gd[fin] - g64[fin]).max())
        print(f"row {b}: pred_len {pl}, mem_len {ml}; max |d enc| {de:.3e}, |d ctc| {dc:.3e}, |d score| {ds:.3e}, "
              f"|d gathered| {dgat:.3e}")
        assert de <= 1e-4 and dc <= 1e-4
        assert ds <= 1e-9
        assert dgat <= 1e-4
        # (d) the pick on the device's own gathered values, totals bit for bit
        want = D.pick_best(got, gd)
        assert trace["best"][b] == want and list(out[b]) == got[want][0]
        f32 = np.float32
        for i_, (t, s0) in enumerate(got):
            tot = f32(0.0)
            for j in range(len(t) + 1):
                tot = f32(tot + gd[i_, j])
            tot = f32(tot + f32(s0 * 0.5))
            assert trace["totals"][b][i_] == tot, (b, i_)


# --------------------------------------------------------------------------- 6. short batch, hygiene
def test_short_batch_and_state_hygiene(monkeypatch):
    from liteasr_amd import decoding as D

    model, d = _golden_model()
    fresh, _ = _golden_model()
    xs = torch.cat([_ragged(d), _ragged(d)[1:2]]).cuda()
    lens = list(XLENS) + [XLENS[1]]
    with torch.no_grad():
        t4, t1, tf = {}, {}, {}
        out4 = D.attention_rescore_batch(model, xs, lens, trace=t4)
        assert t4["caps"] == (4, 64, 64) and out4[3] == out4[1]
        # one row in the state captured at Bcap 4: the spare rows are inert
        out1 = D.attention_rescore_batch(model, xs[1:2], lens[1:2], trace=t1)
        assert t1["caps"] == (4, 64, 64) and t1["state"] is t4["state"]
        want1 = D.attention_rescore_batch(fresh, xs[1:2], lens[1:2], trace=tf)
        assert tf["caps"] == (1, 64, 64)
        assert out1 == want1 == [out4[1]]
        assert [t for t, _ in t1["nbest"][0]] == [t for t, _ in tf["nbest"][0]] == [t for t, _ in t4["nbest"][1]]
        # and the full batch again after the short one
        again = {}
        assert D.attention_rescore_batch(model, xs, lens, trace=again) == out4
        assert again["nbest"] == t4["nbest"] and all(np.array_equal(a, b) for a, b in
                                                     zip(again["gathered"], t4["gathered"]))
        # an in-place weight update drops the states
        for m in (model, fresh):
            st = m.store
            ver = st.flat._version
            name = next(n for n in st.offsets if n.endswith("after_norm.weight"))
            st.view(name).add_(0.01)
            assert st.flat._version != ver
        t5 = {}
        out5 = D.attention_rescore_batch(model, xs, lens, trace=t5)
        assert t5["state"] is not t4["state"] and t5["caps"] == (4, 64, 64)
        assert out5 == D.attention_rescore_batch(fresh, xs, lens)
        x0 = xs[0:1]
    host_out, _, _ = _host_path(model, x0, monkeypatch)
    assert list(out5[0]) == list(host_out)


# --------------------------------------------------------------------------- 7. bf16
def test_bf16_equal_length_batch_against_host_path(monkeypatch):
    from liteasr_amd import decoding as D

    model, d = _golden_model("bf16")
    for u in range(int(d["n_utt"])):
        x = _xu(d, u)
        T = x.shape[0]
        other = torch.randn(T, 40, generator=torch.Generator().manual_seed(70 + u))
        trace = {}
        with torch.no_grad():
            D.attention_rescore_batch(model, torch.stack([other, x]).cuda(), [T, T], trace=trace)
        _, host_hyps, host_g = _host_path(model, x.unsqueeze(0).cuda(), monkeypatch)
        assert [t for t, _ in trace["nbest"][1]] == [t for t, _ in host_hyps], u
        got = trace["gathered"][1]
        fin = np.isfinite(host_g)
        assert np.array_equal(fin, np.isfinite(got))
        dg = np.abs(got[fin] - host_g[fin]).max()
        big = np.abs(host_g[fin]).max()
        print(f"utt {u} bf16: max |d gathered| {dg:.3e}, largest magnitude {big:.3f}")
        assert dg <= 1e-2 * big


# --------------------------------------------------------------------------- 8. errors
def test_errors(golden):
    from liteasr_amd import decoding as D
    from liteasr_amd import kernels as K

    model, d = golden
    xs = _ragged(d).cuda()
    with pytest.raises(ValueError, match="row 1: 5 frames subsample to none"):
        D.attention_rescore_batch(model, xs, [120, 5, 64])
    with pytest.raises(ValueError, match="frame counts"):
        D.attention_rescore_batch(model, xs, [120, 64])
    with pytest.raises(RuntimeError, match="HIP device only"):
        D.attention_rescore_batch(model, xs.cpu(), list(XLENS))
    with pytest.raises(RuntimeError, match="HIP device only"):
        model.inference_batch(xs.cpu(), list(XLENS))
    # the wrappers hand raw pointers to the kernels: a host tensor is refused
    B, Tcap, Lcap, L1 = 2, 64, 64, 65
    arena = torch.zeros(K.rescore_workspace_batch(B, Tcap, Lcap), dtype=torch.uint8, device="cuda")
    v = torch.zeros(B * Tcap, 10, device="cuda")
    i = torch.zeros(B * Tcap, 10, dtype=torch.int32, device="cuda")
    tp = torch.zeros(B, dtype=torch.int32, device="cuda")
    for bad in ((v.cpu(), i, tp), (v, i.cpu(), tp), (v, i, tp.cpu())):
        with pytest.raises(ValueError, match="same HIP device"):
            K.rescore_search_batch(arena, B, Tcap, Lcap, *bad, 0)
    with pytest.raises(ValueError, match="same HIP device"):
        K.rescore_search_batch(arena.cpu(), B, Tcap, Lcap, v, i, tp, 0)
    with pytest.raises(ValueError, match="same HIP device"):
        K.rescore_pick_batch(arena, B, Tcap, Lcap, torch.zeros(B * 10 * L1), 0.5)
    ys_in, dec_full, gidx, mem_mask = _prep_outputs(10 * B, L1, Tcap)
    with pytest.raises(ValueError, match="same HIP device"):
        K.rescore_prep_batch(arena, B, Tcap, Lcap, 29, 29, ys_in, dec_full[:, :, :L1], gidx, mem_mask, tp.cpu())
    with pytest.raises(ValueError, match="arena must be"):
        K.rescore_search_batch(arena, B + 1, Tcap, Lcap, v, i, tp, 0)  # an arena of 2 rows
    with pytest.raises(ValueError, match="candidate rows"):
        K.rescore_search_batch(arena, B, Tcap, Lcap, v[:Tcap], i[:Tcap], tp, 0)


# --------------------------------------------------------------------------- 9. CLI
def test_cli_batch_size(tmp_path, monkeypatch):
    from liteasr_amd import infer as I
    from liteasr_amd import tasks
    from liteasr_amd.config.compose import compose
    from liteasr_amd.utils.score import levenshtein

    conf, data = _cli_tree(tmp_path)
    run_dir = tmp_path / "runs" / "asr_U2"
    (run_dir / "ckpts").mkdir(parents=True)
    monkeypatch.chdir(run_dir)
    ovr = [f"task.test=[{data}]", "inference.ckpt_name=1"]
    cfg = compose(str(conf), "config", ovr + ["inference.batch_size=4"], job_name="infer")
    assert cfg.inference.batch_size == 4
    task = tasks.setup_task(cfg.task)
    task.load_dataset("test", task.cfg.test, None, cfg.postprocess)
    torch.manual_seed(3)
    model = task.build_model(cfg.model)
    torch.save(model.state_dict(), run_dir / "ckpts" / "model.ep.1.pt")
    model = model.cuda().eval()
    ds = task.dataset("test")[0]
    assert len(ds) == N_UTT
    plan = I.batch_plan([ds[i].xlen for i in range(len(ds))], 4)
    assert [len(g) for g in plan] == [4, 1]
    hyps = [None] * len(ds)
    with torch.no_grad():
        for group in plan:
            xs, lens = I.pad_batch([ds[i].x for i in group])
            for i, h in zip(group, task.inference_batch(xs.cuda(), lens, model)):
                hyps[i] = h
    refs = [ds[i].text for i in range(len(ds))]
    want_utt = [I.utt_line(r, h)[0][1:] for r, h in zip(refs, hyps)]
    errs = sum(levenshtein(r, h) for r, h in zip(refs, hyps))
    want_rate = I.rate_line(errs, sum(len(r) for r in refs))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    logs = {}
    for name, extra in (("4", ["inference.batch_size=4"]), ("1", ["inference.batch_size=1"]), ("none", [])):
        log = run_dir / "infer.log"
        if log.exists():
            log.unlink()
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "liteasr_amd.infer", "-cd", str(conf)]
                           + ovr + extra, cwd=tmp_path, env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        logs[name] = log.read_text()
    utt, rate = _blocks(logs["4"])
    assert utt == want_utt, (utt, want_utt)  # dataset order, each block what inference_batch returns
    assert rate == [want_rate] and logs["4"].rstrip("\n").endswith(want_rate)
    assert _blocks(logs["1"]) == _blocks(logs["none"])
    strip = lambda s: [ln for ln in s.splitlines() if "batch_size" not in ln]  # noqa: E731
    assert strip(logs["1"]) == strip(logs["none"])
    shutil.rmtree(run_dir, ignore_errors=True)


def test_infer_dataset_batches_paraformer_and_not_transducer(tmp_path, monkeypatch, caplog):
    """batch_size 4 goes through Paraformer.inference_batch, one call per group of batch_plan; a
    model without inference_batch is decoded utterance by utterance, with one log line."""
    import logging

    from liteasr_amd import infer as I
    from liteasr_amd import tasks
    from liteasr_amd.config.compose import compose
    from liteasr_amd.models.paraformer import Paraformer, ParaformerConfig
    from liteasr_amd.utils.cfg import resolve_self

    conf, data = _cli_tree(tmp_path)
    monkeypatch.chdir(tmp_path)
    cfg = compose(str(conf), "config", [f"task.test=[{data}]", "inference.ckpt_name=1"], job_name="infer")
    task = tasks.setup_task(cfg.task)
    task.load_dataset("test", task.cfg.test, None, cfg.postprocess)
    ds = task.dataset("test")[0]
    c = ParaformerConfig(input_dim=task.feat_dim, enc_dim=64, enc_ff_dim=128, enc_attn_heads=4, enc_layers=2,
                         vocab_size=task.vocab_size, dec_dim=64, dec_ff_dim=128, dec_attn_heads=4, dec_layers=1,
                         dropout_rate=0.0, compute_dtype="fp32")
    resolve_self(c)
    torch.manual_seed(5)
    model = Paraformer(c).cuda().eval()
    calls = []
    inner = model.inference_batch

    def recording(xs, xlens):
        calls.append((tuple(xs.shape[:2]), list(xlens)))
        return inner(xs, xlens)

    monkeypatch.setattr(model, "inference_batch", recording)
    _, _, hyps = I.infer_dataset(task, model, ds, torch.device("cuda"), batch_size=4)
    xlens = [ds[i].xlen for i in range(len(ds))]
    plan = I.batch_plan(xlens, 4)
    assert [c_[1] for c_ in calls] == [[xlens[i] for i in g] for g in plan]
    assert [c_[0] for c_ in calls] == [(len(g), max(xlens[i] for i in g)) for g in plan]
    with torch.no_grad():
        xs, lens = I.pad_batch([ds[i].x for i in plan[0]])
        assert [hyps[i] for i in plan[0]] == task.inference_batch(xs.cuda(), lens, model)

    class OneByOne:
        def inference(self, x):
            return [1, 2]

    with caplog.at_level(logging.INFO, logger="liteasr_amd.infer"):
        I.infer_dataset(task, OneByOne(), ds, torch.device("cuda"), batch_size=4)
    assert sum("no inference_batch" in r.getMessage() for r in caplog.records) == 1
