"""Inference searches of U2 (liteasr/models/u2.py:160-317), SURVEY §8 f3, and the Transducer
beam search (liteasr/models/transducer.py:137-206; device-resident, csrc/rnnt_search.hip).

Device side: the encoder / decoder run through the same HIP kernels as training
(nets/decode.py: encoder_out, ctc_logits, decoder_logits); per-frame log_softmax +
top-k and the rescoring gathers are one HIP kernel (lasr_logsoftmax_topk).  Host side:
the CTC prefix beam search is native C++ (libliteasr_decode.so, csrc/decode/), fed
with the [T', beam] candidates; the attention beam's (beam x beam) bookkeeping is a few
float32 numpy operations mirroring the reference's torch ops.  No CPU fallback: both
libraries must be present.
"""

from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from . import kernels as K
from .graph_step import collect_before_capture
from .nets import decode as DN

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libliteasr_decode.so")
_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(_LIB_PATH):
            raise RuntimeError(f"{_LIB_PATH} missing: run `make` (or __graft_entry__.build())")
        L = C.CDLL(_LIB_PATH)
        L.lasr_ctc_prefix_beam_search.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                  C.c_int, C.c_void_p, C.c_int64, C.c_void_p,
                                                  C.c_void_p]
        L.lasr_ctc_prefix_beam_search.restype = C.c_int
        L.lasr_decode_last_error.restype = C.c_char_p
        _LIB = L
    return _LIB


def prefix_beam_search(topk_val: np.ndarray, topk_idx: np.ndarray, beam: int, blank: int = 0):
    """Native CTC prefix beam search over per-frame candidates [T, k] (float32 log-probs,
    int32 ids, descending).  Returns [(tokens list, score float)], best first."""
    v = np.ascontiguousarray(topk_val, dtype=np.float32)
    i = np.ascontiguousarray(topk_idx, dtype=np.int32)
    T, k = v.shape
    cap = max(1, beam * T)
    tok = np.empty(cap, dtype=np.int32)
    lens = np.empty(beam, dtype=np.int32)
    score = np.empty(beam, dtype=np.float64)
    n = _lib().lasr_ctc_prefix_beam_search(v.ctypes.data, i.ctypes.data, T, k, blank, beam,
                                           tok.ctypes.data, cap, lens.ctypes.data, score.ctypes.data)
    if n < 0:
        raise RuntimeError("lasr_ctc_prefix_beam_search: " + _lib().lasr_decode_last_error().decode())
    out, o = [], 0
    for j in range(n):
        out.append((tok[o:o + lens[j]].tolist(), float(score[j])))
        o += int(lens[j])
    return out


def _mem_mask(B, T, dev):
    return torch.zeros(B, T, dtype=torch.uint8, device=dev)


def encode(model, x, graph=True, fp32=False):
    """`self.encoder(x)` for one utterance x [1, T, F] (no padding mask) -> (h [T', d], T').
    h is in the compute dtype; with ``fp32`` it is the fp32 after_norm output (what the
    Paraformer predictor integrates).

    With ``graph`` the ~250 encoder launches of a batch-1 utterance (launch-latency-bound)
    are captured once per input shape into a hipGraph and replayed; the returned h is that
    graph's static output, valid until the next encode of the same shape.  The cache is
    keyed on the flat parameter version, so a weight update re-captures (the working-copy
    cast is host-conditional and must not be skipped by a stale graph), and on the
    train/eval mode.  (The fused Adam kernel rewrites flat and its working copy in place,
    without a version bump: the graph reads them through the same pointers, so replays
    after optimizer steps see the new weights.)"""
    if x.device.type != "cuda":
        raise RuntimeError("liteasr_amd decoding runs on the HIP device only")
    if not graph:
        return _encode_eager(model, x, fp32)
    st = model.store
    # model.training too: dropout and BatchNorm (batch vs running statistics) are baked
    # into the captured launches, so a train()/eval() switch must re-capture
    key = (tuple(x.shape), x.dtype, st.flat._version, st.generation, bool(model.training), bool(fp32))
    cache = model.__dict__.setdefault("_encode_graphs", {})
    e = cache.get(key)
    if e is None:
        cache.clear()
        static = x.clone()
        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        side.wait_stream(cur)
        with torch.cuda.stream(side):  # warm-up: workspaces, working copies, allocator pools
            _encode_eager(model, static, fp32)
        cur.wait_stream(side)
        torch.cuda.synchronize()
        collect_before_capture()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            h, T = _encode_eager(model, static, fp32)
        # keep the workspace the graph was captured against alive even if it is regrown
        e = cache[key] = (g, static, h, T, K.WS.buf.get(x.device.index))
    g, static, h, T, _ = e
    static.copy_(x)
    g.replay()
    return h, T


def _encode_eager(model, x, fp32=False):
    B, Tx = x.shape[0], x.shape[1]
    xlens = torch.full((B,), Tx, dtype=torch.int64, device=x.device)
    ys = torch.full((B, 1), -1, dtype=torch.int64, device=x.device)
    ylens = torch.zeros(B, dtype=torch.int64, device=x.device)
    xe, prep, _ = model._run_encoder(x, xlens, ys, ylens)
    return DN.encoder_out(xe, model, torch.float32 if fp32 else model.compute_dtype), prep.T


def ctc_prefix_beam_search_nbest(model, x, beam=10):
    """u2.py:218-263: (n-best [(tokens, score)], h [T', d], T')."""
    h, T = encode(model, x)
    logits = DN.ctc_logits(h, model)
    vals, idx, _ = K.logsoftmax_topk(logits, min(beam, logits.shape[1]))
    hyps = prefix_beam_search(vals.cpu().numpy(), idx.cpu().numpy(), beam, model.blank)
    return hyps, h, T


def rescore(model, hyps, h, T, ctc_weight=0.5):
    """u2.py:268-317: decoder over the n-best (memory = h repeated, no memory mask),
    score = sum of attention log-probs at the tokens + eos (fp32, as the reference's
    0-d tensor sum) + ctc_weight * CTC score; first strict maximum wins."""
    dev = h.device
    n = len(hyps)
    Lmax = max(1, max(len(t) for t, _ in hyps))
    L1 = Lmax + 1
    ys = torch.full((n, Lmax), -1, dtype=torch.int64)
    for i, (t, _) in enumerate(hyps):
        ys[i, :len(t)] = torch.tensor(t, dtype=torch.int64)
    ylens = torch.tensor([len(t) for t, _ in hyps], dtype=torch.int64)
    Tx = 4 * T + 3  # any Tx with ((Tx-1)//2-1)//2 == T; all frames valid
    prep = model._prep_targets(ys.to(dev), ylens.to(dev), n, Tx)
    mem = h.view(1, T, -1).expand(n, T, h.shape[1]).reshape(n * T, h.shape[1])
    h_attn = DN.decoder_logits(model, mem, prep.ys_in, prep.dec_mask, _mem_mask(n, T, dev), n, L1, T)
    gidx = torch.full((n, L1), -1, dtype=torch.int32)
    for i, (t, _) in enumerate(hyps):
        gidx[i, :len(t)] = torch.tensor(t, dtype=torch.int32)
        gidx[i, len(t)] = model.eos
    _, _, g = K.logsoftmax_topk(h_attn, 0, gather_idx=gidx.view(-1).to(dev))
    return pick_best(hyps, g.view(n, L1).cpu().numpy(), ctc_weight)


def pick_best(hyps, g, ctc_weight=0.5):
    """Host half of rescoring (u2.py:300-315): g[i, j] = attention log-prob of hypothesis
    i's j-th token (j = len: eos).  float32 running sum like the reference's 0-d tensor,
    python-float CTC term cast to float32, first strict maximum wins."""
    f32 = np.float32
    best, best_i = -float("inf"), 0
    for i, (t, sc) in enumerate(hyps):
        s = f32(0.0)
        for j in range(len(t) + 1):  # tokens, then eos at position len(t)
            s = f32(s + g[i, j])
        s = f32(s + f32(sc * ctc_weight))
        if s > best:
            best, best_i = s, i
    return best_i


def attention_beam_search(model, x, beam=10, trace=None):
    """u2.py:163-216: left-to-right attention beam search (memory h repeated, no memory
    mask), max T' steps, the decoder advanced one position per step through its key/value
    cache (DN.DecoderStepCache: the reference's forward_one_step cache semantics, incl. its
    never-reordered cache of layers >= 1), per-step log_softmax + topk(beam) on the device,
    the (beam x beam) score bookkeeping in float32 on the host.  trace (a list): per step
    (hyps fed to the step [beam, i], log-prob top-k values [beam, beam]) for tests."""
    h, T = encode(model, x)
    dev = h.device
    sos, eos = model.sos, model.eos
    init = np.array([0.0] + [-np.inf] * (beam - 1), dtype=np.float32)
    hyps = np.full((beam, 1), sos, dtype=np.int64)
    scores = init.reshape(beam, 1).copy()
    end = np.zeros(beam, dtype=bool)
    dec = DN.DecoderStepCache(model, h, beam, T, T + 1)
    sel_d = None
    for i in range(1, T + 1):
        if end.sum() == beam:
            break
        ids = torch.from_numpy(np.ascontiguousarray(hyps[:, -1]).astype(np.int32)).to(dev)
        logits = dec.step(ids, i, sel_d)
        vals, idx, _ = K.logsoftmax_topk(logits, beam)
        st = vals.cpu().numpy()
        it = idx.cpu().numpy().astype(np.int64)
        if trace is not None:
            trace.append((hyps.copy(), st.copy()))
        st[end] = init
        it[end] = eos
        cand = (scores + st).reshape(-1).astype(np.float32)
        order = np.argsort(-cand.astype(np.float64), kind="stable")[:beam]
        scores = cand[order].reshape(beam, 1)
        sel, off = order // beam, order % beam
        hyps = np.concatenate([hyps[sel], it[sel, off][:, None]], axis=1)
        sel_d = torch.from_numpy(sel.astype(np.int64)).to(dev)
        end = hyps[:, -1] == eos
    best = int(np.argmax(scores.reshape(-1)))
    return hyps[best].tolist()


_BEAM = 10  # the reference's beam (u2.py:160-317, transducer.py:137): the only one the device searches build

# ============================================== attention rescoring on the device ===
def attention_rescore_host(model, x, ctc_weight=0.5, encoder_graph=True):
    """u2.py:269-317 through the host: top-k copied down, native prefix search, the n-best
    padded in Python, an eager decoder pass at the utterance's shapes, the gathers copied down.
    This is what U2.inference runs (the device-resident pass below beats it only at T = 400,
    not at T = 1000).  encoder_graph=False: the same steps after an eager encoder
    pass."""
    if encoder_graph:
        hyps, h, T = ctc_prefix_beam_search_nbest(model, x, beam=10)
    else:
        h, T = encode(model, x, graph=False)
        logits = DN.ctc_logits(h, model)
        vals, idx, _ = K.logsoftmax_topk(logits, min(10, logits.shape[1]))
        hyps = prefix_beam_search(vals.cpu().numpy(), idx.cpu().numpy(), 10, model.blank)
    return tuple(hyps[rescore(model, hyps, h, T, ctc_weight=ctc_weight)][0])


# result block words of the rescoring arena (include/liteasr_hip.h)
_R_ERR, _R_N, _R_BEST, _R_BESTLEN, _R_TP, _R_LENS, _R_SCORE, _R_TOTAL, _R_HEAD = 0, 1, 2, 3, 4, 8, 20, 40, 64
_RESCORE_ERRORS = {2: "prefix table full", 4: "a frame without k finite candidates"}
_CTC_WEIGHT = 0.5  # u2.py:269


def rescore_layout(Tcap, Lcap):
    """Word offsets of the result block's variable part: best tokens, tokens [10, Lcap], the
    copy of the gathered log-probs [10, Lcap + 1]; head_words = the words the host reads."""
    best = _R_HEAD
    toks = best + Lcap
    gath = toks + _BEAM * Lcap
    return {"best": best, "toks": toks, "gath": gath, "head_words": gath + _BEAM * (Lcap + 1)}


class _Rescore:
    """Arena, static buffers and the captured graph of one model at one (Tcap, Lcap)."""

    def __init__(self, model, Tcap, Lcap, d, adt, dev):
        self.Tcap, self.Lcap, self.L1 = Tcap, Lcap, Lcap + 1
        self.k = min(_BEAM, model.vocab_size)
        self.off = rescore_layout(Tcap, Lcap)
        self.arena = torch.zeros(K.rescore_workspace(Tcap, Lcap), dtype=torch.uint8, device=dev)
        self.mem = torch.zeros(Tcap, d, dtype=adt, device=dev)  # rows >= T' stay zero
        self.tp = torch.zeros(1, dtype=torch.int32, device=dev)
        L1 = self.L1
        self.ys_in = torch.zeros(_BEAM, L1, dtype=torch.int32, device=dev)
        # 16-B aligned mask rows, as _prep allocates them (the attention kernels stage tiles by LDS-DMA)
        self.dec_mask = torch.ones(_BEAM, L1, (L1 + 15) // 16 * 16, dtype=torch.uint8, device=dev)[:, :, :L1]
        self.gidx = torch.full((_BEAM * L1,), -1, dtype=torch.int32, device=dev)
        self.mem_mask = torch.ones(_BEAM, Tcap, dtype=torch.uint8, device=dev)
        self.filled = 0
        self.graph = None
        self.keep = None

    def launches(self, model):
        """ctc_lo + log-softmax top-k over all Tcap rows, the search (T' on the device), the
        decoder inputs, the decoder at (10, L1cap, Tcap) under the memory mask, the gather, the
        pick: one stream, in this order."""
        Tcap, Lcap, L1 = self.Tcap, self.Lcap, self.L1
        logits = DN.ctc_logits(self.mem, model)
        vals, idx, _ = K.logsoftmax_topk(logits, self.k)
        K.rescore_search(self.arena, Tcap, Lcap, vals, idx, self.tp, model.blank, _BEAM)
        K.rescore_prep(self.arena, Tcap, Lcap, model.sos, model.eos, self.ys_in, self.dec_mask, self.gidx,
                       self.mem_mask)
        d = self.mem.shape[1]
        mem = self.mem.view(1, Tcap, d).expand(_BEAM, Tcap, d).reshape(_BEAM * Tcap, d)
        h_attn = DN.decoder_logits(model, mem, self.ys_in, self.dec_mask, self.mem_mask, _BEAM, L1, Tcap)
        _, _, g = K.logsoftmax_topk(h_attn, 0, gather_idx=self.gidx)
        K.rescore_pick(self.arena, Tcap, Lcap, g, _CTC_WEIGHT)
        return vals, idx, g

    def capture(self, model):
        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        side.wait_stream(cur)
        with torch.cuda.stream(side):  # warm-up: workspaces, working copies, allocator pools
            self.launches(model)
        cur.wait_stream(side)
        torch.cuda.synchronize()
        collect_before_capture()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self.keep = self.launches(model)
        self.graph = g
        self.ws = K.WS.buf.get(self.arena.device.index)  # the workspace the graph was captured against

    def run(self, model, h, Tp):
        """One utterance: memory rows and T' in, one replay, the result block out (ONE copy)."""
        if self.graph is None:
            self.capture(model)
        self.mem[:Tp].copy_(h[:Tp])
        if self.filled > Tp:
            self.mem[Tp:self.filled].zero_()
        self.filled = Tp
        self.tp.fill_(Tp)
        self.graph.replay()
        return self.arena[: 4 * self.off["head_words"]].cpu().numpy().view(np.int32)


def _rescore_state(model, Tcap, Lcap, h):
    st = model.store
    ver = (st.flat._version, st.generation, h.dtype, h.shape[1])
    cache = model.__dict__.setdefault("_rescore_states", {})
    if cache.get("ver") != ver:  # a weight update: the working copies a graph reads may be stale
        cache.clear()
        cache["ver"] = ver
        cache["lcap"] = {}
    if Lcap is None:
        return cache["lcap"]
    s = cache.get((Tcap, Lcap))
    if s is None:
        s = cache[(Tcap, Lcap)] = _Rescore(model, Tcap, Lcap, h.shape[1], h.dtype, h.device)
    return s


def rescore_nbest(head, Lcap):
    """[(tokens, score)] of a result block (int32 words)."""
    off = rescore_layout(0, Lcap)
    n = int(head[_R_N])
    lens = head[_R_LENS:_R_LENS + _BEAM]
    score = head[_R_SCORE:_R_SCORE + 2 * _BEAM].view(np.float64)
    toks = head[off["toks"]:off["toks"] + _BEAM * Lcap].reshape(_BEAM, Lcap)
    return [(toks[i, :lens[i]].tolist(), float(score[i])) for i in range(n)]


def attention_rescore_device(model, x, trace=None, encoder_graph=True):
    """u2.py:269-317 (beam 10, ctc weight 0.5) for one utterance x [1, T, F] with everything
    after the encoder on the device: the encoder output goes into a static memory buffer
    [Tcap, d] (rows >= T' zero), T' into a device word, and ONE replay of a captured linear
    hipGraph runs ctc_lo, the per-frame log-softmax top-k, the CTC prefix beam search
    (csrc/rescore.hip), the decoder inputs, the decoder at the static shape (10, Lcap + 1,
    Tcap) under the memory mask, the gather and the pick; ONE device-to-host copy brings back
    the result block.  Tcap = the power of two >= max(T', 64); Lcap starts at 64 and doubles
    (the utterance is run again) when a kept hypothesis is longer; a Tcap bucket then keeps the
    largest Lcap it has needed.  States, and so graphs, are
    cached per (Tcap, Lcap) and dropped on a weight update.  trace (a dict) receives "nbest"
    [(tokens, score)], "gathered" [n, Lmax + 1], "best" and "totals"."""
    if x.device.type != "cuda":
        raise RuntimeError("liteasr_amd decoding runs on the HIP device only")
    if x.dim() != 3 or x.shape[0] != 1:
        raise ValueError("attention_rescore_device: one utterance x [1, T, F]")
    h, Tp = encode(model, x, graph=encoder_graph)
    if Tp <= 0:
        raise ValueError(f"attention_rescore_device: {x.shape[1]} frames subsample to none")
    Tcap = 64
    while Tcap < Tp:
        Tcap *= 2
    # a bucket starts at Lcap 64 and keeps the largest Lcap it has needed: after an overflow,
    # later utterances of the bucket are not run again from 64
    hint = _rescore_state(model, Tcap, None, h)
    Lcap = hint.get(Tcap, 64)
    while True:
        s = _rescore_state(model, Tcap, Lcap, h)
        head = s.run(model, h, Tp)
        err = int(head[_R_ERR])
        if err & ~1:
            raise RuntimeError("attention_rescore_device: " + _RESCORE_ERRORS.get(err & ~1, f"error {err}"))
        if not err:
            break
        if Lcap >= Tcap:
            raise RuntimeError(f"attention_rescore_device: hypothesis longer than T' cap {Tcap}")
        Lcap *= 2
    hint[Tcap] = Lcap
    assert int(head[_R_TP]) == Tp, (int(head[_R_TP]), Tp)
    n, best, blen = int(head[_R_N]), int(head[_R_BEST]), int(head[_R_BESTLEN])
    off = s.off
    if trace is not None:
        hyps = rescore_nbest(head, Lcap)
        Lmax = max(1, max(len(t) for t, _ in hyps))
        g = head[off["gath"]:off["gath"] + _BEAM * (Lcap + 1)].view(np.float32).reshape(_BEAM, Lcap + 1)
        trace["nbest"] = hyps
        trace["gathered"] = g[:n, :Lmax + 1].copy()
        trace["best"] = best
        trace["totals"] = head[_R_TOTAL:_R_TOTAL + n].view(np.float32).copy()
        trace["caps"] = (Tcap, Lcap)
    return tuple(head[off["best"]:off["best"] + blen].tolist())


# ================================================== attention rescoring, batched ===
# One group's attention logits, 10 n (Lcap + 1) V elements, are the largest buffer of the pass:
# 352 MB in fp32 for all of B 32 at Lcap 64, V 4233, and 1.4 GB at Lcap 256.  The decoder pass
# runs over groups of utterances whose logits stay under this many bytes.  The logits are written
# once by the output projection and read once by the log-softmax gather, so half of the 256 MB
# Infinity Cache keeps that hand-off on chip with room for the memory and the weights; and the
# graph pool of every cached state then holds one group's logits, not Bcap's.  (Reasoned, not
# tuned: the pass is bounded by the serial search)
_LOGITS_BUDGET_BYTES = 128 << 20


def _pow2_cap(n):
    c = 64
    while c < n:
        c *= 2
    return c


class _RescoreBatch:
    """Batch arena, static buffers and the captured graph of one model at one (Bcap, Tcap, Lcap).
    Utterance b owns arena b, memory row b and the hypothesis rows [10 b, 10 b + 10)."""

    def __init__(self, model, Bcap, Tcap, Lcap, d, adt, dev):
        self.Bcap, self.Tcap, self.Lcap, self.L1 = Bcap, Tcap, Lcap, Lcap + 1
        self.k = min(_BEAM, model.vocab_size)
        self.off = rescore_layout(Tcap, Lcap)
        self.stride = K.rescore_workspace(Tcap, Lcap)
        self.arena = torch.zeros(K.rescore_workspace_batch(Bcap, Tcap, Lcap), dtype=torch.uint8, device=dev)
        self.mem = torch.zeros(Bcap, Tcap, d, dtype=adt, device=dev)
        self.tp = torch.zeros(Bcap, dtype=torch.int32, device=dev)
        self.mem_len = torch.ones(Bcap, dtype=torch.int32, device=dev)
        L1, R = self.L1, _BEAM * Bcap
        self.ys_in = torch.zeros(R, L1, dtype=torch.int32, device=dev)
        self.dec_mask = torch.ones(R, L1, (L1 + 15) // 16 * 16, dtype=torch.uint8, device=dev)[:, :, :L1]
        self.gidx = torch.full((R * L1,), -1, dtype=torch.int32, device=dev)
        self.mem_mask = torch.ones(R, Tcap, dtype=torch.uint8, device=dev)
        self.gathered = torch.zeros(R * L1, dtype=torch.float32, device=dev)
        # the decoder groups: as few as the budget allows, of equal size (static per state)
        row_bytes = _BEAM * L1 * ((model.vocab_size + 7) // 8 * 8) * self.mem.element_size()  # one utterance's
        ngroups = -(-Bcap // max(1, _LOGITS_BUDGET_BYTES // row_bytes))
        size = -(-Bcap // ngroups)
        self.groups = [(a, min(a + size, Bcap)) for a in range(0, Bcap, size)]
        self.filled = (0, 0)
        self.graph = None
        self.keep = None

    def launches(self, model):
        """ctc_lo + log-softmax top-k over all Bcap Tcap rows, the batched search, the decoder
        inputs, then per group the decoder at (10 n, L1cap, Tcap) under the memory mask and the
        gather, and the pick: one stream, in this order."""
        Bcap, Tcap, Lcap, L1 = self.Bcap, self.Tcap, self.Lcap, self.L1
        d = self.mem.shape[2]
        logits = DN.ctc_logits(self.mem.view(Bcap * Tcap, d), model)
        vals, idx, _ = K.logsoftmax_topk(logits, self.k)
        K.rescore_search_batch(self.arena, Bcap, Tcap, Lcap, vals, idx, self.tp, model.blank, _BEAM)
        K.rescore_prep_batch(self.arena, Bcap, Tcap, Lcap, model.sos, model.eos, self.ys_in, self.dec_mask, self.gidx,
                             self.mem_mask, self.mem_len)
        for a, b in self.groups:
            n, r0, r1 = _BEAM * (b - a), _BEAM * a, _BEAM * b
            mem = self.mem[a:b].unsqueeze(1).expand(b - a, _BEAM, Tcap, d).reshape(n * Tcap, d)
            h_attn = DN.decoder_logits(model, mem, self.ys_in[r0:r1], self.dec_mask[r0:r1], self.mem_mask[r0:r1], n, L1,
                                       Tcap)
            _, _, g = K.logsoftmax_topk(h_attn, 0, gather_idx=self.gidx[r0 * L1:r1 * L1])
            self.gathered[r0 * L1:r1 * L1].copy_(g)
        K.rescore_pick_batch(self.arena, Bcap, Tcap, Lcap, self.gathered, _CTC_WEIGHT)
        return vals, idx

    capture = _Rescore.capture

    def run(self, model, h, pred_len, mem_len):
        """One batch: h [B, T', d], the search lengths and memory lengths (int32 [B], device) in,
        one replay, the B result heads out (ONE copy).  Rows >= B are inert: T' = 0 (no frame
        is searched) and one visible frame of zero memory, so that their softmax has a key."""
        if self.graph is None:
            self.capture(model)
        B, Tp = h.shape[0], h.shape[1]
        fB, fT = self.filled
        self.mem[:B, :Tp].copy_(h)
        if fT > Tp:
            self.mem[:B, Tp:fT].zero_()
        if fB > B:
            self.mem[B:fB, :fT].zero_()
        self.filled = (B, Tp)
        self.tp.zero_()
        self.tp[:B].copy_(pred_len)
        self.mem_len.fill_(1)
        self.mem_len[:B].copy_(mem_len)
        self.graph.replay()
        heads = self.arena.view(self.Bcap, self.stride)[:B, :4 * self.off["head_words"]]
        return heads.cpu().numpy().view(np.int32)


def _rescore_batch_state(model, key, h):
    """The cache of the batched states: dropped, like _rescore_state's, on a weight update or a
    store-generation change.  key None: the hints {"bcaps": {Bcap, ...}, (Bcap, Tcap): Lcap}."""
    st = model.store
    ver = (st.flat._version, st.generation, h.dtype, h.shape[-1])
    cache = model.__dict__.setdefault("_rescore_batch_states", {})
    if cache.get("ver") != ver:
        cache.clear()
        cache["ver"] = ver
        cache["hint"] = {}
    if key is None:
        return cache["hint"]
    s = cache.get(key)
    if s is None:
        s = cache[key] = _RescoreBatch(model, *key, h.shape[-1], h.dtype, h.device)
    return s


def attention_rescore_batch(model, xs, xlens, trace=None):
    """u2.py:269-317 (beam 10, ctc weight 0.5, the first strict maximum wins) for a padded batch
    xs [B, T, F] with frame counts xlens: a list of B token tuples.

    The reference has no batched inference; this composes its modules as ``U2.forward`` composes
    them, in eval mode (the precedent of ``Paraformer.inference_batch``): the encoder runs on the
    padded batch under padding_mask(xlens); the CTC prefix beam search of row b covers
    ``get_pred_len(xlens)[b]`` frames; the decoder sees memory row b under the encoder's own
    subsampled padding mask (frame t' valid iff 4 t' < xlen_b, capped at T').  So a row with
    xlen_b == T is the computation of ``U2.inference(xs[b:b+1])``, while a padded row is the
    computation training sees for that row (its frames next to the padding see the padding
    through the convolutions; the memory mask is up to two frames longer than the search), not the
    unpadded single-utterance one.  A row depends on its own padding only, never on
    the content of another row.

    After the (eager) encoder pass everything stays on the device: ONE replay of a captured
    linear hipGraph at the static shape (Bcap, Tcap, Lcap) runs ctc_lo, the per-frame log-softmax
    top-k, the batched search (csrc/rescore.hip, one workgroup per row), the decoder inputs, the
    decoder at (10 n, Lcap + 1, Tcap) per group of n utterances (_LOGITS_BUDGET_BYTES), the gathers
    and the pick, and ONE device-to-host copy brings back the B result heads.  Tcap and Lcap
    follow attention_rescore_device (powers of two >= 64; Lcap doubles, and only the graph is
    run again, when any row overflows; a bucket keeps the largest Lcap it has needed).  Bcap is
    the smallest batch capacity that holds B among those used since the states were last
    dropped, else B itself: a shorter batch (the last of a set) runs in a state of the set's
    batch size with its spare rows inert.  States are cached per (Bcap, Tcap, Lcap) and dropped
    on a weight update or a store-generation change.

    trace (a dict) receives, as lists over the rows, what attention_rescore_device's receives:
    "nbest", "gathered", "best", "totals"; "caps" = (Bcap, Tcap, Lcap); and "state", the
    _RescoreBatch that ran (its ``keep`` holds the candidates the search read)."""
    if xs.device.type != "cuda":
        raise RuntimeError("liteasr_amd decoding runs on the HIP device only")
    if xs.dim() != 3:
        raise ValueError("attention_rescore_batch: xs [B, T, F]")
    B, T = xs.shape[0], xs.shape[1]
    lens = [int(n) for n in (xlens.tolist() if torch.is_tensor(xlens) else xlens)]
    if len(lens) != B or B < 1:
        raise ValueError(f"attention_rescore_batch: {len(lens)} frame counts for {B} rows")
    for b, n in enumerate(lens):
        if n > T:
            raise ValueError(f"attention_rescore_batch: row {b} has {n} frames, xs holds {T}")
        if _sub_len(n) <= 0:
            raise ValueError(f"attention_rescore_batch: row {b}: {n} frames subsample to none")
    dev = xs.device
    xl = torch.tensor(lens, dtype=torch.int64, device=dev)
    ys = torch.full((B, 1), -1, dtype=torch.int64, device=dev)
    xe, prep, _ = model._run_encoder(xs, xl, ys, torch.zeros(B, dtype=torch.int64, device=dev))
    Tp = prep.T
    h = DN.encoder_out(xe, model, model.compute_dtype).view(B, Tp, -1)
    mem_len = (prep.enc_mask == 0).sum(1, dtype=torch.int32)
    hint = _rescore_batch_state(model, None, h)
    bcaps = hint.setdefault("bcaps", set())
    Bcap = min((c for c in bcaps if c >= B), default=B)
    bcaps.add(Bcap)
    Tcap = _pow2_cap(Tp)
    Lcap = hint.get((Bcap, Tcap), 64)
    while True:
        s = _rescore_batch_state(model, (Bcap, Tcap, Lcap), h)
        heads = s.run(model, h, prep.pred_len, mem_len)
        errs = heads[:, _R_ERR]
        for b in range(B):
            if errs[b] & ~1:
                what = _RESCORE_ERRORS.get(int(errs[b]) & ~1, f"error {int(errs[b])}")
                raise RuntimeError(f"attention_rescore_batch: row {b}: {what}")
        if not errs.any():
            break
        if Lcap >= Tcap:
            raise RuntimeError(f"attention_rescore_batch: hypothesis longer than T' cap {Tcap}")
        Lcap *= 2
    hint[(Bcap, Tcap)] = Lcap
    off = s.off
    out = []
    for b in range(B):
        head = heads[b]
        assert int(head[_R_TP]) == _sub_len(lens[b]), (b, int(head[_R_TP]), lens[b])
        out.append(tuple(head[off["best"]:off["best"] + int(head[_R_BESTLEN])].tolist()))
    if trace is not None:
        for key in ("nbest", "gathered", "best", "totals"):
            trace[key] = []
        for b in range(B):
            head = heads[b]
            n = int(head[_R_N])
            hyps = rescore_nbest(head, Lcap)
            Lmax = max(1, max(len(t) for t, _ in hyps))
            g = head[off["gath"]:off["gath"] + _BEAM * (Lcap + 1)].view(np.float32).reshape(_BEAM, Lcap + 1)
            trace["nbest"].append(hyps)
            trace["gathered"].append(g[:n, :Lmax + 1].copy())
            trace["best"].append(int(head[_R_BEST]))
            trace["totals"].append(head[_R_TOTAL:_R_TOTAL + n].view(np.float32).copy())
        trace["caps"] = (Bcap, Tcap, Lcap)
        trace["state"] = s
    return out


# ============================================================= CTC forced alignment ===
def ctc_align(model, xs, xlens, ys, ylens, trace=None):
    """Viterbi alignment of the transcripts ys [B, L] (padded with -1 as in training, ylens
    tokens each) to the padded batch xs [B, T, F] with frame counts xlens, through the CTC head.

    Composed as ``attention_rescore_batch`` composes its encoder pass, in eval mode: the encoder
    runs on the padded batch under padding_mask(xlens), and row b's lattice covers
    ``get_pred_len(xlens)[b]`` encoder frames.  Then ctc_lo, the first stage of the CTC loss
    (``K.ctc_fwd(..., alpha=None)``: the log-softmax and the gather of the blank / target
    log-probs) and ``K.ctc_align`` (csrc/ctc_align.hip), and ONE device-to-host copy of (states,
    spans, score).  So a row with xlen_b == T is the unpadded computation of that utterance alone,
    while a padded row is the computation training sees for that row (the documented convention of
    ``inference_batch``): its frames next to the padding see the padding through the convolutions.

    Returns one record per row, ``{"score": float, "states": [Tb ints], "spans": [(first, end)] *
    L_b}`` in encoder frames (``states`` the extended-lattice state of each frame, ``spans`` the
    first frame and one past the last frame of each token), or None for a row whose score is not
    finite (more tokens, counting a blank between adjacent repeats, than encoder frames).

    trace (a dict) receives "lp", "targets", "pred_len", "ylen" (the device tensors the kernel
    read) and "d2h", the number of device-to-host copies made (1)."""
    if xs.device.type != "cuda":
        raise RuntimeError("liteasr_amd decoding runs on the HIP device only")
    if xs.dim() != 3 or ys.dim() != 2 or ys.shape[0] != xs.shape[0]:
        raise ValueError("ctc_align: xs [B, T, F] and ys [B, L]")
    if model.training:
        raise RuntimeError("ctc_align: call it on a model in eval mode (model.eval())")
    B, T = xs.shape[0], xs.shape[1]
    lens = [int(n) for n in (xlens.tolist() if torch.is_tensor(xlens) else xlens)]
    ylen = [int(n) for n in (ylens.tolist() if torch.is_tensor(ylens) else ylens)]
    if len(lens) != B or len(ylen) != B or B < 1:
        raise ValueError(f"ctc_align: {len(lens)} frame counts and {len(ylen)} token counts for {B} rows")
    for b, (n, l) in enumerate(zip(lens, ylen)):
        if n > T or _sub_len(n) <= 0:
            raise ValueError(f"ctc_align: row {b} has {n} frames, xs holds {T} (and at least 7 are needed)")
        if not 0 <= l <= ys.shape[1]:
            raise ValueError(f"ctc_align: row {b} has {l} tokens, ys holds {ys.shape[1]}")
    dev = xs.device
    if ys.shape[1] == 0:  # the bookkeeping kernel wants a column
        ys = torch.full((B, 1), -1, dtype=torch.int64, device=dev)
    xl = torch.tensor(lens, dtype=torch.int64, device=dev)
    yl = torch.tensor(ylen, dtype=torch.int64, device=dev)
    with torch.no_grad():
        xe, prep, _ = model._run_encoder(xs, xl, ys.to(dev), yl)
        Tp, L = prep.T, prep.L
        h = DN.encoder_out(xe, model, model.compute_dtype)
        hc = DN.ctc_logits(h, model).view(B, Tp, -1)
        lse = torch.empty(B * Tp, dtype=torch.float32, device=dev)
        lp = torch.empty(B, Tp, L + 1, dtype=torch.float32, device=dev)
        K.ctc_fwd(hc, prep.tgt_ctc, prep.pred_len, prep.ylen, lse, lp, None, None)
        states, spans, score = K.ctc_align(lp, prep.tgt_ctc, prep.pred_len, prep.ylen)
        # one copy: the three outputs side by side as int32 words
        packed = torch.cat([states, spans.view(B, 2 * L), score.view(torch.int32).view(B, 1)], dim=1).cpu().numpy()
    st, sp, sc = packed[:, :Tp], packed[:, Tp:Tp + 2 * L].reshape(B, L, 2), packed[:, Tp + 2 * L].view(np.float32)
    out = []
    for b in range(B):
        if not np.isfinite(sc[b]):
            out.append(None)
            continue
        Tb = _sub_len(lens[b])
        out.append({"score": float(sc[b]), "states": st[b, :Tb].tolist(),
                    "spans": [tuple(p) for p in sp[b, :ylen[b]].tolist()]})
    if trace is not None:
        trace.update(lp=lp, targets=prep.tgt_ctc, pred_len=prep.pred_len, ylen=prep.ylen, d2h=1)
    return out


# ======================================================= transducer beam search ===
_ERRORS ={1: "node arena full", 2: "state-slot arena full", 3: "trie hash full", 4: "non-finite joint logits",
           5: "empty hypothesis list"}
# ctrl words of the search arena (include/liteasr_hip.h)
_C_ERR, _C_POPS, _C_CUR, _C_DOSTEP, _C_STEPS, _C_DONE, _C_BEST, _C_BESTLEN = 0, 1, 3, 4, 10, 11, 12, 13


def _rnnt_layout(Tcap, layers, H, J, V, node_cap, slot_cap):
    """Byte offsets of the arena sections (the formula of include/liteasr_hip.h)."""
    up = lambda n: -(-n // 256) * 256  # noqa: E731
    hash_cap = 64
    while hash_cap < 2 * node_cap:
        hash_cap *= 2
    slot_floats = -(-(2 * layers * H + J) // 64) * 64
    sizes = [("ctrl", 64 * 4), ("cand", 2 * 16 * 4), ("yseq", (_BEAM * Tcap + 2) * 4), ("lists", 120 * 16),
             ("trace", _BEAM * Tcap * 16), ("nodes", node_cap * 16), ("hash", hash_cap * 4), ("logits", V * 4),
             ("slots", slot_cap * slot_floats * 4)]
    off, o = {}, 0
    for name, n in sizes:
        off[name] = o
        o += up(n)
    off["total"], off["slot_floats"] = o, slot_floats
    return off


class _RnntSearch:
    """Arena, argument block and the captured frame graph of one model (one parameter
    generation, one set of capacities)."""

    def __init__(self, model, Tcap, node_cap, slot_cap):
        dec = model.decoder
        wd, wj = dec.weights(), model.joint_params.weights()
        dev = wj.Wj.device
        self.Tcap, self.layers, self.H = Tcap, dec.n_layer, dec.h_units
        self.J, self.V = wj.Wd.shape[0], wj.Wj.shape[0]
        self.node_cap = int(node_cap) if node_cap else _BEAM * _BEAM * Tcap + 1
        self.slot_cap = int(slot_cap) if slot_cap else _BEAM * Tcap + 1
        if self.node_cap < 1 or self.slot_cap < 1:
            raise ValueError("transducer_beam_search: capacities must be positive")
        self.off = _rnnt_layout(Tcap, self.layers, self.H, self.J, self.V, self.node_cap, self.slot_cap)
        nbytes = K.rnnt_search_workspace(Tcap, self.layers, self.H, self.J, self.V, self.node_cap, self.slot_cap)
        assert nbytes == self.off["total"], (nbytes, self.off["total"])
        self.arena = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        self.enc_proj = torch.zeros(Tcap, self.J, dtype=torch.float32, device=dev)
        self.weights = (wd, wj)  # keeps the views the argument block points into
        self.args = K.rnnt_search_args(self.arena, Tcap, self.node_cap, self.slot_cap, wd.E,
                                       [(l.Wih, l.Whh, l.bih, l.bhh) for l in wd.layers], wj.Wd, wj.Wj, wj.bj,
                                       self.enc_proj)
        self.graph = None

    def view(self, name, dtype, count):
        o = self.off[name]
        return self.arena[o: o + count * torch.empty((), dtype=dtype).element_size()].view(dtype)

    def start(self, model, h, Tp):
        """enc_proj = lin_enc(h) for all frames (transducer.py:221), then the init launch."""
        wj = self.weights[1]
        K.linear(h, wj.We, self.enc_proj[:Tp], bias=wj.be)
        K.rnnt_search_init(self.args, Tp)

    def frame_graph(self):
        """The launches of one frame (10 expansions), captured once as a linear hipGraph; the
        frame index advances on the device, so the same graph serves every frame and T'."""
        if self.graph is None:
            cur = torch.cuda.current_stream()
            side = torch.cuda.Stream()
            side.wait_stream(cur)
            with torch.cuda.stream(side):  # warm-up: code objects loaded before the capture
                K.rnnt_search_init(self.args, 1)
                for _ in range(_BEAM):
                    K.rnnt_search_expand(self.args, 0)
            cur.wait_stream(side)
            torch.cuda.synchronize()
            collect_before_capture()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(_BEAM):
                    K.rnnt_search_expand(self.args, 0)
            self.graph = g
        return self.graph

    def pops(self, n):
        """The first n pops as [(yseq tuple, score, |A|)] (reads the trace and the trie)."""
        tr = self.view("trace", torch.int32, 4 * n).cpu().numpy().reshape(n, 4)
        score = np.ascontiguousarray(tr[:, :2]).view(np.float64).reshape(n)
        nodes = self.view("nodes", torch.int32, 4 * self.node_cap).cpu().numpy().reshape(-1, 4)
        memo, out = {-1: ()}, []

        def yseq(k):
            if k not in memo:
                memo[k] = yseq(int(nodes[k, 0])) + (int(nodes[k, 1]),)
            return memo[k]

        for j in range(n):
            out.append((yseq(int(tr[j, 2])), float(score[j]), int(tr[j, 3])))
        return out


def _rnnt_search_state(model, x, Tp, node_cap, slot_cap):
    if x.device.type != "cuda":
        raise RuntimeError("liteasr_amd decoding runs on the HIP device only")
    if x.dim() != 3 or x.shape[0] != 1:
        raise ValueError("transducer_beam_search: one utterance x [1, T, F]")
    if model.vocab_size < _BEAM + 1:
        raise ValueError(f"transducer_beam_search: vocab_size {model.vocab_size} < 11 (topk(10) over the non-blank "
                         "tokens, transducer.py:168)")
    h, T = encode(model, x)
    assert T == Tp
    st = model.store
    Tcap = 64
    while Tcap < Tp:
        Tcap *= 2
    key = (st.flat._version, st.generation, Tcap, node_cap, slot_cap)
    cache = model.__dict__.setdefault("_rnnt_search", {})
    s = cache.get(key)
    if s is None:
        cache.clear()
        s = cache[key] = _RnntSearch(model, Tcap, node_cap, slot_cap)
    return s, h


def _sub_len(T):
    return ((T - 1) // 2 - 1) // 2


def transducer_beam_search(model, x, beam=10, trace=None, node_cap=None, slot_cap=None):
    """transducer.py:137-206 for one utterance x [1, T, F] (no padding mask): the token list
    of the best hypothesis, leading blank included.

    The encoder runs through encode(); enc_proj = lin_enc(h) is one GEMM; the search itself
    (LSTM steps memoised by yseq, joint, log-softmax, top-10, the lists A / B with double
    scores, the pops) stays on the device: the launches of one frame are a hipGraph replayed
    T' times, and ONE device-to-host copy per utterance brings back the error flag, the best
    hypothesis and its tokens.  trace (a dict) receives "pops": [(yseq, score, |A|)] per
    expansion, and "steps": the LSTM steps actually executed (a device counter).  node_cap /
    slot_cap: capacities of the trie and of the state slots (default: the worst case
    100 T'cap + 1 / 10 T'cap + 1); running out raises after the utterance."""
    if beam != _BEAM:
        raise ValueError("transducer_beam_search: only the reference's beam of 10 is built")
    Tp = _sub_len(x.shape[1])
    if Tp <= 0:
        return [0]
    s, h = _rnnt_search_state(model, x, Tp, node_cap, slot_cap)
    g = s.frame_graph()
    s.start(model, h, Tp)
    for _ in range(Tp):
        g.replay()
    head = s.arena[: s.off["lists"]].cpu().numpy()  # ctrl, candidates, result tokens
    ctrl = head[:256].view(np.int32)
    if ctrl[_C_ERR] != 0:
        raise RuntimeError(f"transducer_beam_search: {_ERRORS.get(int(ctrl[_C_ERR]), 'error')} "
                           f"(node_cap {s.node_cap}, slot_cap {s.slot_cap}, T' {Tp})")
    assert ctrl[_C_DONE] == 1 and ctrl[_C_POPS] == _BEAM * Tp, ctrl[:16]
    n = int(ctrl[_C_BESTLEN])
    yseq = head[s.off["yseq"]: s.off["yseq"] + 4 * n].view(np.int32).tolist()
    if trace is not None:
        trace["pops"] = s.pops(_BEAM * Tp)
        trace["steps"] = int(ctrl[_C_STEPS])
        trace["score"] = float(ctrl[18:20].view(np.float64)[0]) / n
    return yseq


def _transducer_beam_search_hostloop(model, x, trace=None):
    """The same kernels driven one expansion at a time, with the reference's list logic in
    Python (one host round trip per expansion).  For tests and tools only: it is the
    exactness yardstick of the device-resident search, which must agree with it bit for bit.
    trace additionally receives "cand": per expansion the (log-probs, tokens) the device
    returned (10 best non-blank, then blank)."""
    Tp = _sub_len(x.shape[1])
    if Tp <= 0:
        return [0]
    s, h = _rnnt_search_state(model, x, Tp, None, None)
    s.start(model, h, Tp)
    ctrl = s.view("ctrl", torch.int32, 64)
    nodes = s.view("nodes", torch.int32, 4 * s.node_cap).view(-1, 4)
    cand = s.view("cand", torch.int32, 32)
    tab = [[-1, 0, 1, -1]]  # parent, token, len, slot
    child = {}
    seqs = {0: (0,)}
    kept, n_slots, steps, pops, cands = [(0, 0.0)], 0, 0, [], []
    for t in range(Tp):
        A, B = kept, []
        while len(B) < _BEAM:
            i = max(range(len(A)), key=lambda j: A[j][1])
            pops.append((seqs[A[i][0]], A[i][1], len(A)))
            node, score = A.pop(i)
            dostep = tab[node][3] < 0
            if dostep:
                tab[node][3] = n_slots
                n_slots += 1
                steps += 1
                nodes[node].copy_(torch.tensor(tab[node], dtype=torch.int32), non_blocking=False)
            ctrl[1:5].copy_(torch.tensor([_BEAM * t, Tp, node, int(dostep)], dtype=torch.int32))
            K.rnnt_search_expand(s.args, 1)
            c = cand.cpu().numpy()
            vals, toks = c[:16].view(np.float32), c[16:]
            cands.append((vals[:_BEAM + 1].copy(), toks[:_BEAM + 1].copy()))
            for j in range(_BEAM):
                k = (node, int(toks[j]))
                if k not in child:
                    child[k] = len(tab)
                    tab.append([node, k[1], tab[node][2] + 1, -1])
                    seqs[child[k]] = seqs[node] + (k[1],)
                A.append((child[k], score + float(vals[j])))
            B.append((node, score + float(vals[_BEAM])))
        kept = B
    norm = [sc / tab[n][2] for n, sc in kept]
    b = max(range(len(kept)), key=lambda j: norm[j])
    if int(ctrl[0].item()) != 0:
        raise RuntimeError("transducer hostloop: device error flag set")
    if trace is not None:
        trace["pops"], trace["steps"], trace["score"], trace["cand"] = pops, steps, norm[b], cands
    return list(seqs[kept[b][0]])
