"""Host-only launch trace of the deferred weight-gradient / reduction queue in kernels.py: the
real gemm(group=True), the fused-epilogue GEMMs and the backward wrappers run on small CPU tensors
under a fake N.call that records every native call in order.  The expected traces are literals:
they pin the launch order, the K slices, the slab / serial choice, which buffer the partial sums
go to and which form each kernel call takes.  No GPU, no library call."""

import os
import sys
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F32, BF16 = torch.float32, torch.bfloat16

# positions of the gradient-output pointers in the argument lists of the kernels that take them
_GRAD_OUTS = {"lasr_layernorm_bwd": (13, 14), "lasr_qbias_bwd": (9, 10), "lasr_glu_dwconv_bwd": (10, 11),
              "lasr_bn_act_glu_dwconv_bwd": (23, 24)}
# ... and of their partials buffer
_PART = {"lasr_layernorm_bwd": 15, "lasr_qbias_bwd": 11, "lasr_glu_dwconv_bwd": 12, "lasr_bn_act_glu_dwconv_bwd": 25}
_GEMM_FIRST = ("lasr_gemm", "lasr_gemm_ln_fwd", "lasr_gemm_ln_bwd", "lasr_gemm_qbias_bwd")


def _prime_pushed(monkeypatch, K):
    """The "last value pushed to the library" caches start primed: no setter call in the traces."""
    if hasattr(K, "_PUSHED"):
        monkeypatch.setattr(K, "_PUSHED", {"lasr_gemm_dw_group_order": K.DW_GROUP_LPT,
                                           "lasr_gemm_narrow_tiles": K.GEMM_NARROW_TILES})
    else:
        monkeypatch.setattr(K, "_dw_order_set", [K.DW_GROUP_LPT])
        monkeypatch.setattr(K, "_narrow_set", [K.GEMM_NARROW_TILES])


@pytest.fixture
def tr(monkeypatch):
    """kernels with an empty queue and a recording N.call; (K, calls)."""
    from liteasr_amd import kernels as K

    calls = []
    ws = torch.empty(64 * 2048 * 512 + 192 * 2048 + 4096, dtype=F32)  # (never touched: no pages)
    lo, hi = ws.data_ptr(), ws.data_ptr() + ws.numel() * 4

    def in_ws(p):
        return p is not None and lo <= p < hi

    def where(p):
        return "ws" if in_ws(p) else "own" if p else None

    def _prob(g):
        return (g.M, g.N, g.split_k, g.beta, where(g.workspace))

    def call(name, *a):
        if name == "lasr_gemm_plan":
            g = a[0]._obj
            big = g.M >= 1024 or g.N >= 1024
            a[1]._obj.value, a[2]._obj.value = (64, 128) if big else (64, 64)
            a[3]._obj.value = 8 if g.split_k == 0 else -g.split_k
            a[4]._obj.value = 3
        elif name == "lasr_gemm_dw_group":
            calls.append((name, [_prob(a[0][i]) for i in range(a[1])]))
        elif name == "lasr_reduce_multi":
            segs = [a[0][i] for i in range(a[1])]
            assert not any(in_ws(s.part) for s in segs), "a reduced partial lives in the workspace"
            calls.append((name, [(s.N, s.P, s.accumulate, s.split, bool(s.out1)) for s in segs]))
        elif name in _GEMM_FIRST:
            calls.append((name, _prob(a[0]._obj)))
        elif name == "lasr_linear_dx_ln_bwd":
            r = a[0]._obj
            calls.append((name, (not r.dgamma, not r.dbeta), where(r.part)))
        elif name == "lasr_layernorm2_bwd":  # (two partials buffers, no gradient outputs)
            calls.append((name, where(a[9]), where(a[15])))
        else:
            calls.append((name, tuple(a[i] is None for i in _GRAD_OUTS[name]), where(a[_PART[name]])))
        return 0

    monkeypatch.setattr(K.N, "call", call)
    monkeypatch.setattr(K, "stream", lambda: 0)
    monkeypatch.setattr(K, "dwconv_nparts", lambda B, T: 3)
    monkeypatch.setitem(K.WS.buf, None, ws)
    monkeypatch.setattr(K, "_DEFER", type(K._DEFER)())
    _prime_pushed(monkeypatch, K)
    return K, calls


def _dw(K, M, Nn, rows=512, rowsum=True, group=True):
    """One weight-gradient GEMM as the FFN backward issues it: dW[M, N] += dy^T x, db += colsum(dy)."""
    dy, x = torch.zeros(rows, M, dtype=BF16), torch.zeros(rows, Nn, dtype=BF16)
    K.gemm(dy.t(), x, torch.zeros(M, Nn), beta=1.0, split_k=0, rowsum=torch.zeros(M) if rowsum else None, group=group)


def _ln(K, rows=40, D=64):
    z, v = torch.zeros(rows, D), torch.zeros(D)
    K.layernorm_bwd(z, z, v, torch.zeros(rows), torch.zeros(rows), z.clone(), v.clone(), v.clone())


def _ln2(K, rows=40, D=64):
    z, v, r = torch.zeros(rows, D), torch.zeros(D), torch.zeros(rows)
    K.layernorm2_bwd(z, z, z, v, r, r, v.clone(), v.clone(), z, v, r, r, z.clone(), v.clone(), v.clone())


def _dx_ln(K, M=40, Kd=128, D=256):
    z, v, r = torch.zeros(M, D), torch.zeros(D), torch.zeros(M)
    K.linear_dx_ln_bwd(torch.zeros(M, Kd, dtype=BF16), torch.zeros(Kd, D, dtype=BF16), z, v, r, r, z.clone(),
                       v.clone(), v.clone())


def _qb_args(B=2, T=50, H=4, dk=8):
    D = H * dk
    dqkv = torch.zeros(B * T, 3 * D, dtype=BF16)
    return (torch.zeros(B * T, D, dtype=BF16), torch.zeros(B * T, D, dtype=BF16), B, T, H, dk, dqkv,
            torch.zeros(D), torch.zeros(D))


def _qbias(K):
    K.qbias_bwd(*_qb_args())


def _dwconv(K, B=2, T=30, Cc=16, Kw=5):
    K.glu_dwconv_bwd(torch.zeros(B * T, 2 * Cc), torch.zeros(B * T, Cc), B, T, Cc, Kw, torch.zeros(Cc, Kw),
                     torch.zeros(B * T, 2 * Cc), torch.zeros(Cc, Kw), torch.zeros(Cc))


def _bn_dwconv(K, B=2, T=30, Cc=16, Kw=5):
    y, v = torch.zeros(B * T, Cc), torch.zeros(Cc)
    K.bn_act_glu_dwconv_bwd(y, y, v, v, v, v, v, v.clone(), v.clone(), torch.zeros(B * T, 2 * Cc), B, T, Cc, Kw,
                            torch.zeros(Cc, Kw), torch.zeros(B * T, 2 * Cc), torch.zeros(Cc, Kw), torch.zeros(Cc))


def _gemm_ln_bwd(K, M=40, Kd=128, D=64):
    z, v, r = torch.zeros(M, D), torch.zeros(D), torch.zeros(M)
    q = SimpleNamespace(x=z, g=v, mean=r, rstd=r, dx=z.clone(), dgamma=v.clone(), dbeta=v.clone(), dres=None, gb=None,
                        bscale=1.0, bp=0.0, bseed=0)
    K.gemm(torch.zeros(M, Kd, dtype=BF16), torch.zeros(Kd, D, dtype=BF16), torch.zeros(M, D, dtype=BF16), ln_bwd=q)


def _gemm_qbias(K, T=50, H=4, dk=8):
    """The positional-projection gradient (batched over heads, split K) with qbias_bwd's blocks."""
    qb = _qb_args(T=T, H=H, dk=dk)
    K.gemm(torch.zeros(H, T, 100, dtype=BF16), torch.zeros(H, 100, dk, dtype=BF16), torch.zeros(H, T, dk, dtype=BF16),
           split_k=0, qbias=qb)


def _lone_dw(K):
    """A split-K weight gradient that does not group: partials deferred inside a block."""
    _dw(K, 256, 256, group=False)


SITES = {"layernorm_bwd": _ln, "layernorm2_bwd": _ln2, "linear_dx_ln_bwd": _dx_ln, "qbias_bwd": _qbias,
         "glu_dwconv_bwd": _dwconv, "bn_act_glu_dwconv_bwd": _bn_dwconv, "gemm(ln_bwd=)": _gemm_ln_bwd,
         "gemm(qbias=)": _gemm_qbias, "gemm(split_k=0)": _lone_dw}


# ------------------------------------------------------------------ scenarios ---
def lone_block(K, calls):
    with K.deferred_reductions():
        _dw(K, 256, 2048)
        _dw(K, 2048, 256)
        _ln(K)
        assert len(calls) == 1  # (the LayerNorm backward itself; the GEMMs wait for the block's end)


def _held_segment(K, calls, d, ff=2048):
    for i, hold in enumerate((True,) * 5 + (False,)):
        with K.deferred_reductions(hold=hold, on_done=lambda i=i: calls.append(("on_done", i))):
            _dw(K, d, ff)
            _ln(K)
            _dw(K, ff, d)


def hold_serial(K, calls):
    _held_segment(K, calls, 512)


def hold_slab(K, calls):
    _held_segment(K, calls, 256)


def raising_hold(K, calls):
    with K.deferred_reductions(hold=True, on_done=lambda: calls.append(("on_done", 0))):
        _dw(K, 512, 2048)
        _ln(K)
    with pytest.raises(ValueError):
        with K.deferred_reductions(hold=True, on_done=lambda: calls.append(("on_done", 1))):
            _dw(K, 2048, 512)
            _ln(K)
            raise ValueError


def ungrouped(K, calls):
    with K.deferred_reductions():
        _dw(K, 256, 2048)
        _dw(K, 2048, 256)
        _dw(K, 256, 256, rowsum=False)


# The recorded traces.  A GEMM problem is (M, N, split_k, beta, workspace: "ws" the shared one /
# "own" a buffer of its own / None); a reduction segment is (N, P, accumulate, split, has_out1);
# every other kernel call is (name, gradient outputs null?, partials buffer).
LN_SEG = (128, 3, 1, 64, True)  # _ln's gamma / beta partials
LN_CALL = ("lasr_layernorm_bwd", (True, True), "own")
DONE = [("on_done", i) for i in range(6)]
# dW + db segments of the 512 x 2048 / 2048 x 512 pair and of the 256 x 2048 / 2048 x 256 pair, 4 K slices
SEGS512 = [(1048576, 4, 1, 1048576, False), (512, 4, 1, 512, False), (1048576, 4, 1, 1048576, False),
           (2048, 4, 1, 2048, False)]
SEGS256 = [(524288, 4, 1, 524288, False), (256, 4, 1, 256, False), (524288, 4, 1, 524288, False),
           (2048, 4, 1, 2048, False)]

EXPECTED = {
    "lone_block": [
        LN_CALL,
        ("lasr_gemm_dw_group", [(256, 2048, -4, 1.0, "own"), (2048, 256, -4, 1.0, "own")]),
        ("lasr_reduce_multi", SEGS256 + [LN_SEG])],
    "hold_serial": [
        LN_CALL, LN_CALL, LN_CALL, LN_CALL,
        ("lasr_gemm_dw_group", [(512, 2048, -4, 1.0, None), (2048, 512, -4, 1.0, None)] * 4),
        LN_CALL, LN_CALL,
        ("lasr_gemm_dw_group", [(512, 2048, -4, 1.0, "own"), (2048, 512, -4, 1.0, "own")] * 2),
        ("lasr_reduce_multi", [LN_SEG] * 5 + SEGS512 * 2 + [LN_SEG])] + DONE,
    "hold_slab": [
        LN_CALL, LN_CALL, LN_CALL, LN_CALL,
        ("lasr_gemm_dw_group", [(256, 2048, -4, 1.0, "own"), (2048, 256, -4, 1.0, "own")] * 4),
        LN_CALL, LN_CALL,
        ("lasr_gemm_dw_group", [(256, 2048, -4, 1.0, "own"), (2048, 256, -4, 1.0, "own")] * 2),
        ("lasr_reduce_multi", [LN_SEG] * 4 + SEGS256 * 4 + [LN_SEG] + SEGS256 * 2 + [LN_SEG])] + DONE,
    "raising_hold": [
        LN_CALL, LN_CALL,
        ("lasr_gemm_dw_group", [(512, 2048, -4, 1.0, "own")]),
        ("lasr_reduce_multi", [LN_SEG, (1048576, 4, 1, 1048576, False), (512, 4, 1, 512, False), LN_SEG]),
        ("on_done", 0), ("on_done", 1)],
    "ungrouped": [
        ("lasr_gemm", (256, 2048, -8, 1.0, "own")),
        ("lasr_gemm", (2048, 256, -8, 1.0, "own")),
        ("lasr_gemm", (256, 256, -8, 1.0, "own")),
        ("lasr_reduce_multi", [(524288, 8, 1, 524288, False), (256, 8, 1, 256, False), (524288, 8, 1, 524288, False),
                               (2048, 8, 1, 2048, False), (65536, 8, 1, 65536, False)])],
    # per site: (outside a block, inside one, at the block's end)
    "sites": {
        "layernorm_bwd": ([("lasr_layernorm_bwd", (False, False), "ws")], [LN_CALL],
                          [("lasr_reduce_multi", [LN_SEG])]),
        "layernorm2_bwd": ([("lasr_layernorm2_bwd", "own", "own"), ("lasr_reduce_multi", [LN_SEG, LN_SEG])],
                           [("lasr_layernorm2_bwd", "own", "own")],
                           [("lasr_reduce_multi", [LN_SEG, LN_SEG])]),
        "linear_dx_ln_bwd": ([("lasr_linear_dx_ln_bwd", (False, False), "ws")],
                             [("lasr_linear_dx_ln_bwd", (True, True), "own")],
                             [("lasr_reduce_multi", [(512, 3, 1, 256, True)])]),
        "qbias_bwd": ([("lasr_qbias_bwd", (False, False), "ws")],
                      [("lasr_qbias_bwd", (True, True), "own")],
                      [("lasr_reduce_multi", [(64, 2, 1, 32, True)])]),
        "glu_dwconv_bwd": ([("lasr_glu_dwconv_bwd", (False, False), "ws")],
                           [("lasr_glu_dwconv_bwd", (True, True), "own")],
                           [("lasr_reduce_multi", [(96, 3, 1, 80, True)])]),
        "bn_act_glu_dwconv_bwd": ([("lasr_bn_act_glu_dwconv_bwd", (False, False), "ws")],
                                  [("lasr_bn_act_glu_dwconv_bwd", (True, True), "own")],
                                  [("lasr_reduce_multi", [(96, 3, 1, 80, True)])]),
        "gemm(ln_bwd=)": ([("lasr_gemm_ln_bwd", (40, 64, 1, 0.0, None)), ("lasr_reduce_multi", [LN_SEG])],
                          [("lasr_gemm_ln_bwd", (40, 64, 1, 0.0, None))],
                          [("lasr_reduce_multi", [LN_SEG])]),
        "gemm(qbias=)": ([("lasr_gemm_qbias_bwd", (50, 8, 0, 0.0, "ws")),
                          ("lasr_reduce_multi", [(64, 2, 1, 32, True)])],
                         [("lasr_gemm_qbias_bwd", (50, 8, 0, 0.0, "ws"))],
                         [("lasr_reduce_multi", [(64, 2, 1, 32, True)])]),
        "gemm(split_k=0)": ([("lasr_gemm", (256, 256, 0, 1.0, "ws"))],
                            [("lasr_gemm", (256, 256, -8, 1.0, "own"))],
                            [("lasr_reduce_multi", [(65536, 8, 1, 65536, False), (256, 8, 1, 256, False)])]),
    },
}


# ---------------------------------------------------------------------- tests ---
def test_lone_block_groups_with_slabs_then_one_reduction(tr):
    K, calls = tr
    lone_block(K, calls)
    assert calls == EXPECTED["lone_block"]
    assert [c[0] for c in calls] == ["lasr_layernorm_bwd", "lasr_gemm_dw_group", "lasr_reduce_multi"]
    assert all(p[4] for p in calls[1][1]) and len(calls[1][1]) == 2  # both problems have their slab
    assert calls[2][1][-1] == LN_SEG and len(calls[2][1]) == 5  # dW, db, dW, db, then the LayerNorm's
    assert K.held_reductions() == 0 and not K._DEFER.gemms and not K._DEFER.segs


def test_hold_reaches_the_serial_threshold_after_four_blocks(tr, monkeypatch):
    K, calls = tr
    monkeypatch.setattr(K, "DW_HOLD_LAYERS", 4)
    hold_serial(K, calls)
    assert calls == EXPECTED["hold_serial"]
    groups = [i for i, c in enumerate(calls) if c[0] == "lasr_gemm_dw_group"]
    # 4 LayerNorm backwards, then the slab-free serial launch of the 4 blocks' 8 problems (256 tiles)
    assert groups[0] == 4 and len(calls[4][1]) == 8 and not any(p[4] for p in calls[4][1])
    assert [c for c in calls if c[0] == "on_done"] == [("on_done", i) for i in range(6)]
    assert K.held_reductions() == 0 and not K._DEFER.gemms and not K._DEFER.segs


def test_hold_below_the_threshold_takes_slabs_at_the_flush(tr, monkeypatch):
    K, calls = tr
    monkeypatch.setattr(K, "DW_HOLD_LAYERS", 4)
    hold_slab(K, calls)
    assert calls == EXPECTED["hold_slab"]
    groups = [c for c in calls if c[0] == "lasr_gemm_dw_group"]
    assert [len(c[1]) for c in groups] == [8, 4] and all(p[4] for c in groups for p in c[1])  # slabs made there
    last_reduce = max(i for i, c in enumerate(calls) if c[0] == "lasr_reduce_multi")
    assert calls[last_reduce + 1:] == [("on_done", i) for i in range(6)]
    assert K.held_reductions() == 0 and not K._DEFER.gemms and not K._DEFER.segs


def test_raising_hold_block_drops_its_gemms_and_flushes_the_segments(tr):
    K, calls = tr
    raising_hold(K, calls)
    assert calls == EXPECTED["raising_hold"]
    groups = [c for c in calls if c[0] == "lasr_gemm_dw_group"]
    assert [[p[:2] for p in c[1]] for c in groups] == [[(512, 2048)]]  # the raising block's 2048 x 512 never launched
    assert K.held_reductions() == 0 and not K._DEFER.gemms and not K._DEFER.segs


@pytest.mark.parametrize("site", list(SITES))
def test_reduce_or_defer_site(tr, site):
    K, calls = tr
    SITES[site](K)
    outside = list(calls)
    del calls[:]
    with K.deferred_reductions():
        SITES[site](K)
        inside = list(calls)
    flushed = calls[len(inside):]
    assert (outside, inside, flushed) == EXPECTED["sites"][site]
    # outside a block: the three sites that own their partials reduce them at once, in one launch;
    # the other six hand the real outputs to the kernel and nothing follows
    n_imm = {"layernorm2_bwd": 2, "gemm(ln_bwd=)": 1, "gemm(qbias=)": 1}.get(site, 0)
    assert [c[0] for c in outside[1:]] == ["lasr_reduce_multi"] * bool(n_imm) and len(outside) == 1 + bool(n_imm)
    if n_imm:
        assert len(outside[1][1]) == n_imm
    takes_outputs = site in ("layernorm_bwd", "linear_dx_ln_bwd", "qbias_bwd", "glu_dwconv_bwd",
                             "bn_act_glu_dwconv_bwd")
    if takes_outputs:
        assert outside[0][1:] == ((False, False), "ws")
    # inside: one kernel call, no gradient outputs, its own partials buffer; the block's end reduces them
    assert len(inside) == 1 and [c[0] for c in flushed] == ["lasr_reduce_multi"]
    if takes_outputs:
        assert inside[0][1:] == ((True, True), "own")
    # (two norms; a weight gradient and its bias rowsum)
    assert len(flushed[0][1]) == (2 if site in ("layernorm2_bwd", "gemm(split_k=0)") else 1)


def test_dw_group_off_launches_lone_gemms_in_call_order(tr, monkeypatch):
    K, calls = tr
    monkeypatch.setattr(K, "DW_GROUP", False)
    ungrouped(K, calls)
    assert calls == EXPECTED["ungrouped"]
    assert [c[0] for c in calls] == ["lasr_gemm"] * 3 + ["lasr_reduce_multi"]
    assert [c[1][:2] for c in calls[:3]] == [(256, 2048), (2048, 256), (256, 256)]
