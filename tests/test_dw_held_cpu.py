"""Host-side order of the held weight-gradient GEMMs (kernels.deferred_reductions(hold=True),
kernels._Deferred.flush_held_gemms) with the native calls recorded: no GPU, no library call."""

import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@pytest.fixture
def rec(monkeypatch):
    """kernels with a fresh queue; every N.call is recorded as (name, problems, details)."""
    from liteasr_amd import kernels as K

    calls = []

    def call(name, *a):
        if name == "lasr_gemm_dw_group":
            arr, n = a[0], a[1]
            calls.append((name, [(arr[i].M, arr[i].N) for i in range(n)], [not arr[i].workspace for i in range(n)]))
        elif name == "lasr_reduce_multi":
            calls.append((name, a[1], None))
        else:
            calls.append((name, None, None))
        return 0

    monkeypatch.setattr(K.N, "call", call)
    monkeypatch.setattr(K, "stream", lambda: 0)
    monkeypatch.setattr(K, "_DEFER", K._Deferred())
    monkeypatch.setattr(K, "_PUSHED", {"lasr_gemm_dw_group_order": K.DW_GROUP_LPT})
    monkeypatch.setattr(K, "DW_HOLD_LAYERS", 0)  # (the hold-depth test sets its own)
    return K, calls


def _queue(K, key, M, Nn, sp=4, rowsum=False):
    """What kernels.gemm queues for a grouped dW GEMM inside a hold block: no slab yet."""
    a = K.N.GemmArgs()
    a.M, a.N, a.K, a.split_k, a.beta = M, Nn, 4096, -sp, 1.0
    c = torch.zeros(M, Nn)
    K._DEFER.waiting.append(K.QueuedGemm(key, a, K.Refs(None, None, c, torch.zeros(M) if rowsum else None)))


def test_held_gemms_launch_before_held_reductions_in_queue_order(rec):
    K, calls = rec
    events = []
    for layer, hold in ((3, True), (2, True), (1, False)):
        with K.deferred_reductions(hold=hold, on_done=lambda n=layer: events.append((n, len(calls)))):
            _queue(K, (128, 128), 2048 + layer, 256)  # (the widths tell the layers apart)
            _queue(K, (64, 64), 256 + layer, 256)
            K._defer(torch.zeros(8), 2, 4, torch.zeros(4))
        if hold:
            assert calls == [] and events == [] and K.held_reductions() > 0
    # 3 x 18 tiles of 256 x 128 and 3 x 20 of 64 x 64: both families below 256 tiles -> slabs,
    # whose 6 reductions (one per problem: no rowsum) join the 3 held ones
    assert [c[0] for c in calls] == ["lasr_gemm_dw_group", "lasr_gemm_dw_group", "lasr_reduce_multi"]
    assert calls[0][1] == [(2051, 256), (2050, 256), (2049, 256)] and calls[0][2] == [False] * 3
    assert calls[1][1] == [(259, 256), (258, 256), (257, 256)] and calls[1][2] == [False] * 3
    assert calls[2][1] == 3 + 6
    assert events == [(3, 3), (2, 3), (1, 3)]
    assert K.held_reductions() == 0 and not K._DEFER.gemms


def test_family_at_the_threshold_runs_serial_the_other_takes_slabs(rec, monkeypatch):
    K, calls = rec
    monkeypatch.setattr(K, "DW_SERIAL_MIN_TILES", 32)
    with K.deferred_reductions(hold=True):
        _queue(K, (128, 128), 2048, 256, rowsum=True)  # 16 tiles
        _queue(K, (64, 64), 256, 256)  # 16 tiles
    with K.deferred_reductions(hold=True):
        _queue(K, (128, 128), 256, 2048)  # 16 more: the family reaches 32
    assert K.held_reductions() == 3 and calls == []
    K.flush_reductions()
    assert calls[0] == ("lasr_gemm_dw_group", [(2048, 256), (256, 2048)], [True, True])
    assert calls[1] == ("lasr_gemm_dw_group", [(256, 256)], [False])
    assert calls[2] == ("lasr_reduce_multi", 1, None) and len(calls) == 3
    assert K.held_reductions() == 0


def test_a_short_launch_before_the_last_keeps_the_family_on_slabs(rec, monkeypatch):
    """Every serial launch of a family but its last fills the chip: a first chunk below the
    threshold (small problems, few per launch) sends the family down the slab path."""
    K, calls = rec
    monkeypatch.setattr(K, "DW_SERIAL_MIN_TILES", 32)
    monkeypatch.setattr(K, "_GROUP_MAX", 2)
    with K.deferred_reductions(hold=True):
        for _ in range(9):
            _queue(K, (64, 64), 128, 128)  # 4 tiles each: 36 in all, 8 per launch
    K.flush_reductions()
    assert [c[2] for c in calls[:5]] == [[False, False]] * 4 + [[False]]
    assert calls[5] == ("lasr_reduce_multi", 9, None)


def test_hold_depth_flushes_the_gemms_inside_a_segment(rec, monkeypatch):
    K, calls = rec
    monkeypatch.setattr(K, "DW_SERIAL_MIN_TILES", 1)
    monkeypatch.setattr(K, "DW_HOLD_LAYERS", 2)
    for i in range(3):
        with K.deferred_reductions(hold=True):
            _queue(K, (64, 64), 256, 256)
        assert len(calls) == (i + 1) // 2
    assert calls == [("lasr_gemm_dw_group", [(256, 256)] * 2, [True, True])] and K.held_reductions() == 1
    K.flush_reductions()
    assert calls[1] == ("lasr_gemm_dw_group", [(256, 256)], [True]) and K.held_reductions() == 0


def test_raising_hold_block_drops_its_gemms_and_nested_hold_still_raises(rec, monkeypatch):
    K, calls = rec
    monkeypatch.setattr(K, "DW_SERIAL_MIN_TILES", 1)
    with K.deferred_reductions(hold=True):
        _queue(K, (64, 64), 256, 256)
    with pytest.raises(ValueError):
        with K.deferred_reductions(hold=True):
            _queue(K, (64, 64), 512, 256)
            raise ValueError
    assert calls == [("lasr_gemm_dw_group", [(256, 256)], [True])]
    assert K.held_reductions() == 0 and not K._DEFER.gemms
    with K.deferred_reductions():
        with pytest.raises(RuntimeError, match="inside another deferred block"):
            with K.deferred_reductions(hold=True):
                pass
