"""Held, serial-slice grouped weight gradients (kernels.DW_HOLD_GEMMS, lasr_gemm_dw_group's
serial problems): inside hold blocks the dW GEMMs wait for the flush of the held reductions,
and a family that fills the chip by then runs one block per output tile over the planned K
slices, writing the gradient itself.  Pinned bit for bit against the slab path (split-K slabs
+ lasr_reduce_multi) at the same slicing, and against float64 at the bars of
test_kernels_gpu.py::test_gemm_dw_group_bit_identical (1e-2 on dW, 1e-5 on db)."""

import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import u2_oracle as O  # noqa: E402

DEV = "cuda"
SHAPES = [(2048, 256), (256, 2048), (256, 256), (768, 256), (512, 256), (64, 192)]


def _close(got, ref, tol, what):
    scale = ref.abs().max().item() + 1e-12
    err = (got.double() - ref).abs().max().item() / scale
    assert err <= tol, f"{what}: max err {err:.3e} > {tol:.1e} (scale {scale:.3e})"


def _inputs(R, probs, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(R, M, generator=g).to(DEV, torch.bfloat16), torch.randn(R, N, generator=g).to(DEV, torch.bfloat16),
             torch.randn(M, N, generator=g).to(DEV), torch.randn(M, generator=g).to(DEV) if rs else None, beta)
            for M, N, rs, beta in probs]


def _run(kn, ins, blocks=1):
    """The problems queued in `blocks` hold blocks, then the flush; (dW, db) per problem and the
    lasr_gemm_dw_group launches as (problems, serial) pairs."""
    launches = []
    call = kn.N.call

    def rec(name, *a):
        if name == "lasr_gemm_dw_group":
            launches.append((a[1], not a[0][0].workspace))
        return call(name, *a)

    kn.N.call = rec
    try:
        res = []
        per = -(-len(ins) // blocks)
        for i in range(0, len(ins), per):
            with kn.deferred_reductions(hold=True):
                for dy, x, dw0, db0, beta in ins[i:i + per]:
                    dw = dw0.clone()
                    db = db0.clone() if db0 is not None else None
                    kn.gemm(dy.t(), x, dw, beta=beta, split_k=0, rowsum=db, group=True)
                    res.append((dw, db))
        kn.flush_reductions()
    finally:
        kn.N.call = call
    torch.cuda.synchronize()
    assert kn.held_reductions() == 0 and not kn._DEFER.gemms and not kn._DEFER.segs
    return res, launches


def _same(u, v):
    for (a, ab), (b, bb) in zip(u, v):
        assert torch.equal(a, b), (a - b).abs().max().item()
        assert (ab is None) == (bb is None)
        if ab is not None:
            assert torch.equal(ab, bb), (ab - bb).abs().max().item()


@pytest.mark.parametrize("R,gmax", [(333, 32), (256, 8), (1312, 8)])
def test_serial_slices_bit_identical_to_slabs(R, gmax, monkeypatch):
    """Every shape with and without the fused bias row sum, beta 0 and beta 1 on a non-zero dW0
    (24 problems in one queue: with 8 problems per launch the 64 x 64 family crosses the launch
    chunking).  R 333: a ragged last slice (no multiple of 64 or 4 x 64); 256: whole ring stages;
    1312: the decoder's row count.  serial == slabs made at the flush == slabs launched per block
    (today's path), bit for bit; all match float64."""
    from liteasr_amd import kernels as kn

    monkeypatch.setattr(kn, "_GROUP_MAX", gmax)
    probs = [(M, N, rs, beta) for M, N in SHAPES for rs in (True, False) for beta in (1.0, 0.0)]
    ins = _inputs(R, probs, seed=R)
    monkeypatch.setattr(kn, "DW_SERIAL_MIN_TILES", 1)
    serial, ls = _run(kn, ins)
    assert ls and all(s for _, s in ls), ls  # every family ran serial-slice
    assert max(n for n, _ in ls) <= gmax
    monkeypatch.setattr(kn, "DW_SERIAL_MIN_TILES", 1 << 30)
    late, ll = _run(kn, ins)
    assert ll and not any(s for _, s in ll), ll
    monkeypatch.setattr(kn, "DW_HOLD_GEMMS", False)
    slab, _ = _run(kn, ins)
    _same(serial, slab)
    _same(late, slab)
    for (dy, x, dw0, db0, beta), (dw, db) in zip(ins, serial):
        _close(dw, beta * dw0.double() + dy.double().t() @ x.double(), 1e-2, f"serial dW {tuple(dw.shape)}")
        if db0 is not None:
            _close(db, db0.double() + dy.double().sum(0), 1e-5, f"serial db {tuple(dw.shape)}")


def test_serial_queue_of_20_crosses_launch_chunking(monkeypatch):
    """20 problems of one family queued over 5 hold blocks: 3 launches at 8 problems each, 1 at
    the library's 32; both equal the slab path bit for bit."""
    from liteasr_amd import kernels as kn

    probs = [((256, 256), (512, 256), (768, 256), (64, 192))[i % 4] + (i % 3 != 0, float(i % 2)) for i in range(20)]
    ins = _inputs(333, probs, seed=20)
    monkeypatch.setattr(kn, "DW_SERIAL_MIN_TILES", 1)
    monkeypatch.setattr(kn, "DW_HOLD_LAYERS", 0)  # one flush, at the end
    one, l1 = _run(kn, ins, blocks=5)
    assert l1 == [(20, True)], l1
    monkeypatch.setattr(kn, "_GROUP_MAX", 8)
    three, l3 = _run(kn, ins, blocks=5)
    assert l3 == [(8, True), (8, True), (4, True)], l3
    monkeypatch.setattr(kn, "DW_HOLD_GEMMS", False)
    slab, _ = _run(kn, ins, blocks=5)
    _same(one, slab)
    _same(three, slab)


# ------------------------------------------------------------------ model level
@pytest.fixture(scope="module")
def model():
    """4 encoder layers + 1 decoder layer, d 256, bf16, dropout 0.1; B 4, T 1000, L 12 (the shape
    of test_fusions_gpu.py::test_layer_reductions_held_across_layers)."""
    from test_fusions_gpu import _model

    cfg = O.default_cfg(enc_dim=256, enc_heads=4, enc_layers=4, dec_dim=256, dec_heads=4, dec_layers=1)
    m, crit = _model(cfg)
    batch = [t.cuda() for t in O.synthetic_batch(4, 1000, 12, cfg["vocab_size"], seed=4)]
    return m, crit, batch


def _grad(model, cuts=None):
    """The flat gradient of one step from the same start (same dropout draws, zero gradients)."""
    from liteasr_amd import kernels as kn

    m, crit, batch = model
    m._drop_ctr.zero_()
    m.store.ensure_grad().zero_()
    if cuts is None:
        crit(m, *batch).backward()
    else:
        with m.segmented(cuts) as pairs:
            loss = crit(m, *batch)
        (_, x, leaf), = pairs
        (g,) = torch.autograd.grad(loss, [leaf])
        torch.autograd.backward(x, g)
    torch.cuda.synchronize()
    assert kn.held_reductions() == 0
    return m.store.grad.clone()


@pytest.fixture(scope="module")
def slab_grad(model):
    """The reference: the step with the GEMMs launched per layer node (holding of GEMMs off)."""
    from liteasr_amd import kernels as kn

    kn.DW_HOLD_GEMMS = False
    try:
        ref = _grad(model)
    finally:
        kn.DW_HOLD_GEMMS = True
    assert ref.abs().max().item() > 0
    return ref


@pytest.mark.parametrize("case", ["segment", "cut", "depth2", "product"])
def test_model_step_bit_identical(model, slab_grad, case, monkeypatch):
    """One bf16 step with every held family serial-slice (threshold 1) gives the slab step's flat
    gradient bit for bit: over the whole segment, with a segment cut below layer 2, and with the
    GEMM queue flushed every 2 layers; `product` is the module's own threshold and depth."""
    from liteasr_amd import kernels as kn

    if case != "product":
        monkeypatch.setattr(kn, "DW_SERIAL_MIN_TILES", 1)
        monkeypatch.setattr(kn, "DW_HOLD_LAYERS", 2 if case == "depth2" else 0)
    got = _grad(model, cuts=[2] if case == "cut" else None)
    assert torch.equal(got, slab_grad), (got - slab_grad).abs().max().item()


def test_raising_held_block_leaves_nothing_queued(model, slab_grad, monkeypatch):
    """A hold block that raises after queueing a GEMM drops it unlaunched (its output untouched)
    and flushes what earlier blocks left; the next step is bit-identical again."""
    from liteasr_amd import kernels as kn

    monkeypatch.setattr(kn, "DW_SERIAL_MIN_TILES", 1)
    (dy, x, dw0, _, _), = _inputs(333, [(256, 256, False, 1.0)], seed=7)
    kept, dropped = dw0.clone(), dw0.clone()
    with kn.deferred_reductions(hold=True):
        kn.gemm(dy.t(), x, kept, beta=1.0, split_k=0, group=True)
    assert kn.held_reductions() == 1
    with pytest.raises(ValueError):
        with kn.deferred_reductions(hold=True):
            kn.gemm(dy.t(), x, dropped, beta=1.0, split_k=0, group=True)
            raise ValueError
    torch.cuda.synchronize()
    assert kn.held_reductions() == 0 and not kn._DEFER.gemms and not kn._DEFER.segs
    assert torch.equal(dropped, dw0)
    _close(kept, dw0.double() + dy.double().t() @ x.double(), 1e-2, "kept dW")
    got = _grad(model)
    assert torch.equal(got, slab_grad)
