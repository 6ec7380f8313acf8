"""The phased 128 x 64 GEMM kernel (csrc/gemm_phase.hip) against the kernels it replaces: every
output bit equal between lasr_gemm_phased(2) (forced) and lasr_gemm_phased(0) (never), over the
ring's empty, partial, exact and wrapped fills, ragged and single-row M, one and four column
tiles, both B layouts with their epilogues; and the launcher's routing at the step's two shapes.

The equality runs only screen the loop's wait / barrier placement (an early LDS read passes
most runs); the placement itself is argued from the counts in the header of gemm_phase.hip."""

import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

S = 6  # ring stages of the phased kernel (PH_S, gemm_phase.hip), 64 k each
KS = (64, 64 * (S - 1), 64 * S, 64 * (S + 1), 64 * (2 * S + 1), 2048)
MS = (1, 128, 129, 300)
REPEATS = 20
FORCE, NEVER, BY_SIZE = 2, 0, 1  # lasr_gemm_phased modes


_CTR = []  # the registered dropout step counter (kept alive: the library holds its address)


@pytest.fixture(autouse=True)
def dropout_counter():
    """The dropout epilogue reads the process-wide device step counter: register one of this
    module's own (an earlier test's model may have left the address of a freed tensor).  Not
    restored afterwards: the library keeps a bare address and has no getter, the address it held
    before may be dead, and every user of dropout registers its own counter before its calls;
    this one stays alive with the module."""
    from liteasr_amd import kernels as K

    if not _CTR:
        _CTR.append(torch.full((1,), 3, dtype=torch.int64, device="cuda"))
    K.set_dropout_counter(_CTR[0])


def _lib():
    from liteasr_amd import _native

    return _native.load()


def _launches():
    return _lib().lasr_gemm_phased_launches()


def _case(layout, M, N, Kd, gen):
    """Fresh random operands and the call of one case: (run, out)."""
    from liteasr_amd import kernels as K

    dev = "cuda"
    a = torch.randn(M, Kd, device=dev, generator=gen).bfloat16()
    if layout == "kc_res_drop":  # B K-contiguous, fp32 out, residual + dropout (FFN fc2 forward)
        w = (torch.randn(N, Kd, device=dev, generator=gen) * Kd ** -0.5).bfloat16()
        b = torch.randn(N, device=dev, generator=gen) * 0.02
        res = torch.randn(M, N, device=dev, generator=gen)
        out = torch.empty(M, N, device=dev)
        return (lambda: K.linear(a, w, out, bias=b, res=res, res_scale=0.5, drop_p=0.1, drop_seed=3)), out
    w = (torch.randn(Kd, N, device=dev, generator=gen) * Kd ** -0.5).bfloat16()  # B N-contiguous
    out = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
    return (lambda: K.gemm(a, w, out)), out  # bf16 out, plain epilogue (FFN fc1 input gradient)


@pytest.fixture(autouse=True)
def routing_restored():
    """Every test leaves the library routing by size, its default."""
    yield
    _lib().lasr_gemm_phased(BY_SIZE)


def _run(mode, run, out):
    """One call under lasr_gemm_phased(mode): (the output, launches routed to the phased kernel)."""
    assert _lib().lasr_gemm_phased(mode) == 0
    out.fill_(float("nan"))
    n0 = _launches()
    run()
    torch.cuda.synchronize()
    return out.clone(), _launches() - n0


@pytest.fixture
def unsplit(monkeypatch):
    """The small grids here would otherwise take kernels.gemm's automatic K split, which the
    phased kernel never runs: compare the unsplit launches."""
    from liteasr_amd import kernels as K

    monkeypatch.setattr(K, "SMALL_GRID_SPLIT", False)


@pytest.mark.parametrize("N", [64, 256])
@pytest.mark.parametrize("layout", ["kc_res_drop", "nc_plain"])
def test_phased_bit_identical(unsplit, layout, N):
    gen = torch.Generator(device="cuda").manual_seed(1234 + N)
    for M in MS:
        for Kd in KS:
            for rep in range(REPEATS):
                run, out = _case(layout, M, N, Kd, gen)
                new, n_new = _run(FORCE, run, out)
                old, n_old = _run(NEVER, run, out)
                assert (n_new, n_old) == (1, 0), (layout, M, N, Kd, rep, n_new, n_old)
                assert torch.equal(new, old), (layout, M, N, Kd, rep)


@pytest.mark.parametrize("N", [64, 256])
@pytest.mark.parametrize("layout", ["kc_res_drop", "nc_plain"])
def test_ragged_k_falls_back(unsplit, layout, N):
    """K = 2048 + 32 is no multiple of the 64-deep stage: the old kernel runs even under force."""
    gen = torch.Generator(device="cuda").manual_seed(99 + N)
    for M in MS:
        for rep in range(REPEATS):
            run, out = _case(layout, M, N, 2048 + 32, gen)
            new, n_new = _run(FORCE, run, out)
            old, n_old = _run(NEVER, run, out)
            assert (n_new, n_old) == (0, 0), (layout, M, N, rep)
            assert torch.equal(new, old), (layout, M, N, rep)


@pytest.mark.parametrize("layout", ["kc_res_drop", "nc_plain"])
def test_dispatch(layout):
    """Default routing: the encoder's (B T', d, ff) = (7968, 256, 2048) calls take the phased kernel
    (252 tiles of 128 x 64 on 256 CUs), the decoder's M = 1312 calls (44 tiles) do not -- seen
    through the launcher's counter of phased launches -- and the bits are the old kernel's."""
    gen = torch.Generator(device="cuda").manual_seed(7)
    _lib().lasr_gemm_phased(BY_SIZE)
    for M, want in ((7968, 1), (1312, 0)):
        run, out = _case(layout, M, 256, 2048, gen)
        n0 = _launches()
        run()
        torch.cuda.synchronize()
        assert _launches() - n0 == want, (layout, M)
        got = out.clone()
        old, n_old = _run(NEVER, run, out)
        _lib().lasr_gemm_phased(BY_SIZE)
        assert n_old == 0 and torch.equal(got, old), (layout, M)
