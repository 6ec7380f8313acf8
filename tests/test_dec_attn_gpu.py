"""Plain (decoder) attention on the fused kernels -- lasr_attn_fwd / lasr_attn_bwd and their
key-split variants (csrc/attn_flash.hip, kernels.attn_fwd / attn_bwd) -- against the literal
fp64 chain of liteasr/nets/attention.py:46-59 on the same bf16-rounded operands:

    S = (Q K^T) * scale;  S.masked_fill(mask, -1e38);  P = softmax(S);  ctx = P V

with dq / dk / dv by autograd.  The reference uses plain torch ops on the CPU only.  Operands
sit in the model's layouts (q a column slice of a fused [B*Tq, 3d] buffer, k | v and dk | dv the
halves of [B*Tk, 2d] buffers, ctx / dctx with a padded row stride in some cases); everything
the kernels write is pre-filled with NaN, and what they must not touch has to stay NaN.

Bars: bf16 storage 2e-2 of the reference tensor's max (the project's bf16 bar, as
test_relattn_fused); fp32 storage (Dbuf) 1e-4; the row statistics' bar is LSE_BAR below."""

import functools
from types import SimpleNamespace as NS

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
NAN = float("nan")

# Row statistics, stats[:, 0] - log(stats[:, 1]) against the fp64 logsumexp of the masked scaled
# scores: the worst absolute error measured over every case, split count and input scale of
# test_attn_vs_fp64 was 6.7e-6 (the "self" case, peaked, where the lse itself reaches 36; the
# diffuse runs stay below 1.6e-7); the bar is 4x that (fp32 score accumulation and the
# summation order may differ between builds).  One dropped or duplicated key moves a diffuse
# row's lse by about 1 / Tk, so the bar has to stay below 1 / (4 Tk) of every diffuse case
# (asserted per case; the longest key run here is 330: 7.6e-4).
LSE_MEASURED = 6.7e-6
LSE_BAR = 4 * LSE_MEASURED  # 2.68e-5

# name -> B, H, Tq, Tk, d_k, mask kind, lens, pad columns of the ctx / dctx rows
CASES = {
    "min": ((2, 2, 1, 1, 64), "none", None, 0),
    "tq1": ((3, 2, 1, 70, 32), "pad", (70, 23, 0), 0),  # key tail of 6, one utterance fully masked
    "block": ((2, 2, 64, 64, 64), "none", None, 0),  # exactly one block each way
    "self": ((3, 4, 41, 41, 64), "causal", (41, 17, 1), 8),  # decoder self-attention
    "edge": ((2, 2, 65, 65, 32), "causal", (65, 64), 8),  # one live row in the 2nd query block
    "kb": ((2, 3, 70, 128, 64), "pad", (128, 65), 0),  # Tk a multiple of the key block, odd H
    "rand": ((2, 2, 130, 300, 32), "random", None, 0),  # Tk % 16 != 0 through pad_mask16
    "split": ((2, 2, 41, 249, 64), "pad", (249, 100), 8),  # a split fully masked for one utterance
    "uneven": ((1, 2, 17, 330, 32), "pad", (300,), 0),  # uneven split, one key block per split
}
RUNS = [(n, 1) for n in ("min", "tq1", "block", "self", "edge", "kb", "rand")]
RUNS += [("split", 1), ("split", 2), ("split", 4), ("uneven", 1), ("uneven", 3), ("uneven", 6)]
IN_SCALE = {"diffuse": 0.5, "peaked": 3.0}  # q, k ~ scale * randn; peaked: one or two keys carry each row


def K():
    from liteasr_amd import kernels

    return kernels


def close(got, ref, tol, what=""):
    got = got.float().cpu()
    ref = ref.float().cpu()
    scale = ref.abs().max().item() + 1e-12
    err = (got - ref).abs().max().item() / scale
    assert err <= tol, f"{what}: max err {err:.3e} > {tol:.1e} (scale {scale:.3e})"


@functools.lru_cache(maxsize=None)
def _inputs(name, kind):
    (B, H, Tq, Tk, dk), mkind, _, _ = CASES[name]
    g = torch.Generator().manual_seed(1000 * Tk + 10 * Tq + dk + len(kind))
    D = H * dk
    f = IN_SCALE[kind]
    zq, zk = torch.randn(B * Tq, D, generator=g), torch.randn(B * Tk, D, generator=g)
    if mkind == "causal" and kind == "peaked":
        # self-attention: a token's key is correlated with its own query (rho 0.5, still unit
        # variance), so the diagonal -- the key on the causal mask's edge, and for the last
        # row of a padded utterance the first padded one -- is among the keys that carry a row
        zk = 0.5 * zq + 0.75 ** 0.5 * zk
    return NS(q=(zq * f).to(BF),
              k=(zk * f).to(BF),
              v=(torch.randn(B * Tk, D, generator=g) * 0.5).to(BF),
              dctx=(torch.randn(B * Tq, D, generator=g) * 0.5).to(BF))


def _mask(name, perturb=None):
    """The case's mask as bool [B, Tq, Tk] (True = masked), optionally perturbed the way a
    wrong kernel would see it."""
    (B, H, Tq, Tk, dk), mkind, lens, _ = CASES[name]
    i, j = torch.arange(Tq)[None, :, None], torch.arange(Tk)[None, None, :]
    if mkind == "none":
        m = torch.zeros(B, Tq, Tk, dtype=torch.bool)
    elif mkind == "random":
        m = torch.rand(B, Tq, Tk, generator=torch.Generator().manual_seed(Tk)) < 0.3
        m[0, 7] = True  # one row ...
        m[1] = True  # ... and one utterance fully masked
    else:
        ln = torch.tensor(lens)[:, None, None] + (1 if perturb == "len+1" else 0)
        m = (j >= ln).expand(B, Tq, Tk).clone()
        if mkind == "causal":
            m |= (j >= i) if perturb == "causal>=" else (j > i)
    if perturb == "drop-last-key":
        live = ~m
        last = (live * torch.arange(1, Tk + 1)).amax(-1) - 1  # -1: no unmasked key
        bi, ii = torch.nonzero(last >= 0, as_tuple=True)
        m[bi, ii, last[bi, ii]] = True
    return m


def _reference(name, kind, perturb=None):
    (B, H, Tq, Tk, dk), _, _, _ = CASES[name]
    x = _inputs(name, kind)
    D = H * dk
    m = _mask(name, perturb)

    def heads(t, T):
        return t.double().view(B, T, H, dk).permute(0, 2, 1, 3).requires_grad_()

    Q, Kh, Vh = heads(x.q, Tq), heads(x.k, Tk), heads(x.v, Tk)
    S = (Q @ Kh.transpose(-1, -2)) * dk ** -0.5
    S = S.masked_fill(m[:, None], -1e38)
    P = torch.softmax(S, -1)
    ctx = (P @ Vh).permute(0, 2, 1, 3).reshape(B * Tq, D)
    dctx = x.dctx.double()
    dq, dkk, dv = torch.autograd.grad(ctx, (Q, Kh, Vh), dctx, retain_graph=True)
    if perturb == "last-row-twice":  # dk / dv as if the last live query row were summed twice
        d2 = dctx.clone().view(B, Tq, D)
        d2[:, Tq - 1] *= 2
        _, dkk, dv = torch.autograd.grad(ctx, (Q, Kh, Vh), d2.view(B * Tq, D))
    unh = lambda t, T: t.permute(0, 2, 1, 3).reshape(B * T, D)  # noqa: E731
    return NS(ctx=ctx.detach(), dq=unh(dq, Tq), dk=unh(dkk, Tk), dv=unh(dv, Tk),
              lse=torch.logsumexp(S.detach(), -1),  # [B, H, Tq]
              full=m.all(-1),  # [B, Tq] rows without an unmasked key
              keydead=m.all(1),  # [B, Tk] keys masked for every query of their utterance
              Tk=Tk)


_reference_cached = functools.lru_cache(maxsize=None)(_reference)


def _run(name, kind, nsplit):
    """The kernels on the case in the model's layouts; returns CPU tensors.  Asserts on the way
    that nothing outside the outputs' live regions was written."""
    kn = K()
    (B, H, Tq, Tk, dk), mkind, _, cpad = CASES[name]
    x = _inputs(name, kind)
    D, R = H * dk, B * Tq
    qkv = torch.full((R, 3 * D), NAN, dtype=BF, device=DEV)
    qkv[:, :D] = x.q.to(DEV)
    kv = torch.cat([x.k, x.v], 1).to(DEV)
    q, k, v = qkv[:, :D], kv[:, :D], kv[:, D:]
    m = _mask(name)
    if mkind == "none":
        mask, msb, msq = None, 0, 0
    elif mkind == "pad":  # key padding: one row per utterance
        mask, msb, msq = m[:, 0].to(torch.uint8).contiguous().to(DEV), Tk, 0
    else:  # query-dependent, rows of Tk bytes (re-laid out by kernels._fwd_mask when Tk % 16 != 0)
        mask, msb, msq = m.to(torch.uint8).contiguous().to(DEV), Tq * Tk, Tk
    scale = dk ** -0.5
    stats = torch.full((B * H * Tq * 2,), NAN, device=DEV)
    cbuf = torch.full((R, D + cpad), NAN, dtype=BF, device=DEV)
    dcbuf = torch.full((R, D + cpad), NAN, dtype=BF, device=DEV)
    dcbuf[:, :D] = x.dctx.to(DEV)
    ctx, dctx = cbuf[:, :D], dcbuf[:, :D]
    kn.attn_fwd(q, k, v, B, H, Tq, Tk, mask, msb, msq, scale, stats, ctx, nsplit=nsplit)
    Dbuf = torch.full((B * H * Tq,), NAN, device=DEV)
    dqkv = torch.full((R, 3 * D), NAN, dtype=BF, device=DEV)
    dkv = torch.full((B * Tk, 2 * D), NAN, dtype=BF, device=DEV)
    kn.attn_bwd(q, k, v, B, H, Tq, Tk, mask, msb, msq, scale, stats, ctx, dctx, Dbuf, dqkv[:, :D], dkv[:, :D],
                dkv[:, D:], nsplit=nsplit)
    torch.cuda.synchronize()
    assert cbuf[:, D:].isnan().all(), "ctx pad columns written"
    assert dqkv[:, D:].isnan().all(), "dq wrote outside its column slice"
    got = NS(ctx=ctx.float().cpu(), dq=dqkv[:, :D].float().cpu(), dk=dkv[:, :D].float().cpu(),
             dv=dkv[:, D:].float().cpu(), stats=stats.view(B, H, Tq, 2).cpu(), Dbuf=Dbuf.view(B, H, Tq).cpu(),
             dctx=x.dctx)
    for n in ("ctx", "dq", "dk", "dv", "stats", "Dbuf"):
        assert not getattr(got, n).isnan().any(), f"{n}: entries left unwritten (or NaN)"
    return got


def lse_error(got, ref):
    """Worst |stats[:, 0] - log(stats[:, 1]) - logsumexp| over the rows with an unmasked key."""
    live = ~ref.full[:, None, :].expand_as(ref.lse)
    if not live.any():
        return 0.0
    lse = got.stats[..., 0].double() - got.stats[..., 1].double().log()
    return (lse - ref.lse).abs()[live].max().item()


def compare(got, ref, what=""):
    """Every reference-backed assertion on one run of the kernels (the negative control feeds
    it perturbed references and expects it to raise)."""
    for n in ("ctx", "dq", "dk", "dv"):
        close(getattr(got, n), getattr(ref, n), 2e-2, f"{what} {n}")
    # keys masked for every query of their utterance (dk / dv rows) and fully masked query rows
    # (dq rows): the reference's values on those rows' own scale, and exact zeros where it has them
    for n, rows in (("dk", ref.keydead.reshape(-1)), ("dv", ref.keydead.reshape(-1)), ("dq", ref.full.reshape(-1))):
        g, r = getattr(got, n)[rows], getattr(ref, n)[rows]
        if r.numel() == 0:
            continue
        assert (g[r == 0] == 0).all(), f"{what} {n}: nonzero where the reference is exactly 0 (masked rows)"
        if r.abs().max() > 0:
            close(g, r, 2e-2, f"{what} {n} (masked rows)")
    # row statistics: rows with an unmasked key against the fp64 logsumexp ...
    err = lse_error(got, ref)
    assert err <= LSE_BAR, f"{what} lse: max abs err {err:.3e} > {LSE_BAR:.1e}"
    # ... fully masked rows keep the masked score as their max and attend uniformly over Tk keys
    dead = ref.full[:, None, :].expand_as(ref.lse)
    if dead.any():
        st = got.stats[dead]
        assert (st[:, 0] == torch.tensor(-1e38, dtype=torch.float32)).all(), f"{what}: max of a fully masked row"
        rel = (st[:, 1].double() * ref.Tk - 1).abs().max().item()
        assert rel <= 1e-6, f"{what}: 1/sum of a fully masked row off 1/Tk by {rel:.2e}"


@pytest.mark.parametrize("kind", ["diffuse", "peaked"])
@pytest.mark.parametrize("name,nsplit", RUNS, ids=[f"{n}-ns{s}" for n, s in RUNS])
def test_attn_vs_fp64(name, nsplit, kind):
    """ctx, dq, dk, dv, the row statistics and D of the one-pass and the key-split launches
    against the fp64 chain, at the sizes where the tiling can go wrong (64 queries per
    workgroup, 64 keys per block): Tq = 1 (63 of 64 query rows are clamped duplicates), one
    block exactly, one live row in a second query block with the mask edge on the block edge, a
    key tail, Tk a multiple of the block, d_k 32 and 64, masks with fully masked rows, keys and
    utterances, and splits whose whole key range is masked.

    Row statistics: the worst |lse error| measured over all of these runs is 6.7e-6 (peaked;
    1.6e-7 over the diffuse runs), the bar LSE_BAR = 4 x 6.7e-6 = 2.68e-5; in the diffuse runs
    the bar is below 1 / (4 Tk) (7.6e-4 at the longest key run, 330), asserted here."""
    (B, H, Tq, Tk, dk), _, _, _ = CASES[name]
    ref = _reference_cached(name, kind)
    got = _run(name, kind, nsplit)
    print(f"lse error {name} nsplit {nsplit} {kind}: {lse_error(got, ref):.3e} (bar {LSE_BAR:.2e})")
    if kind == "diffuse":
        assert LSE_BAR < 1 / (4 * Tk), "the lse bar cannot see one dropped key at this Tk"
    compare(got, ref, f"{name} nsplit {nsplit} {kind}")
    # D = per-head rowsum(dctx * ctx) over the stored (bf16) ctx, as the backward's preamble forms
    # it: fp32 storage, the kernel's own ctx
    Dref = (got.dctx.double() * got.ctx.double()).view(B, Tq, H, dk).sum(-1).permute(0, 2, 1)
    close(got.Dbuf, Dref, 1e-4, f"{name} nsplit {nsplit} {kind} D")


@pytest.mark.parametrize("name,kind", [("edge", "peaked"), ("tq1", "diffuse")])
def test_reference_perturbations_are_detected(name, kind):
    """Negative control, on the reference side only (no kernel is changed): the comparison that
    test_attn_vs_fp64 applies accepts the true reference and rejects each reference perturbed
    the way a subtly wrong kernel would be -- the last unmasked key of every row dropped, the
    padding lengths off by one, the last live query row summed twice into dk / dv, and (where
    the case has a causal mask) `>` for `>=` in it."""
    got = _run(name, kind, 1)
    compare(got, _reference_cached(name, kind), "unperturbed")
    perturbs = ["drop-last-key", "len+1", "last-row-twice"]
    if CASES[name][1] == "causal":
        perturbs.append("causal>=")
    for p in perturbs:
        with pytest.raises(AssertionError):
            compare(got, _reference(name, kind, p), p)
