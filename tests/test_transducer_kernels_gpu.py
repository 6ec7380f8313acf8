"""The Transducer's elementwise kernels -- lasr_joint_fwd, lasr_joint_reduce,
lasr_lstm_cell_fwd, lasr_lstm_cell_bwd (csrc/rnnt.hip) -- and lasr_glancing_mix (csrc/cif.hip)
against plain fp64 torch restatements of the same ops, on the inputs as the kernels read them
(bf16-rounded where they read bf16), at the sizes where their launch geometry changes: the
blockIdx.y path of the reductions (J > 256), every T % 4 tail, the grid-stride wrap, every
dtype combination, every nullable argument present and absent, rows wider than their data.

Bars (derived, not measured): fp32 outputs 1e-4 of the reference tensor's max (the project's
fp32 bar); bf16 outputs elementwise |got - ref| <= 2^-8 |ref| + 1e-5 max|ref| -- one
round-to-nearest bf16 rounding is 2^-9 relative, doubled for an fp32 result that lands on the
other side of a rounding boundary.  Outputs are pre-filled with NaN; the padding between rows
has to stay NaN."""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF = torch.float32, torch.bfloat16
NAN = float("nan")


def K():
    from liteasr_amd import kernels

    return kernels


def check(got, ref, what=""):
    """got (fp32 or bf16 storage) against the fp64 ref at the storage type's bar."""
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    if got.numel() == 0:
        return
    g, r = got.double(), ref.double()
    assert torch.isfinite(g).all(), f"{what}: entries left unwritten, or not finite"
    top = r.abs().max()
    if got.dtype == BF:
        bound = r.abs() * 2.0 ** -8 + 1e-5 * top
        over = ((g - r).abs() - bound).max().item()
        assert over <= 0, f"{what}: bf16 bound exceeded by {over:.3e} (max |ref| {top.item():.3e})"
    else:
        err = ((g - r).abs().max() / (top + 1e-12)).item()
        assert err <= 1e-4, f"{what}: max err {err:.3e} > 1e-4 (scale {top.item():.3e})"


def padded(rows, cols, pad, dtype, fill=NAN):
    """A [rows, cols] view of a NaN-filled [rows, cols + pad] buffer: (view, buffer)."""
    buf = torch.full((rows, cols + pad), fill, dtype=dtype, device=DEV)
    return buf[:, :cols], buf


# --------------------------------------------------------------------------- joint
def _joint_ref(e, d, B, T, U1):
    J = e.shape[1]
    z = torch.tanh(e.double().view(B, T, 1, J) + d.double().view(U1, B, J).permute(1, 0, 2)[:, None])
    return z.reshape(B * T * U1, J)


@pytest.mark.parametrize("zdt", [F32, BF])
@pytest.mark.parametrize("B,T,U1,J", [(1, 1, 1, 8), (2, 5, 3, 24), (3, 7, 4, 264), (2, 6, 1, 512)])
def test_joint_fwd(B, T, U1, J, zdt):
    """z[(b T + t) U1 + u] = tanh(e[b T + t] + d[u B + b]): the prediction network's rows are
    time-major, the encoder's batch-major."""
    g = torch.Generator().manual_seed(J + T)
    e = (torch.randn(B * T, J, generator=g) * 1.5).to(DEV)
    d = (torch.randn(U1 * B, J, generator=g) * 1.5).to(DEV)
    z = torch.full((B * T * U1, J), NAN, dtype=zdt, device=DEV)
    K().joint_fwd(e, d, B, T, U1, z)
    check(z, _joint_ref(e, d, B, T, U1), "joint z")


def test_joint_fwd_grid_stride():
    """B T U1 J / 8 above 16384 blocks x 256 threads: the kernel's loop takes a second trip."""
    B, T, U1, J = 2, 64, 33, 8192
    assert B * T * U1 * J // 8 > 16384 * 256
    g = torch.Generator().manual_seed(5)
    e = torch.randn(B * T, J, generator=g).to(DEV)
    d = torch.randn(U1 * B, J, generator=g).to(DEV)
    z = torch.full((B * T * U1, J), NAN, dtype=BF, device=DEV)
    K().joint_fwd(e, d, B, T, U1, z)
    check(z, _joint_ref(e, d, B, T, U1), "joint z (grid stride)")


def test_joint_fwd_refuses_bad_width():
    """J % 8 != 0 is refused with an error, not computed."""
    from liteasr_amd._native import NativeError

    e = torch.zeros(2, 12, device=DEV)
    d = torch.zeros(2, 12, device=DEV)
    z = torch.full((4, 12), NAN, device=DEV)
    with pytest.raises(NativeError, match="lasr_joint_fwd: bad sizes"):
        K().joint_fwd(e, d, 1, 2, 2, z)
    assert z.isnan().all()


def _reduce_cases():
    """T x J crossed, twice: every T % 4 tail and T < 4 at every J (8, 24: one partial block;
    264, 520: the blockIdx.y path with a partial last block), the (dz, out) dtype pairs and
    (U1, B) rotating so that each appears with every T and every J."""
    pairs = [(F32, F32), (F32, BF), (BF, F32), (BF, BF)]
    ub = [(1, 1), (4, 3), (1, 3), (4, 1)]
    cases = []
    for ti, T in enumerate([1, 3, 4, 5, 7, 8]):
        for ji, J in enumerate([8, 24, 264, 520]):
            for rep in (0, 2):
                (U1, B), (zdt, odt) = ub[(ti + ji + rep) % 4], pairs[(ti + 2 * ji + rep + rep // 2) % 4]
                cases.append(pytest.param(B, T, U1, J, zdt, odt,
                                          id=f"B{B}-T{T}-U{U1}-J{J}-{str(zdt)[6:]}-{str(odt)[6:]}"))
    return cases


@pytest.mark.parametrize("B,T,U1,J,zdt,odt", _reduce_cases())
def test_joint_reduce(B, T, U1, J, zdt, odt):
    """de = sum_u dz, dd[u B + b] = sum_t dz; each t-slice has its own magnitude, so a tail
    element added to the wrong accumulator (or twice, or not at all) is visible."""
    g = torch.Generator().manual_seed(100 * T + J + U1)
    dz4 = torch.randn(B, T, U1, J, generator=g) * torch.arange(1, T + 1).view(1, T, 1, 1)
    dz = dz4.to(zdt).to(DEV).view(B * T * U1, J)
    de = torch.full((B * T, J), NAN, dtype=odt, device=DEV)
    dd = torch.full((U1 * B, J), NAN, dtype=odt, device=DEV)
    K().joint_reduce(dz, B, T, U1, de, dd)
    r = dz.double().view(B, T, U1, J)
    check(de, r.sum(2).reshape(B * T, J), "de")
    check(dd, r.sum(1).permute(1, 0, 2).reshape(U1 * B, J), "dd")


# ----------------------------------------------------------------------- LSTM cell
def _lstm_ref(gates, bias, c_prev, dh, dc_next):
    """fp64 cell with gate order i | f | g | o and, by autograd of <h, dh> + <c, dc_next>, the
    gradients of the pre-activation gates and of c_prev."""
    G = gates.double()
    if bias is not None:
        G = G + bias.double()
    G.requires_grad_()
    cp = (c_prev.double() if c_prev is not None else torch.zeros_like(G[:, : G.shape[1] // 4])).requires_grad_()
    i, f, gg, o = G.chunk(4, 1)
    c = torch.sigmoid(f) * cp + torch.sigmoid(i) * torch.tanh(gg)
    h = torch.sigmoid(o) * torch.tanh(c)
    out = dict(c=c.detach(), h=h.detach())
    if dh is not None:
        loss = (h * dh).sum()
        if dc_next is not None:
            loss = loss + (c * dc_next.double()).sum()
        out["dgates"], out["dc_prev"] = torch.autograd.grad(loss, (G, cp))
    return out


# row padding of gates / h_out (and dh_out) / dgates, the three storage types, the nullables
LSTM_VARIANTS = {
    "plain": dict(pg=0, ph=0, pd=0, hdt=F32, dhdt=F32, gdt=F32,
                  absent=()),
    "padded-bf16": dict(pg=12, ph=5, pd=4, hdt=BF, dhdt=BF, gdt=BF,
                        absent=()),
    "first-step": dict(pg=12, ph=0, pd=4, hdt=F32, dhdt=BF, gdt=F32,
                       absent=("bias", "c_prev", "dh_rec", "dc_next", "dc_prev")),
    "rec-only": dict(pg=0, ph=5, pd=0, hdt=BF, dhdt=F32, gdt=BF,
                     absent=("dh_out",)),
}


def _lstm_case(B, H, variant, gate_scale=2.0, clamp=None):
    kn = K()
    v = LSTM_VARIANTS[variant]
    has = lambda n: n not in v["absent"]  # noqa: E731
    g = torch.Generator().manual_seed(B * 1000 + H)
    rnd = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    gv = rnd(B, 4 * H) * gate_scale
    if clamp is not None:
        gv = gv.clamp(-clamp, clamp)
        gv.view(-1)[::7] = clamp  # some pre-activations exactly at the ends of the range
        gv.view(-1)[3::11] = -clamp
    gates, _ = padded(B, 4 * H, v["pg"], F32)
    gates.copy_(gv)
    bias = (rnd(4 * H) * 0.5).to(DEV) if has("bias") else None
    c_prev = rnd(B, H).to(DEV) if has("c_prev") else None
    c_out = torch.full((B, H), NAN, device=DEV)
    h_out, hbuf = padded(B, H, v["ph"], v["hdt"])
    kn.lstm_cell_fwd(gates, bias, c_prev, c_out, h_out)

    dh_out = None
    if has("dh_out"):
        dh_out, _ = padded(B, H, v["ph"], v["dhdt"])
        dh_out.copy_(rnd(B, H))
    dh_rec = rnd(B, H).to(DEV) if has("dh_rec") else None
    dc_next = rnd(B, H).to(DEV) if has("dc_next") else None
    dgates, dgbuf = padded(B, 4 * H, v["pd"], v["gdt"])
    dc_prev = torch.full((B, H), NAN, device=DEV) if has("dc_prev") else None
    kn.lstm_cell_bwd(gates, bias, c_out, c_prev, dh_out, dh_rec, dc_next, dgates, dc_prev)
    torch.cuda.synchronize()

    dh = sum(t.double() for t in (dh_out, dh_rec) if t is not None)
    ref = _lstm_ref(gates, bias, c_prev, dh, dc_next)
    what = f"lstm {B}x{H} {variant}"
    check(c_out, ref["c"], f"{what} c")
    check(h_out, ref["h"], f"{what} h")
    check(dgates, ref["dgates"], f"{what} dgates")
    if dc_prev is not None:
        check(dc_prev, ref["dc_prev"], f"{what} dc_prev")
    assert hbuf[:, H:].isnan().all(), f"{what}: h_out row padding written"
    assert dgbuf[:, 4 * H:].isnan().all(), f"{what}: dgates row padding written"


@pytest.mark.parametrize("variant", list(LSTM_VARIANTS))
@pytest.mark.parametrize("B,H", [(1, 1), (3, 7), (5, 48), (2, 300)])
def test_lstm_cell(B, H, variant):
    """lasr_lstm_cell_fwd / _bwd: c = sigm(f) c_prev + sigm(i) tanh(g), h = sigm(o) tanh(c) and
    the pre-activation gradients, with row strides wider than the rows (ldg 4H + 12, ldh H + 5,
    lddg 4H + 4), h_out / dh_out / dgates in fp32 and bf16, and each of bias, c_prev, dh_out,
    dh_rec, dc_next, dc_prev present and absent."""
    _lstm_case(B, H, variant)


@pytest.mark.parametrize("variant", ["plain", "padded-bf16"])
def test_lstm_cell_saturated(variant):
    """Gate pre-activations out to +-90 (exp(90) overflows fp32: the fast-exp sigmoid has to
    saturate to 0 / 1, not to NaN); outputs finite (check() asserts it) and on the reference."""
    _lstm_case(5, 48, variant, gate_scale=30.0, clamp=90.0)


def test_lstm_cell_vs_torch_lstmcell():
    """The kernel on fp64-matmul gates against torch.nn.LSTMCell (fp64) with the same weights:
    pins the chunk order i | f | g | o to torch's.  b_hh goes in through the bias argument."""
    B, I, H = 3, 5, 7
    torch.manual_seed(11)
    cell = torch.nn.LSTMCell(I, H).double()
    x, h0, c0 = torch.randn(B, I).double(), torch.randn(B, H).double(), torch.randn(B, H).double()
    with torch.no_grad():
        h1, c1 = cell(x, (h0, c0))
        gates = x @ cell.weight_ih.T + cell.bias_ih + h0 @ cell.weight_hh.T
    c_out = torch.full((B, H), NAN, device=DEV)
    h_out = torch.full((B, H), NAN, device=DEV)
    K().lstm_cell_fwd(gates.float().to(DEV), cell.bias_hh.detach().float().to(DEV), c0.float().to(DEV), c_out, h_out)
    check(h_out, h1.to(DEV), "h vs LSTMCell")
    check(c_out, c1.to(DEV), "c vs LSTMCell")


def test_lstm_cell_fwd_grid_stride():
    """B H above 16384 blocks x 256 threads: the forward's loop takes a second trip."""
    B, H = 2100, 2048
    assert B * H > 16384 * 256
    g = torch.Generator().manual_seed(3)
    gates = (torch.randn(B, 4 * H, generator=g) * 2).to(DEV)
    c_prev = torch.randn(B, H, generator=g).to(DEV)
    c_out = torch.full((B, H), NAN, device=DEV)
    h_out = torch.full((B, H), NAN, dtype=BF, device=DEV)
    K().lstm_cell_fwd(gates, None, c_prev, c_out, h_out)
    ref = _lstm_ref(gates, None, c_prev, None, None)
    check(c_out, ref["c"], "c (grid stride)")
    check(h_out, ref["h"], "h (grid stride)")


# ------------------------------------------------------------------- glancing mix
@pytest.mark.parametrize("rows,D", [(0, 24), (1, 1), (37, 24), (2049, 512)])
def test_glancing_mix(rows, D):
    """out = replace ? a : b and its two branch gradients, bit for bit; 2049 x 512 is above
    the 4096-block grid (a second trip of the loop), rows = 0 is a no-op, not an error."""
    kn = K()
    g = torch.Generator().manual_seed(rows + D)
    rep = (torch.rand(rows, generator=g) < 0.4).to(torch.uint8).to(DEV)
    a = torch.randn(rows, D, generator=g).to(DEV)
    b = torch.randn(rows, D, generator=g).to(DEV)
    r = rep.bool()[:, None]
    out = torch.full((rows, D), NAN, device=DEV)
    kn.glancing_mix(rep, a, b, out)
    assert torch.equal(out, torch.where(r, a, b))
    g_emb = torch.full((rows, D), NAN, device=DEV)
    g_cif = torch.full((rows, D), NAN, device=DEV)
    kn.glancing_mix(rep, a, None, g_emb, g_cif, backward=True)
    zero = torch.zeros_like(a)
    assert torch.equal(g_emb, torch.where(r, a, zero))
    assert torch.equal(g_cif, torch.where(r, zero, a))
