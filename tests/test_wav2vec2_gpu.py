"""wav2vec 2.0 on the GPU: each kernel group of csrc/w2v.hip (through its stage in
liteasr_amd/nets/wav2vec2.py) against the fp64 restatement (tests/wav2vec2_ref.py), and the whole
model against the reference's own run (tests/golden/wav2vec2.npz).

Bars (error = max |difference| / max |reference| per tensor):
  fp32 build  1e-3, the bar of tests/test_model_gpu.py's fp32 parity.
  bf16 build  1e-2 per stage on bf16-representable inputs, the project's node bar
              (tests/test_nodes_gpu.py).  The other candidate, twice the error of fp32 torch against
              fp64 on the same tensors, is of the order 1e-6 and never the larger of the two.
W2V_PARITY_OUT=<file> appends every measured error as a JSON line (profiles/wav2vec2_parity.jsonl
was written that way).  A key projection's bias gradient is exactly zero in exact arithmetic and
is measured on the scale of the query bias's (wav2vec2_cases.grad_errors).
"""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import wav2vec2_cases as C
import wav2vec2_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
BAR = {"fp32": 1e-3, "bf16": 1e-2}
ADT = {"fp32": F32, "bf16": BF16}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_STEP_COUNTER = [None]


def _check(name, dtype, errs):
    out = os.environ.get("W2V_PARITY_OUT")
    if out:
        with open(out, "a") as fh:
            fh.write(json.dumps({"case": name, "build": dtype, "bar": BAR[dtype],
                                 "err": {k: float(f"{v:.3e}") for k, v in errs.items()}}) + "\n")
    print(name, dtype, {k: f"{v:.2e}" for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if not v <= BAR[dtype]}
    assert not bad, (name, dtype, bad)


def _rep(t, dtype):
    """fp32 tensor, rounded to bf16-representable values for the bf16 build."""
    return t.bfloat16().float() if dtype == "bf16" else t


def _leaf(t):
    return t.double().clone().requires_grad_()


# ------------------------------------------------------------------ extractor
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("C_,k,s,Tin,B", [(32, 3, 2, 399, 3), (48, 2, 2, 199, 2)])
def test_extractor_layer(C_, k, s, Tin, B, dtype):
    """An odd input length that drops a tail sample, T_out no multiple of 64 (LN + GELU blocks
    with a ragged tail), C 48 no tile multiple, k 3 > s 2: overlapping rows in the input gradient."""
    from liteasr_amd.nets import wav2vec2 as WN

    g = torch.Generator().manual_seed(300 + C_)
    a = _rep(torch.randn(B, Tin, C_, generator=g), dtype)
    W = _rep(torch.randn(C_, C_, k, generator=g) * (C_ * k) ** -0.5, dtype)
    gam, bet = 1 + 0.1 * torch.randn(C_, generator=g), 0.1 * torch.randn(C_, generator=g)
    Tout = (Tin - k) // s + 1
    dy = torch.randn(B, Tout, C_, generator=g)
    la, lW, lg, lb = _leaf(a), _leaf(W), _leaf(gam), _leaf(bet)
    y_r = R.ext_layer(la, lW, None, lg, lb, k, s)
    (y_r * dy.double()).sum().backward()

    adt = ADT[dtype]
    Wk = W.permute(0, 2, 1).contiguous().view(C_, k * C_).to(DEV, adt)
    gd, bd = gam.to(DEV), bet.to(DEV)
    y, sv = WN.ext_layer_fwd(a.to(DEV, adt), Wk, None, gd, bd, k, s, adt)
    gW = torch.zeros(C_, k * C_, device=DEV)
    gg, gb = torch.zeros(C_, device=DEV), torch.zeros(C_, device=DEV)
    da = WN.ext_layer_bwd(dy.to(DEV), sv, Wk, gd, bd, k, s, adt, gW, None, gg, gb)
    torch.cuda.synchronize()
    assert y.shape == (B, Tout, C_) and da.shape == a.shape
    _check(f"ext_layer C{C_} k{k} s{s} T{Tin}", dtype, {
        "y": C.rel_max(y.float().cpu(), y_r.detach()), "da": C.rel_max(da.cpu(), la.grad),
        "dW": C.rel_max(gW.view(C_, k, C_).permute(0, 2, 1).cpu(), lW.grad),
        "dgamma": C.rel_max(gg.cpu(), lg.grad), "dbeta": C.rel_max(gb.cpu(), lb.grad)})


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_extractor_layer0(dtype):
    """C_in 1, k 10, s 5 on 4000 samples (799 frames): the direct kernel and its weight gradient."""
    from liteasr_amd.nets import wav2vec2 as WN

    g = torch.Generator().manual_seed(310)
    x = torch.randn(3, 4000, generator=g)
    W = torch.randn(32, 1, 10, generator=g) * 10 ** -0.5
    gam, bet = 1 + 0.1 * torch.randn(32, generator=g), 0.1 * torch.randn(32, generator=g)
    dy = torch.randn(3, 799, 32, generator=g)
    lW, lg, lb = _leaf(W), _leaf(gam), _leaf(bet)
    y_r = R.ext_layer(x.double().unsqueeze(-1), lW, None, lg, lb, 10, 5)
    (y_r * dy.double()).sum().backward()
    adt = ADT[dtype]
    Wd, gd, bd = W.view(32, 10).to(DEV), gam.to(DEV), bet.to(DEV)
    y, sv = WN.ext_layer_fwd(x.to(DEV), Wd, None, gd, bd, 10, 5, adt)
    gW, gg, gb = torch.zeros(32, 10, device=DEV), torch.zeros(32, device=DEV), torch.zeros(32, device=DEV)
    assert WN.ext_layer_bwd(dy.to(DEV), sv, Wd, gd, bd, 10, 5, adt, gW, None, gg, gb) is None
    torch.cuda.synchronize()
    _check("ext_layer0", dtype, {"y": C.rel_max(y.float().cpu(), y_r.detach()),
                                 "dW": C.rel_max(gW.view(32, 1, 10).cpu(), lW.grad),
                                 "dgamma": C.rel_max(gg.cpu(), lg.grad), "dbeta": C.rel_max(gb.cpu(), lb.grad)})


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_layernorm_width_768(dtype):
    """The BASE model's width on the library LayerNorm (12 values per lane, the one width that is
    no power of two): forward, and the backward with a residual gradient added, 37 rows."""
    from liteasr_amd import kernels as K

    rows, D = 37, 768
    g = torch.Generator().manual_seed(315)
    x = _rep(torch.randn(rows, D, generator=g), dtype)
    gam, bet = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    dy, dres = _rep(torch.randn(rows, D, generator=g), dtype), torch.randn(rows, D, generator=g)
    lx, lg, lb = _leaf(x), _leaf(gam), _leaf(bet)
    y_r = R.layer_norm(lx, lg, lb, R.LN_EPS)
    (y_r * dy.double()).sum().backward()
    adt = ADT[dtype]
    xd, gd, bd = x.to(DEV, adt), gam.to(DEV), bet.to(DEV)
    y = torch.empty(rows, D, dtype=adt, device=DEV)
    mean, rstd = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    K.layernorm_fwd(xd, gd, bd, R.LN_EPS, y, mean, rstd)
    dx, gg, gb = torch.empty(rows, D, device=DEV), torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    K.layernorm_bwd(xd, dy.to(DEV, adt), gd, mean, rstd, dx, gg, gb, dres=dres.to(DEV))
    torch.cuda.synchronize()
    _check("layernorm D768", dtype, {"y": C.rel_max(y.float().cpu(), y_r.detach()),
                                     "dx": C.rel_max(dx.cpu(), lx.grad + dres.double()),
                                     "dgamma": C.rel_max(gg.cpu(), lg.grad), "dbeta": C.rel_max(gb.cpu(), lb.grad)})


# --------------------------------------------------------- positional convolution
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("T", [99, 130])
def test_positional_convolution(T, dtype):
    """d 64 (4 channels per group) at T' 99 < the kernel width and T' 130 > it."""
    from liteasr_amd.nets import wav2vec2 as WN

    B, d = 2, 64
    g = torch.Generator().manual_seed(320 + T)
    x = _rep(torch.randn(B, T, d, generator=g), dtype)
    W = _rep(torch.randn(d, d // 16, 128, generator=g) * (4 * 128) ** -0.5, dtype)
    bias = 0.1 * torch.randn(d, generator=g)
    dout = torch.randn(B, T, d, generator=g)
    lx, lW, lb = _leaf(x), _leaf(W), _leaf(bias)
    y_r = R.posconv(lx, lW, lb)
    # the restatement drops the convolution's last (T + 1-th) frame, as Conv1d(...)[:, :, :-1] does
    full = torch.nn.functional.conv1d(x.double().transpose(1, 2), W.double(), bias.double(), padding=64, groups=16)
    assert full.shape[-1] == T + 1
    assert C.rel_max(y_r.detach(), x.double() + R.gelu(full[:, :, :-1].transpose(1, 2))) < 1e-12
    (y_r * dout.double()).sum().backward()
    adt = ADT[dtype]
    Wd, bd = W.to(DEV), bias.to(DEV)
    y, sv = WN.posconv_fwd(x.to(DEV), Wd, bd, adt)
    gW, gb = torch.zeros(d, d // 16, 128, device=DEV), torch.zeros(d, device=DEV)
    dx = WN.posconv_bwd(dout.to(DEV), sv, Wd, bd, adt, gW, gb)
    torch.cuda.synchronize()
    _check(f"posconv T{T}", dtype, {"y": C.rel_max(y.cpu(), y_r.detach()), "dx": C.rel_max(dx.cpu(), lx.grad),
                                    "dW": C.rel_max(gW.cpu(), lW.grad), "dbias": C.rel_max(gb.cpu(), lb.grad)})


# -------------------------------------------------------------- mask and gather
def test_mask_and_gather():
    """M 7 with a masked row at frame 0 and at frame T' - 1."""
    from liteasr_amd import kernels as K

    B, T, M, d = 2, 12, 7, 64
    g = torch.Generator().manual_seed(330)
    x = torch.randn(B, T, d, generator=g)
    emb = torch.rand(d, generator=g)
    idx = torch.tensor([[0, 2, 3, 4, 7, 8, 11], [0, 1, 5, 6, 9, 10, 11]])
    mask = torch.zeros(B, T, dtype=torch.bool)
    mask.scatter_(1, idx, True)
    midx = idx.int().to(DEV)
    xd = x.to(DEV).clone()
    K.w2v_mask_fwd(xd, midx, emb.to(DEV))
    assert torch.equal(xd.cpu(), R.mask_rows(x, mask, emb))
    dx = torch.randn(B, T, d, generator=g)
    dxd, demb = dx.to(DEV).clone(), torch.zeros(d, device=DEV)
    K.w2v_mask_bwd(dxd, midx, demb)
    assert torch.equal(dxd.cpu(), dx.masked_fill(mask.unsqueeze(-1), 0.0))
    assert C.rel_max(demb.cpu(), dx.double()[mask].sum(0)) < 1e-6
    for tm in (False, True):
        src = x.transpose(0, 1).contiguous() if tm else x
        out = torch.empty(B, M, d, device=DEV)
        K.w2v_gather_rows(src.to(DEV), midx, out, time_major=tm)
        assert torch.equal(out.cpu(), R.gather_masked(x, mask))
        back = torch.zeros(src.shape, device=DEV)
        K.w2v_scatter_rows(out, midx, back, time_major=tm)
        want = x.masked_fill(~mask.unsqueeze(-1), 0.0)
        assert torch.equal(back.cpu(), want.transpose(0, 1).contiguous() if tm else want)
    torch.cuda.synchronize()


# ------------------------------------------------------------------- quantizer
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("name", sorted(C.QUANT_CASES))
def test_quantizer(name, train):
    """297 rows, (G 2, V 16) and (G 2, V 320: no power of two, wider than a block).  Codes equal
    the restatement's exactly outside the near-tie rows (at most 1 %, tests/test_wav2vec2_cpu.py);
    those rows' upstream gradient is zeroed on both sides so they stay out of dvars."""
    from liteasr_amd import kernels as K

    logits, noise, vars_, dout = C.quant_case(name)
    G, V, vd, _ = C.QUANT_CASES[name]
    Rr = logits.shape[0]
    ll, lv = _leaf(logits), _leaf(vars_)
    out_r, codes_r, margin = R.quantize(ll, lv, G, C.QUANT_TAU, noise.double(), train)
    keep = ~(margin < C.TIE).any(-1)
    assert float(keep.float().mean()) >= 0.99
    dout = dout * keep.unsqueeze(-1)
    (out_r * dout.double()).sum().backward()
    dl_r = ll.grad if ll.grad is not None else torch.zeros_like(ll)

    lgd, vd_, nd = logits.to(DEV), vars_.to(DEV), noise.to(DEV)
    out = torch.empty(Rr, G * vd, device=DEV)
    codes = torch.empty(Rr, G, dtype=torch.int32, device=DEV)
    K.w2v_gumbel_fwd(lgd, G, vd_, C.QUANT_TAU, not train, out, codes, noise=nd if train else None)
    dlg, dvars = torch.empty(Rr, G * V, device=DEV), torch.zeros(G * V, vd, device=DEV)
    K.w2v_gumbel_bwd(lgd, G, vd_, C.QUANT_TAU, not train, dout.to(DEV), codes, dlg, dvars, noise=nd if train else None)
    torch.cuda.synchronize()
    assert torch.equal(codes.cpu().long()[keep], codes_r[keep])
    errs = {"out": C.rel_max(out.cpu()[keep], out_r.detach()[keep]), "dvars": C.rel_max(dvars.cpu(), lv.grad)}
    if train:
        errs["dlogits"] = C.rel_max(dlg.cpu()[keep], dl_r[keep])
    else:
        assert not dlg.any()
    _check(f"quantizer {name} {'train' if train else 'eval'}", "fp32", errs)


def test_quantizer_device_noise_is_seeded_gumbel():
    """Without injected noise the draw is the counter hash's: the same seed and step give the same
    codes, and the codes spread over the codebook as argmax(logit + Gumbel) must."""
    from liteasr_amd import kernels as K

    G, V, vd, Rr = 2, 16, 8, 297
    ctr = _STEP_COUNTER[0] = torch.zeros(1, dtype=torch.int64, device=DEV)  # stays registered: kept alive
    K.set_dropout_counter(ctr)
    lg = torch.zeros(Rr, G * V, device=DEV)
    vars_ = torch.rand(G * V, vd, device=DEV)
    runs = []
    for seed in (9, 9, 10):
        out, codes = torch.empty(Rr, G * vd, device=DEV), torch.empty(Rr, G, dtype=torch.int32, device=DEV)
        K.w2v_gumbel_fwd(lg, G, vars_, 2.0, False, out, codes, seed=seed)
        runs.append(codes.cpu())
    assert torch.equal(runs[0], runs[1]) and not torch.equal(runs[0], runs[2])
    counts = torch.bincount(runs[0].flatten().long(), minlength=V)
    assert int(counts.min()) > 0 and int(counts.max()) < 4 * Rr * G // V  # uniform logits: ~37 each


# ------------------------------------------------------------ contrastive head
@pytest.mark.parametrize("name", sorted(C.HEAD_CASES))
def test_contrastive_head(name):
    """(N 10, D 32, M 7, B 3) and (N 100, D 48, M 23, B 2) with a 2-entry codebook: many negatives
    equal their positive, and row (b 0, m 0) has every negative masked."""
    from liteasr_amd import kernels as K

    x, y, neg, codes, temp = C.head_case(name)
    N, D, M, B = C.HEAD_CASES[name][:4]
    lx, ly = _leaf(x), _leaf(y)
    logits_r, loss_r = R.contrast(lx, ly, neg, codes, temp)
    (loss_r * 1.5).backward()

    xd, yd = x.to(DEV), y.to(DEV)
    nd, cd = neg.int().to(DEV), codes.int().to(DEV)
    gout = torch.tensor([1.5], device=DEV)
    runs = []
    for _ in range(2):
        logits = torch.empty(M * B, N + 1, device=DEV)
        lse, rl, loss = torch.empty(B * M, device=DEV), torch.empty(B * M, device=DEV), torch.empty((), device=DEV)
        K.w2v_contrast_fwd(xd, yd, nd, cd, N, temp, logits, lse, rl, loss)
        dx, dy = torch.empty_like(xd), torch.empty_like(yd)
        K.w2v_contrast_bwd(xd, yd, nd, cd, N, temp, lse, gout, dx, dy)
        torch.cuda.synchronize()
        runs.append([t.cpu() for t in (logits, loss, dx, dy, rl)])
    for a, b in zip(*runs):
        assert torch.equal(a, b)  # fixed summation order: two runs, the same bits
    logits, loss, dx, dy, rl = runs[0]
    assert torch.equal(torch.isinf(logits), torch.isinf(logits_r.detach()))
    row = logits.view(M, B, N + 1)[0, 0]
    assert torch.isinf(row[1:]).all() and torch.isfinite(row[0]) and float(rl[0]) == 0.0
    assert torch.isfinite(dx).all() and torch.isfinite(dy).all()
    _check(f"contrast {name}", "fp32", {
        "logits": C.rel_max(logits, logits_r.detach()), "loss": abs(float(loss) - loss_r.item()) / abs(loss_r.item()),
        "dx": C.rel_max(dx, lx.grad), "dy": C.rel_max(dy, ly.grad)})


# ------------------------------------------------------------------------ model
def _golden_model(dtype="fp32"):
    from liteasr_amd.models.wav2vec2 import Wav2Vec2

    model = Wav2Vec2(C.model_config(dtype))
    model.load_state_dict(C.golden_state())
    return model.to(DEV)


def _seed_run(run):
    s_np, s_t = (int(v) for v in C.golden()[run + ".seeds"])
    np.random.seed(s_np)
    torch.manual_seed(s_t)


def test_model_eval_matches_reference():
    from liteasr_amd.criterions.wav2vec_loss import Wav2Vec2Loss, Wav2Vec2LossConfig

    g = C.golden()
    model = _golden_model().eval()
    _seed_run("eval")
    src = torch.from_numpy(g["source"]).to(DEV)
    with torch.no_grad():
        loss = Wav2Vec2Loss(Wav2Vec2LossConfig())(model, src, None, None, None)
        _seed_run("eval")
        logits = model(src)
    torch.cuda.synchronize()
    assert np.array_equal(model.last.mask.numpy(), g["eval.mask"]) and np.array_equal(model.last.neg.numpy(), g["eval.neg"])
    assert np.array_equal(model.last.codes.cpu().numpy(), g["eval.codes"])
    assert np.array_equal(np.isinf(logits.cpu().numpy()), np.isinf(g["eval.logits"]))  # -inf positions exactly
    assert float(loss) == float(model.last.loss)
    _check("model eval", "fp32", {"logits": C.rel_max(logits.cpu(), g["eval.logits"]),
                                  "loss": abs(float(loss) - float(g["eval.loss"])) / float(g["eval.loss"])})


def test_model_train_matches_reference():
    """Loss and every parameter's gradient of one train-mode step against the reference's, with
    its recorded Gumbel noise injected and its mask / negatives redrawn under its seeds."""
    g = C.golden()
    model = _golden_model().train()
    model.gumbel_noise = torch.from_numpy(g["train.noise"]).to(DEV)
    _seed_run("train")
    logits = model(torch.from_numpy(g["source"]).to(DEV))
    model.last.loss.backward()
    torch.cuda.synchronize()
    assert np.array_equal(model.last.mask.numpy(), g["train.mask"]) and np.array_equal(model.last.neg.numpy(), g["train.neg"])
    assert np.array_equal(model.last.codes.cpu().numpy(), g["train.codes"])
    assert np.array_equal(np.isinf(logits.detach().cpu().numpy()), np.isinf(g["train.logits"]))
    grads = {}
    for k, p in model.named_parameters():
        assert p.grad is not None, k
        grads[k] = (p.grad.permute(0, 2, 1) if k in model._kc_keys else p.grad).cpu()
    assert set(grads) == {str(k) for k in g["names"]}
    errs = {"logits": C.rel_max(logits.detach().cpu(), g["train.logits"]),
            "loss": abs(model.last.loss.item() - float(g["train.loss"])) / float(g["train.loss"])}
    errs.update(C.grad_errors(grads, {k: g["g." + k] for k in grads}))
    _check("model train", "fp32", errs)


def test_trainer_two_steps_bit_identical_across_processes():
    """Two eager Trainer steps (Noam / Adam, dropout on, device Gumbel noise) in two fresh
    processes seeded alike: finite losses, every parameter moved, the same bits after step two."""
    outs = []
    for _ in range(2):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_w2v_trainer_step.py"), "bf16"],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        outs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    a, b = outs
    assert a["iters"] == 2 and a["skipped"] == 0 and len(a["losses"]) == 2
    assert all(np.isfinite(v) for v in a["losses"]) and a["moved"] == a["params"]
    assert a == b
