"""wav2vec 2.0 pretraining step timing on one MI355X (model=wav2vec2_base criterion=wav2vec).

  python tools/wav2vec2_bench.py [--B 8] [--samples 64000] [--steps 8] [--repeats 9] [--dtype bf16] [--out FILE]

Prints one JSON line (appended to --out when given):

* ``step_ms``: one eager training step of the ``wav2vec2_base`` preset (forward, loss, backward,
  clip + Noam/Adam) on a (B, samples) batch: median / min / max of --steps steps after warm-up,
  host clock around work that ends in a device synchronisation.  The min-max range is the
  run-to-run spread a later change has to exceed.  ``forward_ms`` times the forward alone.
* ``head``: the fused contrastive head (lasr_w2v_contrast_fwd + _bwd) against the same head
  composed from torch ops on the device -- gather of the (N + 1, B, M, D) targets,
  torch.cosine_similarity, masked_fill, cross_entropy and its autograd backward -- on identical
  inputs at the step's (B, M, N, D): microseconds per forward + backward from device events,
  the two alternating, median / min / max over --repeats; whether the ranges overlap; the
  largest difference between the two sides' logits and gradients.
* the library build (first 16 hex of its sha256).
"""

import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(ts):
    return {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}


def head_compare(B, M, N, D, G, V, repeats):
    from liteasr_amd import kernels as K

    dev = "cuda"
    g = torch.Generator().manual_seed(B * 1000 + M)
    x, y = torch.randn(B, M, D, generator=g).to(dev), torch.randn(B, M, D, generator=g).to(dev)
    codes = torch.randint(0, V, (B * M, G), generator=g)
    own = torch.arange(M).unsqueeze(-1).expand(-1, N).flatten()
    neg = torch.randint(0, M - 1, (B, M * N), generator=g)
    neg[neg >= own] += 1
    neg += (torch.arange(B) * M).unsqueeze(-1)
    negd, neg32, codes32 = neg.to(dev), neg.int().to(dev), codes.int().to(dev)
    codesd = codes.to(dev)
    temp = 0.1
    buf = dict(logits=torch.empty(M * B, N + 1, device=dev), lse=torch.empty(B * M, device=dev),
               rl=torch.empty(B * M, device=dev), loss=torch.empty((), device=dev), dx=torch.empty_like(x),
               dy=torch.empty_like(y))

    def fused():
        K.w2v_contrast_fwd(x, y, neg32, codes32, N, temp, buf["logits"], buf["lse"], buf["rl"], buf["loss"])
        K.w2v_contrast_bwd(x, y, neg32, codes32, N, temp, buf["lse"], None, buf["dx"], buf["dy"])

    xt, yt = x.clone().requires_grad_(), y.clone().requires_grad_()
    res = {}

    def composed():
        xt.grad = yt.grad = None
        yf = yt.view(B * M, D)
        negs = yf[negd.view(-1)].view(B, M, N, D).permute(2, 0, 1, 3)
        tgt = torch.cat([yt.unsqueeze(0), negs], dim=0)
        lg = torch.cosine_similarity(xt, tgt, dim=-1) / temp
        same = (codesd[negd.view(-1)].view(B, M, N, G) == codesd.view(B, M, 1, G)).all(-1).permute(2, 0, 1)
        lg = torch.cat([lg[:1], lg[1:].masked_fill(same, float("-inf"))], dim=0)
        lg = lg.transpose(0, 2).reshape(-1, N + 1)
        loss = torch.nn.functional.cross_entropy(lg, lg.new_zeros(lg.size(0), dtype=torch.long))
        loss.backward()
        res["logits"], res["loss"] = lg.detach(), loss.detach()

    fns = {"fused_us": fused, "torch_us": composed}
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    fin = torch.isfinite(res["logits"])
    diff = {"logits": float((buf["logits"][fin] - res["logits"][fin]).abs().max()),
            "inf_positions_equal": bool(torch.equal(torch.isfinite(buf["logits"]), fin)),
            "dx": float((buf["dx"] - xt.grad).abs().max()), "dy": float((buf["dy"] - yt.grad).abs().max())}
    ts = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():  # alternating
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1) * 1e3)
    out = {"B": B, "M": M, "N": N, "D": D, "max_abs_diff": diff}
    out.update({k: _stats(v) for k, v in ts.items()})
    out["ranges_overlap"] = not (out["fused_us"]["max"] < out["torch_us"]["min"]
                                 or out["torch_us"]["max"] < out["fused_us"]["min"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--samples", type=int, default=64000)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wav2vec2_bench: no GPU (nothing is measured on the host)")
    from liteasr_amd.config.compose import compose
    from liteasr_amd.criterions import build_criterion
    from liteasr_amd.models import build_model
    from liteasr_amd.optims.noam import Noam, NoamConfig

    cfg = compose(overrides=["task=asr_kaldi", "model=wav2vec2_base", "criterion=wav2vec", "optimizer=noam_d256",
                             f"model.compute_dtype={a.dtype}"])
    torch.manual_seed(42)
    np.random.seed(42)
    model = build_model(cfg.model, None).cuda().train()
    crit = build_criterion(cfg.criterion, None)
    opt = Noam(model.parameters(), NoamConfig(model_dim=cfg.model.encoder_embed_dim))
    src = torch.randn(a.B, a.samples, generator=torch.Generator().manual_seed(0)).cuda()

    def step():
        opt.zero_grad()
        loss = crit(model, src, None, None, None)
        loss.backward()
        opt.clip_and_step(5.0)
        return loss

    def timed(fn, n):
        ts = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return _stats(ts)

    for _ in range(a.warmup):
        loss = step()
    step_ms = timed(step, a.steps)
    with torch.no_grad():
        fwd_ms = timed(lambda: model(src), a.steps)
    last = model.last
    Fd = model.linear_final.weight.shape[0]
    lib = os.path.join(ROOT, "liteasr_amd", "lib", "libliteasr_hip.so")
    out = {
        "workload": f"wav2vec2_base {a.dtype}, eager step, B={a.B} x {a.samples} samples "
                    f"(T'={model.feature_extractor.out_frames(a.samples)}, M={last.M})",
        "step_ms": step_ms, "forward_ms": fwd_ms, "loss": round(loss.item(), 4), "steps": a.steps, "warmup": a.warmup,
        "head": head_compare(a.B, last.M, int(cfg.model.num_negatives), Fd, int(cfg.model.latent_groups),
                             int(cfg.model.latent_vars), a.repeats),
        "repeats": a.repeats,
        "build": hashlib.sha256(open(lib, "rb").read()).hexdigest()[:16],
    }
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
