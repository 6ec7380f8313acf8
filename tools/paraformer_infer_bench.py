"""Paraformer one-pass decoding timing on one MI355X (liteasr/models/paraformer.py:124-129).

  python tools/paraformer_infer_bench.py [--T 1000] [--repeats 9] [--dtype bf16] [--out FILE]

Paraformer-small (Conformer encoder d 256 / 4 heads / 12 layers, parallel decoder 6 layers,
V 4233, F 80), random init with the predictor's bias at -1 (a token every ~4 frames, as the
golden fixtures).  Prints one JSON line (appended to --out when given):

* ``inference_ms``: one utterance of T frames end to end through Paraformer.inference (median /
  min / max of --repeats after warm-up; host clock around work that ends in the ids'
  device-to-host copy), and the graph-replayed encoder alone;
* ``cif``: lasr_cif_infer (three launches: scalar recursion, one wave per fired frame,
  compaction) against the scan kernel lasr_cif_fwd at the same ulen, D 256, for (B, T') in
  (1, 249), (1, 999), (32, 249): microseconds per call from device events around a hipGraph
  of --calls back-to-back calls, the two kernels alternating, median / min / max over
  --repeats replays each (the min-max range is the run-to-run spread a difference has to
  exceed); whether the two agree bit for bit on these inputs;
* the library build (first 16 hex of its sha256).
"""

import argparse
import hashlib
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(ts):
    return {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}


def _graph_of(fn, calls):
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):  # warm-up: code objects loaded before the capture
        fn()
    cur.wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            fn()
    return g


def cif_compare(B, Tp, D, calls, repeats):
    from liteasr_amd import kernels as K

    dev = "cuda"
    gen = torch.Generator().manual_seed(B * 1000 + Tp)
    z = (torch.randn(B * Tp, 1, generator=gen) - 1.0).to(dev)
    h = torch.randn(B, Tp, D, generator=gen).to(dev)
    plen = torch.randint(Tp // 2, Tp + 1, (B,), generator=gen).int()
    plen[0] = Tp
    plen = plen.to(dev)
    st = K.cif_infer(z, plen, h)
    ulen = st.ulen.clone()
    U = max(1, int(ulen.max()))
    f = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=dev)  # noqa: E731
    sc = SimpleNamespace(alpha=f(B * Tp), acc=f(B * Tp), fired=f(B * Tp, dt=torch.uint8),
                         row=f(B * Tp, dt=torch.int32), sum_alpha=f(B), mae=f(B), out=f(B, U, D))
    K.cif_fwd(z, plen, ulen, h, B, Tp, U, sc)
    torch.cuda.synchronize()
    same = bool(torch.equal(st.out[:, :U].contiguous().view(torch.int32), sc.out.view(torch.int32))
                and torch.equal(st.fired, sc.fired) and torch.equal(st.sum_alpha, sc.sum_alpha))
    graphs = {"cif_infer_us": _graph_of(lambda: K.cif_infer(z, plen, h, st), calls),
              "cif_fwd_us": _graph_of(lambda: K.cif_fwd(z, plen, ulen, h, B, Tp, U, sc), calls)}
    for g in graphs.values():  # clocks, caches
        g.replay()
    torch.cuda.synchronize()
    ts = {k: [] for k in graphs}
    for _ in range(repeats):
        for k, g in graphs.items():  # alternating
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1) * 1e3 / calls)
    out = {"B": B, "Tp": Tp, "D": D, "ulen_max": int(ulen.max()), "ulen_sum": int(ulen.sum()),
           "bit_identical": same}
    out.update({k: _stats(v) for k, v in ts.items()})
    # faster by more than the spread: the ranges do not overlap
    out["infer_faster_beyond_spread"] = out["cif_infer_us"]["max"] < out["cif_fwd_us"]["min"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--calls", type=int, default=50, help="kernel calls per captured graph")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("paraformer_infer_bench: no GPU (nothing is measured on the host)")
    from liteasr_amd import decoding as D
    from liteasr_amd.models.paraformer import Paraformer, ParaformerConfig
    from liteasr_amd.utils.cfg import resolve_self

    torch.manual_seed(42)
    c = ParaformerConfig(input_dim=80, vocab_size=4233, enc_dim=256, enc_ff_dim=2048, enc_attn_heads=4,
                         enc_layers=12, dec_dim=256, dec_ff_dim=2048, dec_attn_heads=4, dec_layers=6,
                         dropout_rate=0.0, compute_dtype=a.dtype)
    resolve_self(c)
    model = Paraformer(c)
    with torch.no_grad():
        model.predictor.lin.bias.fill_(-1.0)
    model = model.cuda().eval()
    x = torch.randn(1, a.T, 80, generator=torch.Generator().manual_seed(0)).cuda()
    Tp = ((a.T - 1) // 2 - 1) // 2

    def timed(fn):
        for _ in range(3):  # graph capture, code objects, clocks
            fn()
        ts = []
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return _stats(ts)

    ids = model.inference(x)
    inf = timed(lambda: model.inference(x))
    enc = timed(lambda: D.encode(model, x, fp32=True))
    lib = os.path.join(ROOT, "liteasr_amd", "lib", "libliteasr_hip.so")
    out = {
        "workload": f"Paraformer-small d256 12/6 layers V 4233 {a.dtype}, 1 utt T={a.T} (T'={Tp})",
        "inference_ms": inf,
        "encoder_ms": enc,
        "tokens": len(ids),
        "equals_batch_of_one": model.inference_batch(x, [a.T]) == [ids],
        "repeats": a.repeats,
        "calls_per_graph": a.calls,
        "cif": [cif_compare(B, T, 256, a.calls, a.repeats) for B, T in ((1, 249), (1, 999), (32, 249))],
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
