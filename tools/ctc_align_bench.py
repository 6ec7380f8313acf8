"""CTC forced alignment timing on one MI355X: ``lasr_ctc_align`` against the host alternative (copy
the log-probs down, run the Viterbi pass in numpy) and, as context, against ``lasr_ctc_lattice``.

  python tools/ctc_align_bench.py [--repeats 15] [--iters 20] [--host-repeats 5] [--out FILE]

A synthetic batch: B = 32 utterances, T' = 249 encoder frames each, 20 .. 80 labels per row
(Lmax = 80), V = 4233 random fp32 logits; ``lp`` [B][T'][Lmax+1] is made once by the first stage of
``lasr_ctc_fwd`` (``alpha == NULL``) and every arm reads it.  One JSON line is printed (and
appended to --out when given):

* ``align``: one ``lasr_ctc_align`` launch; ``align_graph``: the same launch replayed from a
  captured hipGraph; ``lattice``: ``lasr_ctc_lattice``, alpha only, on the same inputs -- the
  existing kernel with the same serial-in-T structure (log-sum-exp where the Viterbi pass takes a
  max, no backtrace), reported as context, not as a bar.  Each sample is device time by events
  around --iters back-to-back calls, divided by --iters; the three alternate for --repeats samples
  after an untimed pass; median / min / max.
* ``host``: what a user without the kernel does on identical inputs: ``lp.cpu()`` (the copy is
  part of its time) and tests/ctc_align_ref.py's float32 restatement, vectorised over the lattice
  states, row by row; wall time, --host-repeats samples after an untimed pass.  Its result is
  compared with the kernel's first (states, spans and score bits must be equal).
* ``align_faster_beyond_spread``: the host minimum minus the graph-replayed median exceeds the
  host spread (max - min)."""

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
sys.path.insert(0, os.path.join(ROOT, "tests"))

B, TP, LMIN, LMAX, V = 32, 249, 20, 80, 4233


def _stats(ts, nd=4):
    return {"median": round(statistics.median(ts), nd), "min": round(min(ts), nd), "max": round(max(ts), nd)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ctc_align_bench: no GPU (the device parts are not measured on the host)")
    import ctc_align_ref as R
    from liteasr_amd import _native as N
    from liteasr_amd import kernels as K

    rng = np.random.default_rng(0)
    tlen_h = rng.integers(LMIN, LMAX + 1, B).astype(np.int32)
    tlen_h[0] = LMAX
    targets_h = np.zeros((B, LMAX), dtype=np.int32)
    for b in range(B):
        targets_h[b, :tlen_h[b]] = rng.integers(1, V, tlen_h[b])
    ilen_h = np.full(B, TP, dtype=np.int32)
    logits = torch.from_numpy(rng.standard_normal((B, TP, V)).astype(np.float32)).cuda()
    targets, ilen, tlen = (torch.from_numpy(x).cuda() for x in (targets_h, ilen_h, tlen_h))
    lse = torch.empty(B * TP, dtype=torch.float32, device="cuda")
    lp = torch.empty(B, TP, LMAX + 1, dtype=torch.float32, device="cuda")
    K.ctc_fwd(logits, targets, ilen, tlen, lse, lp, None, None)
    alpha = torch.empty(B, TP, 2 * LMAX + 1, dtype=torch.float32, device="cuda")
    nll = torch.empty(B, dtype=torch.float32, device="cuda")
    states = torch.empty(B, TP, dtype=torch.int32, device="cuda")
    spans = torch.empty(B, LMAX, 2, dtype=torch.int32, device="cuda")
    score = torch.empty(B, dtype=torch.float32, device="cuda")
    ws_bytes = K.ctc_align_workspace(B, TP, LMAX)
    ws = K.WS.get((ws_bytes + 3) // 4, "cuda") if ws_bytes else None

    def run_align():
        N.call("lasr_ctc_align", B, TP, LMAX, K.ptr(targets), K.ptr(ilen), K.ptr(tlen), K.ptr(lp), K.ptr(ws), ws_bytes,
               K.ptr(states), K.ptr(spans), K.ptr(score), K.stream())

    def run_lattice():
        N.call("lasr_ctc_lattice", B, TP, LMAX, K.ptr(targets), K.ptr(ilen), K.ptr(tlen), K.ptr(lp), K.ptr(alpha), None,
               K.ptr(nll), K.stream())

    def run_host():
        return R.align_batch(lp.cpu().numpy(), targets_h, ilen_h, tlen_h, dtype=np.float32)

    for _ in range(3):  # untimed
        run_align()
        run_lattice()
    want = run_host()
    torch.cuda.synchronize()
    got = (states.cpu().numpy(), spans.cpu().numpy(), score.cpu().numpy())
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), "kernel and host paths differ"
    assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)), "kernel and host scores differ"
    assert np.isfinite(got[2]).all()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run_align()
    fns = {"align": run_align, "align_graph": graph.replay, "lattice": run_lattice}
    ts = {k: [] for k in fns}
    host = []
    for r in range(a.repeats):
        for k, fn in fns.items():  # alternating
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1) / a.iters)
        if r < a.host_repeats:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run_host()
            host.append((time.perf_counter() - t0) * 1e3)
    lib = os.path.join(ROOT, "liteasr_amd", "lib", "libliteasr_hip.so")
    out = {"workload": f"CTC forced alignment: B={B}, T'={TP}, L={LMIN}..{LMAX}, V={V}, lp from the first CTC stage",
           "B": B, "Tp": TP, "Lmax": LMAX, "V": V, "labels_total": int(tlen_h.sum()), "workspace_bytes": ws_bytes,
           "iters_per_sample": a.iters, "repeats": a.repeats, "host_repeats": len(host),
           "lp_bytes": lp.numel() * 4}
    out.update({k + "_ms": _stats(v) for k, v in ts.items()})
    out["host_ms"] = _stats(host, 3)
    spread = out["host_ms"]["max"] - out["host_ms"]["min"]
    out["align_faster_beyond_spread"] = out["host_ms"]["min"] - out["align_graph_ms"]["median"] > spread
    out["align_over_lattice"] = round(out["align_graph_ms"]["median"] / out["lattice_ms"]["median"], 3)
    out["build"] = hashlib.sha256(open(lib, "rb").read()).hexdigest()[:16]
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
