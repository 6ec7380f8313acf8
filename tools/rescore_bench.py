"""Attention rescoring: the device-resident pass against the retained host path, on one MI355X.

  python tools/rescore_bench.py [--repeats 7] [--out profiles/rescore_bench.jsonl] [--set 200]

U2-Conformer-small (BASELINE config 2: d 256, 12 + 6 layers, V 4233, bf16, random init, seed
42; the model of tools/decode_bench.py), one utterance each at T = 1000 and T = 400, beam 10.

Per length, after three warm-up calls of each path (graph captures, code objects, clocks), the
two paths are ALTERNATED for --repeats (>= 5) repetitions in this one process; every timing is
the host clock around one whole utterance (encoder included) and ends in a device synchronise:

  device  decoding.attention_rescore_device(model, x)
  host    decoding.attention_rescore_host(model, x): ctc_prefix_beam_search_nbest + rescore +
          pick_best.  Those functions are the parent commit's, byte for byte (git diff of them
          is empty), so the host column is a timing of the parent's U2.inference.  It is
          also what U2.inference runs today: the device pass is the default only once its
          median beats the host's by more than the host's own spread at both lengths.

One JSON line per repetition is appended to --out, each with the library's build hash (first
16 hex of the sha256 of libliteasr_hip.so); then one summary line per length (medians, the
host path's run-to-run spread = max - min, whether the device median beats the host median by
more than that spread, whether both paths return the same tokens), and one line for a seeded
synthetic set of --set utterances with frame counts drawn uniformly from 300..1200, decoded
through liteasr_amd.infer's loop (frame-count order, encoder graph only for counts that occur
at least four times), once with U2.inference and once with the device pass, each after one
untimed pass of the set (graph captures excluded): utterances per second, graphed / eager
encoder passes.
"""

import argparse
import hashlib
import json
import logging
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _Utt:
    def __init__(self, x):
        self.x, self.xlen, self.text = x, x.shape[0], "x"


class _Task:
    """ASRTask.inference without a vocabulary: the ids joined as text.  decode: U2.inference
    (the default path) or decoding.attention_rescore_device."""

    def __init__(self, decode):
        self.decode = decode

    def inference(self, x, model, encoder_graph=None):
        return " ".join(str(t) for t in self.decode(model, x, encoder_graph=bool(encoder_graph)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rescore_bench.jsonl"))
    ap.add_argument("--set", type=int, default=200, help="utterances of the synthetic set (0: skip)")
    ap.add_argument("--lengths", type=int, nargs="*", default=[1000, 400])
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("--repeats must be at least 5")
    from liteasr_amd import decoding as D
    from liteasr_amd import infer as I
    from liteasr_amd.models.u2 import U2, U2Config
    from liteasr_amd.utils.cfg import resolve_self

    torch.manual_seed(42)
    c = U2Config(input_dim=80, vocab_size=4233, enc_dim=256, enc_ff_dim=2048, enc_layers=12, dec_dim=256,
                 dec_ff_dim=2048, dec_layers=6, compute_dtype="bf16")
    resolve_self(c)
    model = U2(c).cuda().eval()
    lib = os.path.join(ROOT, "liteasr_amd", "lib", "libliteasr_hip.so")
    build = hashlib.sha256(open(lib, "rb").read()).hexdigest()[:16]
    workload = "U2-Conformer-small bf16 random init, beam 10, ctc weight 0.5"
    lines = []

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    with torch.no_grad():
        for T in a.lengths:
            x = torch.randn(1, T, 80, generator=torch.Generator().manual_seed(0)).cuda()
            trace = {}
            yd = D.attention_rescore_device(model, x, trace=trace)
            yh = D.attention_rescore_host(model, x)
            for _ in range(3):
                D.attention_rescore_device(model, x)
                D.attention_rescore_host(model, x)
            dev, host = [], []
            for r in range(a.repeats):
                td, _ = timed(lambda: D.attention_rescore_device(model, x))
                th, _ = timed(lambda: D.attention_rescore_host(model, x))
                dev.append(td)
                host.append(th)
                lines.append({"kind": "rep", "T": T, "rep": r, "device_ms": td, "host_ms": th, "build": build})
            enc = [timed(lambda: D.encode(model, x))[0] for _ in range(a.repeats)]
            md, mh = statistics.median(dev), statistics.median(host)
            spread = max(host) - min(host)
            lines.append({"kind": "summary", "workload": workload, "T": T, "T_sub": ((T - 1) // 2 - 1) // 2,
                          "caps": trace["caps"], "longest_hyp": max(len(t) for t, _ in trace["nbest"]),
                          "device_ms": {"median": md, "min": min(dev), "max": max(dev)},
                          "host_ms": {"median": mh, "min": min(host), "max": max(host)},
                          "encoder_graph_ms": statistics.median(enc), "host_spread_ms": spread,
                          "device_beats_host_by_more_than_spread": (mh - md) > spread,
                          "same_tokens": list(yd) == list(yh), "repeats": a.repeats, "build": build})
        if a.set:
            rng = np.random.default_rng(0)
            lens = rng.integers(300, 1201, a.set).tolist()
            g = torch.Generator().manual_seed(1)
            data = [_Utt(torch.randn(n, 80, generator=g)) for n in lens]
            logging.getLogger("liteasr_amd.infer").setLevel(logging.WARNING)
            _, graphed = I.graph_plan(lens)
            paths = {"U2.inference": lambda m, x, encoder_graph: m.inference(x, encoder_graph=encoder_graph),
                     "attention_rescore_device": lambda m, x, encoder_graph: D.attention_rescore_device(
                         m, x, encoder_graph=encoder_graph)}
            rate = {}
            for name, fn in paths.items():
                # one untimed pass first: the device pass captures a graph per (Tcap, Lcap) it meets,
                # which the host path has no counterpart of; the timed pass measures steady state
                I.infer_dataset(_Task(fn), model, data, torch.device("cuda"))
                model.__dict__.pop("_encode_graphs", None)
                t, _ = timed(lambda: I.infer_dataset(_Task(fn), model, data, torch.device("cuda")))
                rate[name] = a.set / (t / 1e3)
            lines.append({"kind": "set", "workload": workload, "utterances": a.set, "frames": "uniform 300..1200, seed 0",
                          "utt_per_s": rate, "warm_up": "one untimed pass of the set per path", "encoder_graphed": int(sum(graphed)),
                          "encoder_eager": int(a.set - sum(graphed)), "distinct_frame_counts": len(set(lens)),
                          "build": build})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
    for ln in lines:
        if ln["kind"] != "rep":
            print(json.dumps(ln))


if __name__ == "__main__":
    main()
