"""Transducer beam-search timing on one MI355X (liteasr/models/transducer.py:137-206).

  python tools/rnnt_search_bench.py [--T 1000] [--repeats 7] [--dtype bf16]

Default config: Conformer encoder d 256 / 4 heads / 4 layers, prediction network 2048 units x 2,
joint 768, V 4233, random init, one utterance of T frames (T' = ((T-1)//2-1)//2), beam 10.
Prints one JSON line: ms per utterance (median of --repeats after warm-up; host clock around
work that ends in the result's device-to-host copy) of the device-resident search
(decoding.transducer_beam_search, encoder included) and of the host-loop variant that drives
the same kernels one expansion at a time; the encoder alone; launches per expansion; LSTM steps
actually executed per pop; whether both variants return the same tokens; the library build
(first 16 hex of its sha256).  A random-init model emits almost only blanks; --gain scales
lin_jnt / lin_dec (6 / 4, blank bias -3, as the golden fixtures) so the search leaves the
all-blank path.
"""

import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--gain", type=int, default=1, help="1: peaked joint (default), 0: plain random init")
    a = ap.parse_args()
    from liteasr_amd import decoding as D
    from liteasr_amd.models.transducer import Transducer, TransducerConfig
    from liteasr_amd.utils.cfg import resolve_self

    torch.manual_seed(42)
    c = TransducerConfig(input_dim=80, vocab_size=4233, enc_dim=256, enc_ff_dim=2048, enc_attn_heads=4, enc_layers=4,
                         enc_arch="conformer", activation="swish", dec_dim=256, dec_units=2048, dec_layers=2,
                         joint_dim=768, compute_dtype=a.dtype)
    resolve_self(c)
    model = Transducer(c)
    if a.gain:
        with torch.no_grad():
            model.lin_jnt.weight.mul_(6.0)
            model.lin_dec.weight.mul_(4.0)
            model.lin_jnt.bias[0] -= 3.0
    model = model.cuda().eval()
    x = torch.randn(1, a.T, 80, generator=torch.Generator().manual_seed(0)).cuda()
    Tp = ((a.T - 1) // 2 - 1) // 2

    def timed(fn, repeats):
        for _ in range(2):  # graph captures, code objects, clocks
            fn()
        ts = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), min(ts), max(ts)

    with torch.no_grad():
        td, th = {}, {}
        yd = D.transducer_beam_search(model, x, trace=td)
        yh = D._transducer_beam_search_hostloop(model, x, trace=th)
        dev = timed(lambda: D.transducer_beam_search(model, x), a.repeats)
        host = timed(lambda: D._transducer_beam_search_hostloop(model, x), max(3, a.repeats // 2))
        enc = timed(lambda: D.encode(model, x), a.repeats)
    lib = os.path.join(ROOT, "liteasr_amd", "lib", "libliteasr_hip.so")
    out = {
        "workload": f"Transducer d256x4 / LSTM 2048x2 / J 768 / V 4233 {a.dtype}, 1 utt T={a.T} (T'={Tp}), beam 10",
        "device_search_ms": {"median": dev[0], "min": dev[1], "max": dev[2]},
        "hostloop_search_ms": {"median": host[0], "min": host[1], "max": host[2]},
        "encoder_ms": {"median": enc[0], "min": enc[1], "max": enc[2]},
        "repeats": a.repeats,
        "pops": 10 * Tp,
        "launches_per_expansion": model.decoder.n_layer + 3,
        "graph_replays_per_utterance": Tp,
        "lstm_steps_executed": td["steps"],
        "lstm_steps_per_pop": td["steps"] / (10 * Tp),
        "output_len": len(yd),
        "distinct_tokens": len(set(yd) - {0}),
        "device_equals_hostloop": yd == yh and td["pops"] == th["pops"] and td["steps"] == th["steps"],
        "build": hashlib.sha256(open(lib, "rb").read()).hexdigest()[:16],
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
