"""Batched evaluation (inference.batch_size) against the utterance-by-utterance loop, on one MI355X.

  python tools/infer_batch_bench.py [--repeats 5] [--out profiles/infer_batch_bench.jsonl]
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/infer_batch_bench.py --trace-leg 32

U2-Conformer-small (BASELINE config 2: d 256, 12 + 6 layers, V 4233, bf16, random init, seed 42)
on the synthetic set of tools/rescore_bench.py: 200 utterances, frame counts uniform in
300..1200 (seed 0), decoded through liteasr_amd.infer.infer_dataset at batch_size 1, 8 and 32.

Every leg first runs the set once untimed (graph captures, code objects, allocator pools); then
the three legs are ALTERNATED for --repeats (>= 5) repetitions in this one process.  A timing is
the host clock around one whole pass of the set, ending in a device synchronise.  The
batch_size 1 leg is infer_dataset's utterance-by-utterance loop (U2.inference, the host search),
which this tool does not touch, so its column is a timing of the loop as it was before
batch_size existed.

One JSON line per repetition and one summary line (median, min, max utterances per second of
each leg; whether a batched leg's median beats the batch_size 1 median by more than the latter's
own min-max spread; how many hypotheses differ from batch_size 1's, which padded rows may) are
appended to --out, each with the library's build hash.  --trace-leg N runs one untimed and one
more pass of leg N only and writes nothing: the run to put under rocprofv3 for the kernel times
of the batched search.
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

LEGS = (1, 8, 32)


class _Utt:
    def __init__(self, x):
        self.x, self.xlen, self.text = x, x.shape[0], "x"


class _Task:
    """ASRTask.inference / inference_batch without a vocabulary: the ids joined as text."""

    def inference(self, x, model, encoder_graph=None):
        return " ".join(str(t) for t in model.inference(x, encoder_graph=bool(encoder_graph)))

    def inference_batch(self, xs, xlens, model):
        return [" ".join(str(t) for t in ids) for ids in model.inference_batch(xs, xlens)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "infer_batch_bench.jsonl"))
    ap.add_argument("--set", type=int, default=200)
    ap.add_argument("--trace-leg", type=int, default=0, choices=(0,) + LEGS)
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("--repeats must be at least 5")
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
    lens = np.random.default_rng(0).integers(300, 1201, a.set).tolist()
    g = torch.Generator().manual_seed(1)
    data = [_Utt(torch.randn(n, 80, generator=g)) for n in lens]
    logging.getLogger("liteasr_amd.infer").setLevel(logging.WARNING)
    task, dev = _Task(), torch.device("cuda")

    def one_pass(bs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, _, hyps = I.infer_dataset(task, model, data, dev, batch_size=bs)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, hyps

    if a.trace_leg:
        one_pass(a.trace_leg)
        t, _ = one_pass(a.trace_leg)
        print(json.dumps({"kind": "trace", "batch_size": a.trace_leg, "utt_per_s": a.set / t, "build": build}))
        return
    hyps = {bs: one_pass(bs)[1] for bs in LEGS}  # untimed
    lines, rate = [], {bs: [] for bs in LEGS}
    for r in range(a.repeats):
        for bs in LEGS:
            t, _ = one_pass(bs)
            rate[bs].append(a.set / t)
            lines.append({"kind": "rep", "rep": r, "batch_size": bs, "seconds": t, "utt_per_s": a.set / t,
                          "build": build})
    stat = {bs: {"median": statistics.median(v), "min": min(v), "max": max(v)} for bs, v in rate.items()}
    spread = stat[1]["max"] - stat[1]["min"]
    caps = sorted(k for k in model.__dict__.get("_rescore_batch_states", {}) if isinstance(k, tuple))
    lines.append({"kind": "summary",
                  "workload": "U2-Conformer-small bf16 random init, beam 10, ctc weight 0.5",
                  "utterances": a.set, "frames": "uniform 300..1200, seed 0", "repeats": a.repeats,
                  "warm_up": "one untimed pass of the set per leg", "utt_per_s": {str(bs): s for bs, s in stat.items()},
                  "batch_size_1_spread": spread,
                  "beats_batch_size_1_by_more_than_its_spread": {
                      str(bs): stat[bs]["median"] - stat[1]["median"] > spread for bs in LEGS[1:]},
                  "hypotheses_differing_from_batch_size_1": {
                      str(bs): sum(x != y for x, y in zip(hyps[bs], hyps[1])) for bs in LEGS[1:]},
                  "states_of_the_last_leg": caps, "build": build})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
    print(json.dumps(lines[-1]))


if __name__ == "__main__":
    main()
