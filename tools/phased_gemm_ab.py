"""The phased 128 x 64 GEMM kernel (csrc/gemm_phase.hip) against the planner's instance, outside the
step: FFN fc2 forward (fp32 out, residual + dropout) and FFN fc1 dX (bf16 out, B N-contiguous) at
M 7968, N 256, K 2048 and 4864, and K = 64 (prologue + epilogue alone, routing forced).  Rounds
alternate lasr_gemm_phased(0) and (1) in one process; each is timed as a replayed hipGraph of 50
launches (tile_ab.graph_time), the first round also with cold operands (a 640 MB buffer rewritten
before every launch).  One JSON line per (case, K, mode, round); `phased_launches` = calls the
launcher routed while the graph was captured.  With an ablation build of gemm_phase.hip
(-DLASR_EXP=1 no MFMAs, 4 no loads, 5 neither; tools/with_lib.py) the same lines give the loop's
ablation rows.
    python tools/phased_gemm_ab.py        (ROUNDS=5 COLD=1 in the environment)"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from liteasr_amd import kernels as K  # noqa: E402
from liteasr_amd import _native  # noqa: E402
from tools.tile_ab import graph_time  # noqa: E402

ROUNDS = int(os.environ.get("ROUNDS", "5"))
COLD = int(os.environ.get("COLD", "1"))
label = os.environ.get("LITEASR_HIP_LIB", "tree")


def mk(M, D, F):
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(M, F, device=dev, generator=g).bfloat16()
    w2 = (torch.randn(D, F, device=dev, generator=g) * F ** -0.5).bfloat16()
    b2 = torch.randn(D, device=dev, generator=g) * 0.02
    res = torch.randn(M, D, device=dev, generator=g)
    out = torch.empty(M, D, device=dev)
    dz = torch.randn(M, F, device=dev, generator=g).bfloat16()
    w1 = (torch.randn(F, D, device=dev, generator=g) * F ** -0.5).bfloat16()
    dln = torch.empty(M, D, device=dev, dtype=torch.bfloat16)
    return {
        "fc2_fwd": (lambda: K.linear(x, w2, out, bias=b2, res=res, res_scale=0.5, drop_p=0.1, drop_seed=3), out),
        "fc1_dx": (lambda: K.gemm(dz, w1, dln), dln),
    }


def cold_time(fn, flush, n=20):
    ts = []
    for _ in range(n):
        flush.add_(1.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def main():
    L = _native.load()
    flush = torch.zeros(160 * 1024 * 1024, device="cuda")  # 640 MB > L2 + Infinity Cache
    for (M, D, F) in ((7968, 256, 2048), (7968, 256, 4864), (7968, 256, 64)):
        cases = mk(M, D, F)
        for name, (fn, o) in cases.items():
            outs = {}
            for r in range(ROUNDS):
                for mode in (0, 1 if F >= 1024 else 2):
                    L.lasr_gemm_phased(mode)
                    n0 = L.lasr_gemm_phased_launches()
                    us = graph_time(fn)
                    n1 = L.lasr_gemm_phased_launches()
                    rec = {"lib": label, "case": name, "M": M, "N": D, "K": F, "phased": mode, "round": r,
                           "graph_us": round(us, 2), "phased_launches": n1 - n0}
                    if COLD and r == 0:
                        rec["cold_us"] = round(cold_time(fn, flush), 2)
                    outs[mode] = o.clone()
                    print(json.dumps(rec), flush=True)
            print(json.dumps({"lib": label, "case": name, "K": F, "equal": bool(torch.equal(*outs.values()))}),
                  flush=True)
    L.lasr_gemm_phased(1)


if __name__ == "__main__":
    main()
