"""Generate tests/golden/rnnt_search.npz by running the *reference's* own
``Transducer.inference`` (liteasr/models/transducer.py:137-206, imported through refshim) on
the CPU.  Data only; the tests and the GPU box read the .npz.

    python tests/golden/make_golden_rnnt_search.py [--scan N]

The model is the tiny Transducer of make_golden.py gen_transducer (Conformer d 64 x 2, LSTM
dec_dim 16 / 48 units x 2, joint 24, F 40).  Its encoder weights are the seed-42 ones stored
in transducer.npz (``init.encoder.*``; not stored again, which keeps this file small); the
prediction network and the joint projections are drawn per case from ``torch.manual_seed(
seed)``.  A random-init transducer emits almost only blanks, so ``lin_jnt.weight`` is scaled
by 6, ``lin_dec.weight`` by 4 and the blank bias lowered by 3: the outputs then hold several
distinct tokens.

The search is recorded without touching the reference's text: ``max`` and ``sorted`` are
shadowed in the reference module's namespace at run time (they see every pop and the final
ranking), ``decoder.rnn_forward`` and ``model.joint`` are wrapped on the instance.

Per case ``c<i>.``:
  V, T, seed             the shape and the seed
  init.<key>             state_dict entries outside the encoder
  x [T, 40]              the utterance
  yseq                   the returned token list (leading 0 included)
  best_score             its score / len(yseq)
  pop_yseq / pop_off     the popped hypotheses' yseq, concatenated, with offsets [pops + 1]
  pop_score, pop_nA      the popped score and len(A) when ``max`` was called
  steps                  number of decoder.rnn_forward calls (memoisation pinned)
  logp [pops, V]         the log_softmax row of every pop
  margin_a               smallest (best - second best) score in A over all pops
  margin_b               gap between the best two normalised final scores

A case is kept only if margin_a >= 10 * MAX_DLOGP * (T' + len(yseq)): MAX_DLOGP is the
largest |log-prob difference| between the fp32 device build and the rows recorded here
(measured in tests/test_rnnt_search_gpu.py, which prints it), T' + len the number of addends
of the longest score sum.  Seeds are chosen by --scan: the seed with the largest margin_a
over that requirement among those whose output holds at least three distinct tokens.
"""

import argparse
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import refshim  # noqa: E402

refshim.install()

import liteasr.models.transducer as ref_mod  # noqa: E402
from liteasr.models.transducer import DecoderArch, EncoderArch, Transducer  # noqa: E402

# bound on the largest |device fp32 log-prob - recorded log-prob| over all pops of all cases
# (see the module docstring; the measured values are in tests/test_rnnt_search_gpu.py)
MAX_DLOGP = 2e-5

# (V, T, seed)
CASES = [(20, 64, 145), (97, 47, 223), (11, 33, 263), (20, 7, 130)]


def build(V, seed):
    cfg = types.SimpleNamespace(joint_dim=24, dropout_rate=0.0, enc_arch=EncoderArch.Conformer, use_rel=True,
                                input_dim=40, enc_dim=64, enc_ff_dim=128, enc_attn_heads=4, enc_dropout_rate=0.0,
                                enc_pos_dropout_rate=0.0, enc_attn_dropout_rate=0.0, enc_ff_dropout_rate=0.0,
                                enc_layers=2, activation="swish", dec_arch=DecoderArch.LSTM, vocab_size=V, dec_dim=16,
                                dec_units=48, dec_dropout_rate=0.0, dec_layers=2)
    torch.manual_seed(seed)
    model = Transducer(cfg)
    d = np.load(os.path.join(HERE, "transducer.npz"))
    enc = {k[len("init.encoder."):]: torch.from_numpy(d[k]) for k in d.files if k.startswith("init.encoder.")}
    missing, unexpected = model.encoder.load_state_dict(enc, strict=False)
    assert not unexpected and all(k.endswith(".pe") for k in missing), (missing, unexpected)
    with torch.no_grad():
        model.lin_jnt.weight.mul_(6.0)
        model.lin_dec.weight.mul_(4.0)
        model.lin_jnt.bias[0] -= 3.0
    model.eval()
    return model


def run(V, T, seed):
    model = build(V, seed)
    x = torch.randn(1, T, 40, generator=torch.Generator().manual_seed(1000 + seed))
    pops, final, rows, steps = [], [], [], [0]

    def rec_max(hyps, key):
        best = max(hyps, key=key)
        sc = sorted((key(h) for h in hyps), reverse=True)
        pops.append((list(best.yseq), float(best.score), len(hyps), sc[0] - sc[1] if len(sc) > 1 else np.inf))
        return best

    def rec_sorted(hyps, key, reverse=False):
        out = sorted(hyps, key=key, reverse=reverse)
        final.extend(key(h) for h in out)
        return out

    rnn, joint = model.decoder.rnn_forward, model.joint

    def rec_rnn(*a):
        steps[0] += 1
        return rnn(*a)

    def rec_joint(hi, y):
        z = joint(hi, y)
        rows.append(torch.log_softmax(z, dim=-1).clone())
        return z

    model.decoder.rnn_forward, model.joint = rec_rnn, rec_joint
    ref_mod.max, ref_mod.sorted = rec_max, rec_sorted
    try:
        with torch.no_grad():
            yseq = model.inference(x)
    finally:
        del ref_mod.max, ref_mod.sorted
    Tp = ((T - 1) // 2 - 1) // 2
    assert len(pops) == 10 * Tp == len(rows) and len(final) == 10
    init = {k: v.clone() for k, v in model.state_dict().items() if not k.startswith("encoder.")}
    return dict(V=np.array(V), T=np.array(T), seed=np.array(seed), x=x[0], yseq=np.array(yseq, dtype=np.int64),
                best_score=np.array(final[0]), pop_yseq=np.array([t for p in pops for t in p[0]], dtype=np.int32),
                pop_off=np.cumsum([0] + [len(p[0]) for p in pops]).astype(np.int32),
                pop_score=np.array([p[1] for p in pops]), pop_nA=np.array([p[2] for p in pops], dtype=np.int32),
                steps=np.array(steps[0]), logp=torch.stack(rows), margin_a=np.array(min(p[3] for p in pops)),
                margin_b=np.array(final[0] - final[1]), **{"init." + k: v for k, v in init.items()})


def needed(c):
    Tp = ((int(c["T"]) - 1) // 2 - 1) // 2
    return 10 * MAX_DLOGP * (Tp + len(c["yseq"]))


def scan(n):
    for V, T, _ in CASES:
        best = None
        for seed in range(n):
            c = run(V, T, seed)
            distinct = len(set(c["yseq"].tolist()) - {0})
            ratio = float(c["margin_a"]) / needed(c)
            if (distinct >= 3 or T == 7) and (best is None or ratio > best[1]):
                best = (seed, ratio, float(c["margin_a"]), float(c["margin_b"]), len(c["yseq"]), distinct)
        print(f"V {V} T {T}: seed, margin_a / needed, margin_a, margin_b, len, distinct = {best}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scan", type=int, default=0, help="scan this many seeds per shape and print the best")
    a = ap.parse_args()
    torch.set_num_threads(4)
    if a.scan:
        return scan(a.scan)
    arrs = {"n_cases": np.array(len(CASES))}
    for i, (V, T, seed) in enumerate(CASES):
        c = run(V, T, seed)
        assert float(c["margin_a"]) >= needed(c), (V, T, seed, float(c["margin_a"]), needed(c))
        print(f"case {i}: V {V} T {T} seed {seed} yseq {c['yseq'].tolist()} steps {int(c['steps'])} "
              f"margin_a {float(c['margin_a']):.3g} (needs {needed(c):.3g}) margin_b {float(c['margin_b']):.3g}")
        arrs.update({f"c{i}.{k}": (v.detach().numpy() if torch.is_tensor(v) else v) for k, v in c.items()})
    path = os.path.join(HERE, "rnnt_search.npz")
    np.savez_compressed(path, **arrs)
    print("wrote rnnt_search.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
