"""Transducer beam search without a GPU: the project's restatement of the reference's
search (tests/rnnt_search_ref.py), fed with torch CPU fp32 arithmetic (oracle encoder, LSTM
cells and joint from the golden state_dict), reproduces the reference's own run recorded in
tests/golden/rnnt_search.npz: every pop's yseq, the final yseq, the number of executed LSTM
steps exactly, the popped and final scores to 1e-5.  And the host-only size entry
lasr_rnnt_search_workspace answers the formula documented in include/liteasr_hip.h."""

import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rnnt_search_ref as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
N_CASES = 4


def load_case(i):
    """Case i of rnnt_search.npz: dict with the full init state_dict (encoder from
    transducer.npz, as the generator built it), x [1, T, 40] and the recorded run."""
    d = np.load(os.path.join(GOLDEN, "rnnt_search.npz"))
    t = np.load(os.path.join(GOLDEN, "transducer.npz"))
    pre = f"c{i}."
    c = {k[len(pre):]: d[k] for k in d.files if k.startswith(pre)}
    init = {k[5:]: torch.from_numpy(t[k]) for k in t.files if k.startswith("init.encoder.")}
    init.update({k[5:]: torch.from_numpy(v) for k, v in c.items() if k.startswith("init.")})
    off = c["pop_off"]
    return dict(V=int(c["V"]), T=int(c["T"]), init=init, x=torch.from_numpy(c["x"])[None],
                yseq=c["yseq"].tolist(), best_score=float(c["best_score"]),
                pops=[tuple(c["pop_yseq"][off[j]:off[j + 1]].tolist()) for j in range(len(off) - 1)],
                pop_score=c["pop_score"], pop_nA=c["pop_nA"].tolist(), steps=int(c["steps"]), logp=c["logp"],
                margin_a=float(c["margin_a"]), margin_b=float(c["margin_b"]))


def cpu_arith(case):
    """(T', step, logp) in torch CPU fp32 from the case's state_dict."""
    from oracle import transducer_ref as TR
    from oracle import u2_oracle as O

    cfg = O.default_cfg(enc_dim=64, enc_heads=4, enc_ff=128, enc_layers=2, vocab_size=case["V"], input_dim=40,
                        dec_layers=2, dec_units=48)
    p = case["init"]
    x = case["x"]
    with torch.no_grad():
        h, _ = O.encoder(x, torch.tensor([x.shape[1]]), p, cfg, p, False)
    h = h[0]

    def step(node):
        xin = p["decoder.embed.weight"][node.token][None]
        hs, cs = [], []
        for n in range(2):
            if node.parent is None:
                h0 = c0 = torch.zeros(1, 48)
            else:
                h0, c0 = node.parent.state[0][n], node.parent.state[1][n]
            hn, cn = TR.lstm_cell(xin, h0, c0, p, f"decoder.dec_layers.{n}")
            hs.append(hn)
            cs.append(cn)
            xin = hn
        return hs, cs

    def logp(t, node):
        return torch.log_softmax(TR.joint(h[t], node.state[0][-1][0], p), -1).tolist()

    return h.shape[0], step, logp


@pytest.mark.parametrize("i", range(N_CASES))
def test_restatement_reproduces_reference_run(i):
    case = load_case(i)
    Tp, step, logp = cpu_arith(case)
    assert Tp == ((case["T"] - 1) // 2 - 1) // 2
    trace = []
    with torch.no_grad():
        yseq, best, steps = R.beam_search(Tp, step, logp, trace)
    assert [t[0] for t in trace] == case["pops"]
    assert [t[2] for t in trace] == case["pop_nA"]
    assert yseq == case["yseq"]
    assert steps == case["steps"]
    assert np.abs(np.array([t[1] for t in trace]) - case["pop_score"]).max() <= 1e-5
    assert abs(best - case["best_score"]) <= 1e-5


def test_restatement_edges():
    assert R.beam_search(0, None, None) == ([0], 0.0, 0)
    # uniform rows: ties go to the smaller token, the first maximum in list order is popped
    trace = []
    yseq, best, steps = R.beam_search(1, lambda n: 0, lambda t, n: [-2.0] * 12, trace)
    assert trace[0] == ((0,), 0.0, 1) and trace[1] == ((0, 1), -2.0, 10) and trace[2][0] == (0, 2)
    assert steps == 10 and yseq == [0] and best == -2.0


def _formula(Tcap, layers, H, J, V, node_cap=0, slot_cap=0):
    up = lambda x: -(-x // 256) * 256  # noqa: E731
    node_cap = node_cap if node_cap > 0 else 100 * Tcap + 1
    slot_cap = slot_cap if slot_cap > 0 else 10 * Tcap + 1
    hash_cap = 64
    while hash_cap < 2 * node_cap:
        hash_cap *= 2
    slot_floats = -(-(2 * layers * H + J) // 64) * 64
    return (up(64 * 4) + up(2 * 16 * 4) + up((10 * Tcap + 2) * 4) + up(120 * 16) + up(10 * Tcap * 16)
            + up(node_cap * 16) + up(hash_cap * 4) + up(V * 4) + up(slot_cap * slot_floats * 4))


def test_workspace_formula():
    from liteasr_amd import _native

    L = _native.load()
    for shape in ((16, 2, 48, 24, 20, 0, 0), (249, 2, 2048, 768, 4233, 0, 0), (7, 1, 200, 24, 97, 33, 5)):
        assert L.lasr_rnnt_search_workspace(*shape) == _formula(*shape), shape
    assert L.lasr_rnnt_search_workspace(0, 2, 48, 24, 20, 0, 0) == 0
