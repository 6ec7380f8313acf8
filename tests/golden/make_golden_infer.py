"""Generate tests/golden/infer.json by running the *reference's* own ``levenshtein``
(liteasr/utils/score.py) and ``load_ckpt`` (liteasr/utils/checkpoint.py) through refshim.

    python tests/golden/make_golden_infer.py

The fixture holds data only:

* ``lev``: seeded pairs of strings and of integer lists with the reference's distance; the
  first ones are the edge cases (an empty side, both empty, equal inputs, swapped lengths);
* ``ckpt``: five small state dicts (float tensors and one int64 counter), the order of their
  modification times, the ``valid loss:`` log lines in the trainer's format, and what the
  reference's ``load_ckpt`` returns for the averaging cases of tests/test_infer_cpu.py;
* ``lines``: the per-utterance and error-rate log lines as the reference's format strings
  (liteasr/infer.py:60,90-94) render them for a few (ref, hyp) pairs.
"""

import json
import os
import sys
import tempfile
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import refshim  # noqa: E402

refshim.install()
from liteasr.utils.checkpoint import load_ckpt  # noqa: E402
from liteasr.utils.score import levenshtein  # noqa: E402

LOSSES = [5.0, 1.5, 4.0, 1.0, 3.0]  # epochs 1..5: the two lowest (4, 2) are not the two latest
LOG_LINE = "[2024-01-01 00:00:0{e},000][liteasr_amd.trainer][INFO] - {i} / 30 iters, {e} / 5 epochs - valid loss: {l:.2f}"


def lev_pairs():
    rng = np.random.default_rng(11)
    pairs = [("", ""), ("", "abc"), ("abc", ""), ("kitten", "kitten"), ("kitten", "sitting"), ("sitting", "kitten"),
             ([], [1, 2, 3]), ([4, 5, 6], [4, 5, 6]), ([1, 2, 3, 4, 5, 6, 7], [2, 3]), ([2, 3], [1, 2, 3, 4, 5, 6, 7])]
    alpha = "abcde"
    for _ in range(20):
        a = "".join(rng.choice(list(alpha), rng.integers(0, 12)))
        b = "".join(rng.choice(list(alpha), rng.integers(0, 12)))
        pairs.append((a, b))
    for _ in range(20):
        a = rng.integers(0, 6, rng.integers(0, 15)).tolist()
        b = rng.integers(0, 6, rng.integers(0, 15)).tolist()
        pairs.append((a, b))
    return [{"a": a, "b": b, "d": int(levenshtein(a, b))} for a, b in pairs]


def states():
    g = torch.Generator().manual_seed(5)
    out = []
    for e, nb in enumerate([3, 10, 7, 12, 20]):
        out.append({"enc.weight": torch.randn(3, 4, generator=g), "enc.bias": torch.randn(4, generator=g) * 10,
                    "bn.num_batches_tracked": torch.tensor(nb, dtype=torch.int64)})
    return out


def write_run(d, sts):
    """Checkpoints with increasing mtimes in d/ckpts, the log next to (not inside) it."""
    ck = os.path.join(d, "ckpts")
    os.makedirs(ck)
    for e, sd in enumerate(sts, 1):
        p = os.path.join(ck, f"model.ep.{e}.pt")
        torch.save(sd, p)
        os.utime(p, (1_000_000 + 10 * e, 1_000_000 + 10 * e))
    log = os.path.join(d, "train.log")
    with open(log, "w") as f:
        f.write("[2024-01-01 00:00:00,000][liteasr_amd.train][INFO] - set random seed as 7\n")
        for e, l in enumerate(LOSSES, 1):
            f.write(LOG_LINE.format(e=e, i=6 * e, l=l) + "\n")
            f.write(f"[2024-01-01 00:00:0{e},500][liteasr_amd.trainer][INFO] - saving model.ep.{e}.pt\n")
    return ck, log


def tolist(sd):
    return {k: {"dtype": str(v.dtype).replace("torch.", ""), "shape": list(v.shape),
                "data": v.reshape(-1).tolist()} for k, v in sd.items()}


def main():
    sts = states()
    out = {"lev": lev_pairs(), "ckpt": {"states": [tolist(s) for s in sts], "losses": LOSSES, "log_line": LOG_LINE}}
    cases = {"single": dict(ckpt_name=2, model_avg=False, avg_num=1, avg_policy=None),
             "last3": dict(ckpt_name=4, model_avg=True, avg_num=3, avg_policy=None),
             "loss2": dict(ckpt_name=5, model_avg=True, avg_num=2, avg_policy="LOG")}
    for name, c in cases.items():
        with tempfile.TemporaryDirectory() as d:
            ck, log = write_run(d, sts)
            cfg = SimpleNamespace(ckpt_path=ck, **dict(c, avg_policy=log if c["avg_policy"] else None))
            out["ckpt"][name] = {"cfg": c, "expect": tolist(load_ckpt(cfg))}
    lines = []
    for ref, hyp in [("abc", "abc"), ("hello world", "helo wrld"), ("", "x"), ("a" * 120, "b")]:
        err = levenshtein(ref, hyp)
        lines.append({"ref": ref, "hyp": hyp,
                      "utt": "\n{} {}\n{:>3} {}".format("[X]" if ref == hyp else "[ ]", hyp, err, ref)})
    out["lines"] = {"utt": lines, "rate": [{"err": e, "len": n, "text": "Error rate: {} / {} = {:.2%}".format(e, n, e / n)}
                                           for e, n in [(0, 10), (7, 123), (250, 200), (1, 3)]]}
    path = os.path.join(HERE, "infer.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote infer.json", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
