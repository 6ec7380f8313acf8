"""Child process of tests/test_switches_gpu.py: one bf16 training step (forward + hybrid loss +
backward) of BASELINE config 2's full model (12 / 6 layers, d 256, V 4233) at B 2 x T 1000,
dropout 0.1, from seeded weights and batch; saves the loss, the flat gradient and the BN
running statistics.  The A/B switch under test: a C-side one through the environment of the
process (read once, at library load), a Python one as a MODULE.ATTR=VALUE argument after the
output path (tools/flag_ab.py's format), set here before the model is built."""

import ast
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(out_path, sets=()):
    for item in sets:
        name, val = item.split("=", 1)
        mod, attr = name.rsplit(".", 1)
        m = importlib.import_module(mod)
        assert hasattr(m, attr), name
        setattr(m, attr, ast.literal_eval(val))
    from bench import CONFIGS, V, build
    from liteasr_amd.criterions.hybrid_ctc_attn import HybridCTCLoss, HybridCTCLossConfig
    from liteasr_amd.utils.synthetic import synthetic_batch

    torch.manual_seed(42)
    dev = torch.device("cuda", 0)
    cfgd = dict(CONFIGS["small"], B=2)
    model = build(cfgd, "bf16", 0.1, dev)
    crit = HybridCTCLoss(HybridCTCLossConfig(vocab_size=V, smoothing=0.1, ctc_weight=0.3))
    xs, xlens, ys, ylens = (t.to(dev) for t in synthetic_batch(2, 1000, 40, V, seed=7))
    model.store.ensure_grad().zero_()
    loss = crit(model, xs, xlens, ys, ylens)
    loss.backward()
    torch.cuda.synchronize()
    torch.save({"loss": loss.detach().cpu(), "grad": model.store.grad.detach().cpu(),
                "bn": [b.detach().cpu() for b in model.bn_flat_buffers()]}, out_path)
    print("saved", out_path, float(loss), flush=True)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2:])
