"""Child process of tests/test_pretrain_gpu.py: two eager Trainer steps of the tiny wav2vec 2.0
model with Noam/Adam under fixed seeds, fed by RawAudioFileDataset over a realised copy of
tests/golden/pretrain_data/seg (argv[1]) with the collation named by argv[2] ("pcm": int16
batches converted on the device, "float": the reference's float32 batches); prints one JSON line
(losses, iterations, skipped steps, the dtype the criterion saw, a digest of every parameter)."""

import hashlib
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import pretrain_cases as P
    import wav2vec2_cases as C
    from liteasr_amd.criterions.wav2vec_loss import Wav2Vec2Loss, Wav2Vec2LossConfig
    from liteasr_amd.dataset import RawAudioFileDataset
    from liteasr_amd.models.wav2vec2 import Wav2Vec2
    from liteasr_amd.optims.noam import Noam, NoamConfig
    from liteasr_amd.trainer import Trainer

    data_dir, mode = sys.argv[1], sys.argv[2]
    torch.manual_seed(5)
    np.random.seed(5)
    cfg_m = C.model_config("bf16")
    cfg_m.dropout = 0.1
    model = Wav2Vec2(cfg_m).to("cuda").train()
    data = RawAudioFileDataset(data_dir, P.small_cfg(), None, raw_pcm=mode == "pcm")
    task = SimpleNamespace(dataset=lambda split: data)
    cfg = SimpleNamespace(distributed=SimpleNamespace(num_workers=0), common=SimpleNamespace(trigger=[]),
                          optimization=SimpleNamespace(max_epoch=-1, max_iter=2, accum_grad=1, clip_grad_norm=5.0))
    tr = Trainer(cfg, task, model, Wav2Vec2Loss(Wav2Vec2LossConfig()),
                 Noam(model.parameters(), NoamConfig(model_dim=64, warmup=100)), device="cuda")
    losses, seen = [], []
    crit = tr.criterion

    def recording(m, xs, *rest):
        assert rest == (None, None, None)
        seen.append([str(xs.dtype), list(xs.shape)])
        loss = crit(m, xs, *rest)
        losses.append(float(loss.detach()))
        return loss

    tr.criterion = recording
    tr.run()
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for k, v in model.named_parameters():
        h.update(v.detach().cpu().numpy().tobytes())
    print(json.dumps({"losses": losses[:2], "iters": tr.iter, "skipped": tr.skipped, "seen": seen[:2],
                      "digest": h.hexdigest()}))


if __name__ == "__main__":
    main()
