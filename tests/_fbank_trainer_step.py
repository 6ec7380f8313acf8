"""Child process of tests/test_fbank_gpu.py: ``task=asr_wav`` composed like the CLI composes it
(tiny conformer, SpecAugment on, fixed seeds) over the data directory argv[1], which holds either
wav.scp (raw audio: features from the device front end) or feats.scp (the same features dumped
beforehand); two Trainer steps, ``Trainer.valid()`` over the same directory, then
``task.inference`` on the first utterance.  Prints one JSON line: the two losses, the validation
loss, the dtype and shape of what the collator delivered and of what the criterion saw, the
hypothesis and its token ids."""

import json
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from liteasr_amd import train as T

    d, run = sys.argv[1], sys.argv[2]
    argv = ["task=asr_wav", f"task.vocab={d}/vocab.txt", f"task.train={d}", f"task.valid={d}",
            f"task.save_dir={run}/ckpts", "model=conformer_tiny", "criterion=hybrid_ctc_w03", "optimizer=noam_d256",
            "optimizer.model_dim=64", "dataset.batch_count=seq", "dataset.batch_size=2", "dataset.min_batch_size=1",
            "dataset.max_len_in=1000", "dataset.max_len_out=150", "postprocess.spec_aug.time_warp=5",
            "postprocess.spec_aug.freq_mask=4", "postprocess.spec_aug.freq_mask_times=2",
            "postprocess.spec_aug.time_mask=8", "postprocess.spec_aug.time_mask_times=2", "distributed.num_workers=0",
            "optimization.max_epoch=-1", "optimization.max_iter=2", "optimization.clip_grad_norm=5.0", "common.seed=7",
            f"hydra.run.dir={run}"]
    cfg, _ = T.prepare(argv)
    tr = T.build_trainer(cfg)
    delivered, seen, losses = [], [], []
    feats_of = tr._features

    def recording_features(batch):
        delivered.append([str(batch[0].dtype), list(batch[0].shape), len(batch)])
        return feats_of(batch)

    tr._features = recording_features
    crit = tr.criterion

    def recording(m, xs, xlens, ys, ylens):
        seen.append([str(xs.dtype), list(xs.shape), xlens.tolist()])
        loss = crit(m, xs, xlens, ys, ylens)
        losses.append(float(loss.detach()))
        return loss

    tr.criterion = recording
    random.seed(11)  # the SpecAugment plans are drawn from these two in the collator
    np.random.seed(11)
    tr.run()
    torch.cuda.synchronize()
    before = len(seen)  # the preset's epoch triggers may have validated already
    valid = tr.valid()
    task, model = tr.task, tr._model.eval()
    task.load_dataset("test", d, None, None)
    item = task.dataset("test")[0]
    ids = []
    inner = model.inference

    def recording_inference(x, *a, **k):
        ids.append([str(x.dtype), list(x.shape)])
        out = list(inner(x, *a, **k))
        ids.append([int(v) for v in out])
        return out

    model.inference = recording_inference
    with torch.no_grad():
        hyp = task.inference(item.x.unsqueeze(0).to("cuda"), model)
    print(json.dumps({"losses": losses[:2], "iters": tr.iter, "skipped": tr.skipped, "delivered": delivered[:2],
                      "seen": seen[:2], "valid": valid, "valid_batches": len(seen) - before,
                      "feat_dim": task.feat_dim, "item": str(item.x.dtype), "hyp": hyp, "model_saw": ids[0],
                      "ids": ids[1]}))


if __name__ == "__main__":
    main()
