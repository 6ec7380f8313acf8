"""Child process of tests/test_resample_gpu.py: ``task=asr_wav`` composed like the CLI composes it
(tiny conformer, SpecAugment on, fixed seeds) with the train directory argv[1], the valid
directory argv[2], the run directory argv[3] and ``task.frontend.speed_perturb`` argv[4] (a list
such as [0.9,1.0,1.1], or null); two Trainer steps, then ``Trainer.valid()``.  Prints one JSON
line: the two losses, the validation loss, the dtype, shape and tuple length of what the collator
delivered, whether a ResamplePlan rode along, and the shapes and lengths the criterion saw."""

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
    from liteasr_amd.utils.frontend import ResamplePlan

    train, valid, run, speed = sys.argv[1:5]
    argv = ["task=asr_wav", f"task.vocab={train}/vocab.txt", f"task.train={train}", f"task.valid={valid}",
            f"task.save_dir={run}/ckpts", f"task.frontend.speed_perturb={speed}", "model=conformer_tiny",
            "criterion=hybrid_ctc_w03", "optimizer=noam_d256", "optimizer.model_dim=64", "dataset.batch_count=seq",
            "dataset.batch_size=3", "dataset.min_batch_size=1", "dataset.max_len_in=1000", "dataset.max_len_out=150",
            "postprocess.spec_aug.time_warp=5", "postprocess.spec_aug.freq_mask=4",
            "postprocess.spec_aug.freq_mask_times=2", "postprocess.spec_aug.time_mask=8",
            "postprocess.spec_aug.time_mask_times=2", "distributed.num_workers=0", "optimization.max_epoch=-1",
            "optimization.max_iter=2", "optimization.clip_grad_norm=5.0", "common.seed=7", f"hydra.run.dir={run}"]
    cfg, _ = T.prepare(argv)
    tr = T.build_trainer(cfg)
    delivered, seen, losses = [], [], []
    feats_of = tr._features

    def recording_features(batch):
        delivered.append([str(batch[0].dtype), list(batch[0].shape), len(batch), isinstance(batch[-1], ResamplePlan)])
        return feats_of(batch)

    tr._features = recording_features
    crit = tr.criterion

    def recording(m, xs, xlens, ys, ylens):
        seen.append([str(xs.dtype), list(xs.shape), xlens.tolist(), list(ys.shape), ylens.tolist()])
        loss = crit(m, xs, xlens, ys, ylens)
        losses.append(float(loss.detach()))
        return loss

    tr.criterion = recording
    random.seed(11)  # the SpecAugment plans are drawn from these two in the collator
    np.random.seed(11)
    tr.run()
    torch.cuda.synchronize()
    before = len(seen)  # the preset's epoch triggers may have validated already
    value = tr.valid()
    print(json.dumps({"losses": losses[:2], "iters": tr.iter, "skipped": tr.skipped, "delivered": delivered[:2],
                      "seen": seen[:2], "valid": value, "valid_seen": seen[before:],
                      "valid_delivered": delivered[len(delivered) - (len(seen) - before):],
                      "train_records": len(tr.task.dataset("train").data)}))


if __name__ == "__main__":
    main()
