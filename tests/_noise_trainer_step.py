"""Child process of tests/test_noise_gpu.py: ``task=asr_wav`` composed like the CLI composes it (tiny
conformer, SpecAugment on, fixed seeds) with the train directory argv[1], the valid directory
argv[2], the run directory argv[3] and ``task.frontend.noise`` argv[4] (a list of noise
directories, or null); ``Trainer.valid()`` on the freshly initialised model, then two Trainer steps.
Prints one JSON line: the two losses, the validation loss, the dtype, shape and tuple length of what
the collator delivered, whether a NoisePlan rode along and how many sources it held, and the shapes
and lengths the criterion saw."""

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
    from liteasr_amd.utils.frontend import NoisePlan

    train, valid, run, noise = sys.argv[1:5]
    argv = ["task=asr_wav", f"task.vocab={train}/vocab.txt", f"task.train={train}", f"task.valid={valid}",
            f"task.save_dir={run}/ckpts", f"task.frontend.noise={noise}", "task.frontend.noise_prob=0.9",
            "task.frontend.noise_snr=[0,10,5,15]", "task.frontend.noise_sources=[1,2,3,5]",
            "task.frontend.noise_seed=5", "model=conformer_tiny",
            "criterion=hybrid_ctc_w03", "optimizer=noam_d256", "optimizer.model_dim=64", "dataset.batch_count=seq",
            "dataset.batch_size=3", "dataset.min_batch_size=1", "dataset.max_len_in=1000", "dataset.max_len_out=150",
            "postprocess.spec_aug.time_warp=5", "postprocess.spec_aug.freq_mask=4",
            "postprocess.spec_aug.freq_mask_times=2", "postprocess.spec_aug.time_mask=8",
            "postprocess.spec_aug.time_mask_times=2", "distributed.num_workers=0", "optimization.max_epoch=-1",
            "optimization.max_iter=2", "optimization.clip_grad_norm=5.0", "common.seed=7", f"hydra.run.dir={run}"]
    cfg, _ = T.prepare(argv)
    tr = T.build_trainer(cfg)
    delivered, seen, losses, sources = [], [], [], []
    feats_of = tr._features

    def recording_features(batch):
        has = isinstance(batch[-1], NoisePlan)
        delivered.append([str(batch[0].dtype), list(batch[0].shape), len(batch), has])
        sources.append(int(batch[-1].rows[:, 2].sum()) if has else 0)
        return feats_of(batch)

    tr._features = recording_features
    crit = tr.criterion

    def recording(m, xs, xlens, ys, ylens):
        seen.append([str(xs.dtype), list(xs.shape), xlens.tolist(), list(ys.shape), ylens.tolist()])
        loss = crit(m, xs, xlens, ys, ylens)
        losses.append(float(loss.detach()))
        return loss

    tr.criterion = recording
    value = tr.valid()  # before any step: the weights are those of the seed, whatever the option
    nvalid = len(seen)
    random.seed(11)  # the SpecAugment plans are drawn from these two in the collator
    np.random.seed(11)
    tr.run()
    torch.cuda.synchronize()
    print(json.dumps({"losses": losses[nvalid:nvalid + 2], "iters": tr.iter, "skipped": tr.skipped,
                      "delivered": delivered[nvalid:nvalid + 2], "sources": sources[nvalid:nvalid + 2],
                      "seen": seen[nvalid:nvalid + 2], "valid": value, "valid_seen": seen[:nvalid],
                      "valid_delivered": delivered[:nvalid]}))


if __name__ == "__main__":
    main()
