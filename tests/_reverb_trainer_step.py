"""Child process of tests/test_reverb_gpu.py: ``task=asr_wav`` composed like the CLI composes it (tiny
conformer, SpecAugment on, fixed seeds) with the train directory argv[1], the valid directory
argv[2], the run directory argv[3] and options ``key=value`` after them: ``rir``, ``rir_prob``,
``rir_seed``, ``noise`` and ``speed_perturb`` go to ``task.frontend``; ``dump=DIR`` writes, before
anything else, a copy of the train directory whose WAV files hold every utterance reverberated by
RIR 0 of the bank, each through a call of its own; ``check=1`` compares what ``_features`` hands to
the fbank kernel with the resampler, ``reverb_i16`` and ``mix_i16`` called by hand on the delivered
plans.  ``Trainer.valid()`` on the freshly initialised model, then two Trainer steps.  Prints one
JSON line: the two losses, the validation loss, the dtype, shape, tuple length and plan names of
what the collator delivered, how many rows were reverberated and with which RIRs, and the shapes and
lengths the criterion saw."""

import json
import os
import random
import shutil
import sys
import wave

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def dump_reverberated(train, dest, reverb):
    """``train`` again at ``dest``, every utterance convolved with RIR 0, alone in its batch."""
    from liteasr_amd.utils.frontend import ReverbPlan
    from liteasr_amd.utils.synthetic import write_wav

    os.makedirs(os.path.join(dest, "wav"), exist_ok=True)
    for name in ("text", "vocab.txt"):
        shutil.copy(os.path.join(train, name), os.path.join(dest, name))
    with open(os.path.join(train, "wav.scp")) as f, open(os.path.join(dest, "wav.scp"), "w") as scp:
        for line in f:
            uttid, path = line.split()
            with wave.open(path, "rb") as w:
                x = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").copy()
            pcm = torch.from_numpy(x).view(1, -1).cuda()
            y = reverb(pcm, ReverbPlan(torch.tensor([[x.shape[0], 0]], dtype=torch.int32)))
            out = os.path.join(dest, "wav", uttid + ".wav")
            write_wav(out, y[0].cpu().numpy())
            scp.write(f"{uttid} {out}\n")


def main():
    from liteasr_amd import kernels as K
    from liteasr_amd import train as T
    from liteasr_amd.utils.frontend import NoisePlan, ResamplePlan, ReverbPlan

    train, valid, run = sys.argv[1:4]
    opts = dict(a.split("=", 1) for a in sys.argv[4:])
    argv = ["task=asr_wav", f"task.vocab={train}/vocab.txt", f"task.train={train}", f"task.valid={valid}",
            f"task.save_dir={run}/ckpts", "model=conformer_tiny",
            "criterion=hybrid_ctc_w03", "optimizer=noam_d256", "optimizer.model_dim=64", "dataset.batch_count=seq",
            "dataset.batch_size=3", "dataset.min_batch_size=1", "dataset.max_len_in=1000", "dataset.max_len_out=150",
            "postprocess.spec_aug.time_warp=5", "postprocess.spec_aug.freq_mask=4",
            "postprocess.spec_aug.freq_mask_times=2", "postprocess.spec_aug.time_mask=8",
            "postprocess.spec_aug.time_mask_times=2", "distributed.num_workers=0", "optimization.max_epoch=-1",
            "optimization.max_iter=2", "optimization.clip_grad_norm=5.0", "common.seed=7", f"hydra.run.dir={run}"]
    for key in ("rir", "rir_prob", "rir_seed", "noise", "speed_perturb"):
        if key in opts:
            argv.append(f"task.frontend.{key}={opts[key]}")
    if "noise" in opts:
        argv += ["task.frontend.noise_prob=0.8", "task.frontend.noise_seed=5"]
    cfg, _ = T.prepare(argv)
    tr = T.build_trainer(cfg)
    fe = tr.task.frontend
    if "dump" in opts:
        dump_reverberated(train, opts["dump"], fe.reverb)
    delivered, seen, losses, counts, rirs, handed = [], [], [], [], [], []
    checked = 0
    feats_of = tr._features

    class Spy(type(fe)):
        def __call__(self, pcm, *args, **kw):
            handed.append(pcm.clone())
            return super().__call__(pcm, *args, **kw)

    fe.__class__ = Spy

    def by_hand(batch):
        """speed -> reverb -> noise through the kernels, on the plans the collator delivered."""
        plans = {type(p): p for p in batch[4:] if isinstance(p, (ResamplePlan, ReverbPlan, NoisePlan))}
        pcm = batch[0].cuda()
        rp, vp, nz = plans[ResamplePlan], plans[ReverbPlan], plans[NoisePlan]
        table, taps = (torch.from_numpy(v).cuda() for v in K.resample_tables(rp.ratios))
        pcm = K.resample_i16(pcm, rp.rows.cuda(), table, taps, max_out=rp.max_out)
        assert vp.rows[:, 0].tolist() == rp.rows[:, 1].tolist() == nz.rows[:, 0].tolist()
        bank, rtab = fe.reverb.tables_on(pcm.device)
        wet = K.reverb_i16(pcm, bank, vp.rows.cuda(), rtab)
        return K.mix_i16(wet, fe.noise.bank_on(pcm.device), nz.rows.cuda(), nz.sources.cuda())

    def recording_features(batch):
        nonlocal checked
        names = [type(p).__name__ for p in batch[4:] if isinstance(p, (ResamplePlan, ReverbPlan, NoisePlan))]
        delivered.append([str(batch[0].dtype), list(batch[0].shape), len(batch), names])
        vp = [p for p in batch[4:] if isinstance(p, ReverbPlan)]
        ids = vp[0].rows[:, 1].tolist() if vp else []
        rirs.append(ids)
        counts.append(sum(i >= 0 for i in ids))
        out = feats_of(batch)
        if opts.get("check") and len(names) == 3:
            want = by_hand(batch)
            assert handed[-1].dtype == torch.int16 and torch.equal(handed[-1], want)
            checked += 1
        return out

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
                      "delivered": delivered[nvalid:nvalid + 2], "reverberated": counts[nvalid:nvalid + 2],
                      "rirs": rirs[nvalid:nvalid + 2], "seen": seen[nvalid:nvalid + 2], "valid": value,
                      "valid_seen": seen[:nvalid], "valid_delivered": delivered[:nvalid], "checked": checked}))


if __name__ == "__main__":
    main()
