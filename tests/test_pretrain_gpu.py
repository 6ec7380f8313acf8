"""The pretraining data path on the GPU: ``lasr_pcm_to_float`` bit for bit, Wav2Vec2.forward on
an int16 source against the same samples as fp32, two Trainer steps fed by the int16 and by the
float collation of RawAudioFileDataset, and ``task=pretrain`` through the CLI path
(tests/golden/pretrain_data/, made by tests/golden/make_golden_pretrain.py)."""

import json
import logging
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import pretrain_cases as P
import wav2vec2_cases as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
SIZES = [1, 7, 8, 9, 255, 2048, 2049, 12000]


def _buffer():
    """12003 int16 samples holding -32768, 32767 and 0 in each of the views' first three."""
    pcm = torch.from_numpy(np.random.default_rng(11).integers(-32768, 32768, size=max(SIZES) + 3).astype(np.int16))
    pcm[:9] = torch.tensor([-32768, 32767, 0, 32767, -32768, 0, -32768, 32767, 0], dtype=torch.int16)
    return pcm


@pytest.mark.parametrize("offset", [0, 1, 3])
def test_pcm_to_float_is_exact(offset):
    """Every n of SIZES on the buffer itself (16-byte aligned), on buf[1:] (2-byte aligned only:
    a 7-sample head) and on buf[3:] (a 5-sample head): equal bits to int16 / 32768 on the host."""
    from liteasr_amd import kernels as K

    host = _buffer()
    buf = host.to(DEV)
    assert buf.data_ptr() % 16 == 0
    for n in SIZES:
        view = buf[offset:offset + n]
        assert view.data_ptr() % 16 == (2 * offset) % 16
        out = K.pcm_to_float(view)
        ref = host[offset:offset + n].float() / 32768
        assert out.dtype == torch.float32 and out.shape == (n,)
        assert torch.equal(out.cpu(), ref), (offset, n)
        if n >= 3:
            assert out[:3].cpu().tolist() == [v / 32768 for v in host[offset:offset + 3].tolist()]
    # a (B, S) batch into a caller's buffer, guard values around it untouched
    guard = torch.full((3 * 255 + 16,), 7.0, device=DEV)
    K.pcm_to_float(buf[:3 * 255].view(3, 255), out=guard[8:8 + 3 * 255])
    torch.cuda.synchronize()
    assert torch.equal(guard[8:8 + 3 * 255].cpu(), host[:3 * 255].float() / 32768)
    assert (guard[:8] == 7).all() and (guard[8 + 3 * 255:] == 7).all()
    with pytest.raises(TypeError):
        K.pcm_to_float(buf.float())


def _golden_source():
    """3 x 4000 int16 samples: the first three segments of the golden directory."""
    from liteasr_amd.utils import wavio

    g = P.golden()
    rows = []
    for i in range(3):
        pcm, got = wavio.read(os.path.join(P.WAV, str(g["seg.wav"][i])), int(g["seg.start"][i]), 4000)
        assert got == 4000 and int(g["seg.shape"][i]) >= 4000
        rows.append(torch.from_numpy(pcm))
    return torch.stack(rows)


def test_model_int16_source_equals_fp32_source():
    """Train mode, the tiny fp32 model, freshly built and seeded alike for each forward: logits,
    loss and every parameter gradient of the int16 source equal the fp32 source's bit for bit."""
    from liteasr_amd.models.wav2vec2 import Wav2Vec2

    pcm = _golden_source()
    sources = [(pcm.float() / 32768).to(DEV), pcm.to(DEV)]
    assert sources[0].dtype == torch.float32 and sources[1].dtype == torch.int16
    runs = []
    for src in sources:
        model = Wav2Vec2(C.model_config("fp32"))
        model.load_state_dict(C.golden_state())
        model = model.to(DEV).train()
        np.random.seed(31)
        torch.manual_seed(32)
        logits = model(src)
        model.last.loss.backward()
        torch.cuda.synchronize()
        grads = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()}
        runs.append((logits.detach().cpu(), model.last.loss.detach().cpu(), grads))
    (la, sa, ga), (lb, sb, gb) = runs
    assert la.shape[1] == 11 and torch.isfinite(sa)
    assert torch.equal(la, lb) and torch.equal(sa, sb)
    assert set(ga) == set(gb) and len(ga) > 20
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
    assert any(float(v.abs().max()) > 0 for v in ga.values())


def test_trainer_int16_and_float_collation_agree(tmp_path):
    """Two eager Trainer steps in a fresh process per collation, seeded alike: the same iteration
    count, no skipped step, finite losses, the same parameter bits."""
    d = P.data_dir(tmp_path, "seg")
    outs = {}
    for mode in ("pcm", "float"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_pretrain_trainer_step.py"), d, mode],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        outs[mode] = json.loads(r.stdout.strip().splitlines()[-1])
    a, b = outs["pcm"], outs["float"]
    assert [s[0] for s in a["seen"]] == ["torch.int16"] * 2 and [s[0] for s in b["seen"]] == ["torch.float32"] * 2
    assert [s[1] for s in a["seen"]] == [s[1] for s in b["seen"]]
    for o in (a, b):
        assert o["iters"] == 2 and o["skipped"] == 0 and len(o["losses"]) == 2
        assert all(math.isfinite(v) for v in o["losses"])
    assert a["losses"] == b["losses"] and a["digest"] == b["digest"]


def test_cli_pretrain_end_to_end(tmp_path, monkeypatch):
    """``task=pretrain`` composed from the presets with the tiny model by overrides: two iterations,
    their loss lines in train.log, then Trainer.valid() over the same directory."""
    from liteasr_amd import train as T

    d = P.data_dir(tmp_path, "seg")
    monkeypatch.chdir(tmp_path)
    root = logging.getLogger()
    saved = root.handlers[:], root.level
    argv = ["task=pretrain", f"task.train={d}", f"task.valid={d}", "model=wav2vec2", "criterion=wav2vec",
            "optimizer=noam", "optimizer.model_dim=64", "model.encoder_layers=2", "model.encoder_embed_dim=64",
            "model.encoder_ffn_embed_dim=128", "model.encoder_attention_heads=4", "model.final_dim=32",
            "model.latent_vars=16", "model.num_negatives=10",
            "model.conv_feature_layers='[(32, 10, 5)] + [(32, 3, 2)] * 2 + [(32, 2, 2)]'",
            f"+dataset.max_batch_frame={P.SMALL_BUDGET}", "distributed.num_workers=0", "optimization.max_epoch=-1",
            "optimization.max_iter=2", "common.trigger=[{name: report_loss, interval: 1, unit: iteration}]",
            "hydra.run.dir=runs/pretrain"]
    try:
        cfg, run_dir = T.prepare(argv)
        assert cfg.task.name == "pretrain" and cfg.model.conv_feature_layers.startswith("[(32, 10, 5)]")
        tr = T.build_trainer(cfg)
        assert type(tr.task).__name__ == "PreTrainTask" and len(tr.task.dataset("train")) == 5
        tr.run()
        torch.cuda.synchronize()
        assert tr.iter == 2 and tr.skipped == 0
        valid = tr.valid()
        assert math.isfinite(valid)
        for h in root.handlers:
            h.flush()
        log = open(os.path.join(run_dir, "train.log")).read()
        vals = [float(v) for v in re.findall(r"current loss: (\S+)", log)]
        assert len(vals) == 2 and all(math.isfinite(v) for v in vals), log[-2000:]
        assert "valid loss" in log
    finally:
        for h in root.handlers[:]:
            if h not in saved[0]:
                root.removeHandler(h)
                h.close()
        root.setLevel(saved[1])
