"""Host side of the evaluation CLI (liteasr_amd.infer, utils/score.py, utils/checkpoint.py)
against the reference's own results (tests/golden/infer.json, made by
tests/golden/make_golden_infer.py from liteasr/utils/score.py and liteasr/utils/checkpoint.py).
CPU only."""

import json
import os
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "infer.json")))
GROUPS = ["task=asr_kaldi", "model=conformer_small", "criterion=hybrid_ctc_w03", "optimizer=noam_d256"]


def test_levenshtein_matches_reference():
    from liteasr_amd.utils.score import levenshtein

    pairs = GOLD["lev"]
    assert len(pairs) >= 40
    assert any(len(p["a"]) == 0 and len(p["b"]) > 0 for p in pairs) and any(p["a"] == p["b"] and p["a"] for p in pairs)
    for p in pairs:
        assert levenshtein(p["a"], p["b"]) == p["d"], p
        assert levenshtein(p["b"], p["a"]) == p["d"], p  # the reference swaps to the shorter side itself
        assert levenshtein(tuple(p["a"]), tuple(p["b"])) == p["d"]


def _tensors(sd):
    return {k: torch.tensor(v["data"], dtype=getattr(torch, v["dtype"])).reshape(v["shape"]) for k, v in sd.items()}


@pytest.fixture()
def run_dir(tmp_path):
    """Five checkpoints with increasing mtimes in ckpts/, the training log next to it."""
    c = GOLD["ckpt"]
    ck = tmp_path / "ckpts"
    ck.mkdir()
    for e, sd in enumerate(c["states"], 1):
        p = ck / f"model.ep.{e}.pt"
        torch.save(_tensors(sd), p)
        os.utime(p, (1_000_000 + 10 * e, 1_000_000 + 10 * e))
    log = tmp_path / "train.log"
    lines = ["[2024-01-01 00:00:00,000][liteasr_amd.train][INFO] - set random seed as 7"]
    for e, l in enumerate(c["losses"], 1):
        lines.append(c["log_line"].format(e=e, i=6 * e, l=l))
        lines.append(f"[2024-01-01 00:00:0{e},500][liteasr_amd.trainer][INFO] - saving model.ep.{e}.pt")
    log.write_text("\n".join(lines) + "\n")
    return str(ck), str(log)


def _cfg(run_dir, case):
    ck, log = run_dir
    c = dict(GOLD["ckpt"][case]["cfg"])
    c["avg_policy"] = log if c["avg_policy"] else None
    return SimpleNamespace(ckpt_path=ck, **c)


def _check(got, want):
    want = _tensors(want)
    assert set(got) == set(want)
    for k, w in want.items():
        assert got[k].dtype == w.dtype and got[k].shape == w.shape, k
        if w.is_floating_point():
            assert torch.allclose(got[k], w, atol=1e-6, rtol=0), (k, (got[k] - w).abs().max())
        else:
            assert torch.equal(got[k], w), (k, got[k], w)


def test_log_line_is_the_trainers_format():
    """The fixture's log lines end as liteasr_amd.trainer formats its validation line."""
    import inspect

    from liteasr_amd import trainer

    assert '"{} / {} iters, {} / {} epochs - valid loss: {:.2f}"' in inspect.getsource(trainer)
    assert GOLD["ckpt"]["log_line"].endswith("{i} / 30 iters, {e} / 5 epochs - valid loss: {l:.2f}")


def test_load_ckpt_single_is_exact(run_dir):
    from liteasr_amd.utils.checkpoint import load_ckpt

    got = load_ckpt(_cfg(run_dir, "single"))
    want = _tensors(GOLD["ckpt"]["states"][1])
    assert set(got) == set(want) and all(torch.equal(got[k], want[k]) for k in want)
    _check(got, GOLD["ckpt"]["single"]["expect"])


def test_load_ckpt_average_of_last(run_dir):
    from liteasr_amd.utils.checkpoint import load_ckpt, pickup

    cfg = _cfg(run_dir, "last3")
    assert (cfg.avg_num, cfg.ckpt_name, cfg.avg_policy) == (3, 4, None)
    assert [os.path.basename(p) for p in pickup(cfg)] == ["model.ep.2.pt", "model.ep.3.pt", "model.ep.4.pt"]
    got = load_ckpt(cfg)
    _check(got, GOLD["ckpt"]["last3"]["expect"])
    assert got["bn.num_batches_tracked"].item() == (10 + 7 + 12) // 3


def test_load_ckpt_average_by_valid_loss(run_dir):
    from liteasr_amd.utils.checkpoint import load_ckpt, pickup, valid_losses

    cfg = _cfg(run_dir, "loss2")
    assert valid_losses(cfg.avg_policy) == GOLD["ckpt"]["losses"]
    # the two lowest losses (epochs 4 and 2) are not the two latest files
    assert [os.path.basename(p) for p in pickup(cfg)] == ["model.ep.4.pt", "model.ep.2.pt"]
    _check(load_ckpt(cfg), GOLD["ckpt"]["loss2"]["expect"])


def test_load_ckpt_average_reaching_before_the_first_raises(run_dir):
    from liteasr_amd.utils.checkpoint import load_ckpt

    ck, _ = run_dir
    with pytest.raises(AssertionError):
        load_ckpt(SimpleNamespace(ckpt_path=ck, ckpt_name=3, model_avg=True, avg_num=5, avg_policy=None))


def test_inference_overrides_compose():
    from liteasr_amd.config.compose import compose, missing_keys

    cfg = compose(overrides=GROUPS + ["inference.ckpt_name=7", "inference.model_avg=true", "inference.avg_num=3",
                                      "inference.avg_policy=null", "inference.thread_num=1",
                                      "inference.ckpt_path=/x/ckpts", "task.test=[/data/a,/data/b]"], job_name="infer")
    inf = cfg.inference
    assert (inf.ckpt_name, inf.model_avg, inf.avg_num, inf.avg_policy, inf.thread_num) == (7, True, 3, None, 1)
    assert inf.ckpt_path == "/x/ckpts" and list(cfg.task.test) == ["/data/a", "/data/b"]
    assert "inference.ckpt_name" not in missing_keys(cfg)
    assert cfg.hydra.job_logging.handlers.file.filename == "infer.log"
    # defaults: the trainer's checkpoint directory and the run's training log
    cfg = compose(overrides=GROUPS, job_name="infer")
    assert cfg.inference.ckpt_path == "ckpts" and cfg.inference.avg_policy == cfg.run_cfg.dir + "/train.log"
    assert "inference.ckpt_name" in missing_keys(cfg)


def test_cli_help_and_print_config(tmp_path, monkeypatch, capsys):
    from liteasr_amd import infer as I

    from cfgtree import user_tree

    conf, data = user_tree(tmp_path)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit):
        I.main(["--help"])
    out = capsys.readouterr().out
    assert "liteasr_amd.infer" in out and "configuration groups" in out and "--config-dir" in out
    assert I.main(["-cd", str(conf), "--cfg", "job"]) is None
    assert "inference:" in capsys.readouterr().out


def test_log_lines_format_as_the_reference():
    from liteasr_amd import infer as I

    for u in GOLD["lines"]["utt"]:
        line, err = I.utt_line(u["ref"], u["hyp"])
        assert line == u["utt"]
    for r in GOLD["lines"]["rate"]:
        assert I.rate_line(r["err"], r["len"]) == r["text"]


def test_graph_plan():
    from liteasr_amd import infer as I

    xlens = [300, 500, 300, 300, 700, 300, 500, 500]
    order, graphed = I.graph_plan(xlens)
    assert order == [0, 2, 3, 5, 1, 6, 7, 4]  # equal frame counts adjacent, dataset order within
    assert graphed == [True, False, True, True, False, True, False, False]  # 300 x 4; 500 x 3; 700 x 1


def test_documented_command_line_needs_no_training_data(tmp_path, monkeypatch):
    """The usage block of INTEGRATION.md (shipped presets, no task.train / task.valid) through
    ``infer.main``: composition, run dir, test set, model and checkpoint, up to the device.  What
    evaluation does read is still demanded."""
    import logging

    from cfgtree import data_dir
    from liteasr_amd import infer as I
    from liteasr_amd import tasks
    from liteasr_amd.config.compose import ConfigError, compose

    data = data_dir(tmp_path)
    monkeypatch.chdir(tmp_path)
    small = ["model.enc_layers=1", "model.dec_layers=1", "model.enc_dim=32", "model.dec_dim=32",
             "model.enc_ff_dim=64", "model.dec_ff_dim=64"]
    argv = GROUPS + [f"task.vocab={data / 'vocab.txt'}", f"task.test=[{data}]", f"inference.ckpt_path={tmp_path}/ck",
                     "inference.ckpt_name=40", "hydra.run.dir=run"] + small
    with pytest.raises(ConfigError, match=r"missing mandatory value\(s\): inference.ckpt_name$"):
        I.main([a for a in argv if not a.startswith("inference.ckpt_name")])
    with pytest.raises(ConfigError, match="task.vocab"):
        I.main([a for a in argv if not a.startswith("task.vocab")])
    with pytest.raises(ConfigError, match="task.test names no test set"):
        I.main([a for a in argv if not a.startswith("task.test")])
    monkeypatch.chdir(tmp_path)
    # the checkpoint the command line names, from the same composition
    cfg = compose(overrides=argv, job_name="infer")
    assert cfg.task.train == "???" and cfg.task.valid == "???"
    (tmp_path / "ck").mkdir()
    task = tasks.setup_task(cfg.task)
    task.load_dataset("test", task.cfg.test, None, cfg.postprocess)
    torch.manual_seed(0)
    torch.save(task.build_model(cfg.model).state_dict(), tmp_path / "ck" / "model.ep.40.pt")
    root = logging.getLogger()
    saved = root.handlers[:], root.level
    try:
        if torch.cuda.is_available():
            I.main(argv)
        else:
            with pytest.raises(RuntimeError, match="GPU|HIP|CUDA|cuda"):
                I.main(argv)  # model.to("cuda"): everything before it has run
        for h in root.handlers:
            h.flush()
        log = (tmp_path / "run" / "infer.log").read_text()
        assert "loading test data from" in log and "checkpoint: " in log
        if torch.cuda.is_available():
            assert "Error rate: " in log
    finally:
        for h in root.handlers[:]:
            if h not in saved[0]:
                root.removeHandler(h)
                h.close()
        root.setLevel(saved[1])
