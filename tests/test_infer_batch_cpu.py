"""Host side of batched evaluation (liteasr_amd.infer.batch_plan, the batch arena's size helpers,
``inference.batch_size``).  CPU only."""

import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GROUPS = ["task=asr_kaldi", "model=conformer_small", "criterion=hybrid_ctc_w03", "optimizer=noam_d256"]


def test_batch_plan():
    from liteasr_amd import infer as I

    xlens = [300, 500, 300, 300, 700, 300, 500, 500, 450, 300, 620]
    plan = I.batch_plan(xlens, 4)
    flat = [i for g in plan for i in g]
    assert sorted(flat) == list(range(len(xlens)))  # every index once
    # consecutive groups of the stable frame-count order
    assert flat == sorted(range(len(xlens)), key=lambda i: xlens[i])
    assert flat == [0, 2, 3, 5, 9, 8, 1, 6, 7, 10, 4]
    assert [len(g) for g in plan] == [4, 4, 3]  # the last group is short
    assert plan == [[0, 2, 3, 5], [9, 8, 1, 6], [7, 10, 4]]
    # batch_size 1 is graph_plan's order, one utterance per group
    assert [g[0] for g in I.batch_plan(xlens, 1)] == I.graph_plan(xlens)[0]
    assert all(len(g) == 1 for g in I.batch_plan(xlens, 1))
    assert I.batch_plan([], 4) == [] and I.batch_plan([9, 3], 32) == [[1, 0]]
    with pytest.raises(ValueError, match="batch_size"):
        I.batch_plan(xlens, 0)


def test_pad_batch():
    import torch

    from liteasr_amd import infer as I

    xs = [torch.full((3, 2), 1.0), torch.full((5, 2), 2.0), torch.full((1, 2), 3.0)]
    out, lens = I.pad_batch(xs)
    assert lens == [3, 5, 1] and tuple(out.shape) == (3, 5, 2) and out.dtype == torch.float32
    for b, x in enumerate(xs):
        assert torch.equal(out[b, :lens[b]], x) and (out[b, lens[b]:] == 0).all()
    pcm, lens = I.pad_batch([torch.arange(4, dtype=torch.int16), torch.arange(7, dtype=torch.int16)])
    assert pcm.dtype == torch.int16 and tuple(pcm.shape) == (2, 7) and lens == [4, 7] and (pcm[0, 4:] == 0).all()


@pytest.mark.parametrize("Tcap,Lcap", [(64, 64), (256, 64), (256, 128), (1024, 256)])
def test_batch_arena_is_single_arenas_end_to_end(Tcap, Lcap):
    from liteasr_amd import kernels as K

    stride = K.rescore_workspace(Tcap, Lcap)
    assert stride > 0 and stride % 256 == 0  # every row's arena keeps the 256-B alignment
    for B in (1, 2, 5, 32):
        assert K.rescore_workspace_batch(B, Tcap, Lcap) == B * stride
    assert K.rescore_workspace_batch(0, Tcap, Lcap) == 0


def test_batch_size_composes_and_defaults_to_one():
    from liteasr_amd.config.compose import compose

    cfg = compose(overrides=GROUPS + ["inference.ckpt_name=7", "inference.batch_size=4"], job_name="infer")
    assert cfg.inference.batch_size == 4
    cfg = compose(overrides=GROUPS + ["inference.ckpt_name=7"], job_name="infer")
    assert cfg.inference.batch_size == 1


def test_models_with_a_batched_entry():
    from liteasr_amd.models.paraformer import Paraformer
    from liteasr_amd.models.transducer import Transducer
    from liteasr_amd.models.u2 import U2

    assert hasattr(U2, "inference_batch") and hasattr(Paraformer, "inference_batch")
    assert not hasattr(Transducer, "inference_batch")  # infer falls back to the per-utterance loop
