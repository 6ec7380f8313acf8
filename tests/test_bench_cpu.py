"""bench.py --dump-outputs on the CPU: file names, dtypes, the size bound and that the
parameter sample is the same selection on every call."""

import types

import numpy as np
import torch


def _model(n):
    g = torch.Generator().manual_seed(3)
    return types.SimpleNamespace(store=types.SimpleNamespace(flat=torch.randn(n, generator=g)))


def test_dump_outputs_small_store_is_written_whole(tmp_path):
    import bench

    assert bench.DUMP_MAX_PARAMS * 4 + 12 <= 64 << 20  # the whole dump stays under 64 MB
    m = _model(1000)
    bench.dump_outputs(str(tmp_path / "d"), torch.tensor(2.5), m, {"grad_norm": 0.75})
    assert sorted(p.name for p in (tmp_path / "d").iterdir()) == ["grad_norm.npy", "loss.npy", "params.npy"]
    loss, gn, par = (np.load(tmp_path / "d" / f"{n}.npy") for n in ("loss", "grad_norm", "params"))
    assert loss.dtype == np.float32 and loss.tolist() == [2.5]
    assert gn.dtype == np.float64 and gn.tolist() == [0.75]
    assert par.dtype == np.float32 and np.array_equal(par, m.store.flat.numpy())


def test_dump_outputs_large_store_is_a_fixed_sample(tmp_path, monkeypatch):
    import bench

    monkeypatch.setattr(bench, "DUMP_MAX_PARAMS", 256)
    m = _model(5000)
    bench.dump_outputs(str(tmp_path / "a"), torch.tensor(1.0), m, {"grad_norm": 1.0})
    bench.dump_outputs(str(tmp_path / "b"), torch.tensor(1.0), m, {"grad_norm": 1.0})
    a, b = np.load(tmp_path / "a" / "params.npy"), np.load(tmp_path / "b" / "params.npy")
    assert a.shape == (256,) and np.array_equal(a, b)
    # a selection of the store's own values, in index order
    flat = m.store.flat.numpy()
    pos = np.searchsorted(np.sort(flat), a)
    assert np.array_equal(np.sort(flat)[pos], a)
    idx = np.argsort(flat)[pos]
    assert np.all(np.diff(idx) > 0)
