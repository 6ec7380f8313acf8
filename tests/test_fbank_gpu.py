"""``lasr_fbank`` on the GPU against the float64 restatement of Kaldi fbank (tests/fbank_ref.py),
its exact edges and bit-exact structure, CMVN, the argument checks, and task=asr end to end from a
wav.scp directory against the same features read from feats.scp.

The bars of the parity test are set by the reference, never by the kernel: tests/fbank_ref.py run
in float32 (numpy float32, scipy.fft on float32) loses FP32_LOSS against float64 on these inputs
(``python tests/fbank_cases.py`` prints the table); the kernel, whose FFT and sums run in another
order, gets 4 times that, per signal and metric:
  (a) energy error relative to the frame's largest mel energy, every bin of every signal;
  (b) absolute error of the log values, every bin of the broad-band signals and of the two floor
      signals (which must also sit on log(FLT_EPSILON) exactly).
"""

import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fbank_cases as C
import fbank_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
F = 80
# float32 restatement against float64, (metric a, metric b), measured with tests/fbank_cases.py
FP32_LOSS = {
    "noise_full": (1.063e-06, 4.631e-05),
    "noise_small": (5.564e-07, 1.229e-04),
    "square": (1.017e-06, 2.409e-04),
    "tone_noise": (1.217e-06, 1.901e-04),
    "sine_bin64": (2.162e-07, 7.177e-03),  # (b) is not asserted for the tones: bins 1e8 below the peak
    "sine_1234": (1.029e-06, 3.762e-03),
    "zeros": (4.330e-07, 4.330e-07),  # the float32 rounding of log(FLT_EPSILON) itself
    "constant": (4.330e-07, 4.330e-07),
}
BAR_FACTOR = 4.0
NFRAMES = [R.num_frames(n) for n in C.LENGTHS]
TMAX = max(NFRAMES)


def _guarded(host, pad=37, fill=32767):
    """``host`` (B, S) int16 as a view with row stride S + pad inside a device buffer of ``fill``,
    starting 3 samples in (2-byte aligned only)."""
    B, S = host.shape
    buf = torch.full((3 + B * (S + pad) + 5,), fill, dtype=torch.int16, device=DEV)
    view = buf[3:3 + B * (S + pad)].view(B, S + pad)[:, :S]
    view.copy_(torch.from_numpy(host))
    return buf, view


def _run(view, nframes, tmax=None, cmvn=None, sentinel=-7.5):
    """The kernel into a view of a buffer of ``sentinel``; returns (out view, the whole buffer)."""
    from liteasr_amd import kernels as K

    B = view.shape[0]
    tmax = max(nframes) if tmax is None else tmax
    nf = torch.tensor(nframes, dtype=torch.int32, device=DEV)
    guard = torch.full((16 + B * tmax * F + 16,), sentinel, dtype=torch.float32, device=DEV)
    out = guard[16:16 + B * tmax * F].view(B, tmax, F)
    got = K.fbank(view, nf, F, cmvn=cmvn, out=out, max_frames=max(nframes))
    assert got is out
    torch.cuda.synchronize()
    assert (guard[:16] == sentinel).all() and (guard[-16:] == sentinel).all()
    return out, guard


@pytest.mark.parametrize("name", C.SIGNALS)
def test_parity_with_float64(name):
    """Rows of 399 (no frame), 400, 559, 560, 4000 and 16000 samples of one signal in one call."""
    host = C.batch(name)
    buf, view = _guarded(host)
    out, _ = _run(view, NFRAMES)
    out = out.cpu().numpy()
    refs = C.reference(name, F)
    err_a = max(C.energy_error(out[i, :t], refs[i]) for i, t in enumerate(NFRAMES))
    err_b = max(C.log_error(out[i, :t], refs[i]) for i, t in enumerate(NFRAMES))
    loss_a, loss_b = FP32_LOSS[name]
    print(f"fbank parity {name}: (a) {err_a:.3e} bar {BAR_FACTOR * loss_a:.3e}   (b) {err_b:.3e} "
          f"bar {BAR_FACTOR * loss_b:.3e}")
    for i, t in enumerate(NFRAMES):
        assert np.isfinite(out[i, :t]).all() and (out[i, t:] == 0).all()
    assert err_a <= BAR_FACTOR * loss_a
    if name in C.BROADBAND or name in C.FLOOR:
        assert err_b <= BAR_FACTOR * loss_b
    if name in C.FLOOR:
        for i, t in enumerate(NFRAMES):
            assert (out[i, :t] == R.LOG_EPS32).all()
    assert (buf[:3] == 32767).all() and (buf[-5:] == 32767).all()


def _cmvn(seed=9):
    rng = np.random.default_rng(seed)
    mean = rng.uniform(5.0, 14.0, F).astype(np.float32)
    istd = (1.0 / rng.uniform(1.0, 4.0, F)).astype(np.float32)
    return mean, istd


def test_edges_are_exact():
    """Padding rows are zero with and without CMVN, a row without frames is all zero, and nothing
    past a row's last used sample is read: the stride padding and the rows' tails may change."""
    host = C.batch("noise_full")
    buf, view = _guarded(host)
    mean, istd = _cmvn()
    cm = (torch.from_numpy(mean).to(DEV), torch.from_numpy(istd).to(DEV))
    plain, _ = _run(view, NFRAMES)
    normed, _ = _run(view, NFRAMES, cmvn=cm)
    for out in (plain, normed):
        assert out.shape == (len(NFRAMES), TMAX, F)
        assert (out[0] == 0).all()  # 399 samples
        for i, t in enumerate(NFRAMES):
            assert (out[i, t:] == 0).all() and (t == 0 or (out[i, :t] != 0).any())
    # every sample that no frame reads, inside the rows and in the buffer around them, changes
    B, S = host.shape
    rng = np.random.default_rng(1)
    buf2 = torch.from_numpy(rng.integers(-32768, 32768, buf.numel()).astype(np.int16)).to(DEV)
    view2 = buf2[3:3 + B * (S + 37)].view(B, S + 37)[:, :S]
    for i, t in enumerate(NFRAMES):
        used = 160 * (t - 1) + 400 if t else 0
        view2[i, :used] = view[i, :used]
    again, _ = _run(view2, NFRAMES)
    assert torch.equal(again, plain)
    # frame counts above max_frames are clamped, negative ones are no frames
    from liteasr_amd import kernels as K

    nf = torch.tensor([5, -3, 1, 99, 23, 98], dtype=torch.int32, device=DEV)
    out = K.fbank(view, nf, F, max_frames=2)
    assert out.shape == (6, 2, F) and (out[1] == 0).all() and (out[2, 1] == 0).all()
    assert torch.equal(out[3], plain[3, :2]) and torch.equal(out[5], plain[5, :2])
    assert K.fbank(view[:, :399], torch.zeros(6, dtype=torch.int32, device=DEV), F).shape == (6, 0, F)


def test_structure_is_bit_exact():
    from liteasr_amd import kernels as K

    x = C.signal("tone_noise")
    n = 8000
    host = np.zeros((4, n), dtype=np.int16)
    host[0], host[1, :n - 160], host[2, :4000], host[3] = x[:n], x[160:n], x[:4000], C.signal("square")[:n]
    nfr = [R.num_frames(n), R.num_frames(n - 160), R.num_frames(4000), R.num_frames(n)]
    buf, view = _guarded(host)
    out, _ = _run(view, nfr)
    # a shift by one frame shift moves the features by one frame
    assert nfr[1] == nfr[0] - 1 and torch.equal(out[1, :nfr[1]], out[0, 1:nfr[0]])
    # a prefix gives a prefix
    assert torch.equal(out[2, :nfr[2]], out[0, :nfr[2]])
    # alone, at another batch index, with another Tmax, packed instead of strided
    row = torch.from_numpy(host[0:1]).to(DEV)
    alone = K.fbank(row, torch.tensor([nfr[0]], dtype=torch.int32, device=DEV), F)
    assert alone.shape == (1, nfr[0], F) and torch.equal(alone[0], out[0])
    perm = [3, 2, 0, 1]
    packed = torch.from_numpy(host[perm]).to(DEV)
    assert packed.is_contiguous() and not view.is_contiguous()
    wide, _ = _run(packed, [nfr[i] for i in perm], tmax=nfr[0] + 7)
    for j, i in enumerate(perm):
        assert torch.equal(wide[j, :nfr[i]], out[i, :nfr[i]]) and (wide[j, nfr[i]:] == 0).all()
    # and twice the same call gives the same bits
    assert torch.equal(_run(view, nfr)[0], out)


def test_cmvn(tmp_path):
    """Statistics file -> (mean, istd) -> the kernel: (plain - mean) istd to 2 ulps, padding 0."""
    from liteasr_amd.utils.frontend import Fbank, write_cmvn_stats

    host = C.batch("tone_noise")
    _, view = _guarded(host)
    plain, _ = _run(view, NFRAMES)
    p64 = plain.cpu().numpy().astype(np.float64)
    live = np.arange(TMAX)[None, :] < np.array(NFRAMES)[:, None]
    count = float(live.sum())
    stats = np.zeros((2, F + 1))
    stats[0, :F], stats[0, F], stats[1, :F] = p64[live].sum(0), count, (p64[live] ** 2).sum(0)
    path = str(tmp_path / "cmvn.stats")
    write_cmvn_stats(path, stats)
    fe = Fbank(F, cmvn=path)
    xlens = torch.tensor(NFRAMES, dtype=torch.long, device=DEV)
    out = fe(view, xlens, max_frames=TMAX).cpu().numpy()
    mean, istd = (v.astype(np.float64) for v in fe.cmvn)
    want = (p64 - mean) * istd
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    assert (np.abs(out - want)[live] <= 2 * ulp[live]).all()
    assert (out[~live] == 0).all() and live.sum() == sum(NFRAMES)
    # the statistics are the features' own: normalised features have zero mean and unit variance
    assert np.abs(out[live].mean(0)).max() < 1e-4 and np.abs(out[live].std(0) - 1).max() < 1e-3
    assert torch.equal(fe(view, xlens.to(torch.int32)).cpu(), torch.from_numpy(out))  # max_frames read back


def test_compute_cmvn_tool(tmp_path):
    """tools/compute_cmvn.py over a wav.scp directory: the frame count is exact, and mean and istd
    agree with the float64 reference's to what the features themselves do (metric (b): the log
    values of broad-band signals are within 1e-3 of float64, the widest bar of the parity test; a
    mean cannot move further, and a standard deviation moves by at most the rms difference)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import compute_cmvn as T

    from liteasr_amd.utils import wavio
    from liteasr_amd.utils.frontend import Fbank
    from liteasr_amd.utils.synthetic import synthetic_wav_dir

    lengths = [8000, 399, 12345, 16001, 560]
    wav = synthetic_wav_dir(str(tmp_path / "wav"), lengths, seed=2)
    out = str(tmp_path / "cmvn.stats")
    T.main([wav, out, "--batch", "2"])
    fe = Fbank(F, cmvn=out)
    ref = np.concatenate([R.fbank(wavio.read(ln.split()[1])[0], F) for ln in open(os.path.join(wav, "wav.scp"))])
    assert ref.shape[0] == sum(R.num_frames(n) for n in lengths)
    from liteasr_amd.utils.frontend import read_cmvn_stats

    stats = read_cmvn_stats(out)
    assert stats.shape == (2, F + 1) and stats[0, F] == ref.shape[0] and stats[1, F] == 0
    assert np.abs(fe.cmvn[0] - ref.mean(0)).max() <= 1e-3
    assert (np.abs(fe.cmvn[1] * ref.std(0) - 1) <= 1e-3 / ref.std(0) + 1e-6).all()


def test_argument_checks():
    """Each raises before anything is launched: the output buffer keeps its sentinel."""
    from liteasr_amd import _native as N
    from liteasr_amd import kernels as K

    pcm = torch.zeros(2, 1000, dtype=torch.int16, device=DEV)
    nf = torch.tensor([4, 4], dtype=torch.int32, device=DEV)
    out = torch.full((2, 4, F), -7.5, device=DEV)
    with pytest.raises(TypeError):
        K.fbank(pcm.float(), nf, F, out=out)
    with pytest.raises(TypeError):
        K.fbank(pcm.cpu(), nf, F, out=out)
    with pytest.raises(TypeError):
        K.fbank(pcm, nf.long(), F, out=out)
    with pytest.raises(TypeError):
        K.fbank(pcm, nf.cpu(), F, out=out)
    with pytest.raises(TypeError):
        K.fbank(pcm.t().contiguous().t(), nf, F, out=out)  # rows not contiguous
    with pytest.raises(ValueError):
        K.fbank(pcm, nf, 0)
    with pytest.raises(ValueError):
        K.fbank(pcm, nf, 129)
    with pytest.raises(ValueError):
        K.fbank(pcm, torch.tensor([4, 5], dtype=torch.int32, device=DEV), F)  # 5 frames need 1040 samples
    with pytest.raises(ValueError):
        K.fbank(pcm, nf, F, out=out, max_frames=5)
    with pytest.raises(TypeError):
        K.fbank(pcm, nf, F, out=torch.empty(2, 4, F + 1, device=DEV))
    with pytest.raises(TypeError):
        K.fbank(pcm, nf, F, cmvn=(torch.zeros(F, device=DEV), torch.ones(F + 1, device=DEV)), out=out)
    # the C entry checks for itself
    tab, seg = K._fbank_device_tables(F, pcm.device)
    st = K.stream()
    args = dict(pcm=pcm.data_ptr(), stride=1000, B=2, S=1000, nf=nf.data_ptr(), mx=4, tab=tab.data_ptr(),
                seg=seg.data_ptr(), F=F, mean=None, istd=None, out=out.data_ptr(), T=4)

    def call(**kw):
        a = dict(args, **kw)
        N.call("lasr_fbank", a["pcm"], a["stride"], a["B"], a["S"], a["nf"], a["mx"], a["tab"], a["seg"], a["F"],
               a["mean"], a["istd"], a["out"], a["T"], st)

    for bad in (dict(F=0), dict(F=129), dict(S=1039, mx=5), dict(mx=5), dict(pcm=None), dict(out=None),
                dict(nf=None), dict(tab=None), dict(seg=None), dict(pcm=pcm.data_ptr() + 1),
                dict(out=out.data_ptr() + 2), dict(B=-1), dict(T=-1), dict(S=-1), dict(mx=-1), dict(stride=999),
                dict(mean=out.data_ptr())):
        with pytest.raises(N.NativeError):
            call(**bad)
    torch.cuda.synchronize()
    assert (out == -7.5).all()
    call()
    torch.cuda.synchronize()
    assert (out == R.LOG_EPS32).all()


def test_task_asr_from_wav_equals_feats(tmp_path):
    """Two Trainer steps (tiny conformer, SpecAugment on, equal seeds), a validation pass and one
    decoded utterance, from a wav.scp directory and from a feats.scp directory holding the front
    end's own output for the same files: equal losses bit for bit, equal token ids."""
    import shutil

    from liteasr_amd.dataclass.vocab import Vocab
    from liteasr_amd.dataset import AudioFileDataset
    from liteasr_amd.utils.frontend import Fbank
    from liteasr_amd.utils.kaldiio import save_ark
    from liteasr_amd.utils.synthetic import synthetic_wav_dir

    wav = synthetic_wav_dir(str(tmp_path / "wav"), [8000, 19200, 12345, 16001], seed=1)  # 0.5 .. 1.2 s
    ds = AudioFileDataset("valid", wav, None, None, None, Vocab(os.path.join(wav, "vocab.txt")))
    xs, xlens, _, _ = ds.collator([ds.data])
    feats = Fbank(F)(xs.to(DEV), xlens.to(DEV), max_frames=int(xlens.max())).cpu().numpy()
    dumped = str(tmp_path / "feats")
    os.makedirs(dumped)
    keys = [ln.split()[0] for ln in open(os.path.join(wav, "wav.scp"))]
    save_ark(os.path.join(dumped, "feats.ark"), {k: feats[i, :int(xlens[i])].copy() for i, k in enumerate(keys)},
             scp=os.path.join(dumped, "feats.scp"))
    with open(os.path.join(dumped, "utt2num_frames"), "w") as f:
        f.writelines(f"{k} {int(xlens[i])}\n" for i, k in enumerate(keys))
    for fn in ("text", "vocab.txt"):
        shutil.copy(os.path.join(wav, fn), dumped)
    outs = {}
    for name, d in (("wav", wav), ("feats", dumped)):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_fbank_trainer_step.py"), d,
                            str(tmp_path / ("run_" + name))], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        outs[name] = json.loads(r.stdout.strip().splitlines()[-1])
    a, b = outs["wav"], outs["feats"]
    assert [s[0] for s in a["delivered"]] == ["torch.int16"] * 2 and a["item"] == "torch.int16"
    assert [s[0] for s in b["delivered"]] == ["torch.float32"] * 2 and b["item"] == "torch.float32"
    assert all(s[2] == 5 for s in a["delivered"] + b["delivered"])  # the SpecAugment plan rides along
    assert a["seen"] == b["seen"] and all(s[0] == "torch.float32" and s[1][2] == F for s in a["seen"])
    assert a["feat_dim"] == b["feat_dim"] == F and a["model_saw"] == b["model_saw"] and a["model_saw"][1][2] == F
    for o in (a, b):
        assert o["iters"] == 2 and o["skipped"] == 0 and len(o["losses"]) == 2
        assert all(math.isfinite(v) for v in o["losses"])
    assert a["losses"] == b["losses"]
    assert a["valid"] == b["valid"] and math.isfinite(a["valid"]) and a["valid_batches"] == b["valid_batches"] == 2
    assert a["ids"] == b["ids"] and a["hyp"] == b["hyp"]
