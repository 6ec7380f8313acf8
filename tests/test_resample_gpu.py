"""``lasr_resample_i16`` on the GPU against the rounded, saturated float64 restatement of the
transform (tests/resample_ref.py), its exact edges and bit-exact structure, the argument checks,
task=asr end to end with ``speed_perturb`` against the resampler's own output read back from WAV
files, and ``tools/compute_cmvn.py --speed-perturb``.

The bars of the parity test are set by the reference, never by the kernel: tests/resample_ref.py
run in float32 loses FP32_LOSS (LSB of the int16 output) against float64 on these inputs
(``python tests/resample_cases.py`` prints the table).  Every sample must be within 1 LSB of the
quantised float64 value, and exactly equal to it unless the float64 value lies within
BAR_FACTOR x FP32_LOSS of a point where the quantisation changes (a half-integer, or the
saturation point): there a kernel that sums in another order may land on the other side.  That
excused share is capped at 10 % by tests/resample_cases.py on the reference alone."""

import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import resample_cases as C
import resample_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
# float32 restatement against float64, LSB, measured with tests/resample_cases.py
FP32_LOSS = {
    ("noise_full", (9, 10)): 1.185e-02, ("noise_full", (11, 10)): 9.024e-03, ("noise_full", (1, 1)): 0.0,
    ("noise_full", (4, 5)): 9.657e-03, ("noise_full", (5, 4)): 8.272e-03,
    ("sine_1234", (9, 10)): 3.512e-03, ("sine_1234", (11, 10)): 2.630e-03, ("sine_1234", (1, 1)): 0.0,
    ("sine_1234", (4, 5)): 2.841e-03, ("sine_1234", (5, 4)): 3.024e-03,
    ("square", (9, 10)): 5.908e-03, ("square", (11, 10)): 7.398e-03, ("square", (1, 1)): 0.0,
    ("square", (4, 5)): 5.908e-03, ("square", (5, 4)): 8.987e-03,
    ("noise_small", (9, 10)): 1.043e-05, ("noise_small", (11, 10)): 7.715e-06, ("noise_small", (1, 1)): 0.0,
    ("noise_small", (4, 5)): 8.486e-06, ("noise_small", (5, 4)): 9.100e-06,
}
FILL_IN, FILL_OUT = 32767, -21555


def _guarded(host, pad=37, fill=FILL_IN):
    """``host`` (B, S) int16 as a view with row stride S + pad inside a device buffer of ``fill``,
    starting 3 samples in (2-byte aligned only)."""
    B, S = host.shape
    buf = torch.full((3 + B * (S + pad) + 5,), fill, dtype=torch.int16, device=DEV)
    view = buf[3:3 + B * (S + pad)].view(B, S + pad)[:, :S]
    view.copy_(torch.from_numpy(host))
    return buf, view


def _tables(ratios):
    from liteasr_amd import kernels as K

    return tuple(torch.from_numpy(v).to(DEV) for v in K.resample_tables(ratios))


def _run(view, rows, ratios=C.RATIOS, s_out=None, packed=False, pad=29):
    """The kernel into a strided (or packed) view of a buffer of FILL_OUT that starts 3 samples in;
    ``rows``: the plan, [n_in, n_out, ratio index] per row.  Returns (out view, the whole buffer)."""
    from liteasr_amd import kernels as K

    B = view.shape[0]
    s_out = max(r[1] for r in rows) if s_out is None else s_out
    pad = 0 if packed else pad
    guard = torch.full((3 + B * (s_out + pad) + 5,), FILL_OUT, dtype=torch.int16, device=DEV)
    out = guard[3:3 + B * (s_out + pad)].view(B, s_out + pad)[:, :s_out]
    plan = torch.tensor(rows, dtype=torch.int32, device=DEV).reshape(B, 3)
    table, taps = _tables(ratios)
    got = K.resample_i16(view, plan, table, taps, out=out)
    assert got is out
    torch.cuda.synchronize()
    assert (guard[:3] == FILL_OUT).all() and (guard[-5:] == FILL_OUT).all()
    if pad:
        assert (guard[3:3 + B * (s_out + pad)].view(B, s_out + pad)[:, s_out:] == FILL_OUT).all()
    return out, guard


def _plan_rows():
    return [[n, R.num_samples(n, *pq), C.RATIOS.index(pq)] for n, pq in C.rows()]


@pytest.mark.parametrize("name", C.SIGNALS)
def test_parity_with_float64(name):
    """Rows of 0, 1, 9, 10, 399, 400, 4000 and 16000 samples at 9/10, 11/10, 1/1, 4/5 and 5/4,
    neighbouring rows at different ratios, of one signal in one call."""
    host = C.batch(name)
    buf, view = _guarded(host)
    rows = _plan_rows()
    out, _ = _run(view, rows)
    out = out.cpu().numpy()
    assert (buf[:3] == FILL_IN).all() and (buf[-5:] == FILL_IN).all()
    differed, excused, total, lo, hi = {}, {}, {}, False, False
    for r, ((n, pq), (_, m, _)) in enumerate(zip(C.rows(), rows)):
        y64 = C.reference(name, n, pq)
        want = R.quantise(y64)
        got = out[r, :m]
        assert y64.shape == (m,) and (out[r, m:] == 0).all()
        diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
        assert diff.max(initial=0) <= 1
        strict = R.boundary_distance(y64) > C.BAR_FACTOR * FP32_LOSS[name, pq]
        assert (diff[strict] == 0).all()
        if pq == (1, 1):
            assert np.array_equal(got, host[r, :n]) and m == n
        differed[pq] = differed.get(pq, 0) + int((diff != 0).sum())
        excused[pq] = excused.get(pq, 0) + int((~strict).sum())
        total[pq] = total.get(pq, 0) + m
        lo, hi = lo or bool((got == -32768).any()), hi or bool((got == 32767).any())
    for pq in C.RATIOS:
        print(f"resample parity {name} {pq[0]}/{pq[1]}: {differed[pq]} of {total[pq]} samples differ by 1 LSB, "
              f"{excused[pq]} excused")
        assert excused[pq] <= C.EXCUSED_CAP * total[pq]
    if name in C.SATURATING:
        assert lo and hi


def test_edges_are_exact():
    """Padding is zero up to S_out, an empty row is zero, nothing at or past n_in is read (the rows'
    tails, the stride padding and the buffer around them may change), and a plan that asks for
    more than the buffers hold is clamped or gives a zero row."""
    host = C.batch("noise_full")
    buf, view = _guarded(host)
    rows = _plan_rows()
    s_out = max(r[1] for r in rows) + 1500  # more than one tile of padding only
    out, _ = _run(view, rows, s_out=s_out)
    assert out.shape == (len(rows), s_out)
    for r, (n, m, _) in enumerate(rows):
        assert (out[r, m:] == 0).all() and (m < 400 or (out[r, :m] != 0).any())
        if n == 0:
            assert m == 0 and (out[r] == 0).all()
    B, S = host.shape
    rng = np.random.default_rng(1)
    buf2 = torch.from_numpy(rng.integers(-32768, 32768, buf.numel()).astype(np.int16)).to(DEV)
    view2 = buf2[3:3 + B * (S + 37)].view(B, S + 37)[:, :S]
    for r, (n, _, _) in enumerate(rows):
        view2[r, :n] = view[r, :n]
    again, _ = _run(view2, rows, s_out=s_out)
    assert torch.equal(again, out)
    # a hostile plan: counts past the buffers are clamped, negative counts and ratio indices
    # outside the table give zero rows; the guards of _run hold throughout
    base = out[:, :2000].clone()
    long_rows = [r for r, (n, m, _) in enumerate(rows) if n == 16000]
    hostile = [list(r) for r in rows]
    a, b, c, d, e = long_rows[:5]
    hostile[a][1] = 10 ** 9          # n_out > S_out: all S_out samples are the row's
    hostile[b][0] = 10 ** 9          # n_in > S_in: the row's S samples
    hostile[c][0] = -5               # no input: zeros
    hostile[d][1] = -5               # no output
    hostile[e][2] = len(C.RATIOS)    # no such ratio
    hostile[0][2] = -1
    hostile[1][0], hostile[1][1], hostile[1][2] = 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1
    got, _ = _run(view, hostile, s_out=2000)
    assert torch.equal(got[a], base[a]) and torch.equal(got[b], base[b])
    for r in (c, d, e, 0, 1):
        assert (got[r] == 0).all()
    for r in range(len(rows)):
        if r not in (a, b, c, d, e, 0, 1):
            m = min(rows[r][1], 2000)
            assert torch.equal(got[r, :m], base[r, :m]) and (got[r, m:] == 0).all()
    # a ratio table the kernel cannot hold gives zero rows as well
    from liteasr_amd import kernels as K

    table, taps = _tables(C.RATIOS)
    for col, val in ((0, 33), (1, 0), (2, 14), (2, -1), (3, taps.numel()), (3, -4), (0, 21)):
        bad = table.clone()
        bad[0, col] = val
        plan = torch.tensor([[16000, 2000, 0], [16000, 2000, 1]], dtype=torch.int32, device=DEV)
        two = K.resample_i16(view[[a, a]].contiguous(), plan, bad, taps, max_out=2000)
        assert (two[0] == 0).all() and (two[1] != 0).any()


def test_structure_is_bit_exact():
    from liteasr_amd import kernels as K

    x = C.signal("noise_full")
    n = 8000
    table, taps = _tables(C.RATIOS)
    for ri, (p, q) in enumerate(C.RATIOS):
        width = int(table[ri, 2])
        host = np.zeros((4, n), dtype=np.int16)
        host[0], host[1, :n - p], host[2, :3001], host[3] = x[:n], x[p:n], x[:3001], C.signal("square")[:n]
        lens = [n, n - p, 3001, n]
        rows = [[v, R.num_samples(v, p, q), ri] for v in lens]
        rows[3][2] = (ri + 1) % len(C.RATIOS)  # a neighbour at another ratio
        rows[3][1] = R.num_samples(n, *C.RATIOS[rows[3][2]])
        buf, view = _guarded(host)
        out, _ = _run(view, rows)
        m0, m1, m2 = rows[0][1], rows[1][1], rows[2][1]
        # a shift by p input samples is a shift by q output samples, away from the row's start
        first = q * (width + 1)
        assert m1 == m0 - q and torch.equal(out[1, first:m1], out[0, first + q:m0])
        # a prefix gives a prefix wherever no tap reaches past it: m p / q + width <= N'
        safe = min(((3001 - width) * q) // p, m2 - 1)
        assert safe * p + width * q <= 3001 * q and safe > 3000 * q // p - 2 * q
        assert torch.equal(out[2, :safe + 1], out[0, :safe + 1])
        # alone, at another batch index, packed instead of strided, with another S_out
        row = torch.from_numpy(host[0:1]).to(DEV)
        alone = K.resample_i16(row, torch.tensor([rows[0]], dtype=torch.int32, device=DEV), table, taps)
        assert alone.shape == (1, m0) and torch.equal(alone[0], out[0, :m0])
        perm = [3, 2, 0, 1]
        packed = torch.from_numpy(host[perm]).to(DEV)
        wide, _ = _run(packed, [rows[i] for i in perm], s_out=max(r[1] for r in rows) + 1031, packed=True)
        assert wide.is_contiguous() and not out.is_contiguous()
        for j, i in enumerate(perm):
            assert torch.equal(wide[j, :rows[i][1]], out[i, :rows[i][1]]) and (wide[j, rows[i][1]:] == 0).all()
        # and twice the same call gives the same bits
        assert torch.equal(_run(view, rows)[0], out)


def test_argument_checks():
    """Each raises before anything is launched: the output buffer keeps its sentinel."""
    from liteasr_amd import _native as N
    from liteasr_amd import kernels as K

    pcm = torch.zeros(2, 1000, dtype=torch.int16, device=DEV)
    plan = torch.tensor([[1000, 1112, 0], [1000, 910, 1]], dtype=torch.int32, device=DEV)
    table, taps = _tables(C.RATIOS)
    out = torch.full((2, 1200), FILL_OUT, dtype=torch.int16, device=DEV)
    for bad in (dict(pcm=pcm.float()), dict(pcm=pcm.cpu()), dict(pcm=pcm.t().contiguous().t()), dict(pcm=pcm[0]),
                dict(plan=plan.long()), dict(plan=plan.cpu()), dict(plan=plan[:1]), dict(plan=plan[:, :2]),
                dict(plan=plan.t().contiguous().t()), dict(ratios=table.long()), dict(ratios=table[:, :3]),
                dict(ratios=table[:0]), dict(ratios=table.cpu()), dict(taps=taps.double()), dict(taps=taps.cpu()),
                dict(taps=taps.view(1, -1)), dict(out=out.float()), dict(out=out[:1]), dict(out=out.cpu()),
                dict(out=out.t().contiguous().t()), dict(out=out[0])):
        args = dict(dict(pcm=pcm, plan=plan, ratios=table, taps=taps, out=out), **bad)
        with pytest.raises(TypeError):
            K.resample_i16(args["pcm"], args["plan"], args["ratios"], args["taps"], out=args["out"])
    with pytest.raises(ValueError):
        K.resample_i16(pcm, plan, table, taps, out=out, max_out=1201)
    with pytest.raises(ValueError):
        K.resample_i16(pcm, plan, table, taps, max_out=-1)
    # the C entry checks for itself
    st = K.stream()
    args = dict(pcm=pcm.data_ptr(), istride=1000, B=2, S=1000, plan=plan.data_ptr(), ratios=table.data_ptr(),
                R=table.shape[0], taps=taps.data_ptr(), ntaps=taps.numel(), out=out.data_ptr(), ostride=1200, So=1200)

    def call(**kw):
        a = dict(args, **kw)
        N.call("lasr_resample_i16", a["pcm"], a["istride"], a["B"], a["S"], a["plan"], a["ratios"], a["R"], a["taps"],
               a["ntaps"], a["out"], a["ostride"], a["So"], st)

    for bad in (dict(B=-1), dict(S=-1), dict(So=-1), dict(R=-1), dict(R=0), dict(ntaps=-1), dict(pcm=None),
                dict(out=None), dict(plan=None), dict(ratios=None), dict(taps=None), dict(pcm=pcm.data_ptr() + 1),
                dict(out=out.data_ptr() + 1), dict(plan=plan.data_ptr() + 2), dict(ratios=table.data_ptr() + 2),
                dict(taps=taps.data_ptr() + 2), dict(istride=999), dict(ostride=1199), dict(S=2 ** 29 + 1),
                dict(So=2 ** 29 + 1), dict(B=65536), dict(out=pcm.data_ptr() + 1000), dict(pcm=out.data_ptr() + 2400)):
        with pytest.raises(N.NativeError):
            call(**bad)
    torch.cuda.synchronize()
    assert (out == FILL_OUT).all()
    call()
    call(B=0, out=None)
    call(So=0, out=None)
    torch.cuda.synchronize()
    assert (out == 0).all()


def _write_resampled_dir(wav, dst):
    """The device resampler's own int16 output for every copy of the speed-perturbed train set over
    ``wav``, as WAV files listed in the dataset's record order.  Returns (records, delivered dtype)."""
    import shutil

    from liteasr_amd.dataclass.vocab import Vocab
    from liteasr_amd.dataset import AudioFileDataset
    from liteasr_amd.utils.frontend import Fbank
    from liteasr_amd.utils.synthetic import write_wav

    ds = AudioFileDataset("train", wav, None, None, None, Vocab(os.path.join(wav, "vocab.txt")),
                          speed_perturb=[0.9, 1.0, 1.1])
    xs, _, _, _, plan = ds.collator([ds.data])
    pcm = Fbank().speed(xs.to(DEV), plan).cpu().numpy()
    texts = dict(ln.rstrip("\n").split(" ", 1) for ln in open(os.path.join(wav, "text")))
    keys = {ln.split()[1]: ln.split()[0] for ln in open(os.path.join(wav, "wav.scp"))}
    os.makedirs(os.path.join(dst, "wav"))
    shutil.copy(os.path.join(wav, "vocab.txt"), dst)
    with open(os.path.join(dst, "wav.scp"), "w") as scp, open(os.path.join(dst, "text"), "w") as txt:
        for i, a in enumerate(ds.data):
            assert (pcm[i, a.samples:] == 0).all()
            path = os.path.join(dst, "wav", f"copy{i:04d}.wav")
            write_wav(path, pcm[i, :a.samples])
            scp.write(f"copy{i:04d} {path}\n")
            txt.write(f"copy{i:04d} {texts[keys[a.fd]]}\n")
    return ds.data, xs.dtype


def test_task_asr_speed_perturb_end_to_end(tmp_path):
    """Two Trainer steps (tiny conformer, SpecAugment on, equal seeds) and a validation pass, from a
    wav.scp directory with speed_perturb=[0.9, 1.0, 1.1] and from a directory, with the option off,
    of the resampler's own output for every copy: equal losses bit for bit.  Validation reads the
    original directory in both runs: it is never perturbed."""
    from liteasr_amd.utils.synthetic import synthetic_wav_dir

    lengths = [8000, 19200, 12345, 16001, 9000]
    wav = synthetic_wav_dir(str(tmp_path / "wav"), lengths, seed=1)
    records, dtype = _write_resampled_dir(wav, str(tmp_path / "copies"))
    assert len(records) == 3 * len(lengths) and dtype == torch.int16
    outs = {}
    for name, d, speed in (("on", wav, "[0.9,1.0,1.1]"), ("off", str(tmp_path / "copies"), "null")):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_resample_trainer_step.py"), d, wav,
                            str(tmp_path / ("run_" + name)), speed], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        outs[name] = json.loads(r.stdout.strip().splitlines()[-1])
    a, b = outs["on"], outs["off"]
    assert a["train_records"] == b["train_records"] == len(records)
    # the collator still delivers int16, now with the SpecAugment plan and the resampling plan
    assert [s[0] for s in a["delivered"]] == ["torch.int16"] * 2 and [s[2:] for s in a["delivered"]] == [[6, True]] * 2
    assert [s[0] for s in b["delivered"]] == ["torch.int16"] * 2 and [s[2:] for s in b["delivered"]] == [[5, False]] * 2
    by_frames = sorted(records, key=lambda r: -r.xlen)
    groups = [by_frames[k:k + 3] for k in range(0, len(by_frames), 3)]  # the minibatches; their order is shuffled
    for step in range(2):
        hit = [g for g in groups if [r.xlen for r in g] == a["seen"][step][2]]
        assert len(hit) == 1 and len({r.ratio for g in hit for r in g}) > 1  # the speeds interleave
        assert a["delivered"][step][1] == [3, max(r.shape for r in hit[0])]
        assert b["delivered"][step][1] == [3, max(r.samples for r in hit[0])]
    assert a["seen"] == b["seen"] and all(s[0] == "torch.float32" and s[1][2] == 80 for s in a["seen"])
    for o in (a, b):
        assert o["iters"] == 2 and o["skipped"] == 0 and len(o["losses"]) == 2
        assert all(math.isfinite(v) for v in o["losses"])
        assert all(s[2:] == [4, False] and s[0] == "torch.int16" for s in o["valid_delivered"])
    assert a["losses"] == b["losses"]
    assert a["valid"] == b["valid"] and math.isfinite(a["valid"]) and a["valid_seen"] == b["valid_seen"]
    assert sum(len(s[2]) for s in a["valid_seen"]) == len(lengths)


def test_compute_cmvn_speed_perturb(tmp_path):
    """tools/compute_cmvn.py --speed-perturb over a wav.scp directory: the frame count is exact,
    and mean and istd agree with the float64 chain (tests/resample_ref.py, quantised, then
    tests/fbank_ref.py) to the bar of test_fbank_gpu.test_compute_cmvn_tool, for its reason: the log
    values of broad-band signals are within 1e-3 of float64.  (A resampled sample on the other side
    of a rounding boundary moves one of 400 samples of a frame by 1 LSB: far below that.)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import compute_cmvn as T
    import fbank_ref as FR

    from liteasr_amd.utils import wavio
    from liteasr_amd.utils.frontend import Fbank, read_cmvn_stats
    from liteasr_amd.utils.synthetic import synthetic_wav_dir

    lengths = [8000, 399, 12345, 16001, 400]
    wav = synthetic_wav_dir(str(tmp_path / "wav"), lengths, seed=2)
    out = str(tmp_path / "cmvn.stats")
    T.main([wav, out, "--batch", "4", "--speed-perturb", "0.9,1.0,1.1"])
    fe = Fbank(80, cmvn=out)
    ref = []
    for speed in (0.9, 1.0, 1.1):
        p, q = R.ratio(speed)
        for ln in open(os.path.join(wav, "wav.scp")):
            ref.append(FR.fbank(R.quantise(R.resample(wavio.read(ln.split()[1])[0], p, q)), 80))
    ref = np.concatenate(ref)
    assert ref.shape[0] == sum(FR.num_frames(R.num_samples(n, *R.ratio(s))) for s in (0.9, 1.0, 1.1) for n in lengths)
    stats = read_cmvn_stats(out)
    assert stats.shape == (2, 81) and stats[0, 80] == ref.shape[0] and stats[1, 80] == 0
    assert np.abs(fe.cmvn[0] - ref.mean(0)).max() <= 1e-3
    assert (np.abs(fe.cmvn[1] * ref.std(0) - 1) <= 1e-3 / ref.std(0) + 1e-6).all()
    # without the flag the tool is what it was: the plain statistics
    plain = str(tmp_path / "plain.stats")
    T.main([wav, plain, "--batch", "4"])
    assert read_cmvn_stats(plain)[0, 80] == sum(FR.num_frames(n) for n in lengths)
