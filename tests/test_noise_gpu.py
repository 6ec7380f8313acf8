"""``lasr_mix_i16`` on the GPU against the rounded, saturated float64 restatement of the transform
(tests/noise_ref.py), its gains bit for bit, its bit-exact structure, its handling of a malformed
plan, the argument checks, ``Trainer._features`` against the kernels called directly, and task=asr
end to end with ``frontend.noise``.  The reference project has no counterpart.

The bars of the parity test are set by the reference, never by the kernel: tests/noise_ref.py run
in float32 (a rounded product and a rounded sum per source) loses FP32_LOSS (LSB of the int16
output) against float64 on these inputs (``python tests/noise_cases.py`` prints the table).  Every
sample must be within 1 LSB of the quantised float64 value, and exactly equal to it unless the
float64 value lies within BAR_FACTOR x FP32_LOSS of a point where the quantisation changes (a
half-integer, or the saturation point).  That excused share is capped at 10 % by
tests/test_noise_cpu.py on the reference alone."""

import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import noise_cases as C
import noise_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
# float32 restatement against float64, LSB, measured with tests/noise_cases.py
FP32_LOSS = {
    ("noise_full", 0): 0.0, ("noise_full", 1): 1.464e-03, ("noise_full", 3): 8.256e-03, ("noise_full", 8): 1.052e-02,
    ("sine_1234", 0): 0.0, ("sine_1234", 1): 1.460e-03, ("sine_1234", 3): 3.521e-03, ("sine_1234", 8): 5.617e-03,
    ("square", 0): 0.0, ("square", 1): 1.950e-03, ("square", 3): 5.289e-03, ("square", 8): 7.286e-03,
    ("noise_small", 0): 0.0, ("noise_small", 1): 3.544e-07, ("noise_small", 3): 1.178e-06,
    ("noise_small", 8): 1.465e-06,
}
FILL_IN, FILL_OUT, FILL_BANK = 32767, -21555, -32768


def _bank(lead=5):
    """The bank of tests/noise_cases.py inside a device buffer of FILL_BANK, ``lead`` samples in
    (odd: 2-byte aligned only)."""
    flat = C.bank()[0]
    buf = torch.full((lead + flat.shape[0] + 7,), FILL_BANK, dtype=torch.int16, device=DEV)
    buf[lead:lead + flat.shape[0]] = torch.from_numpy(flat.copy())
    return buf[lead:lead + flat.shape[0]]


def _plan(ns, srcs):
    from liteasr_amd import kernels as K

    rows, table = K.mix_plan(ns, srcs)
    return torch.from_numpy(rows).to(DEV), torch.from_numpy(table).to(DEV)


def _run(host, ns, srcs, pad=37, lead=3, inplace=False, plan=None, bank=None, out_pad=29):
    """The kernel on ``host`` (B, S) int16 laid out with row stride S + pad inside a device buffer
    of FILL_IN that starts ``lead`` samples in, into a buffer of FILL_OUT laid out likewise (or in
    place).  Checks every guard; returns (out, gains) on the host."""
    from liteasr_amd import kernels as K

    B, S = host.shape
    buf = torch.full((lead + B * (S + pad) + 5,), FILL_IN, dtype=torch.int16, device=DEV)
    view = buf[lead:lead + B * (S + pad)].view(B, S + pad)[:, :S]
    view.copy_(torch.from_numpy(host))
    rows, table = _plan(ns, srcs) if plan is None else plan
    gains = torch.full((table.shape[0],), -7.0, dtype=torch.float32, device=DEV)
    bank = _bank() if bank is None else bank
    if inplace:
        guard, out, opad = buf, view, pad
    else:
        opad = out_pad
        guard = torch.full((lead + B * (S + opad) + 5,), FILL_OUT, dtype=torch.int16, device=DEV)
        out = guard[lead:lead + B * (S + opad)].view(B, S + opad)[:, :S]
    got = K.mix_i16(view, bank, rows, table, out=out, gains=gains)
    assert got is out
    torch.cuda.synchronize()
    fill = FILL_IN if inplace else FILL_OUT
    assert (guard[:lead] == fill).all() and (guard[-5:] == fill).all()
    if opad:
        assert (guard[lead:lead + B * (S + opad)].view(B, S + opad)[:, S:] == fill).all()
    if not inplace:  # the input is untouched
        assert (buf[:lead] == FILL_IN).all() and (buf[-5:] == FILL_IN).all()
        assert torch.equal(view.cpu(), torch.from_numpy(host))
        if pad:
            assert (buf[lead:lead + B * (S + pad)].view(B, S + pad)[:, S:] == FILL_IN).all()
    return out.cpu().numpy(), gains.cpu().numpy()


def _case(name):
    ns = [n for n, _, _ in C.rows()]
    return C.batch(name), ns, [C.plan_sources(r) for r in range(len(ns))]


@pytest.fixture(scope="module")
def base():
    """The out-of-place, strided run of every signal's batch, shared by the tests below."""
    return {name: _run(*_case(name)) for name in C.SIGNALS}


@pytest.mark.parametrize("name", C.SIGNALS)
def test_parity_with_float64(name, base):
    """Rows of 0, 1, 399, 400, 4000 and 16000 samples with 0, 1, 3 and 8 sources, neighbouring rows
    with different counts, recordings of 1 to 16000 samples (shorter and longer than the row, the
    first and the last of the bank, starts at L - 1, an all-zero one), SNRs from -5 to 40 dB, an
    all-zero row, of one signal in one call."""
    host = C.batch(name)
    out, gains = base[name]
    differed, excused, total, lo, hi = {}, {}, {}, False, False
    first = 0
    for r, (n, srcs, zero) in enumerate(C.rows()):
        k = len(srcs)
        y64 = C.reference(name, r)
        want = R.quantise(y64)
        got = out[r, :n]
        assert y64.shape == (n,) and (out[r, n:] == 0).all()
        # the gains are float32(sqrt(Ex / Ev r)) of numpy, bit for bit
        g = gains[first:first + k]
        assert np.array_equal(g.view(np.int32), C.reference_gains(name, r).view(np.int32)), (r, g)
        first += k
        diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
        assert diff.max(initial=0) <= 1
        strict = R.boundary_distance(y64) > C.BAR_FACTOR * FP32_LOSS[name, k]
        assert (diff[strict] == 0).all()
        if k == 0 or zero or all(rec == C.ZERO_REC for rec, _, _ in srcs):
            assert np.array_equal(got, host[r, :n])  # nothing to mix, a zero row, a zero recording: a copy
            assert zero or k == 0 or (g == 0).all()
        differed[k] = differed.get(k, 0) + int((diff != 0).sum())
        excused[k] = excused.get(k, 0) + int((~strict).sum())
        total[k] = total.get(k, 0) + n
        lo, hi = lo or bool((got == -32768).any()), hi or bool((got == 32767).any())
    assert first == gains.shape[0]
    for k in C.KS:
        print(f"noise parity {name} k={k}: {differed[k]} of {total[k]} samples differ by 1 LSB, {excused[k]} excused")
        assert excused[k] <= C.EXCUSED_CAP * total[k]
    if name in C.SATURATING:
        assert lo and hi


def test_structure_is_bit_exact(base):
    """The same bytes whatever the row order, alone in a batch of one, at other strides and base
    alignments, packed, in place, and with another bank alignment."""
    name = "noise_full"
    host, ns, srcs = _case(name)
    out, gains = base[name]
    B = host.shape[0]
    again, g2 = _run(host, ns, srcs, inplace=True)
    assert np.array_equal(again, out) and np.array_equal(g2.view(np.int32), gains.view(np.int32))
    for kw in (dict(pad=0, lead=0, out_pad=0), dict(pad=1, lead=1, out_pad=3), dict(pad=8, lead=8, out_pad=16),
               dict(pad=0, lead=0, inplace=True), dict(bank=_bank(lead=8))):
        o, g = _run(host, ns, srcs, **kw)
        assert np.array_equal(o, out) and np.array_equal(g.view(np.int32), gains.view(np.int32)), kw
    perm = np.random.default_rng(5).permutation(B)
    o, _ = _run(host[perm], [ns[i] for i in perm], [srcs[i] for i in perm])
    assert np.array_equal(o, out[perm])
    assert [(ns[r], len(srcs[r])) for r in (22, 21, 14, 0)] == [(16000, 8), (16000, 3), (400, 1), (0, 0)]
    for r in (22, 21, 14, 0):
        for inplace in (False, True):
            o, _ = _run(host[r:r + 1], ns[r:r + 1], srcs[r:r + 1], inplace=inplace)
            assert np.array_equal(o[0], out[r])
        o, _ = _run(host[r:r + 1, :max(ns[r], 1)], ns[r:r + 1], srcs[r:r + 1])  # S = n: no padding at all
        assert np.array_equal(o[0], out[r, :max(ns[r], 1)])


def test_malformed_plan_is_clamped_or_skipped(base):
    """n past S is clamped, a negative n is an empty row; a source outside the bank, a start outside
    its recording, an r that is no finite number >= 0, a count of 9 or a source range outside the
    table mix nothing; the guards of _run hold throughout."""
    from liteasr_amd import kernels as K

    name = "sine_1234"
    host, ns, srcs = _case(name)
    out, _ = base[name]
    total = C.bank()[0].shape[0]
    long_rows = [r for r, (n, s, _) in enumerate(C.rows()) if n == 16000 and len(s) >= 1]
    a, b = long_rows[0], long_rows[1]
    rows, table = K.mix_plan(ns, srcs)
    fa, fb = int(rows[a, 1]), int(rows[b, 1])
    rows[a, 0] = 10 ** 9  # n > S: the row's S samples (they are all there: n = S = 16000)
    bad = []
    for col, val in ((0, total), (0, -1), (1, 0), (1, total + 1), (2, -1), (2, 10 ** 12), (1, 2 ** 62)):
        t = table.copy()
        t[fb:fb + int(rows[b, 2]), col] = val
        bad.append((rows.copy(), t))
    for val in (np.nan, np.inf, -1.0):
        t = table.copy()
        t[fb:fb + int(rows[b, 2]), 3] = np.asarray([val]).view(np.int64)[0]
        bad.append((rows.copy(), t))
    for first, count in ((fb, 9), (fb, -1), (-1, 1), (table.shape[0], 1), (table.shape[0] - 1, 3), (2 ** 31 - 1, 8)):
        r2 = rows.copy()
        r2[b, 1], r2[b, 2] = first, count
        bad.append((r2, table.copy()))
    for r2, t in bad:
        o, _ = _run(host, ns, srcs, plan=(torch.from_numpy(r2).to(DEV), torch.from_numpy(t).to(DEV)))
        assert np.array_equal(o[b], host[b])  # nothing mixed into row b
        keep = [r for r in range(host.shape[0]) if r != b]
        assert np.array_equal(o[keep], out[keep])  # row a clamped, the others as they were
    r2 = rows.copy()
    r2[b, 0], r2[a, 0] = -5, 4000
    o, _ = _run(host, ns, srcs, plan=(torch.from_numpy(r2).to(DEV), torch.from_numpy(table).to(DEV)), inplace=True)
    assert (o[b] == 0).all() and (o[a, 4000:] == 0).all() and (o[a, :4000] != host[a, :4000]).any()
    # an empty bank and an empty table: every source is skipped
    empty = torch.zeros(0, dtype=torch.int16, device=DEV)
    o, _ = _run(host, ns, srcs, bank=empty)
    assert np.array_equal(o, host)
    o, _ = _run(host, ns, srcs, plan=(torch.from_numpy(rows).to(DEV), torch.zeros(0, 4, dtype=torch.int64, device=DEV)))
    assert np.array_equal(o, host)


def test_argument_checks():
    """Each raises before anything is launched: the output buffer keeps its sentinel."""
    from liteasr_amd import _native as N
    from liteasr_amd import kernels as K

    pcm = torch.zeros(2, 1000, dtype=torch.int16, device=DEV)
    bank = _bank(lead=8)
    rows, table = _plan([1000, 900], [[(0, 1, 0, 1.0)], [(1, 777, 3, 0.1), (778, 5000, 0, 0.5)]])
    out = torch.full((2, 1000), FILL_OUT, dtype=torch.int16, device=DEV)
    gains = torch.zeros(3, dtype=torch.float32, device=DEV)
    good = dict(pcm=pcm, bank=bank, rows=rows, sources=table, out=out, gains=gains)
    for bad in (dict(pcm=pcm.float()), dict(pcm=pcm.cpu()), dict(pcm=pcm.t().contiguous().t()), dict(pcm=pcm[0]),
                dict(pcm=pcm[:1].expand(2, 1000)), dict(bank=bank.float()), dict(bank=bank.cpu()),
                dict(bank=bank.view(1, -1)), dict(bank=bank[::2]), dict(rows=rows.long()), dict(rows=rows.cpu()),
                dict(rows=rows[:1]), dict(rows=rows[:, :2]), dict(rows=rows.t().contiguous().t()),
                dict(sources=table.int()), dict(sources=table[:, :3]), dict(sources=table.cpu()),
                dict(sources=table.t().contiguous().t()), dict(gains=gains.double()), dict(gains=gains[:2]),
                dict(gains=gains.cpu()), dict(out=out.float()), dict(out=out[:1]), dict(out=out.cpu()),
                dict(out=out.t().contiguous().t()), dict(out=out[0])):
        a = dict(good, **bad)
        with pytest.raises(TypeError):
            K.mix_i16(a["pcm"], a["bank"], a["rows"], a["sources"], out=a["out"], gains=a["gains"])
    with pytest.raises(ValueError):
        K.mix_i16(pcm, bank, rows, table, out=torch.empty(2, 1001, dtype=torch.int16, device=DEV))
    with pytest.raises(ValueError):
        K.mix_plan([1, 2], [[]])
    with pytest.raises(ValueError):
        K.mix_plan([1], [[(0, 1, 0, 1.0)] * 9])
    # the C entry checks for itself
    st = K.stream()
    need = N.load().lasr_mix_ws_bytes(2, 1000)
    assert need == 2 * 1 * 9 * 8 and N.load().lasr_mix_ws_bytes(3, 4097) == 3 * 2 * 9 * 8
    assert N.load().lasr_mix_ws_bytes(0, 1000) == 0 and N.load().lasr_mix_ws_bytes(2, 0) == 0
    ws = torch.zeros(need // 8 + 1, dtype=torch.int64, device=DEV)
    args = dict(pcm=pcm.data_ptr(), istride=1000, B=2, S=1000, bank=bank.data_ptr(), blen=bank.numel(),
                plan=rows.data_ptr(), src=table.data_ptr(), nsrc=3, out=out.data_ptr(), ostride=1000,
                gains=gains.data_ptr(), ws=ws.data_ptr(), wsb=need)

    def call(**kw):
        a = dict(args, **kw)
        N.call("lasr_mix_i16", a["pcm"], a["istride"], a["B"], a["S"], a["bank"], a["blen"], a["plan"], a["src"],
               a["nsrc"], a["out"], a["ostride"], a["gains"], a["ws"], a["wsb"], st)

    for bad in (dict(B=-1), dict(S=-1), dict(blen=-1), dict(nsrc=-1), dict(wsb=-1), dict(S=2 ** 29 + 1), dict(pcm=None),
                dict(out=None), dict(plan=None), dict(bank=None), dict(src=None), dict(ws=None),
                dict(pcm=pcm.data_ptr() + 1), dict(out=out.data_ptr() + 1), dict(bank=bank.data_ptr() + 1),
                dict(plan=rows.data_ptr() + 2), dict(src=table.data_ptr() + 4), dict(gains=gains.data_ptr() + 2),
                dict(ws=ws.data_ptr() + 4), dict(istride=999), dict(ostride=999), dict(B=65536), dict(wsb=need - 8),
                dict(out=pcm.data_ptr() + 1000), dict(out=pcm.data_ptr() + 2), dict(out=pcm.data_ptr(), ostride=1001),
                dict(pcm=out.data_ptr() + 1000, B=1), dict(out=bank.data_ptr() + 16), dict(ws=out.data_ptr() + 8),
                dict(ws=pcm.data_ptr() + 8)):
        with pytest.raises(N.NativeError):
            call(**bad)
    torch.cuda.synchronize()
    assert (out == FILL_OUT).all() and (pcm == 0).all() and (gains == 0).all()
    call(B=0, out=None)
    call(S=0, out=None, pcm=None)
    call(gains=None)
    call(bank=None, blen=0)
    call(src=None, nsrc=0)
    call(out=pcm.data_ptr())  # in place
    torch.cuda.synchronize()
    assert (out == 0).all() and (pcm == 0).all()


def _noise_dirs(root):
    from liteasr_amd.utils.synthetic import synthetic_wav_dir

    return [synthetic_wav_dir(os.path.join(root, "noise_a"), [5000, 777, 24000], seed=21),
            synthetic_wav_dir(os.path.join(root, "noise_b"), [16000, 1, 9000, 3000], seed=22)]


@pytest.mark.parametrize("speed", [None, [0.9, 1.0, 1.1]])
def test_trainer_features_equal_the_kernels(tmp_path, speed):
    """Trainer._features on a collated batch, with noise alone and with speed_perturb on, equals
    Fbank(mix(resample(pcm))) called through the kernels with the delivered plans, bit for bit."""
    from types import SimpleNamespace

    from liteasr_amd import kernels as K
    from liteasr_amd.dataclass.vocab import Vocab
    from liteasr_amd.dataset import AudioFileDataset
    from liteasr_amd.trainer import Trainer
    from liteasr_amd.utils.frontend import Fbank, NoisePlan, NoiseSpec, ResamplePlan
    from liteasr_amd.utils.synthetic import synthetic_wav_dir

    wav = synthetic_wav_dir(str(tmp_path / "wav"), [8000, 19200, 12345, 16001, 9000, 400], seed=1)
    spec = NoiseSpec(_noise_dirs(str(tmp_path)), prob=0.9, snr=[0, 15, 5, 20], sources=[2, 2, 3, 8], seed=3)
    ds = AudioFileDataset("train", wav, None, None, None, Vocab(os.path.join(wav, "vocab.txt")), speed_perturb=speed,
                          noise=spec)
    fe = Fbank(80, noise=spec)
    tr = SimpleNamespace(device=torch.device(DEV), task=SimpleNamespace(frontend=fe))
    batch = ds.collator([ds.data])
    assert isinstance(batch[-1], NoisePlan) and len(batch) == (6 if speed else 5)
    assert bool(speed) == isinstance(batch[-2], ResamplePlan) and batch[0].dtype == torch.int16
    nplan = batch[-1]
    assert (nplan.rows[:, 2] > 0).any() and int(nplan.rows[:, 2].max()) > 1
    got = Trainer._features(tr, batch)
    assert len(got) == 4 and got[0].dtype == torch.float32
    pcm = batch[0].to(DEV)
    if speed:
        rp = batch[-2]
        table, taps = (torch.from_numpy(v).to(DEV) for v in K.resample_tables(rp.ratios))
        pcm = K.resample_i16(pcm, rp.rows.to(DEV), table, taps, max_out=rp.max_out)
        assert nplan.rows[:, 0].tolist() == rp.rows[:, 1].tolist()
    bank = fe.noise.read_bank().to(DEV)
    mixed = K.mix_i16(pcm, bank, nplan.rows.to(DEV), nplan.sources.to(DEV))
    assert not torch.equal(mixed, pcm)
    want = K.fbank(mixed, batch[1].to(DEV).to(torch.int32), 80, max_frames=int(batch[1].max()))
    assert torch.equal(got[0], want)
    assert all(torch.equal(u.cpu(), v) for u, v in zip(got[1:], batch[1:4]))
    assert batch[0].device.type == "cpu"  # the collated batch itself is untouched


def test_task_asr_noise_end_to_end(tmp_path):
    """Two Trainer steps (tiny conformer, SpecAugment on) and a validation pass from a synthetic
    wav.scp directory with two small noise directories: finite losses, equal bit for bit across
    two runs with equal seeds, different from the run with the option off, whose validation loss
    they equal bit for bit; the delivered batch is still int16."""
    from liteasr_amd.utils.synthetic import synthetic_wav_dir

    wav = synthetic_wav_dir(str(tmp_path / "wav"), [8000, 19200, 12345, 16001, 9000, 11000], seed=1)
    dirs = _noise_dirs(str(tmp_path))
    outs, procs = {}, {}
    for name, noise in (("on", "[" + ",".join(dirs) + "]"), ("again", "[" + ",".join(dirs) + "]"), ("off", "null")):
        procs[name] = subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_noise_trainer_step.py"), wav, wav,
                                        str(tmp_path / ("run_" + name)), noise], stdout=subprocess.PIPE,
                                       stderr=subprocess.PIPE, text=True)  # the three runs side by side
    for name, p in procs.items():
        stdout, stderr = p.communicate(timeout=300)
        assert p.returncode == 0, stderr[-3000:]
        outs[name] = json.loads(stdout.strip().splitlines()[-1])
    a, b, off = outs["on"], outs["again"], outs["off"]
    for o in (a, b, off):
        assert o["iters"] == 2 and o["skipped"] == 0 and len(o["losses"]) == 2
        assert all(math.isfinite(v) for v in o["losses"]) and math.isfinite(o["valid"])
        assert all(s[0] == "torch.int16" for s in o["delivered"] + o["valid_delivered"])
        assert all(s[2:] == [4, False] for s in o["valid_delivered"])  # validation is never augmented
    assert [s[2:] for s in a["delivered"]] == [[6, True]] * 2 and [s[2:] for s in off["delivered"]] == [[5, False]] * 2
    assert a["sources"] == b["sources"] and sum(a["sources"]) > 0
    assert a["losses"] == b["losses"] and a["valid"] == b["valid"]
    assert a["losses"] != off["losses"]
    assert a["seen"] == off["seen"]  # the same batches, frame counts and SpecAugment plan sizes
    assert a["valid"] == off["valid"] and a["valid_seen"] == off["valid_seen"]
