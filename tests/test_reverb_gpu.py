"""``lasr_reverb_i16`` on the GPU against the rounded, saturated float64 restatement of the transform
(tests/reverb_ref.py), its gains, its bit-exact structure, its handling of a malformed plan, the
argument checks, and task=asr end to end with ``frontend.rir``.  The reference project has no
counterpart.

The bars of the parity test are set by the reference, never by the kernel: tests/reverb_ref.py run
in float32 (the larger of a direct convolution and of overlap-save with scipy.fft at the kernel's
block size) loses FP32_LOSS (LSB of the int16 output) against float64 on these inputs, and its gain
deviates by GAIN_DEV (relative) from the float64 gain (``python tests/reverb_cases.py`` prints both
tables).  Every sample must be within 1 LSB of the quantised float64 value, and exactly equal to it
unless the float64 value lies within BAR_FACTOR x FP32_LOSS of a point where the quantisation changes
(a half-integer, or the saturation point); the gain within BAR_FACTOR x GAIN_DEV of the float64
gain.  The excused share is capped at 10 % by tests/test_reverb_cpu.py on the reference alone."""

import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import reverb_cases as C
import reverb_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
P = C.BLOCK
# float32 restatements against float64, LSB, measured with tests/reverb_cases.py
FP32_LOSS = {
    ("gauss", 1): 1.754e-03, ("gauss", 2): 2.210e-03, ("gauss", 257): 2.173e-03, ("gauss", 300): 2.049e-03,
    ("gauss", P - 1): 2.302e-03, ("gauss", P): 1.919e-03, ("gauss", P + 1): 2.494e-03, ("gauss", 4000): 2.333e-03,
    ("gauss", 2 * P + 1000): 2.694e-03,
    ("gauss_small", 1): 6.521e-06, ("gauss_small", 2): 8.268e-06, ("gauss_small", 257): 9.030e-06,
    ("gauss_small", 300): 9.562e-06, ("gauss_small", P - 1): 8.582e-06, ("gauss_small", P): 8.036e-06,
    ("gauss_small", P + 1): 8.430e-06, ("gauss_small", 4000): 9.644e-06, ("gauss_small", 2 * P + 1000): 8.262e-06,
    ("bursts", 4000): 8.392e-03, ("square", 4000): 1.467e-02,
}
# the float32 restatements' gain against the float64 gain, relative, from the same run
GAIN_DEV = {"gauss": 1.203e-07, "gauss_small": 1.204e-07, "bursts": 7.304e-08, "square": 1.166e-07}
FILL_IN, FILL_OUT, FILL_BANK = 32767, -21555, -32768


def _bank(lead=5, flat=None):
    """The bank of tests/reverb_cases.py inside a device buffer of FILL_BANK, ``lead`` samples in
    (odd: 2-byte aligned only)."""
    flat = C.bank()[0] if flat is None else flat
    buf = torch.full((lead + flat.shape[0] + 7,), FILL_BANK, dtype=torch.int16, device=DEV)
    buf[lead:lead + flat.shape[0]] = torch.from_numpy(flat.copy())
    return buf[lead:lead + flat.shape[0]]


def _plan(ns, ids):
    from liteasr_amd import kernels as K

    return torch.from_numpy(K.reverb_plan(ns, ids)).to(DEV)


def _table(table=None):
    return torch.from_numpy(np.ascontiguousarray(C.bank()[1] if table is None else table)).to(DEV)


def _run(host, ns, ids, pad=37, lead=3, inplace=False, plan=None, table=None, bank=None, out_pad=29, max_taps=None):
    """The kernel on ``host`` (B, S) int16 laid out with row stride S + pad inside a device buffer
    of FILL_IN that starts ``lead`` samples in, into a buffer of FILL_OUT laid out likewise (or in
    place).  Checks every guard; returns (out, gains) on the host."""
    from liteasr_amd import kernels as K

    B, S = host.shape
    buf = torch.full((lead + B * (S + pad) + 5,), FILL_IN, dtype=torch.int16, device=DEV)
    view = buf[lead:lead + B * (S + pad)].view(B, S + pad)[:, :S]
    view.copy_(torch.from_numpy(host))
    rows = _plan(ns, ids) if plan is None else plan
    gains = torch.full((B,), -7.0, dtype=torch.float32, device=DEV)
    bank = _bank() if bank is None else bank
    if inplace:
        guard, out, opad = buf, view, pad
    else:
        opad = out_pad
        guard = torch.full((lead + B * (S + opad) + 5,), FILL_OUT, dtype=torch.int16, device=DEV)
        out = guard[lead:lead + B * (S + opad)].view(B, S + opad)[:, :S]
    got = K.reverb_i16(view, bank, rows, _table(table), out=out, gains=gains, max_taps=max_taps)
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
    rows = C.rows(name)
    return C.batch(name), [n for n, _, _ in rows], [i for _, i, _ in rows]


@pytest.fixture(scope="module")
def base():
    """The out-of-place, strided run of every signal's batch, shared by the tests below."""
    return {name: _run(*_case(name)) for name in C.SIGNALS}


@pytest.mark.parametrize("name", C.SIGNALS)
def test_parity_with_float64(name, base):
    """Rows of 0, 1, 399, 400, 4000 and 16000 samples with RIRs of 1 to 2 P + 1000 taps (peaks at 0,
    at L - 1 and inside), neighbouring rows with different RIRs, one row in four with none, an
    all-zero row, of one signal in one call."""
    host = C.batch(name)
    out, gains = base[name]
    differed, excused, total, lo, hi = {}, {}, {}, False, False
    worst_gain = 0.0
    for r, (n, i, zero) in enumerate(C.rows(name)):
        y64, _ = C.reference(name, r)
        want = R.quantise(y64)
        got = out[r, :n]
        assert y64.shape == (n,) and (out[r, n:] == 0).all()
        if i < 0:
            assert np.array_equal(got, host[r, :n]) and gains[r] == 1.0  # a copy
            continue
        L = C.RIR_SPECS[i][0]
        g64 = C.exact_gain(name, r)
        if g64 == 0.0:
            assert gains[r] == 0.0 and (got == 0).all() and (zero or not host[r, :n].any())  # no energy: zeros
            continue
        dev = abs(float(gains[r]) - g64) / g64
        worst_gain = max(worst_gain, dev)
        assert dev <= C.BAR_FACTOR * GAIN_DEV[name], (r, dev)
        diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
        assert diff.max(initial=0) <= 1, (r, int(diff.max()))
        strict = R.boundary_distance(y64) > C.BAR_FACTOR * FP32_LOSS[name, L]
        assert (diff[strict] == 0).all(), (r, n, L)
        if i in C.DELTAS:
            assert np.array_equal(got, host[r, :n])  # a delta of any amplitude, at its own peak: the input
        differed[L] = differed.get(L, 0) + int((diff != 0).sum())
        excused[L] = excused.get(L, 0) + int((~strict).sum())
        total[L] = total.get(L, 0) + n
        lo, hi = lo or bool((got == -32768).any()), hi or bool((got == 32767).any())
    print(f"reverb parity {name}: worst gain deviation {worst_gain:.3e} (bar {C.BAR_FACTOR * GAIN_DEV[name]:.3e})")
    for L in C.taps(name):
        print(f"reverb parity {name} L={L}: {differed[L]} of {total[L]} samples differ by 1 LSB, {excused[L]} excused")
        assert excused[L] <= C.EXCUSED_CAP * total[L]
    if name in C.SATURATING:
        assert lo and hi


def test_structure_is_bit_exact(base):
    """The same bytes whatever the row order, alone in a batch of one, beside other neighbours, at
    other strides and base alignments, packed, with a larger S, in place, run twice, with another
    bank alignment and with a workspace made for longer RIRs."""
    name = "gauss"
    host, ns, ids = _case(name)
    out, gains = base[name]
    B, S = host.shape
    again, g2 = _run(host, ns, ids, inplace=True)
    assert np.array_equal(again, out) and np.array_equal(g2.view(np.int32), gains.view(np.int32))
    for kw in (dict(), dict(pad=0, lead=0, out_pad=0), dict(pad=1, lead=1, out_pad=3), dict(pad=8, lead=8, out_pad=16),
               dict(pad=0, lead=0, inplace=True), dict(bank=_bank(lead=8)), dict(max_taps=65536)):
        o, g = _run(host, ns, ids, **kw)
        assert np.array_equal(o, out) and np.array_equal(g.view(np.int32), gains.view(np.int32)), kw
    perm = np.random.default_rng(5).permutation(B)
    o, g = _run(host[perm], [ns[i] for i in perm], [ids[i] for i in perm])
    assert np.array_equal(o, out[perm]) and np.array_equal(g.view(np.int32), gains[perm].view(np.int32))
    wide = np.zeros((B, S + 2 * P + 77), dtype=np.int16)  # a larger S: more blocks per row in the workspace
    wide[:, :S] = host
    o, g = _run(wide, ns, ids)
    assert np.array_equal(o[:, :S], out) and (o[:, S:] == 0).all()
    assert np.array_equal(g.view(np.int32), gains.view(np.int32))
    picks = []  # per length the two rows with the longest RIRs
    for n in (16000, 4000, 400):
        rs = [r for r, (m, i, _) in enumerate(C.rows(name)) if m == n and i >= 0 and i not in C.DELTAS]
        picks += sorted(rs, key=lambda r: -C.RIR_SPECS[ids[r]][0])[:2]
    assert len(picks) == 6 and C.RIR_SPECS[ids[picks[0]]][0] == 2 * P + 1000
    for r in picks:
        for inplace in (False, True):
            o, g = _run(host[r:r + 1], ns[r:r + 1], ids[r:r + 1], inplace=inplace)
            assert np.array_equal(o[0], out[r]) and g[0] == gains[r]
        o, _ = _run(host[r:r + 1, :ns[r]], ns[r:r + 1], ids[r:r + 1])  # S = n: no padding at all
        assert np.array_equal(o[0], out[r, :ns[r]])


def test_malformed_plan_is_clamped_or_zeroed(base):
    """n past S is clamped, a negative n is an empty row; an RIR index outside the table, a table
    entry that leaves the bank, a length of 0 or 65537 or a peak outside [0, L) gives a zero row;
    the guards of _run hold throughout and the other rows are what they were."""
    from liteasr_amd import kernels as K

    name = "gauss"
    host, ns, ids = _case(name)
    out, gains = base[name]
    flat, table = C.bank()
    total, nr = flat.shape[0], table.shape[0]
    long_rows = [r for r, (n, i, _) in enumerate(C.rows(name)) if n == 16000 and i >= 0 and i not in C.DELTAS]
    a, b = long_rows[0], long_rows[1]
    keep = [r for r in range(host.shape[0]) if r != b]
    rows = K.reverb_plan(ns, ids)
    rows[a, 0] = 10 ** 9  # n > S: the row's S samples (they are all there: n = S = 16000)
    for idx in (-2, nr, 2 ** 31 - 1, -2 ** 31):
        r2 = rows.copy()
        r2[b, 1] = idx
        o, g = _run(host, ns, ids, plan=torch.from_numpy(r2).to(DEV))
        assert (o[b] == 0).all() and g[b] == 0.0 and np.array_equal(o[keep], out[keep])
    ib = ids[b]
    off, L, p = (int(v) for v in table[ib])
    for col, val in ((0, -1), (0, total - L + 1), (0, 2 ** 62), (1, 0), (1, -5), (1, 65537), (1, total - off + 1),
                     (1, 2 ** 62), (2, -1), (2, L), (2, 2 ** 40)):
        t = table.copy()
        t[ib, col] = val
        use = [r for r in keep if ids[r] != ib]  # the other rows that name this RIR are zeroed with it
        o, g = _run(host, ns, ids, plan=torch.from_numpy(rows).to(DEV), table=t)
        assert (o[b] == 0).all() and g[b] == 0.0 and np.array_equal(o[use], out[use]), (col, val)
    r2 = rows.copy()
    r2[b, 0], r2[a, 0] = -5, 4000
    o, g = _run(host, ns, ids, plan=torch.from_numpy(r2).to(DEV), inplace=True)
    assert (o[b] == 0).all() and g[b] == 0.0 and (o[a, 4000:] == 0).all() and o[a, :4000].any()
    # a workspace made for shorter RIRs refuses the longer ones and nothing else
    o, g = _run(host, ns, ids, max_taps=P)
    long_ids = [i for i, (L, _, _) in enumerate(C.RIR_SPECS) if L > P]
    for r in range(host.shape[0]):
        if ids[r] in long_ids:
            assert (o[r] == 0).all() and g[r] == 0.0
        else:
            assert np.array_equal(o[r], out[r])
    # an empty bank and an empty table: every RIR is refused, the copies stay
    for kw in (dict(bank=torch.zeros(0, dtype=torch.int16, device=DEV)), dict(table=np.zeros((0, 3), dtype=np.int64))):
        o, g = _run(host, ns, ids, **kw)
        for r in range(host.shape[0]):
            assert np.array_equal(o[r], host[r] if ids[r] < 0 else np.zeros_like(host[r]))


def test_argument_checks():
    """Each raises before anything is launched: the output buffer keeps its sentinel."""
    from liteasr_amd import _native as N
    from liteasr_amd import kernels as K

    pcm = torch.zeros(2, 1000, dtype=torch.int16, device=DEV)
    bank = _bank(lead=8)
    rows = _plan([1000, 900], [1, 6])
    table = _table()
    out = torch.full((2, 1000), FILL_OUT, dtype=torch.int16, device=DEV)
    gains = torch.zeros(2, dtype=torch.float32, device=DEV)
    good = dict(pcm=pcm, bank=bank, rows=rows, rirs=table, out=out, gains=gains)
    for bad in (dict(pcm=pcm.float()), dict(pcm=pcm.cpu()), dict(pcm=pcm.t().contiguous().t()), dict(pcm=pcm[0]),
                dict(pcm=pcm[:1].expand(2, 1000)), dict(bank=bank.float()), dict(bank=bank.cpu()),
                dict(bank=bank.view(1, -1)), dict(bank=bank[::2]), dict(rows=rows.long()), dict(rows=rows.cpu()),
                dict(rows=rows[:1]), dict(rows=rows[:, :1]), dict(rows=rows.t().contiguous().t()),
                dict(rirs=table.int()), dict(rirs=table[:, :2]), dict(rirs=table.cpu()),
                dict(rirs=table.t().contiguous().t()), dict(gains=gains.double()), dict(gains=gains[:1]),
                dict(gains=gains.cpu()), dict(out=out.float()), dict(out=out[:1]), dict(out=out.cpu()),
                dict(out=out.t().contiguous().t()), dict(out=out[0])):
        a = dict(good, **bad)
        with pytest.raises(TypeError):
            K.reverb_i16(a["pcm"], a["bank"], a["rows"], a["rirs"], out=a["out"], gains=a["gains"])
    with pytest.raises(ValueError):
        K.reverb_i16(pcm, bank, rows, table, out=torch.empty(2, 1001, dtype=torch.int16, device=DEV))
    with pytest.raises(ValueError):
        K.reverb_plan([1, 2], [0])
    # the C entry checks for itself
    st = K.stream()
    lib = N.load()
    need = lib.lasr_reverb_ws_bytes(2, 1000, 4000)
    # per row 1 block and 2 partitions: 4 spectra of 16 KB, 2048 fp32, one double and one int64
    assert need == 2 * (4 * 16384 + 8192 + 8 + 8)
    assert lib.lasr_reverb_ws_bytes(2, 1000, 10 ** 9) == lib.lasr_reverb_ws_bytes(2, 1000, 65536) > need
    assert lib.lasr_reverb_ws_bytes(2, 1000, 0) == lib.lasr_reverb_ws_bytes(2, 1000, 2048) < need
    assert lib.lasr_reverb_ws_bytes(0, 1000, 4000) == 0 and lib.lasr_reverb_ws_bytes(2, 0, 4000) == 0
    tab = torch.from_numpy(K.reverb_tables()).to(DEV)
    assert tab.shape == (4 * K.REVERB_BLOCK,) and tab.dtype == torch.float32
    ws = torch.zeros(need // 8 + 2, dtype=torch.int64, device=DEV)
    small = lib.lasr_reverb_ws_bytes(2, 1000, 1)
    args = dict(pcm=pcm.data_ptr(), istride=1000, B=2, S=1000, bank=bank.data_ptr(), blen=bank.numel(),
                plan=rows.data_ptr(), rirs=table.data_ptr(), nrir=table.shape[0], tab=tab.data_ptr(),
                out=out.data_ptr(), ostride=1000, gains=gains.data_ptr(), ws=ws.data_ptr(), wsb=need)

    def call(**kw):
        a = dict(args, **kw)
        N.call("lasr_reverb_i16", a["pcm"], a["istride"], a["B"], a["S"], a["bank"], a["blen"], a["plan"], a["rirs"],
               a["nrir"], a["tab"], a["out"], a["ostride"], a["gains"], a["ws"], a["wsb"], st)

    for bad in (dict(B=-1), dict(S=-1), dict(blen=-1), dict(nrir=-1), dict(wsb=-1), dict(S=2 ** 29 + 1), dict(pcm=None),
                dict(out=None), dict(plan=None), dict(bank=None), dict(rirs=None), dict(tab=None), dict(ws=None),
                dict(pcm=pcm.data_ptr() + 1), dict(out=out.data_ptr() + 1), dict(bank=bank.data_ptr() + 1),
                dict(plan=rows.data_ptr() + 2), dict(rirs=table.data_ptr() + 4), dict(gains=gains.data_ptr() + 2),
                dict(tab=tab.data_ptr() + 4), dict(ws=ws.data_ptr() + 8), dict(istride=999), dict(ostride=999),
                dict(B=65536), dict(wsb=small - 8), dict(wsb=0),
                dict(out=pcm.data_ptr() + 1000), dict(out=pcm.data_ptr() + 2), dict(out=pcm.data_ptr(), ostride=1001),
                dict(pcm=out.data_ptr() + 1000, B=1), dict(out=bank.data_ptr() + 16), dict(ws=out.data_ptr() + 16),
                dict(ws=pcm.data_ptr() + 16), dict(ws=bank.data_ptr() + 16)):
        with pytest.raises(N.NativeError):
            call(**bad)
    torch.cuda.synchronize()
    assert (out == FILL_OUT).all() and (pcm == 0).all() and (gains == 0).all()
    call(B=0, out=None)
    call(S=0, out=None, pcm=None)
    call(gains=None)
    call(wsb=small)  # made for one partition: the 4000-tap RIR of row 1 is refused, not an error
    call(out=pcm.data_ptr())  # in place
    torch.cuda.synchronize()
    assert (out == 0).all() and (pcm == 0).all()
    call(bank=None, blen=0)
    call(rirs=None, nrir=0)
    torch.cuda.synchronize()
    assert (out == 0).all()


def test_task_asr_rir_end_to_end(tmp_path):
    """tests/_reverb_trainer_step.py in fresh child processes.  (1) Two Trainer steps and a validation
    pass (tiny conformer, SpecAugment on) from a wav.scp directory with one RIR at rir_prob = 1
    equal, bit for bit, the steps from a directory of the kernel's own output written as WAV files
    with the option off, and validation is identical.  (2) With several RIRs at rir_prob = 0.5 two
    runs with equal seeds give equal losses, another rir_seed different ones.  (3) With speed_perturb,
    rir and noise all on, what _features hands to the fbank kernel is speed -> reverb -> noise called
    by hand on the delivered plans, byte for byte (checked in the child)."""
    from liteasr_amd.utils.synthetic import synthetic_rir_dir, synthetic_wav_dir

    lengths = [8000, 19200, 12345, 16001, 9000, 11000]
    wav = synthetic_wav_dir(str(tmp_path / "wav"), lengths, seed=1)
    one = synthetic_rir_dir(str(tmp_path / "rir_one"), [3000], seed=31)
    many = synthetic_rir_dir(str(tmp_path / "rir_many"), [500, 2500, 4100, 1], seed=32)
    noise = synthetic_wav_dir(str(tmp_path / "noise"), [5000, 777, 24000], seed=21)
    wet = str(tmp_path / "wet")
    script = os.path.join(ROOT, "tests", "_reverb_trainer_step.py")

    def start(run, train, *opts):
        return subprocess.Popen([sys.executable, script, train, wav, str(tmp_path / run)] + list(opts),
                                stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)

    def result(p):
        stdout, stderr = p.communicate(timeout=300)
        assert p.returncode == 0, stderr[-3000:]
        return json.loads(stdout.strip().splitlines()[-1])

    procs = {"on": start("run_on", wav, f"rir=[{one}]", "rir_prob=1.0", f"dump={wet}"),
             "half": start("run_half", wav, f"rir=[{many},{one}]", "rir_prob=0.5", "rir_seed=3"),
             "again": start("run_again", wav, f"rir=[{many},{one}]", "rir_prob=0.5", "rir_seed=3"),
             "other": start("run_other", wav, f"rir=[{many},{one}]", "rir_prob=0.5", "rir_seed=4"),
             "all": start("run_all", wav, f"rir=[{many}]", "rir_prob=0.7", f"noise=[{noise}]",
                          "speed_perturb=[0.9,1.0,1.1]", "check=1")}
    outs = {k: result(p) for k, p in procs.items()}
    outs["wet"] = result(start("run_wet", wet))  # the option off, from the reverberated files the first run wrote
    for o in outs.values():
        assert o["iters"] == 2 and o["skipped"] == 0 and len(o["losses"]) == 2
        assert all(math.isfinite(v) for v in o["losses"]) and math.isfinite(o["valid"])
        assert all(s[0] == "torch.int16" for s in o["delivered"] + o["valid_delivered"])
        assert all(s[2:] == [4, []] for s in o["valid_delivered"])  # validation is never augmented
        assert o["valid"] == outs["wet"]["valid"] and o["valid_seen"] == outs["wet"]["valid_seen"]
    on, wetrun = outs["on"], outs["wet"]
    assert [s[2:] for s in on["delivered"]] == [[6, ["ReverbPlan"]]] * 2
    assert [s[2:] for s in wetrun["delivered"]] == [[5, []]] * 2
    assert on["reverberated"] == [3, 3] and on["seen"] == wetrun["seen"]
    assert on["losses"] == wetrun["losses"]
    half, again, other = outs["half"], outs["again"], outs["other"]
    assert half["losses"] == again["losses"] and half["rirs"] == again["rirs"]
    assert half["rirs"] != other["rirs"] and half["losses"] != other["losses"]
    assert 0 < sum(half["reverberated"]) + sum(other["reverberated"]) < 12
    full = outs["all"]
    assert [s[2:] for s in full["delivered"]] == [[8, ["ResamplePlan", "ReverbPlan", "NoisePlan"]]] * 2
    assert full["checked"] == 2 and sum(full["reverberated"]) > 0
