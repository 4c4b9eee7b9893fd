"""True peak and loudness report on the MI355X (vfx_loudness_tp_rows_f32, vfx_loudness_report_rows_f32): the fused
oversample-and-reduce kernel against the float64 definition at every oversampling factor with ragged rows, a 30-minute row,
the ceiling binding between the samples, the public surface with ``true_peak=True`` against float32(g) times the plain
output, and the report against the float64 EBU Tech 3341 / 3342 reference."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import voicefixer_amd  # noqa: E402
from voicefixer_amd import _lib, loudness, ops  # noqa: E402
from test_loudness_cpu import ref_loudness  # noqa: E402
from test_true_peak_cpu import TECH_3342, ref_report, ref_true_peak, sine_segments  # noqa: E402

RATES = [8000, 16000, 22050, 44100, 48000, 96000, 192000]
TP_BOUND = 2e-6           # |TP - ref| <= 2e-6 max(1, ref): the bound tests/test_resample_gpu.py holds the same sum to


@pytest.fixture(scope="module")
def vf(seeded_states):
    return voicefixer_amd.VoiceFixer.from_state(*seeded_states)


@pytest.fixture(scope="module")
def utterance(vf):
    rng = np.random.default_rng(21)
    t = np.arange(3 * 44100) / 44100.0
    x = (0.05 * rng.standard_normal(t.size) * (1 + np.sin(2 * np.pi * 1.5 * t)) + 0.2 * np.sin(2 * np.pi * 180 * t))
    return vf.restore_inmem(x.astype(np.float32), cuda=True)[0]


def _quarter_sine(n, amp, fade=False):
    """A sine at fs / 4 sampled at 45 degrees: every sample is amp / sqrt(2), the peaks lie between the samples.  ``fade``:
    Hann ramps over the first and last eighth (an abrupt start overshoots the amplitude once it is interpolated)."""
    x = amp * np.sin(2 * np.pi * np.arange(n) / 4 + math.pi / 4)
    if fade:
        k = n // 8
        ramp = 0.5 - 0.5 * np.cos(np.pi * np.arange(k) / k)
        x[:k] *= ramp
        x[n - k:] *= ramp[::-1]
    return x.astype(np.float32)


def _tp_ok(tp, ref):
    return abs(tp - ref) <= TP_BOUND * max(1.0, ref)


@pytest.mark.parametrize("fs", RATES)
def test_kernel_matches_float64(fs, utterance):
    rng = np.random.default_rng(fs)
    R = loudness.oversampling(fs)
    first = (0.3 * rng.uniform(-1, 1, int(0.9 * fs))).astype(np.float32)
    first[0] = 0.95
    last = (0.3 * rng.uniform(-1, 1, int(1.1 * fs) + 3)).astype(np.float32)
    last[-1] = -0.95
    rows = [(0.8 * rng.uniform(-1, 1, 100)).astype(np.float32),        # shorter than J
            np.zeros(int(0.7 * fs), np.float32),                       # silence
            rng.uniform(-1, 1, int(2.3 * fs) + 1).astype(np.float32),  # full-scale uniform noise
            _quarter_sine(int(1.6 * fs) + 2, 0.5),                     # fs / 4 at 45 degrees
            utterance[: int(2.9 * fs)].copy(),                         # a restored seeded utterance (read as audio at fs)
            first, last]
    B = len(rows)
    lens = [len(r) for r in rows]
    W = max(lens) + 40
    x = np.full((B, W), np.nan, np.float32)                            # NaN canaries past every row end
    for r, v in enumerate(rows):
        x[r, :lens[r]] = v
    xd = torch.from_numpy(x).cuda()
    n_rows = torch.tensor(lens, dtype=torch.int32, device="cuda")
    lib = _lib.lib()
    c0 = lib.vfx_launch_count()
    plain = ops.loudness_rows(xd, n_rows, fs).cpu().numpy()
    c1 = lib.vfx_launch_count()
    res = ops.loudness_rows(xd, n_rows, fs, true_peak=True).cpu().numpy()
    c2 = lib.vfx_launch_count()
    # the header's promise: one launch more than the sample-peak path when R > 1, none more when R = 1
    assert c1 - c0 == 3 and (c2 - c1) - (c1 - c0) == (1 if R > 1 else 0)
    assert res.shape == (B, 4) and np.array_equal(res[:, :3], plain)   # L, g = 1, P: the bits of the sample-peak path
    assert np.array_equal(xd.cpu().numpy(), x, equal_nan=True)         # measure only: x and the canaries untouched
    worst = 0.0
    for r in range(B):
        L, g, P, TP = res[r]
        ref = ref_true_peak(x[r, :lens[r]], fs)
        err = abs(TP - ref) / max(1.0, ref)
        worst = max(worst, err)
        print("true peak %d Hz row %d: P %.7f TP %.7f float64 %.7f err %.2e" % (fs, r, P, TP, ref, err))
        assert P == np.abs(x[r, :lens[r]]).max() and TP >= P and g == 1.0, (fs, r)
        assert _tp_ok(TP, ref), (fs, r, TP, ref)
        if R == 1:
            assert TP == P
    print("true peak %d Hz (R = %d): max |TP - ref| / max(1, ref) = %.2e" % (fs, R, worst))
    assert res[1, 3] == 0.0 and loudness.to_db(res[1, 3]) == -math.inf and res[1, 0] == -math.inf
    if R > 1:
        assert res[2, 3] > 1.3 * res[2, 2]                            # noise: the continuous peak is far above the samples
        assert res[3, 3] >= 0.5 * (1 - 1e-4) and abs(res[3, 2] - 0.5 / math.sqrt(2)) <= 1e-6
    # a row measured alone gives the same bits as inside the ragged batch
    for r in (2, 4, 6):
        alone = ops.loudness_rows(torch.from_numpy(x[r:r + 1, :lens[r]].copy()).cuda(), n_rows[r:r + 1].clone(), fs,
                                  true_peak=True).cpu().numpy()
        assert np.array_equal(alone[0], res[r]), (fs, r)
    # with a target: the true-peak gain, applied up to every row's own end
    out = torch.full((B, W), float("nan"), device="cuda")
    c0 = lib.vfx_launch_count()
    res2 = ops.loudness_rows(xd, n_rows, fs, target=-14.0, ceiling_db=-2.0, out=out, true_peak=True).cpu().numpy()
    assert lib.vfx_launch_count() - c0 == 4 + (1 if R > 1 else 0)
    got = out.cpu().numpy()
    assert np.array_equal(res2[:, [0, 2, 3]], res[:, [0, 2, 3]])
    for r in range(B):
        L, g, P, TP = res2[r]
        if math.isinf(L):
            assert g == 1.0
        else:
            assert g == pytest.approx(min(10 ** ((-14.0 - L) / 20), 10 ** (-2.0 / 20) / TP), rel=1e-12), (fs, r)
        assert np.array_equal(got[r, :lens[r]], np.float32(g) * x[r, :lens[r]]), (fs, r)
        assert np.all(np.isnan(got[r, lens[r]:])), (fs, r)
    assert np.array_equal(xd.cpu().numpy(), x, equal_nan=True)
    # bad arguments: EINVAL, nothing launched
    import ctypes as C
    p = loudness.plan(fs)
    coef = (C.c_double * 10)(*p["coef"])
    bank, J, c = ops.true_peak_bank("cuda", R) if R > 1 else (torch.zeros(4, device="cuda"), 1, 0)
    nb = lib.vfx_loudness_workspace_bytes(B, W, p["hop"], p["S"]) + lib.vfx_true_peak_workspace_bytes(B, W, R, J)
    ws = torch.empty((nb // 8 + 1,), dtype=torch.float64, device="cuda")
    mp = torch.from_numpy(p["mpow"]).cuda()
    r4 = torch.empty((B, 4), dtype=torch.float64, device="cuda")
    args = [ops._ptr(xd), W, ops._ptr(n_rows), B, W, coef, ops._ptr(mp), p["S"], p["hop"], p["lookback"], float("nan"), -1.0,
            ops._ptr(bank), J, R, c, None, 0, ops._ptr(r4), ops._ptr(ws), nb, None]
    before = lib.vfx_launch_count()
    for i, bad in ((12, None), (13, 0), (14, 3), (14, 8), (20, nb - 1), (15, R * J), (10, -14.0)):
        a = list(args)
        a[i] = bad
        assert lib.vfx_loudness_tp_rows_f32(*a) == _lib.EINVAL, (i, bad)
    assert lib.vfx_launch_count() == before
    assert lib.vfx_loudness_tp_rows_f32(*args) == 0                    # ... and the same arguments, unbroken, run
    assert np.array_equal(r4.cpu().numpy(), res)


def test_30_minute_row_at_44k():
    fs = 44100
    n = 30 * 60 * fs
    rng = np.random.default_rng(30)
    x = rng.uniform(-0.5, 0.5, n).astype(np.float32)
    x[n - 3000:] *= 1.9                                                # the peak lies in the last tiles of ~77 K
    lib = _lib.lib()
    J = ops.true_peak_bank("cuda", 4)[1]
    assert 0 < lib.vfx_true_peak_workspace_bytes(1, n, 4, J) < n // 16  # no scratch proportional to R n
    res = ops.loudness_rows(torch.from_numpy(x).cuda()[None], torch.tensor([n], dtype=torch.int32, device="cuda"), fs,
                            true_peak=True).cpu().numpy()
    ref = ref_true_peak(x, fs)
    print("30 min row: P %.7f TP %.7f float64 %.7f err %.2e" % (res[0, 2], res[0, 3], ref, abs(res[0, 3] - ref) / max(1, ref)))
    assert res[0, 2] == np.abs(x).max() and _tp_ok(res[0, 3], ref)
    assert ref > 1.2 * res[0, 2] and res[0, 2] > 0.9                   # (0.5 before the last 3000 samples)


def test_ceiling_binds_between_the_samples():
    fs, T, Cdb = 44100, -3.0, -12.0
    x = _quarter_sine(5 * fs, 0.9)
    n_rows = torch.tensor([x.size], dtype=torch.int32, device="cuda")
    ceil = 10 ** (Cdb / 20)
    # the sample-peak ceiling leaves the continuous waveform above the ceiling: the gap is real
    out0 = torch.empty((1, x.size), device="cuda")
    r0 = ops.loudness_rows(torch.from_numpy(x).cuda()[None], n_rows, fs, target=T, ceiling_db=Cdb, out=out0).cpu().numpy()
    assert r0[0, 1] == pytest.approx(ceil / r0[0, 2], rel=1e-12) and r0[0, 1] < 10 ** ((T - r0[0, 0]) / 20)
    tp0 = ref_true_peak(out0[0].cpu().numpy(), fs)
    print("sample-peak ceiling %.1f dBFS: true peak of the output %.3f dBTP" % (Cdb, 20 * math.log10(tp0)))
    assert tp0 > ceil * 1.3
    # the true-peak ceiling holds between the samples
    out1 = torch.empty((1, x.size), device="cuda")
    r1 = ops.loudness_rows(torch.from_numpy(x).cuda()[None], n_rows, fs, target=T, ceiling_db=Cdb, out=out1,
                           true_peak=True).cpu().numpy()
    L, g, P, TP = r1[0]
    y = out1[0].cpu().numpy()
    tp1 = ref_true_peak(y, fs)
    print("true-peak ceiling %.1f dBTP: true peak of the output %.5f dBTP (TP before %.7f)" % (Cdb, 20 * math.log10(tp1), TP))
    assert g == pytest.approx(ceil / TP, rel=1e-12) and g < 10 ** ((T - L) / 20)
    assert tp1 <= ceil * (1 + TP_BOUND + 2.0 ** -23)                   # the kernel's bound + one fp32 rounding of the gain
    assert np.array_equal(y, np.float32(g) * x)
    assert ref_loudness(y, fs) < T                                     # a static gain: the ceiling costs loudness


def _expected(plain, target, ceiling=-1.0, fs=44100):
    L = voicefixer_amd.measure_loudness(plain, sample_rate=fs)
    tp = voicefixer_amd.measure_true_peak(plain, sample_rate=fs)
    g = 1.0 if not math.isfinite(L) else min(10.0 ** ((target - L) / 20.0), 10.0 ** (ceiling / 20.0) / 10.0 ** (tp / 20.0))
    return np.float32(g) * plain


@pytest.mark.parametrize("case", ["44k", "48k", "61s"])
def test_restore_inmem_true_peak(vf, case):
    rng = np.random.default_rng(61)
    n = 61 * 44100 if case == "61s" else 3 * 44100
    x = (0.02 * rng.standard_normal(n)).astype(np.float32)
    kw = {"output_sample_rate": 48000} if case == "48k" else {}
    fs = 48000 if case == "48k" else 44100
    lib = _lib.lib()
    plain = vf.restore_inmem(x, cuda=True, **kw)
    c0 = lib.vfx_launch_count()
    loud = vf.restore_inmem(x, cuda=True, loudness=-16, **kw)
    c1 = lib.vfx_launch_count()
    same = vf.restore_inmem(x, cuda=True, loudness=-16, true_peak=False, **kw)
    c2 = lib.vfx_launch_count()
    got = vf.restore_inmem(x, cuda=True, loudness=-16, true_peak=True, **kw)
    c3 = lib.vfx_launch_count()
    assert c2 - c1 == c1 - c0 and np.array_equal(same, loud)           # true_peak=False: today's path, launch for launch
    assert (c3 - c2) - (c1 - c0) == 1
    assert got.shape == plain.shape and np.array_equal(got[0], _expected(plain[0], -16.0, fs=fs))
    tp = ref_true_peak(got[0], fs)
    print("restore_inmem(%s, loudness=-16, true_peak=True): %.4f LUFS, %.4f dBTP (sample peak %.4f dBFS)"
          % (case, ref_loudness(got[0], fs), 20 * math.log10(tp), 20 * math.log10(np.abs(got).max())))
    assert tp <= 10 ** (-1 / 20) * (1 + TP_BOUND + 2.0 ** -23)
    # a ceiling low enough to bind: the gain is the true-peak one
    low = vf.restore_inmem(x, cuda=True, loudness=-3, peak_ceiling=-12, true_peak=True, **kw)
    assert np.array_equal(low[0], _expected(plain[0], -3.0, -12.0, fs=fs))
    tpl = ref_true_peak(low[0], fs)
    assert tpl <= 10 ** (-12 / 20) * (1 + TP_BOUND + 2.0 ** -23) and tpl >= 10 ** (-12 / 20) * (1 - 1e-5)


def test_restore_batch_true_peak(vf):
    rng = np.random.default_rng(23)
    lens = [30000, 52000, 41000, 44100 * 2, 36000]
    wavs = [(a * rng.standard_normal(n)).astype(np.float32) for a, n in zip((0.01, 0.3, 0.05, 0.1, 0.2), lens)]
    plain = vf.restore_batch(wavs, batch_size=8)
    outs = vf.restore_batch(wavs, batch_size=8, loudness=-10, peak_ceiling=-6, true_peak=True)
    for w, p, o in zip(wavs, plain, outs):
        assert np.array_equal(o[0], _expected(p[0], -10.0, -6.0))      # the row's own measurement, whatever its batch
        # ... and what restoring the file alone returns, as closely as the plain rows are (tests/test_api_gpu.py: a batch of
        # one picks other tile shapes, rms < 2e-5 at unit scale; here times the gain)
        one = vf.restore_inmem(w, cuda=True, loudness=-10, peak_ceiling=-6, true_peak=True)
        g = float(np.abs(o).max() / np.abs(p).max())
        rms = float(np.sqrt(np.mean((o.astype(np.float64) - one) ** 2)))
        assert o.shape == one.shape and rms < 2e-5 * max(1.0, g), (rms, g)
        assert ref_true_peak(o[0], 44100) <= 10 ** (-6 / 20) * (1 + TP_BOUND + 2.0 ** -23)
    recs = list(vf.restore_batches(iter([("t", "ragged", torch.from_numpy(np.stack([wavs[0][:30000], wavs[4][:30000]])),
                                          [30000, 30000])]), loudness=-10, peak_ceiling=-6, true_peak=True))
    assert len(recs) == 1 and tuple(recs[0][3].shape) == (2, 4)
    with pytest.raises(NotImplementedError):
        vf.restore_stream(wavs[3], true_peak=True)


def _level_folder(d, n_files=8):
    from scipy.io import wavfile
    os.makedirs(d)
    rng = np.random.default_rng(12)
    for k, db in enumerate(np.linspace(-40, -6, n_files)):
        n = int(44100 * (1.0 + 0.15 * k))
        t = np.arange(n) / 44100
        v = rng.standard_normal(n) * 0.3 + np.sin(2 * np.pi * 200 * t)
        v = v / np.abs(v).max() * 10 ** (db / 20)
        wavfile.write(os.path.join(d, "f%02d.wav" % k), 44100, np.round(v * 32767).astype(np.int16))


def _check_outputs(folder, names, ceiling_db):
    from scipy.io import wavfile
    worst = -math.inf
    for name in names:
        sr, pcm = wavfile.read(os.path.join(folder, name))
        assert sr == 44100 and pcm.dtype == np.int16
        tp = ref_true_peak(pcm.astype(np.float64) / 32768.0, sr)
        worst = max(worst, 20 * math.log10(tp))
        assert tp <= 10 ** (ceiling_db / 20), (name, tp)
    return worst


def test_folder_job_and_cli(vf, seeded_states, tmp_path, monkeypatch):
    ind = str(tmp_path / "in")
    _level_folder(ind)
    st = {}
    names = vf.restore_folder(ind, str(tmp_path / "tp"), batch_size=32, io_threads=2, stats=st, loudness=-23, true_peak=True)
    assert len(names) == 8 and st["failed"] == []
    assert [n for n, _, _ in st["true_peak"]] == [n for n, _, _ in st["loudness"]] == names
    for (_, before, after), (_, L0, gdb) in zip(st["true_peak"], st["loudness"]):
        assert abs(after - (before + gdb)) <= 1e-4 and after <= -1.0 + 1e-4
    print("folder: worst written true peak %.3f dBTP" % _check_outputs(str(tmp_path / "tp"), names, -1.0))
    st0 = {}
    vf.restore_folder(ind, str(tmp_path / "sp"), batch_size=32, io_threads=2, stats=st0, loudness=-23)
    assert "true_peak" not in st0
    from voicefixer_amd import __main__ as cli
    vsd, rsd = seeded_states
    home = str(tmp_path / "home")
    a = os.path.join(home, ".cache/voicefixer/analysis_module/checkpoints")
    v = os.path.join(home, ".cache/voicefixer/synthesis_module/44100")
    os.makedirs(a)
    os.makedirs(v)
    torch.save({"generator": vsd}, os.path.join(v, "model.ckpt-1490000_trimed.pt"))
    torch.save({"generator." + k: t for k, t in rsd.items()}, os.path.join(a, "vf.ckpt"))
    monkeypatch.setenv("HOME", home)
    out = str(tmp_path / "cli")
    assert cli.main(["-ifdr", ind, "-ofdr", out, "--loudness", "-23", "--true-peak", "--silent"]) == 0
    assert sorted(os.listdir(out)) == names
    _check_outputs(out, names, -1.0)
    for name in names:                                                 # the CLI writes what the API wrote
        assert open(os.path.join(out, name), "rb").read() == open(os.path.join(str(tmp_path / "tp"), name), "rb").read()
    one = str(tmp_path / "one.wav")
    assert cli.main(["-i", os.path.join(ind, "f07.wav"), "-o", one, "--loudness", "-23", "--true-peak", "--silent"]) == 0
    _check_outputs(str(tmp_path), ["one.wav"], -1.0)


def test_measure_true_peak_api():
    fs = 44100
    x = _quarter_sine(2 * fs, 0.5, fade=True)
    tp = voicefixer_amd.measure_true_peak(x, sample_rate=fs)
    assert isinstance(tp, float) and abs(tp - (-6.0206)) <= 0.01
    many = voicefixer_amd.measure_true_peak([x, np.zeros(100, np.float32), x[:fs], np.zeros(0, np.float32)], sample_rate=fs)
    assert many[0] == tp and many[1] == -math.inf and many[3] == -math.inf
    assert _tp_ok(10 ** (many[2] / 20), ref_true_peak(x[:fs], fs)) and many[2] > tp      # (cut off abruptly: it overshoots)
    assert voicefixer_amd.measure_true_peak([]) == []
    assert voicefixer_amd.measure_true_peak(x, sample_rate=192000) == pytest.approx(20 * math.log10(0.5 / math.sqrt(2)), abs=1e-5)


def _mod_hum(n, fs, seed):
    """Hum under noise whose level swings slowly by 14 dB: a loudness range to measure, far from both LRA gates."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / fs
    return (0.1 * rng.standard_normal(n) * (0.6 + 0.4 * np.sin(2 * np.pi * t / 37.0)) + 0.02 * np.sin(2 * np.pi * 50 * t)) \
        .astype(np.float32)


def _check_report(rep, x, fs, what):
    L, lra, mm, ms, margin = ref_report(x, fs)
    assert margin > 0.01, (what, margin)                    # no short-term value within 0.01 LU of either LRA gate
    print("report %s: I %.4f (%.4f) LRA %.4f (%.4f) M %.4f (%.4f) S %.4f (%.4f) TP %.4f dBTP; gate margin %.3f LU"
          % (what, rep["integrated"], L, rep["loudness_range"], lra, rep["max_momentary"], mm, rep["max_short_term"], ms,
             rep["true_peak"], margin))
    for key, want, tol in (("integrated", L, 0.005), ("max_momentary", mm, 0.005), ("max_short_term", ms, 0.005),
                           ("loudness_range", lra, 0.01)):
        if math.isinf(want):
            assert rep[key] == want, (what, key, rep[key])
        else:
            assert abs(rep[key] - want) <= tol, (what, key, rep[key], want)
    P = float(np.abs(x).max()) if x.size else 0.0
    assert rep["sample_peak"] == loudness.to_db(P)
    ref = ref_true_peak(x, fs)
    tp = 10 ** (rep["true_peak"] / 20) if ref > 0 else 0.0
    assert abs(tp - ref) <= TP_BOUND * max(1.0, ref) + 1e-12 and rep["true_peak"] >= rep["sample_peak"]


def test_report_on_the_tech_3342_signals():
    fs = 48000
    sigs = [sine_segments(fs, levels).astype(np.float32) for levels, _ in TECH_3342]
    reps = voicefixer_amd.loudness_report(sigs, sample_rate=fs)
    for rep, x, (levels, want) in zip(reps, sigs, TECH_3342):
        _check_report(rep, x, fs, "3342 %s" % (levels,))
        assert abs(rep["loudness_range"] - want) <= 1.0                # the recommendation's own tolerance
    assert voicefixer_amd.loudness_report(sigs[2], sample_rate=fs) == reps[2]     # alone: the bits it has in the list


def test_report_on_a_ragged_list(utterance):
    fs = 44100
    rows = [_mod_hum(int(0.3 * fs), fs, 1),                 # under 400 ms
            _mod_hum(int(1.7 * fs), fs, 2),                 # momentary blocks, no short-term block
            np.zeros(5 * fs, np.float32),                   # silence
            _mod_hum(75 * fs + 123, fs, 3),                 # a 75 s hum under modulated noise
            utterance.copy()]                               # a restored utterance (3 s: exactly one short-term block)
    lib = _lib.lib()
    c0 = lib.vfx_launch_count()
    reps = voicefixer_amd.loudness_report(rows, sample_rate=fs)
    assert lib.vfx_launch_count() - c0 == 5                            # chunk, filter, true peak, gate, report
    for r, (rep, x) in enumerate(zip(reps, rows)):
        _check_report(rep, x, fs, "row %d" % r)
    inf = -math.inf
    assert [reps[0][k] for k in ("integrated", "loudness_range", "max_momentary", "max_short_term")] == [inf, 0.0, inf, inf]
    assert math.isfinite(reps[1]["max_momentary"]) and reps[1]["max_short_term"] == inf and reps[1]["loudness_range"] == 0.0
    assert [reps[2][k] for k in ("integrated", "loudness_range", "max_momentary", "max_short_term", "sample_peak",
                                 "true_peak")] == [inf, 0.0, inf, inf, inf, inf]
    assert reps[3]["loudness_range"] > 3.0 and math.isfinite(reps[4]["max_short_term"]) and reps[4]["loudness_range"] == 0.0
    for r in (1, 3, 4):
        assert voicefixer_amd.loudness_report(rows[r], sample_rate=fs) == reps[r], r
    assert voicefixer_amd.loudness_report([]) == []
    assert reps[3]["integrated"] == voicefixer_amd.measure_loudness(rows[3], sample_rate=fs)
