"""True peak and loudness report without a GPU: independent float64 references of both definitions (used by
tests/test_true_peak_gpu.py as its yardsticks) checked against analytic sines and the EBU Tech 3342 signals, the identity of
the written-out interpolator with the project's one filter design, parameter checks, the CLI flag and the C-ABI bindings."""
import math
import os
import re

import numpy as np
import pytest
from scipy.signal import firwin, lfilter, upfirdn

from voicefixer_amd import _lib, api, audio_io, loudness
from test_loudness_cpu import k_weighting_f64, ref_loudness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ref_oversampling(fs):
    return 4 if fs < 96000 else (2 if fs < 192000 else 1)


def ref_interpolator(R):
    """The R-times interpolator written out (independent of voicefixer_amd.audio_io): a Kaiser-windowed sinc, 125 dB, pass
    band edge 0.913 / R and stop band edge 1 / R of the oversampled Nyquist frequency, odd length, gain R, float32 taps."""
    width = (1.0 - 0.913) / R
    taps = int(math.ceil((125.0 - 7.95) / (2.285 * math.pi * width))) | 1
    h = firwin(taps, 0.5 * (0.913 + 1.0) / R, window=("kaiser", 0.1102 * (125.0 - 8.7)))
    return np.ascontiguousarray(h * R, dtype=np.float32)


def ref_true_peak(x, fs, block=1 << 20):
    """TP = max(P, max |y[m]|), m in [0, R n): y the zero-phase R-times interpolation of x (zero outside the row), in
    float64 with the float32 taps; computed block by block (a FIR: every block with its own halo gives the same values)."""
    x = np.asarray(x, np.float64)
    n, R = x.size, ref_oversampling(fs)
    P = float(np.abs(x).max()) if n else 0.0
    if R == 1 or n == 0:
        return P
    g = ref_interpolator(R).astype(np.float64)
    c, H = (g.size - 1) // 2, -(-g.size // R) + 1
    tp = P
    for a in range(0, n, block):
        b = min(a + block, n)
        lo, hi = max(a - H, 0), min(b + H, n)
        y = upfirdn(g, x[lo:hi], up=R)
        t = c + R * a - R * lo                              # full-convolution index of output m = R a
        tp = max(tp, float(np.abs(y[t:t + R * (b - a)]).max()))
    return tp


def ref_report(x, fs):
    """(integrated, LRA, max momentary, max short-term, margin) in float64: the quarters of ref_loudness, 400 ms blocks
    ungated for the momentary maximum, short-term blocks of 30 quarters at every quarter, LRA after EBU Tech 3342.
    ``margin``: the smallest distance (LU) of a short-term value from either LRA gate (inf without a block)."""
    sb, sa, hb, ha = k_weighting_f64(fs)
    y = lfilter(hb, ha, lfilter(sb, sa, np.asarray(x, np.float64)))
    hop = (fs + 5) // 10
    nq = len(y) // hop
    q = np.sum((y[:nq * hop] ** 2).reshape(nq, hop), axis=1) if nq else np.zeros(0)
    with np.errstate(divide="ignore"):
        mm = -math.inf
        if nq >= 4:
            z = (q[:-3] + q[1:-2] + q[2:-1] + q[3:]) / (4.0 * hop)
            mm = float(np.max(-0.691 + 10.0 * np.log10(z)))
        ms, lra, margin = -math.inf, 0.0, math.inf
        if nq >= 30:
            cs = np.concatenate([[0.0], np.cumsum(q)])
            e = np.array([np.sum(q[j:j + 30]) for j in range(nq - 29)]) / (30.0 * hop)
            assert np.allclose(e * 30.0 * hop, cs[30:] - cs[:-30], rtol=1e-9, atol=1e-300)
            l = -0.691 + 10.0 * np.log10(e)
            ms = float(l.max())
            margin = float(np.abs(l + 70.0).min())
            keep = l > -70.0
            if keep.any():
                gr = -0.691 + 10.0 * math.log10(np.mean(e[keep])) - 20.0
                margin = min(margin, float(np.abs(l[keep] - gr).min()))
                s = np.sort(l[keep & (l > gr)])
                if s.size:
                    lra = float(s[((s.size - 1) * 95 + 50) // 100] - s[((s.size - 1) + 5) // 10])
    return ref_loudness(x, fs), lra, mm, ms, margin


def sine_segments(fs, levels_dbfs, seconds=20.0, f=1000.0):
    """The EBU Tech 3342 test signals: a 1 kHz sine, one segment of ``seconds`` per level (phase-continuous)."""
    n = int(round(seconds * fs))
    t = np.arange(n * len(levels_dbfs)) / fs
    a = np.repeat([10.0 ** (v / 20.0) for v in levels_dbfs], n)
    return a * np.sin(2 * np.pi * f * t)


TECH_3342 = [((-20.0, -30.0), 10.0), ((-20.0, -15.0), 5.0), ((-40.0, -20.0), 20.0),
             ((-50.0, -35.0, -20.0, -35.0, -50.0), 15.0)]


def faded_sine(fs, div, phase_deg, amp, seconds=0.5):
    n = int(seconds * fs)
    x = amp * np.sin(2 * np.pi * np.arange(n) / div + math.radians(phase_deg))
    w = np.ones(n)
    k = n // 8
    ramp = 0.5 - 0.5 * np.cos(np.pi * np.arange(k) / k)
    w[:k], w[n - k:] = ramp, ramp[::-1]
    return x * w


@pytest.mark.parametrize("R", [2, 4])
def test_written_out_interpolator_is_the_projects_filter(R):
    g = audio_io.hq_filter(R, 1)[1]
    assert g.dtype == np.float32 and np.array_equal(g, ref_interpolator(R))
    bank, J, c = audio_io.hq_bank(R, 1)
    assert bank.shape == (R, J) and c == (g.size - 1) // 2
    if R == 4:
        assert g.size == 751 and J == 188
    assert [loudness.oversampling(fs) for fs in (8000, 44100, 95999, 96000, 191999, 192000, 384000)] == \
        [ref_oversampling(fs) for fs in (8000, 44100, 95999, 96000, 191999, 192000, 384000)] == [4, 4, 4, 2, 2, 1, 1]


@pytest.mark.parametrize("fs", [8000, 16000, 44100, 48000])
@pytest.mark.parametrize("div,phase", [(4, 45.0), (6, 60.0), (8, 67.5)])
def test_reference_reads_the_amplitude_of_sines_between_the_samples(fs, div, phase):
    """EBU Tech 3341's true-peak tolerance: +0.2 / -0.4 dB.  The sample peaks are 3.01, 1.25 and 0.69 dB low."""
    amp = 10.0 ** (-6.0 / 20.0)
    x = faded_sine(fs, div, phase, amp)
    tp = 20.0 * math.log10(ref_true_peak(x, fs))
    sp = 20.0 * math.log10(np.abs(x).max())
    print("fs %d, fs/%d at %.1f deg: sample peak %.4f dBFS, true peak %.4f dBTP" % (fs, div, phase, sp, tp))
    assert -0.4 <= tp - (-6.0) <= 0.2
    assert sp < -6.0 - 0.6 and tp >= sp


def test_reference_blocks_and_edges():
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, 5000)
    whole = ref_true_peak(x, 44100)
    assert whole == ref_true_peak(x, 44100, block=777) and whole > 1.0
    g = ref_interpolator(4).astype(np.float64)
    y = upfirdn(g, x, up=4)[375:375 + 4 * x.size]
    assert whole == max(np.abs(x).max(), np.abs(y).max())
    s = np.sin(2 * np.pi * 0.11 * np.arange(5000))           # (in the pass band; the noise above is not)
    ys = upfirdn(g, s, up=4)[375:375 + 4 * s.size]
    assert np.abs(ys[::4] - s)[200:-200].max() < 1e-5        # zero phase: every fourth output is the input
    assert ref_true_peak(np.zeros(0), 44100) == 0.0 and ref_true_peak(np.zeros(9), 44100) == 0.0
    assert ref_true_peak(x, 192000) == np.abs(x).max()       # R = 1
    assert ref_true_peak(np.array([0.5]), 44100) == pytest.approx(0.5, abs=1e-6)


@pytest.mark.parametrize("fs", [16000, 44100, 48000])
@pytest.mark.parametrize("levels,want", TECH_3342)
def test_reference_lra_on_the_tech_3342_signals(fs, levels, want):
    L, lra, mm, ms, margin = ref_report(sine_segments(fs, levels), fs)
    print("fs %d %s: LRA %.7f LU (want %g), margin %.3f LU" % (fs, levels, lra, want, margin))
    assert abs(lra - want) <= 1.0 and margin > 0.01
    top = max(levels)
    assert abs(mm - (top - 3.01)) <= 0.1 and abs(ms - (top - 3.01)) <= 0.1 and ms <= mm + 1e-9


def test_reference_degenerate_rows():
    fs = 44100
    t = np.arange(10 * fs) / fs
    x = 0.1 * np.sin(2 * np.pi * 997 * t)
    assert ref_report(x[: int(0.39 * fs)], fs)[:4] == (-math.inf, 0.0, -math.inf, -math.inf)
    L, lra, mm, ms, _ = ref_report(x[: 2 * fs], fs)
    assert math.isfinite(L) and math.isfinite(mm) and lra == 0.0 and ms == -math.inf
    assert ref_report(np.zeros(5 * fs), fs)[:4] == (-math.inf, 0.0, -math.inf, -math.inf)
    L, lra, mm, ms, _ = ref_report(x, fs)
    assert abs(lra) < 1e-6 and abs(ms - L) < 1e-3


@pytest.mark.parametrize("bad", [None, 1, 0, "yes", 1.0, [True]])
def test_bad_true_peak_flags_raise_before_any_device_work(bad):
    with pytest.raises(ValueError):
        loudness.check_true_peak(bad)
    with pytest.raises(ValueError):
        api.apply_loudness(None, [1], 44100, -16.0, -1.0, bad)
    vf = api.VoiceFixer.__new__(api.VoiceFixer)     # (no device, no weights: the checks come first)
    x = np.zeros(44100, np.float32)
    for call in (lambda: api.VoiceFixer.restore_inmem(vf, x, loudness=-16, true_peak=bad),
                 lambda: api.VoiceFixer.restore_batch(vf, [x], loudness=-16, true_peak=bad),
                 lambda: next(api.VoiceFixer.restore_batches(vf, iter([]), loudness=-16, true_peak=bad)),
                 lambda: api.VoiceFixer.restore_folder(vf, "/nonexistent", "/nonexistent", loudness=-16, true_peak=bad),
                 lambda: api.VoiceFixer.restore(vf, "a.wav", "b.wav", loudness=-16, true_peak=bad),
                 lambda: api.VoiceFixer.restore_stream(vf, x, true_peak=bad)):
        with pytest.raises(ValueError):
            call()


def test_parameters_and_surface():
    assert loudness.check_true_peak(True) is True and loudness.check_true_peak(np.bool_(False)) is False
    assert loudness.to_db(0.0) == -math.inf and loudness.to_db(0.5) == pytest.approx(-6.0206, abs=1e-4)
    vf = api.VoiceFixer.__new__(api.VoiceFixer)
    x = np.zeros(44100, np.float32)
    with pytest.raises(NotImplementedError):        # the stream refuses loudness, so it refuses its true-peak ceiling
        api.VoiceFixer.restore_stream(vf, x, true_peak=True)
    with pytest.raises(NotImplementedError):
        api.VoiceFixer.restore_stream(vf, x, loudness=-16, true_peak=True)
    with pytest.raises(ValueError):                 # the ceiling keeps its range when it is read as dBTP
        api.VoiceFixer.restore_inmem(vf, x, loudness=-16, peak_ceiling=0.5, true_peak=True)
    with pytest.raises(ValueError):
        api.measure_true_peak(x, sample_rate=1000)
    with pytest.raises(ValueError):
        api.loudness_report(x, sample_rate=1000)
    import inspect
    import voicefixer_amd
    assert voicefixer_amd.measure_true_peak is api.measure_true_peak and voicefixer_amd.loudness_report is api.loudness_report
    for fn in (api.apply_loudness, api.VoiceFixer.restore, api.VoiceFixer.restore_inmem, api.VoiceFixer.restore_batch,
               api.VoiceFixer.restore_batches, api.VoiceFixer.restore_folder, api.VoiceFixer.restore_stream):
        sig = inspect.signature(fn).parameters
        assert "peak_ceiling" in sig and sig["true_peak"].default is False, fn


def test_cli_flag():
    from voicefixer_amd.__main__ import build_parser
    a = build_parser().parse_args(["-i", "x.wav", "--loudness", "-23", "--true-peak"])
    assert a.true_peak is True and a.loudness == -23.0 and a.peak_ceiling == -1.0
    assert build_parser().parse_args(["-i", "x.wav", "--loudness", "-23"]).true_peak is False
    assert build_parser().parse_args(["-i", "x.wav"]).true_peak is False
    for bad in (["--true-peak"], ["--true-peak", "--peak-ceiling", "-2"], ["--loudness", "-23", "--true-peak", "yes"]):
        with pytest.raises(SystemExit):
            build_parser().parse_args(["-i", "x.wav"] + bad)


def test_entry_points_declared_mapped_and_bound():
    import ctypes as C
    hdr = open(os.path.join(ROOT, "include", "vfx_hip.h")).read()
    names = ("vfx_true_peak_workspace_bytes", "vfx_loudness_tp_rows_f32", "vfx_loudness_report_workspace_bytes",
             "vfx_loudness_report_rows_f32")
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES, name
    res, args = _lib.SIGNATURES["vfx_loudness_tp_rows_f32"]
    assert res is C.c_int and len(args) == 22 and args[10] is C.c_double and args[11] is C.c_double and args[20] is C.c_size_t
    res, args = _lib.SIGNATURES["vfx_loudness_report_rows_f32"]
    assert res is C.c_int and len(args) == 18 and args[16] is C.c_size_t
    assert _lib.SIGNATURES["vfx_true_peak_workspace_bytes"] == (C.c_size_t, [C.c_int, C.c_int64, C.c_int, C.c_int])
    # the new kernels live in vfx_loudness.hip, every kernel of which check_no_pk_fma covers (the "." pattern)
    mk = open(os.path.join(ROOT, "voicefixer_amd", "csrc", "Makefile")).read()
    src = open(os.path.join(ROOT, "voicefixer_amd", "csrc", "vfx_loudness.hip")).read()
    assert "lk_truepeak_kernel" in src and "lk_report_kernel" in src
    assert '"vfx_loudness:."' in mk and re.search(r"^check_no_pk_fma:.*vfx_loudness\.o", mk, re.M) and "-fno-slp-vectorize" in mk
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    h = _lib.lib()
    for name in names:
        assert hasattr(h, name), name
    # no scratch proportional to the oversampled row: a 30-minute row at 44.1 kHz
    n = 30 * 60 * 44100
    assert 0 < h.vfx_true_peak_workspace_bytes(1, n, 4, 188) < n // 16
    assert 0 < h.vfx_true_peak_workspace_bytes(32, 441000, 4, 188) < 32 * 441000 // 16
    for bad in ((0, 10, 4, 188), (1, -1, 4, 188), (1, 10, 3, 188), (1, 10, 4, 0), (1, 10, 8, 188)):
        assert h.vfx_true_peak_workspace_bytes(*bad) == 0, bad
    assert h.vfx_loudness_report_workspace_bytes(1, n, 4410, 224, 4, 188) > h.vfx_loudness_workspace_bytes(1, n, 4410, 224)
    assert h.vfx_loudness_report_workspace_bytes(1, n, 4410, 224, 3, 188) == 0
    # bad arguments are refused on the host, before any device work (the pointers below are never followed: host memory)
    p = loudness.plan(44100)
    coef = (C.c_double * 10)(*p["coef"])
    buf = (C.c_double * 64)()
    ptr = C.cast(buf, C.c_void_p)
    big = 1 << 40
    good = [ptr, 64, ptr, 1, 64, coef, ptr, p["S"], p["hop"], p["lookback"], float("nan"), -1.0, ptr, 188, 4, 375, None, 0,
            ptr, ptr, big, None]
    for i, bad in ((12, None), (13, 0), (13, 4096), (14, 3), (14, 0), (15, -1), (15, 4 * 188), (20, 1024), (0, None),
                   (18, None), (7, 48)):
        a = list(good)
        a[i] = bad
        assert h.vfx_loudness_tp_rows_f32(*a) == _lib.EINVAL, (i, bad)
    rgood = good[:10] + [ptr, 188, 4, 375, ptr, ptr, big, None]
    for i, bad in ((10, None), (11, 0), (12, 3), (13, -1), (16, 1024), (14, None)):
        a = list(rgood)
        a[i] = bad
        assert h.vfx_loudness_report_rows_f32(*a) == _lib.EINVAL, (i, bad)
