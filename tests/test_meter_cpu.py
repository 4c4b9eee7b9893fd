"""The streaming loudness meter on the host (voicefixer_amd/loudness.py: meter_*): the specification against the EBU
test signals and against one filter over the whole row, the bookkeeping of the span form, and the argument rules of
``open_stream(meter=)`` and ``LoudnessMeter`` -- nothing here needs a device."""
import inspect
import math
import os
import re

import numpy as np
import pytest
from scipy.signal import lfilter

import voicefixer_amd
from voicefixer_amd import VoiceFixer, _lib, loudness, stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sine_segments(fs, levels_dbfs, seconds=20.0, f=1000.0):
    """The EBU Tech 3342 test signals: a 1 kHz sine, one segment of ``seconds`` per level (phase-continuous)."""
    n = int(round(seconds * fs))
    t = np.arange(n * len(levels_dbfs)) / fs
    a = np.repeat([10.0 ** (v / 20.0) for v in levels_dbfs], n)
    return a * np.sin(2 * np.pi * f * t)


TECH_3342 = [((-20.0, -30.0), 10.0), ((-20.0, -15.0), 5.0), ((-40.0, -20.0), 20.0),
             ((-50.0, -35.0, -20.0, -35.0, -50.0), 15.0)]


@pytest.mark.parametrize("levels,want", TECH_3342)
def test_loudness_range_of_the_tech_3342_signals(levels, want):
    """EBU Tech 3342: +-1 LU.  8 kHz keeps the host filter quick; 1 kHz lies where the K-weighting is flat at any rate."""
    fs = 8000
    x = sine_segments(fs, levels).astype(np.float32)
    r = loudness.meter_reference(x, fs)
    print("Tech 3342 %s at %d Hz: LRA %.4f LU (want %g)" % (levels, fs, r["loudness_range"], want))
    assert abs(r["loudness_range"] - want) <= 1.0
    assert list(r) == list(loudness.METER_KEYS) and r["seconds"] == x.size / fs
    # the live figures are those of the signal's end; the maxima those of its loudest level (a mono sine reads 3.01 below its peak)
    assert abs(r["momentary"] - (levels[-1] - 3.01)) <= 0.1 and abs(r["short_term"] - (levels[-1] - 3.01)) <= 0.1
    assert abs(r["max_momentary"] - (max(levels) - 3.01)) <= 0.1 and abs(r["max_short_term"] - (max(levels) - 3.01)) <= 0.1


@pytest.mark.parametrize("fs", [48000, 8000])
def test_integrated_loudness_of_the_tech_3341_sine(fs):
    """EBU Tech 3341 case 1: a stereo 1 kHz sine at -23 dBFS in both channels, 20 s, reads -23.0 +-0.1 LUFS (one channel of it
    reads 3.01 LU less: BS.1770's sum over the channels)."""
    x = sine_segments(fs, (-23.0,)).astype(np.float32)
    r = loudness.meter_reference(np.stack([x, x]), fs)
    print("Tech 3341 sine at %d Hz: %.4f LUFS, sample peak %.3f dBFS, true peak %.3f dBTP" % (fs, r["integrated"], r["sample_peak"],
                                                                                             r["true_peak"]))
    assert abs(r["integrated"] - (-23.0)) <= 0.1 and abs(r["momentary"] - (-23.0)) <= 0.1 and abs(r["short_term"] - (-23.0)) <= 0.1
    assert r["loudness_range"] <= 0.01
    assert r["sample_peak"] <= r["true_peak"] and abs(r["true_peak"] - (-23.0)) <= 0.2
    assert abs(loudness.meter_reference(x, fs)["integrated"] - (-23.0 - 3.0103)) <= 0.1


def _whole_row_quarters(x, fs):
    """The quarter sums of ONE filter over the whole row (float64, the fp32-rounded coefficients)."""
    c = loudness.coefficients(fs).astype(np.float32).astype(np.float64)
    y = lfilter(c[5:8], [1.0, c[8], c[9]], lfilter(c[0:3], [1.0, c[3], c[4]], np.asarray(x, np.float64)))
    hop = loudness.hop_length(fs)
    return np.array([float(np.dot(y[q * hop:(q + 1) * hop], y[q * hop:(q + 1) * hop])) for q in range(len(x) // hop)])


@pytest.mark.parametrize("fs", [8000, 44100, 192000])
def test_energies_against_the_whole_row_filter(fs):
    """The meter's quarters restart the filter two quarters back; the transition powers predict a relative difference < 1e-15 to
    one filter over the whole row, the bound leaves seven decades: only a wrong region fails it."""
    rng = np.random.default_rng(fs)
    n = int(1.2 * fs) + 17
    x = 0.1 * rng.standard_normal((2, n)) + 0.3
    x[:, : n // 3] *= 30.0
    w = [1.0, 1.41]
    E = loudness.meter_energies(x, fs, w)
    W = np.zeros(n // loudness.hop_length(fs))
    for c in range(2):
        W = W + w[c] * _whole_row_quarters(x[c], fs)
    rel = float(np.abs(E / W - 1.0).max())
    print("meter truncation at %d Hz: largest relative difference of E_q = %.2e" % (fs, rel))
    assert E.shape == W.shape and rel < 1e-9
    assert np.array_equal(loudness.meter_energies(x[0], fs), loudness.leveller_energies(x[0], fs))     # one channel: 0 + 1 E = E
    assert np.array_equal(E, loudness.leveller_energies_linked(x, fs, w))


def test_report_degenerate_logs():
    hop = 800
    inf = math.inf
    none = {"integrated": -inf, "loudness_range": 0.0, "max_momentary": -inf, "max_short_term": -inf, "momentary": -inf,
            "short_term": -inf}
    assert loudness.meter_report(np.zeros(0), hop) == none and loudness.meter_report(np.ones(3), hop) == none
    assert loudness.meter_report(np.zeros(40), hop) == none                      # silence: -inf everywhere
    r = loudness.meter_report(np.full(4, 0.01 * hop), hop)                      # one block of mean square 0.01: -20.691 LUFS
    assert abs(r["integrated"] - (-20.691)) < 1e-9 and r["momentary"] == r["max_momentary"] == r["integrated"]
    assert r["short_term"] == -inf and r["loudness_range"] == 0.0
    E = np.concatenate([np.full(40, 0.01 * hop), np.full(40, 0.0001 * hop)])    # 20 dB apart: both pass the -20 LU gate
    r = loudness.meter_report(E, hop)
    assert abs(r["loudness_range"] - 20.0) < 0.5 and abs(r["short_term"] - (-40.691)) < 1e-9 and abs(r["max_short_term"] - (-20.691)) < 1e-9
    x = np.zeros(100, np.float32)
    r = loudness.meter_reference(x, 8000)
    assert r["sample_peak"] == r["true_peak"] == -inf and r["seconds"] == 0.0125
    assert loudness.meter_reference(np.zeros((2, 0), np.float32), 8000)["seconds"] == 0.0


def test_mid_stream_true_peak_is_late_and_never_early():
    """final=False: the interpolated values of the samples below N - Fw only; a click in the last Fw samples counts for the sample
    peak at once and for the true peak's interpolated part later."""
    fs = 8000
    R, Bk, Fw = loudness.meter_reach(fs)
    assert (R, Bk, Fw) == (4, 94, 93) and loudness.meter_reach(96000) == (2, 94, 93) and loudness.meter_reach(192000) == (1, 0, 0)
    rng = np.random.default_rng(5)
    x = rng.uniform(-0.5, 0.5, 3000).astype(np.float32)
    x[2950:2954] = [0.9, -0.9, 0.9, -0.9]                     # overshoots between the samples
    part = loudness.meter_reference(x, fs, final=False)
    full = loudness.meter_reference(x, fs)
    assert part["sample_peak"] == full["sample_peak"] and full["true_peak"] > full["sample_peak"] + 0.5
    assert part["true_peak"] == part["sample_peak"]           # the overshoot is not known yet; the sample peak bounds from below
    later = np.concatenate([x, np.zeros(200, np.float32)])
    assert loudness.meter_reference(later, fs, final=False)["true_peak"] == loudness.meter_reference(later, fs)["true_peak"] == full["true_peak"]
    # what is known mid-stream never changes: the values below N - Fw have all their taps
    head = loudness.meter_reference(x[:2000], fs, final=False)["true_peak"]
    assert head <= loudness.meter_reference(x[:2500], fs, final=False)["true_peak"] <= full["true_peak"]
    quiet = x[:2000].copy()
    quiet[1950:] = 0.0                                        # the last 50 samples: beyond what final=False has folded
    assert loudness.meter_reference(quiet, fs, final=False)["true_peak"] <= head


@pytest.mark.parametrize("fs", [8000, 44100, 96000, 192000])
def test_bookkeeping_tiles_the_row_inside_the_kept_window(fs):
    """Random splits: the metered ranges tile [0, N), the logged quarters tile [0, N // hop), and nothing a call reads lies
    outside the window the keep rule left (the coverage vfx_meter_span_rows_f32 asks for)."""
    hop = loudness.hop_length(fs)
    R, Bk, Fw = loudness.meter_reach(fs)
    assert loudness.meter_counts(0, hop) == 0 and loudness.meter_counts(hop - 1, hop) == 0 and loudness.meter_counts(hop, hop) == 1
    assert loudness.meter_ready(50, Fw) == max(0, 50 - Fw) and loudness.meter_ready(1000, Fw) == 1000 - Fw
    assert loudness.meter_keep(0, hop, Bk) == 0 and loudness.meter_keep(5 * hop + 3, hop, Bk) == 3 * hop
    assert loudness.meter_keep(5 * hop, hop, Bk) == 3 * hop and loudness.meter_keep(hop + 7, hop, 0) == 0
    rng = np.random.default_rng(fs)
    for trial in range(20):
        N = int(rng.integers(1, 12 * hop))
        g0 = m = n = q = 0
        while True:
            end = n == N
            k = int(rng.choice([0, 1, Fw, hop - 1, hop, 3 * hop + 5, N])) if not end else 0
            n = min(N, n + k)
            m1 = N if end else max(m, loudness.meter_ready(n, Fw))
            if m1 > m:
                n_total = N if end else None
                lo = max(0, m - Bk)
                hi = min(N - 1, m1 - 1 + Fw) if end else m1 - 1 + Fw
                q1 = loudness.meter_counts(m1, hop)
                if q1 > q:
                    lo, hi = min(lo, max(0, q - 2) * hop), max(hi, q1 * hop - 1)
                assert g0 <= lo and hi < n, (trial, m, m1, g0, n, n_total)
                assert q == loudness.meter_counts(m, hop)
                m, q = m1, q1
            keep = min(loudness.meter_keep(m, hop, Bk), n - 1)
            g0 = max(g0, keep)
            if end:
                break
        assert m == N and q == N // hop


def _vf():
    return VoiceFixer.__new__(VoiceFixer)       # (no weights, no device: the checks come before either)


def test_arguments_are_checked_without_a_device():
    assert "LoudnessMeter" in voicefixer_amd.__all__ and loudness.METER_STATE == 16
    p = inspect.signature(voicefixer_amd.LoudnessMeter.__init__).parameters
    assert [(k, v.default) for k, v in p.items()][1:] == [("sample_rate", 44100), ("channels", None), ("channel_weights", None)]
    assert inspect.signature(VoiceFixer.open_stream).parameters["meter"].default is False
    assert inspect.signature(stream.RestoreSession.__init__).parameters["meter"].default is False
    for bad in (1, 0, None, "yes", 1.0):
        with pytest.raises(ValueError, match="meter must be True or False"):
            VoiceFixer.open_stream(_vf(), meter=bad)
    with pytest.raises(ValueError, match="192000"):
        VoiceFixer.open_stream(_vf(), meter=True, output_sample_rate=441000)
    VoiceFixer.open_stream(_vf(), meter=False, output_sample_rate=441000)       # (the rate binds the meter only)
    s = VoiceFixer.open_stream(_vf(), meter=True, output_sample_rate=48000, channels="all", channel_weights=[1.0, 0.5])
    assert s._meter.rate == 48000 and s._meter.weights == [1.0, 0.5] and (s._meter.R, s._meter.Bk, s._meter.Fw) == (4, 94, 93)
    assert VoiceFixer.open_stream(_vf()).loudness_report is None
    r = s.loudness_report                                                        # nothing pushed: nothing touches the device
    assert list(r) == list(loudness.METER_KEYS) and r["integrated"] == -math.inf and r["loudness_range"] == 0.0 and r["seconds"] == 0.0
    for kw in (dict(sample_rate=192001), dict(sample_rate=3999), dict(sample_rate=True), dict(sample_rate=44100.5),
               dict(channels="stereo"), dict(channels=2), dict(channel_weights=[1.0, 1.0]),
               dict(channels="mix", channel_weights=[1.0, 1.0]), dict(channels="all", channel_weights=[1.0, -1.0]),
               dict(channels="all", channel_weights="11"), dict(channels="all", channel_weights=[1.0] * 9)):
        with pytest.raises(ValueError):
            voicefixer_amd.LoudnessMeter(**kw)
    m = voicefixer_amd.LoudnessMeter(48000, channels="all", channel_weights=[1.0, 1.0])
    for bad in (np.zeros(5, np.float32), np.zeros((9, 5), np.float32), np.zeros((3, 5), np.float32)):
        with pytest.raises(ValueError):                                          # 1-D, too many channels, not the weights' count
            m.push(bad)
    with pytest.raises(ValueError):
        voicefixer_amd.LoudnessMeter().push(np.zeros((2, 5), np.float32))        # a 2-D block without channels=
    with voicefixer_amd.LoudnessMeter(8000) as m:
        m.push(np.zeros(0, np.float32))                                          # (an empty block: nothing happens)
        assert m.report()["seconds"] == 0.0
    with pytest.raises(RuntimeError):
        m.push(np.zeros(4, np.float32))
    with pytest.raises(RuntimeError):
        m.finish()
    assert m.report()["seconds"] == 0.0                                          # still readable


def test_entry_points_declared_mapped_and_bound():
    header = open(os.path.join(ROOT, "include", "vfx_hip.h")).read()
    assert "#define VFX_METER_STATE 16" in header
    for name, nargs in (("vfx_meter_span_workspace_bytes", 3), ("vfx_meter_span_rows_f32", 23),
                        ("vfx_meter_report_workspace_bytes", 1), ("vfx_meter_report_f32", 7)):
        m = re.search(r"\b(?:int|size_t) %s\(([^;]*)\);" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
    mk = open(os.path.join(ROOT, "voicefixer_amd", "csrc", "Makefile")).read()
    src = open(os.path.join(ROOT, "voicefixer_amd", "csrc", "vfx_loudness.hip")).read()
    assert "vfx_meter_span.inc" in mk and src.index('#include "vfx_level_span.inc"') < src.index('#include "vfx_meter_span.inc"')
    from voicefixer_amd import ops
    assert list(inspect.signature(ops.meter_span_rows).parameters)[:8] == ["xw", "g0", "n_total", "rate", "m0", "m1", "state", "qlog"]
    assert callable(ops.meter_state) and callable(ops.meter_report)
