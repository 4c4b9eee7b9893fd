"""Loudness normalisation without a GPU: the K-weighting design against the BS.1770-4 tables, an independent float64
reference of the integrated-loudness definition (used by tests/test_loudness_gpu.py as its yardstick), parameter checks,
the CLI flags and the C-ABI binding of vfx_loudness_rows_f32."""
import math
import os
import re

import numpy as np
import pytest
from scipy.signal import lfilter

from voicefixer_amd import _lib, api, loudness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def k_weighting_f64(fs):
    """The K-weighting written out from the analog parameters (independent of voicefixer_amd.loudness)."""
    K = math.tan(math.pi * 1681.974450955533 / fs)
    Vh = 10.0 ** (3.999843853973347 / 20.0)
    Vb = Vh ** 0.4996667741545416
    Q = 0.7071752369554196
    a0 = 1.0 + K / Q + K * K
    sb = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0]
    sa = [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    K = math.tan(math.pi * 38.13547087602444 / fs)
    Q = 0.5003270373238773
    d = 1.0 + K / Q + K * K
    return sb, sa, [1.0, -2.0, 1.0], [1.0, 2.0 * (K * K - 1.0) / d, (1.0 - K / Q + K * K) / d]


def ref_loudness(x, fs):
    """Integrated loudness (LUFS) of one channel in float64: K-weighting, 100 ms quarters, 400 ms blocks, -70 LUFS and
    -10 LU gates; -inf when no block passes."""
    sb, sa, hb, ha = k_weighting_f64(fs)
    y = lfilter(hb, ha, lfilter(sb, sa, np.asarray(x, np.float64)))
    hop = (fs + 5) // 10
    nq = len(y) // hop
    if nq < 4:
        return -math.inf
    q = np.sum((y[:nq * hop] ** 2).reshape(nq, hop), axis=1)
    z = (q[:-3] + q[1:-2] + q[2:-1] + q[3:]) / (4.0 * hop)
    with np.errstate(divide="ignore"):
        lj = -0.691 + 10.0 * np.log10(z)
    keep = lj > -70.0
    if not keep.any():
        return -math.inf
    gr = -0.691 + 10.0 * math.log10(np.mean(z[keep])) - 10.0
    keep &= lj > gr
    if not keep.any():
        return -math.inf
    return -0.691 + 10.0 * math.log10(np.mean(z[keep]))


def sine(fs, seconds, dbfs, f=997.0):
    t = np.arange(int(round(seconds * fs))) / fs
    return 10.0 ** (dbfs / 20.0) * np.sin(2 * np.pi * f * t)


def test_design_matches_the_bs1770_tables_at_48k():
    sb, sa, hb, ha = loudness.k_weighting(48000)
    np.testing.assert_allclose(sb, [1.53512485958697, -2.69169618940638, 1.19839281085285], rtol=0, atol=1e-10)
    np.testing.assert_allclose(sa, [1.0, -1.69065929318241, 0.73248077421585], rtol=0, atol=1e-10)
    np.testing.assert_array_equal(hb, [1.0, -2.0, 1.0])
    np.testing.assert_allclose(ha, [1.0, -1.99004745483398, 0.99007225036621], rtol=0, atol=1e-10)


@pytest.mark.parametrize("fs", [8000, 11025, 16000, 22050, 44100, 48000])
def test_design_equals_the_written_out_formulas(fs):
    for a, b in zip(loudness.k_weighting(fs), k_weighting_f64(fs)):
        np.testing.assert_allclose(a, b, rtol=1e-14, atol=0)
    assert loudness.hop_length(fs) == (fs + 5) // 10
    S = loudness.chunk_length(fs)
    assert S % 32 == 0 and 32 <= S <= loudness.hop_length(fs)


def test_plan_state_transition():
    """M^(2^i) are the powers of the one-chunk transition: filtering S samples of zeros from a state equals M times it."""
    fs = 44100
    p = loudness.plan(fs)
    c = p["coef"].astype(np.float32).astype(np.float64)
    s0 = np.array([0.3, -0.2, 0.5, 0.1])
    s = s0.copy()
    for _ in range(p["S"]):
        ys = s[0]
        t0, t1 = -c[3] * ys + s[1], -c[4] * ys
        yh = c[5] * ys + s[2]
        s = np.array([t0, t1, c[6] * ys - c[8] * yh + s[3], c[7] * ys - c[9] * yh])
    np.testing.assert_allclose(p["mpow"][0] @ s0, s, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(p["mpow"][3], np.linalg.matrix_power(p["mpow"][0], 8), rtol=1e-9, atol=1e-30)
    assert p["mpow"].shape == (16, 4, 4) and 1 <= p["lookback"] < 256


@pytest.mark.parametrize("fs,want", [(48000, -23.0103), (44100, -23.0075)])
def test_reference_sine_reads_minus_23(fs, want):
    L = ref_loudness(sine(fs, 20.0, -20.0), fs)
    assert abs(L - (-23.01)) <= 0.01 and abs(L - want) <= 5e-4, L


def test_reference_silence_and_short_inputs_are_minus_inf():
    assert ref_loudness(np.zeros(44100 * 3), 44100) == -math.inf
    assert ref_loudness(sine(44100, 0.399, -20.0), 44100) == -math.inf
    assert math.isfinite(ref_loudness(sine(44100, 0.4, -20.0), 44100))


def test_reference_relative_gate_drops_the_quiet_half():
    fs = 48000
    loud = sine(fs, 20.0, -20.0)
    both = np.concatenate([loud, sine(fs, 20.0, -50.0)])
    d = ref_loudness(both, fs) - ref_loudness(loud, fs)
    assert abs(d) <= 0.05 and abs(d - (-0.033)) <= 0.005, d


@pytest.mark.parametrize("bad", [0.0, 3, -70.5, -100, float("nan"), float("inf"), True, "-16", [-16]])
def test_bad_targets_raise(bad):
    with pytest.raises(ValueError):
        loudness.check_target(bad)
    with pytest.raises(ValueError):
        api.apply_loudness(None, [1], 44100, bad)


@pytest.mark.parametrize("bad", [1, 0.5, -20.5, float("nan"), -float("inf"), False, None])
def test_bad_ceilings_raise(bad):
    with pytest.raises(ValueError):
        loudness.check_ceiling(bad)


def test_good_parameters_pass_and_bad_ones_raise_before_any_device_work():
    assert loudness.check_target(-70) == -70.0 and loudness.check_target(-0.5) == -0.5 and loudness.check_target(None) is None
    assert loudness.check_ceiling(0) == 0.0 and loudness.check_ceiling(-20) == -20.0
    vf = api.VoiceFixer.__new__(api.VoiceFixer)     # (no device, no weights: the checks come first)
    with pytest.raises(ValueError):
        api.VoiceFixer.restore_inmem(vf, np.zeros(44100, np.float32), loudness=5)
    with pytest.raises(ValueError):
        api.VoiceFixer.restore_inmem(vf, np.zeros(44100, np.float32), loudness=-16, peak_ceiling=2)
    with pytest.raises(ValueError):
        loudness.plan(1000)


def test_cli_flags():
    from voicefixer_amd.__main__ import build_parser
    a = build_parser().parse_args(["-i", "x.wav", "--loudness", "-16", "--peak-ceiling", "-1"])
    assert a.loudness == -16.0 and a.peak_ceiling == -1.0
    d = build_parser().parse_args(["-i", "x.wav"])
    assert d.loudness is None and d.peak_ceiling == -1.0
    for bad in (["--loudness", "3"], ["--peak-ceiling", "1"], ["--loudness", "nan"], ["--loudness", "x"]):
        with pytest.raises(SystemExit):
            build_parser().parse_args(["-i", "x.wav"] + bad)


def test_entry_point_declared_mapped_and_bound():
    import ctypes as C
    hdr = open(os.path.join(ROOT, "include", "vfx_hip.h")).read()
    for name in ("vfx_loudness_rows_f32", "vfx_loudness_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    res, args = _lib.SIGNATURES["vfx_loudness_rows_f32"]
    assert res is C.c_int and len(args) == 18
    assert args[10] is C.c_double and args[11] is C.c_double and args[16] is C.c_size_t
    assert _lib.SIGNATURES["vfx_loudness_workspace_bytes"] == (C.c_size_t, [C.c_int, C.c_int64, C.c_int, C.c_int])
    mk = open(os.path.join(ROOT, "voicefixer_amd", "csrc", "Makefile")).read()
    assert "vfx_loudness.hip" in mk and mk.count("vfx_loudness.o") >= 5
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    h = _lib.lib()
    assert hasattr(h, "vfx_loudness_rows_f32")
    assert h.vfx_loudness_workspace_bytes(32, 441000, 4410, 224) > 32 * 441000 // 224 * 32
    assert h.vfx_loudness_workspace_bytes(0, 10, 4410, 224) == 0
    # bad arguments are refused on the host, before any device work
    assert h.vfx_loudness_rows_f32(None, 0, None, 1, 10, None, None, 224, 4410, 1, float("nan"), -1.0, None, 0, None,
                                   None, 0, None) == _lib.EINVAL
