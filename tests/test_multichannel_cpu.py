"""Multichannel restoration and linked BS.1770 loudness, the parts that need no device: the float64 reference
of a programme's loudness and report, its known values, the channel-weight table, the ``channels=`` argument on every entry
point, planning by file, the 1..8-channel WAV / FLAC round trip and the input condition of tests/test_multichannel_gpu.py."""
import math
import os
import re

import numpy as np
import pytest
from scipy.signal import lfilter

from voicefixer_amd import _lib, api, audio_io, loudness
from voicefixer_amd.loudness import channel_weights
from test_loudness_cpu import k_weighting_f64, ref_loudness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _quarters(x, fs):
    """Quarter sums q[c, i] of the K-weighted channels of x (C, N), float64, and hop."""
    sb, sa, hb, ha = k_weighting_f64(fs)
    x = np.atleast_2d(np.asarray(x, np.float64))
    y = lfilter(hb, ha, lfilter(sb, sa, x, axis=-1), axis=-1)
    hop = (fs + 5) // 10
    nq = y.shape[1] // hop
    return np.sum((y[:, :nq * hop] ** 2).reshape(y.shape[0], nq, hop), axis=2), hop


def _blocks(x, fs, weights):
    """Programme quarter sums Q_i = sum_c G_c q_{c,i} and block energies z_j."""
    q, hop = _quarters(x, fs)
    Q = np.zeros(q.shape[1])
    for c in range(q.shape[0]):                          # ascending c, as the definition says
        Q = Q + float(weights[c]) * q[c]
    z = (Q[:-3] + Q[1:-2] + Q[2:-1] + Q[3:]) / (4.0 * hop) if Q.size >= 4 else np.zeros(0)
    return Q, z, hop


def ref_loudness_multi(x, fs, weights, with_margin=False):
    """Integrated loudness (LUFS) of the programme x (C, N) with channel weights G_c in float64 (BS.1770-4: the weighted block
    energies are summed over the channels BEFORE the gates); -inf when no block passes.  ``with_margin``: (L, the smallest
    distance in LU of a block's loudness from the absolute gate or, among the blocks above it, from the relative gate)."""
    _, z, _ = _blocks(x, fs, weights)
    L, margin = -math.inf, math.inf
    if z.size:
        with np.errstate(divide="ignore"):
            lj = -0.691 + 10.0 * np.log10(z)
        margin = float(np.abs(lj + 70.0).min())
        keep = lj > -70.0
        if keep.any():
            gr = -0.691 + 10.0 * math.log10(np.mean(z[keep])) - 10.0
            margin = min(margin, float(np.abs(lj[keep] - gr).min()))
            keep &= lj > gr
            if keep.any():
                L = -0.691 + 10.0 * math.log10(np.mean(z[keep]))
    return (L, margin) if with_margin else L


def ref_report_multi(x, fs, weights):
    """(integrated, LRA, max momentary, max short-term, LRA gate margin): the recipe of test_true_peak_cpu.ref_report on the
    programme quarter sums Q and block energies z."""
    Q, z, hop = _blocks(x, fs, weights)
    with np.errstate(divide="ignore"):
        mm = float(np.max(-0.691 + 10.0 * np.log10(z))) if z.size else -math.inf
        ms, lra, margin = -math.inf, 0.0, math.inf
        if Q.size >= 30:
            e = np.array([np.sum(Q[j:j + 30]) for j in range(Q.size - 29)]) / (30.0 * hop)
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
    return ref_loudness_multi(x, fs, weights), lra, mm, ms, margin


def _noise_hum(n, fs, seed, level=0.05):
    """Noise over a 180 Hz hum: stationary, every 400 ms block within a fraction of an LU of the others."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / fs
    return (level * rng.standard_normal(n) + 0.4 * level * np.sin(2 * np.pi * 180 * t)).astype(np.float32)


def programmes(fs):
    """The programmes of the ragged call of tests/test_multichannel_gpu.py, [(name, x (C, N) float32)], seeds fixed."""
    n6 = int(2.5 * fs)
    t6 = np.arange(n6) / fs
    six = np.stack([_noise_hum(n6, fs, 60 + c, 0.03) for c in range(6)])
    six[3] = (0.45 * np.sin(2 * np.pi * 100 * t6)).astype(np.float32)       # the LFE: a hum 20 dB above the other channels
    n2 = int(1.7 * fs)
    two = np.stack([_noise_hum(n2, fs, 21, 0.08), _noise_hum(n2, fs, 22, 0.02)])     # unequal levels
    n3 = int(1.3 * fs) + 7
    three = np.stack([_noise_hum(n3, fs, 31), np.zeros(n3, np.float32), _noise_hum(n3, fs, 33, 0.1)])
    return [("short mono", _noise_hum(int(0.3 * fs), fs, 11)[None]),
            ("stereo, unequal levels", two),
            ("5.1 with a loud LFE", six),
            ("three channels, one silent", three),
            ("silent stereo", np.zeros((2, int(0.9 * fs) + 3), np.float32))]


def mod_hum(n, fs, seed):
    """The report signal of tests/test_true_peak_gpu.py, hum under noise whose level swings slowly, with a swing of 8 dB
    instead of 14: the quietest 400 ms block then stays ~4 LU above the relative gate of the integrated measurement (with
    14 dB the level sweeps THROUGH that gate and some block always lands within 0.05 LU of it)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / fs
    return (0.1 * rng.standard_normal(n) * (0.7 + 0.3 * np.sin(2 * np.pi * t / 37.0)) + 0.02 * np.sin(2 * np.pi * 50 * t)) \
        .astype(np.float32)


def report_programme(fs):
    """The 2-channel 75 s programme of the report test."""
    n = 75 * fs + 123
    return np.stack([mod_hum(n, fs, 3), 0.5 * mod_hum(n, fs, 4)])


# ---- the reference -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fs", [44100, 48000])
def test_reference_of_one_channel_is_the_mono_reference(fs):
    for seed, secs in ((1, 0.3), (2, 1.7), (3, 6.0)):
        x = _noise_hum(int(secs * fs), fs, seed)
        a, b = ref_loudness_multi(x[None], fs, [1.0]), ref_loudness(x, fs)
        assert a == b or abs(a - b) <= 1e-12, (fs, secs, a, b)


@pytest.mark.parametrize("fs", [44100, 48000])
def test_reference_known_values(fs):
    x = _noise_hum(3 * fs, fs, 5)
    mono = ref_loudness(x, fs)
    assert abs(ref_loudness_multi(np.stack([x, x]), fs, channel_weights(2)) - (mono + 10 * math.log10(2))) <= 1e-6
    assert abs(10 * math.log10(2) - 3.0103) < 1e-5
    six = np.zeros((6, x.size), np.float32)
    six[3] = x
    assert ref_loudness_multi(six, fs, channel_weights(6)) == -math.inf        # only the LFE carries signal
    front, surround = np.zeros_like(six), np.zeros_like(six)
    front[0], surround[4] = x, x
    d = ref_loudness_multi(surround, fs, channel_weights(6)) - ref_loudness_multi(front, fs, channel_weights(6))
    assert abs(d - 10 * math.log10(1.41)) <= 1e-6
    assert abs(ref_loudness_multi(front, fs, channel_weights(6)) - mono) <= 1e-9


def test_reference_report_of_one_channel_is_the_mono_recipe():
    from test_true_peak_cpu import ref_report
    fs = 16000
    x = mod_hum(40 * fs, fs, 9)
    a, b = ref_report_multi(x[None], fs, [1.0]), ref_report(x, fs)
    assert np.allclose(a, b, rtol=0, atol=1e-9)


# ---- arguments -----------------------------------------------------------------------------------------------------------------

def test_channel_weight_table():
    s = 1.41
    want = {1: [1], 2: [1, 1], 3: [1, 1, 1], 4: [1, 1, s, s], 5: [1, 1, 1, s, s], 6: [1, 1, 1, 0, s, s],
            7: [1, 1, 1, 0, 1, s, s], 8: [1, 1, 1, 0, 1, 1, s, s]}
    for C, w in want.items():
        got = channel_weights(C)
        assert got == [float(v) for v in w] and all(isinstance(v, float) for v in got)
        got[0] = 99.0                                                       # (a copy: the table is not the caller's)
        assert channel_weights(C)[0] == 1.0
    import voicefixer_amd
    assert voicefixer_amd.channel_weights is channel_weights
    assert channel_weights(3, [0.5, 0, 2]) == [0.5, 0.0, 2.0]
    assert channel_weights(2, np.array([1.0, 0.25])) == [1.0, 0.25]
    for C in (0, 9, -1, 2.0, True, None, "2"):
        with pytest.raises(ValueError):
            channel_weights(C)
    for C, bad in ((2, [1.0]), (2, [1.0, 1.0, 1.0]), (2, [1.0, -0.5]), (2, [1.0, float("nan")]), (2, [1.0, float("inf")]),
                   (2, "11"), (2, 1.0), (1, [True]), (2, [1.0, "1"]), (2, [1.0, None])):
        with pytest.raises(ValueError):
            channel_weights(C, bad)


@pytest.mark.parametrize("bad", ["stereo", "ALL", 2, True, ["all"], b"all", ""])
def test_bad_channels_raise_on_every_entry_point_before_any_device_work(bad):
    with pytest.raises(ValueError):
        loudness.check_channels(bad)
    vf = api.VoiceFixer.__new__(api.VoiceFixer)     # (no device, no weights: the checks come first)
    x = np.zeros(44100, np.float32)
    for call in (lambda: api.VoiceFixer.restore_inmem(vf, x, channels=bad),
                 lambda: api.VoiceFixer.restore_batch(vf, [x], channels=bad),
                 lambda: api.VoiceFixer.restore_folder(vf, "/nonexistent", "/nonexistent", channels=bad),
                 lambda: api.VoiceFixer.restore(vf, "a.wav", "b.wav", channels=bad)):
        with pytest.raises(ValueError):
            call()


def test_channels_surface():
    assert [loudness.check_channels(c) for c in (None, "mix", "first", "all")] == [None, "mix", "first", "all"]
    with pytest.raises(ValueError):
        loudness.check_channels(None, allow_none=False)
    import inspect
    for fn in (api.VoiceFixer.restore, api.VoiceFixer.restore_inmem, api.VoiceFixer.restore_batch, api.VoiceFixer.restore_folder):
        sig = inspect.signature(fn).parameters
        assert sig["channels"].default is None and sig["channel_weights"].default is None, fn
    for fn in (api.VoiceFixer.restore_stream, api.VoiceFixer.open_stream):              # the streams stay mono
        assert "channels" not in inspect.signature(fn).parameters
    for fn in (api.measure_loudness, api.measure_true_peak, api.loudness_report):
        assert inspect.signature(fn).parameters["channel_weights"].default is None
    vf = api.VoiceFixer.__new__(api.VoiceFixer)
    x2 = np.zeros((2, 44100), np.float32)
    for call in (lambda: api.VoiceFixer.restore_inmem(vf, x2), lambda: api.VoiceFixer.restore_inmem(vf, x2[:1])):
        with pytest.raises(ValueError, match='channels="all"'):
            call()
    for call in (lambda: api.VoiceFixer.restore_inmem(vf, np.zeros((9, 4410), np.float32), channels="all"),
                 lambda: api.VoiceFixer.restore_inmem(vf, np.zeros((2, 2, 4410), np.float32), channels="all"),
                 lambda: api.VoiceFixer.restore_inmem(vf, x2, channels="all", channel_weights=[1.0]),
                 lambda: api.VoiceFixer.restore_inmem(vf, x2, channels="all", channel_weights=[1.0, -1.0]),
                 lambda: api.VoiceFixer.restore_batch(vf, [x2], channels="all", channel_weights="11"),
                 lambda: api.VoiceFixer.restore_batch(vf, [x2, x2[:1]], channels="all", channel_weights=[1.0, 1.0]),
                 lambda: api.VoiceFixer.restore_batch(vf, [np.zeros((6, 4410), np.float32)], channels="all", batch_size=4),
                 lambda: api.measure_loudness(x2, channel_weights=[1.0]),
                 lambda: api.measure_loudness(np.zeros((9, 100), np.float32)),
                 lambda: api.loudness_report([x2, np.zeros((2, 2, 10), np.float32)]),
                 lambda: api.measure_true_peak(x2, sample_rate=1000),
                 lambda: api.apply_loudness_groups(None, [1, 1], [2], 44100, 5.0)):
        with pytest.raises(ValueError):
            call()
    assert api.apply_loudness_groups("rows", [1, 1], [2], 44100, None) == ("rows", None)   # no target: nothing is launched


def test_cli_channels_flag():
    from voicefixer_amd.__main__ import build_parser
    assert build_parser().parse_args(["-i", "x.wav"]).channels is None
    for v in ("mix", "first", "all"):
        assert build_parser().parse_args(["-i", "x.wav", "--channels", v]).channels == v
        assert build_parser().parse_args(["-ifdr", "d", "-ofdr", "o", "--channels", v, "--loudness", "-23", "--true-peak"]).channels == v
    for bad in (["--channels"], ["--channels", "stereo"], ["--channels", "2"], ["--channels", "ALL"]):
        with pytest.raises(SystemExit):
            build_parser().parse_args(["-i", "x.wav"] + bad)


def test_entry_points_declared_mapped_and_bound():
    import ctypes as C
    hdr = open(os.path.join(ROOT, "include", "vfx_hip.h")).read()
    names = ("vfx_loudness_groups_workspace_bytes", "vfx_loudness_groups_f32", "vfx_loudness_report_groups_workspace_bytes",
             "vfx_loudness_report_groups_f32")
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES, name
    res, args = _lib.SIGNATURES["vfx_loudness_groups_f32"]
    assert res is C.c_int and len(args) == 25 and args[13] is C.c_double and args[14] is C.c_double and args[23] is C.c_size_t
    res, args = _lib.SIGNATURES["vfx_loudness_report_groups_f32"]
    assert res is C.c_int and len(args) == 21 and args[19] is C.c_size_t
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    h = _lib.lib()
    for name in names:
        assert hasattr(h, name), name
    B, n, hop, S = 32, 441000, 4410, 224
    per_row = h.vfx_loudness_workspace_bytes(B, n, hop, S) + h.vfx_true_peak_workspace_bytes(B, n, 4, 188)
    assert per_row < h.vfx_loudness_groups_workspace_bytes(B, n, hop, S, 4, 188) <= per_row + 4 * 8 * B + 256
    assert h.vfx_loudness_report_groups_workspace_bytes(B, n, hop, S, 4, 188) == h.vfx_loudness_report_workspace_bytes(B, n, hop, S, 4, 188)
    assert h.vfx_loudness_groups_workspace_bytes(0, n, hop, S, 4, 188) == 0
    assert h.vfx_loudness_groups_workspace_bytes(B, n, hop, S, 3, 188) == 0
    # bad arguments are refused on the host, before any device work: no groups, NULL pointers
    nan = float("nan")
    one = C.c_void_p(64)           # (never dereferenced: a refused call launches nothing)
    coef = (C.c_double * 10)(*([1.0] * 10))
    for G, gs, wt in ((0, one, one), (-1, one, one), (1, None, one), (1, one, None)):
        assert h.vfx_loudness_groups_f32(one, 16, one, 1, 10, gs, wt, G, coef, one, S, hop, 1, nan, -1.0, one, 188, 4, 375, None, 0,
                                         one, one, 1 << 20, None) == _lib.EINVAL
        assert h.vfx_loudness_report_groups_f32(one, 16, one, 1, 10, gs, wt, G, coef, one, S, hop, 1, one, 188, 4, 375, one, one,
                                                1 << 20, None) == _lib.EINVAL
    assert h.vfx_loudness_groups_f32(None, 0, None, 1, 10, one, one, 1, None, None, S, hop, 1, nan, -1.0, None, 0, 1, 0, None, 0,
                                     None, None, 0, None) == _lib.EINVAL


# ---- planning, containers ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(6))
def test_planning_keeps_the_channels_of_a_file_in_one_batch(seed):
    rng = np.random.default_rng(seed)
    n_files = int(rng.integers(1, 40))
    counts = [int(c) for c in rng.integers(1, 9, n_files)]
    lengths = sorted(int(v) for v in rng.integers(600, 3 * api.SEG_LENGTH, n_files))
    if seed % 2:                                                            # equal-length buckets as well
        lengths = sorted(lengths[:n_files // 2] + [2 * api.SEG_LENGTH] * (n_files - n_files // 2))
    for batch_size in (max(counts), max(counts) + 3, 32):
        plan = api.plan_batches(lengths, batch_size, rows=counts)
        assert [g for _, grp in plan for g in grp] == list(range(n_files))          # every file once, in order, whole
        for kind, grp in plan:
            assert 1 <= sum(counts[g] for g in grp) <= batch_size
            if kind == "samples":
                assert len({lengths[g] for g in grp}) == 1
            else:
                assert all(1025 <= lengths[g] <= api.SEG_LENGTH for g in grp)
    with pytest.raises(ValueError, match="batch_size"):
        api.plan_batches(lengths, max(counts) - 1, rows=counts)
    with pytest.raises(ValueError):
        api.plan_batches(lengths, 32, rows=counts[:-1] if n_files > 1 else [1, 1])
    assert api.plan_batches(lengths, 8, rows=[1] * n_files) == api.plan_batches(lengths, 8)     # one row per file: as before


@pytest.mark.parametrize("ext", [".wav", ".flac"])
def test_six_channel_round_trip_and_header_channel_count(ext, tmp_path):
    rng = np.random.default_rng(7)
    for C, n in ((6, 5), (6, 3000), (1, 40), (2, 1), (8, 777)):      # (6, 5): fewer samples than channels
        x = (rng.integers(-20000, 20000, (C, n)) / 32768.0).astype(np.float32)
        path = str(tmp_path / ("c%d_%d%s" % (C, n, ext)))
        audio_io.save_wave(x, path, 48000, channels_first=True)
        assert audio_io.wav_channels(path) == C
        assert audio_io.wav_info(path)[:2] == (48000, n)
        y = audio_io.load_wav(path, 48000, mono=False)
        assert y.dtype == np.float32 and np.array_equal(y if C > 1 else y[None], x)
        assert np.array_equal(audio_io.select_channels(y, "all"), x)
        assert np.array_equal(audio_io.select_channels(y, "first"), x[0])
        assert audio_io.select_channels(y, "mix").shape == (n,)
    for bad in (np.zeros(10, np.float32), np.zeros((9, 100), np.float32), np.zeros((2, 2, 2), np.float32)):
        with pytest.raises(ValueError):
            audio_io.save_wave(bad, str(tmp_path / ("bad" + ext)), 48000, channels_first=True)
    # today's callers: (1, N) and (2, N) are still recognised without the flag, and written as before
    a, b = str(tmp_path / ("a" + ext)), str(tmp_path / ("b" + ext))
    x = (rng.integers(-20000, 20000, (2, 500)) / 32768.0).astype(np.float32)
    audio_io.save_wave(x, a, 44100)
    audio_io.save_wave(x, b, 44100, channels_first=True)
    assert open(a, "rb").read() == open(b, "rb").read()


# ---- the input condition of the GPU test ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("fs", [44100, 48000])
def test_no_block_of_the_gpu_programmes_lies_near_a_gate(fs):
    """The 0.005 LU bound of tests/test_multichannel_gpu.py must never depend on a block flipping sides of a gate."""
    seen = []
    for name, x in programmes(fs) + [("report", report_programme(fs))]:
        L, margin = ref_loudness_multi(x, fs, channel_weights(x.shape[0]), with_margin=True)
        assert margin >= 0.05, (fs, name, margin)
        seen.append((name, L))
        for c in range(x.shape[0]):                                         # and each channel on its own (the per-row comparisons)
            assert ref_loudness_multi(x[c:c + 1], fs, [1.0], with_margin=True)[1] >= 0.05, (fs, name, c)
    L = dict(seen)
    assert L["short mono"] == -math.inf and L["silent stereo"] == -math.inf
    assert all(math.isfinite(L[k]) for k in ("stereo, unequal levels", "5.1 with a loud LFE", "three channels, one silent", "report"))
    six = programmes(fs)[2][1]
    assert ref_loudness_multi(six, fs, [1.0] * 6) - L["5.1 with a loud LFE"] > 5.0      # ignoring the weights fails by many LU
    assert ref_report_multi(report_programme(fs), fs, [1.0, 1.0])[4] > 0.01            # the LRA gates (the report test's margin)
