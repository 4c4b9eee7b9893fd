"""The look-ahead peak limiter without a GPU: the float64 reference of its definition (loudness.py; the
yardstick of tests/test_limiter_gpu.py), the properties the definition promises, what it buys on a signal with transients,
parameter checks, the refusals of the streaming entry points, the CLI flags and the C-ABI bindings."""
import inspect
import math
import os
import re

import numpy as np
import pytest
from scipy.ndimage import minimum_filter1d
from scipy.signal import upfirdn

from voicefixer_amd import _lib, api, loudness
from test_loudness_cpu import ref_loudness
from test_true_peak_cpu import ref_interpolator, ref_oversampling, ref_true_peak

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ref_window(fs, ms):
    H = int(math.floor(fs * ms / 1000.0 + 0.5))
    k = np.arange(-H, H + 1, dtype=np.float64)
    return H, (1.0 + np.cos(np.pi * k / (H + 1))) / (2.0 * H + 2.0)


def ref_envelope(x, fs, true_peak=True):
    """e[n] of one row: |x[n]| and, when the row is oversampled, the interpolated values at times in (n - 1, n]."""
    x = np.asarray(x, np.float64)
    N, R = x.size, ref_oversampling(fs) if true_peak else 1
    e = np.abs(x)
    if R > 1 and N:
        g = ref_interpolator(R).astype(np.float64)
        c = (g.size - 1) // 2
        y = np.abs(upfirdn(g, x, up=R)[c:c + R * N])
        assert y.size == R * N
        n_of_m = np.minimum((np.arange(R * N) + c % R) // R, N - 1)
        np.maximum.at(e, n_of_m, y)
    return e


def ref_limit(x, fs, gL, ceiling_db=-1.0, ms=3.0, true_peak=True):
    """The definition in float64 on a row (N,) or a programme (C, N) of float32 samples: a dict with ``out`` (the shape of
    x), ``bound``, ``TP``, ``c``, ``m``, ``g`` (N,), ``t`` and ``after`` (TPv t; gL TP when not bound)."""
    xs = np.atleast_2d(np.asarray(x, np.float64))
    N = xs.shape[1]
    Cl = 10.0 ** (ceiling_db / 20.0)
    H, w = ref_window(fs, ms)
    e = np.max([ref_envelope(r, fs, true_peak) for r in xs], axis=0) if N else np.zeros(0)
    TP = float(e.max()) if N else 0.0
    one = np.ones(N)
    if not gL * TP > Cl:
        out = gL * xs
        return dict(out=out.reshape(np.shape(x)), bound=False, TP=TP, c=one, m=one, g=one, t=1.0, after=gL * TP, H=H)
    with np.errstate(divide="ignore"):
        c = np.where(e > 0, np.minimum(1.0, Cl / (gL * np.where(e > 0, e, 1.0))), 1.0)
    m = minimum_filter1d(c, size=2 * H + 1, mode="constant", cval=1.0)
    d = np.pad(1.0 - m, H, mode="edge")                       # m[clamp(n + k, 0, N - 1)]
    g = 1.0 - np.convolve(d, w, mode="valid")
    v = gL * g[None] * xs
    if true_peak:
        TPv = max(ref_true_peak(r, fs) for r in v)
    else:
        TPv = float(np.abs(v).max())
    t = min(1.0, Cl / TPv)
    return dict(out=(t * v).reshape(np.shape(x)), bound=True, TP=TP, c=c, m=m, g=g, t=t, after=TPv * t, H=H)


def transient_signal(fs=44100, seed=1):
    """3 s of noise at -26.1 LUFS with two clicks and a short burst at fs / 4: the signal of DESIGN.md 3.14."""
    rng = np.random.default_rng(seed)
    n = 3 * fs
    noise = rng.standard_normal(n)
    a = 10.0 ** ((-26.1 - ref_loudness(noise, fs)) / 20.0)
    for _ in range(4):                                        # (the transients add a little: the noise makes up for it)
        x = a * noise
        x[int(0.7 * fs)] = 0.9
        x[int(2.1 * fs)] = -0.85
        b0, nb = int(1.4 * fs), int(0.004 * fs)
        x[b0:b0 + nb] += 0.6 * np.sin(2 * np.pi * np.arange(nb) / 4 + math.pi / 4) * np.hanning(nb)
        a *= 10.0 ** ((-26.1 - ref_loudness(x, fs)) / 20.0)
    return x.astype(np.float32)


@pytest.mark.parametrize("fs,ms,H", [(4000, 0.25, 1), (4000, 0.5, 2), (44100, 3.0, 132), (409600, 10.0, 4096)])
def test_weights_sum_to_one(fs, ms, H):
    Hw, w = loudness.limiter_window(fs, ms)
    assert Hw == H and w.size == 2 * H + 1 and np.all(w > 0)
    assert abs(float(np.sum(w)) - 1.0) <= 1e-15 and abs(math.fsum(w) - 1.0) <= 1e-15
    assert np.array_equal(w, w[::-1])
    k = np.arange(-H, H + 1, dtype=np.float64)
    assert np.array_equal(w, (1.0 + np.cos(np.pi * k / (H + 1))) / (2.0 * H + 2.0))


def test_window_matches_the_reference_and_its_ranges():
    for fs, ms in ((44100, 3.0), (8000, 3.0), (48000, 1.0), (192000, 10.0), (96000, 0.1)):
        H, w = loudness.limiter_window(fs, ms)
        Hr, wr = ref_window(fs, ms)
        assert H == Hr and np.array_equal(w, wr)
    assert loudness.limiter_window(44100, 3.0)[0] == 132 and loudness.limiter_window(8000)[0] == 24


@pytest.mark.parametrize("true_peak", [True, False])
def test_reference_properties(true_peak):
    fs = 44100
    x = transient_signal(fs)
    ref = ref_limit(x, fs, 4.0, -1.0, 3.0, true_peak)
    H, c, g = ref["H"], ref["c"], ref["g"]
    Cl = 10.0 ** (-1.0 / 20.0)
    assert ref["bound"] and H == 132
    assert np.all(g <= c + 1e-15) and np.all(g > 0)
    hot = np.flatnonzero(c < 1.0)
    far = np.ones(x.size, bool)
    for j in hot:
        far[max(j - 2 * H, 0):j + 2 * H + 1] = False
    assert far.any() and np.all(g[far] == 1.0)                # exactly one outside 2 H of any c < 1
    assert np.all(g[~far] <= 1.0) and g.min() < 0.3
    out = ref["out"]
    tp = ref_true_peak(out, fs) if true_peak else float(np.abs(out).max())
    print("true_peak=%s: %.2f %% of the samples get g < 1, min g %.4f, t %.9f (%.2e dB), peak after %.6f dB"
          % (true_peak, 100.0 * np.mean(g < 1.0), g.min(), ref["t"], 20 * math.log10(ref["t"]), 20 * math.log10(tp)))
    assert tp <= Cl * (1.0 + 1e-12) and ref["t"] > 0.9999
    assert ref["after"] == pytest.approx(tp, rel=1e-12)
    # a row the ceiling does not bind: the static path
    quiet = ref_limit(0.01 * x, fs, 2.0, -1.0, 3.0, true_peak)
    assert not quiet["bound"] and np.array_equal(quiet["out"], 2.0 * (0.01 * x).astype(np.float64)) and quiet["t"] == 1.0


def test_the_limiter_reaches_the_target_where_the_static_ceiling_does_not():
    fs, T = 44100, -14.06
    x = transient_signal(fs)
    L = ref_loudness(x, fs)
    assert abs(L - (-26.1)) < 0.05
    gL = 10.0 ** ((T - L) / 20.0)
    Cl = 10.0 ** (-1.0 / 20.0)
    static = min(gL, Cl / ref_true_peak(x, fs)) * x.astype(np.float64)
    lim = ref_limit(x, fs, gL, -1.0, 3.0, True)
    Ls, Ll = ref_loudness(static, fs), ref_loudness(lim["out"], fs)
    print("input %.2f LUFS, target %.2f: static ceiling %.2f LUFS, limiter %.2f LUFS (%.2f %% of the samples limited)"
          % (L, T, Ls, Ll, 100.0 * np.mean(lim["g"] < 1.0)))
    assert abs(Ll - T) <= 0.5
    assert T - Ls > 10.0


def test_programme_shares_one_gain_curve():
    fs = 44100
    x = transient_signal(fs)[:fs]
    x2 = np.stack([x, 0.5 * np.roll(x, 300)]).astype(np.float32)
    x2[1, int(0.7 * fs) + 300] = 0.0                          # the click stays in channel 0 only
    ref = ref_limit(x2, fs, 4.0)
    assert ref["out"].shape == x2.shape and ref["bound"]
    keep = np.abs(x2[1]) > 1e-3
    ratio = ref["out"][1, keep] / x2[1, keep].astype(np.float64)
    assert np.allclose(ratio, 4.0 * ref["g"][keep] * ref["t"], rtol=1e-12)


@pytest.mark.parametrize("bad", [None, 1, 0, "yes", 1.0])
def test_limiter_must_be_a_bool(bad):
    with pytest.raises(ValueError):
        loudness.check_limiter(bad, 3.0)
    vf = api.VoiceFixer.__new__(api.VoiceFixer)
    x = np.zeros(44100, np.float32)
    for call in (lambda: api.VoiceFixer.restore_inmem(vf, x, loudness=-16, limiter=bad),
                 lambda: api.VoiceFixer.restore_batch(vf, [x], loudness=-16, limiter=bad),
                 lambda: next(api.VoiceFixer.restore_batches(vf, iter([]), loudness=-16, limiter=bad)),
                 lambda: api.VoiceFixer.restore_folder(vf, "/nonexistent", "/nonexistent", loudness=-16, limiter=bad),
                 lambda: api.VoiceFixer.restore(vf, "a.wav", "b.wav", loudness=-16, limiter=bad),
                 lambda: api.VoiceFixer.restore_stream(vf, x, limiter=bad),
                 lambda: api.VoiceFixer.open_stream(vf, limiter=bad)):
        with pytest.raises(ValueError):
            call()


@pytest.mark.parametrize("ms", [0, 11, float("nan"), "3", 0.05, -1.0, True, None])
def test_bad_lookahead_raises_before_any_device_work(ms):
    with pytest.raises(ValueError):
        loudness.check_limiter(True, ms)
    vf = api.VoiceFixer.__new__(api.VoiceFixer)
    x = np.zeros(44100, np.float32)
    with pytest.raises(ValueError):
        api.VoiceFixer.restore_inmem(vf, x, loudness=-16, limiter=True, limiter_lookahead_ms=ms)
    with pytest.raises(ValueError):
        api.VoiceFixer.restore_folder(vf, "/nonexistent", "/nonexistent", loudness=-16, limiter=True, limiter_lookahead_ms=ms)


def test_parameter_rules():
    assert loudness.check_limiter(True, 3) == (True, 3.0) and loudness.check_limiter(np.bool_(False), 0.1) == (False, 0.1)
    assert loudness.check_limiter(True, 10.0) == (True, 10.0)
    with pytest.raises(ValueError):                 # 10 ms at 768 kHz: H = 7680 > 4096
        loudness.limiter_window(768000, 10.0)
    assert loudness.limiter_window(768000, 5.0)[0] == 3840
    vf = api.VoiceFixer.__new__(api.VoiceFixer)
    x = np.zeros(44100, np.float32)
    with pytest.raises(ValueError):
        api.VoiceFixer.restore_inmem(vf, x, loudness=-16, limiter=True, limiter_lookahead_ms=10.0, output_sample_rate=768000)
    for call in (lambda: api.VoiceFixer.restore_inmem(vf, x, limiter=True),              # no target
                 lambda: api.VoiceFixer.restore_batch(vf, [x], limiter=True),
                 lambda: next(api.VoiceFixer.restore_batches(vf, iter([]), limiter=True)),
                 lambda: api.VoiceFixer.restore_folder(vf, "/nonexistent", "/nonexistent", limiter=True),
                 lambda: api.VoiceFixer.restore(vf, "a.wav", "b.wav", limiter=True),
                 lambda: api.apply_limiter(None, [1], 44100, None)):
        with pytest.raises(ValueError):
            call()
    # checked once, forwarded only when set: a stand-in for the device stage that knows no such keyword keeps working
    assert api._Output().kwargs() == {} and "limiter" not in api._Output(loudness=-16.0, true_peak=True).kwargs()
    kw = api._Output(loudness=-16.0, limiter=True, limiter_lookahead_ms=5).kwargs()
    assert kw["limiter"] is True and kw["limiter_lookahead_ms"] == 5.0 and "true_peak" not in kw


def test_streams_refuse_the_limiter():
    vf = api.VoiceFixer.__new__(api.VoiceFixer)
    x = np.zeros(44100, np.float32)
    with pytest.raises(NotImplementedError):
        api.VoiceFixer.restore_stream(vf, x, limiter=True)
    with pytest.raises(NotImplementedError):
        api.VoiceFixer.restore_stream(vf, x, loudness=-16, limiter=True)
    with pytest.raises(NotImplementedError):
        api.VoiceFixer.open_stream(vf, limiter=True)


def test_every_public_signature_has_the_limiter_off_by_default():
    for fn in (api.VoiceFixer.restore, api.VoiceFixer.restore_inmem, api.VoiceFixer.restore_batch,
               api.VoiceFixer.restore_batches, api.VoiceFixer.restore_folder, api.VoiceFixer.restore_stream,
               api.VoiceFixer.open_stream):
        sig = inspect.signature(fn).parameters
        assert sig["limiter"].default is False and sig["limiter_lookahead_ms"].default == 3.0, fn


def test_cli_flags():
    from voicefixer_amd.__main__ import build_parser
    a = build_parser().parse_args(["-i", "x.wav", "--loudness", "-16", "--true-peak", "--limiter"])
    assert a.limiter is True and a.limiter_lookahead_ms == 3.0 and a.true_peak is True
    a = build_parser().parse_args(["-i", "x.wav", "--loudness", "-16", "--limiter", "--limiter-lookahead-ms", "1.5"])
    assert a.limiter is True and a.limiter_lookahead_ms == 1.5 and a.true_peak is False
    a = build_parser().parse_args(["-i", "x.wav", "--loudness", "-16"])
    assert a.limiter is False and a.limiter_lookahead_ms == 3.0
    assert build_parser().parse_args(["-i", "x.wav"]).limiter is False
    for bad in (["--limiter"], ["--limiter-lookahead-ms", "2"], ["--loudness", "-16", "--limiter-lookahead-ms", "2"],
                ["--loudness", "-16", "--limiter", "--limiter-lookahead-ms", "11"],
                ["--loudness", "-16", "--limiter", "--limiter-lookahead-ms", "0"],
                ["--loudness", "-16", "--limiter", "--limiter-lookahead-ms", "soon"],
                ["--loudness", "-16", "--limiter", "yes"]):
        with pytest.raises(SystemExit):
            build_parser().parse_args(["-i", "x.wav"] + bad)


def test_entry_points_declared_mapped_and_bound():
    import ctypes as C
    hdr = open(os.path.join(ROOT, "include", "vfx_hip.h")).read()
    names = ("vfx_loudness_limit_workspace_bytes", "vfx_loudness_limit_f32")
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES, name
    res, args = _lib.SIGNATURES["vfx_loudness_limit_f32"]
    gres, gargs = _lib.SIGNATURES["vfx_loudness_groups_f32"]
    # the arguments of the grouped entry, with H and the true-peak flag before the result
    assert res is C.c_int and len(args) == len(gargs) + 2 == 27 and args[:21] == gargs[:21] and args[23:] == gargs[21:]
    assert args[21] is C.c_int and args[22] is C.c_int and args[25] is C.c_size_t
    assert _lib.SIGNATURES["vfx_loudness_limit_workspace_bytes"] == _lib.SIGNATURES["vfx_loudness_groups_workspace_bytes"]
    decl = re.search(r"int vfx_loudness_limit_f32\(([^;]*)\);", hdr).group(1)
    assert len(decl.split(",")) == 27
    # the kernels live in an .inc of vfx_loudness.hip: the Makefile's check_no_pk_fma covers the whole object
    mk = open(os.path.join(ROOT, "voicefixer_amd", "csrc", "Makefile")).read()
    src = open(os.path.join(ROOT, "voicefixer_amd", "csrc", "vfx_loudness.hip")).read()
    inc = open(os.path.join(ROOT, "voicefixer_amd", "csrc", "vfx_limit.inc")).read()
    assert '#include "vfx_limit.inc"' in src and "lk_limit_kernel" in inc and "lk_env_kernel" in inc
    assert re.search(r"^vfx_loudness\.o:.*vfx_limit\.inc", mk, re.M) and '"vfx_loudness:."' in mk
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    h = _lib.lib()
    for name in names:
        assert hasattr(h, name), name
    # scratch: at most 8 bytes per sample of the batch on top of the grouped entry's workspace
    p = loudness.plan(44100)
    for B, n in ((1, 30 * 60 * 44100), (32, 441000), (3, 1000)):
        base = h.vfx_loudness_groups_workspace_bytes(B, n, p["hop"], p["S"], 4, 188)
        got = h.vfx_loudness_limit_workspace_bytes(B, n, p["hop"], p["S"], 4, 188)
        assert base < got <= base + 8 * B * n + 16384, (B, n, got - base)
    for bad in ((0, 10, 4410, 224, 4, 188), (1, -1, 4410, 224, 4, 188), (1, 10, 4410, 224, 3, 188), (1, 10, 4410, 224, 4, 0),
                (1, 10, 0, 224, 4, 188)):
        assert h.vfx_loudness_limit_workspace_bytes(*bad) == 0, bad
    # bad arguments are refused on the host, before any device work (the pointers below are never followed: host memory)
    coef = (C.c_double * 10)(*p["coef"])
    buf = (C.c_double * 64)()
    ptr = C.cast(buf, C.c_void_p)
    out = C.cast((C.c_double * 64)(), C.c_void_p)
    big = 1 << 40
    good = [ptr, 64, ptr, 1, 64, None, None, 0, coef, ptr, p["S"], p["hop"], p["lookback"], -16.0, -1.0, ptr, 188, 4, 375,
            out, 64, 132, 1, ptr, ptr, big, None]
    before = h.vfx_launch_count()
    for i, bad in ((21, 0), (21, 4097), (21, -1), (22, 2), (22, -1), (13, float("nan")), (13, float("inf")), (25, 1024),
                   (19, None), (0, None), (23, None), (15, None), (16, 0), (17, 3), (18, -1), (18, 4 * 188), (7, 1), (7, -1),
                   (5, ptr), (6, ptr), (14, float("nan")), (10, 48), (3, 0)):
        a = list(good)
        a[i] = bad
        assert h.vfx_loudness_limit_f32(*a) == _lib.EINVAL, (i, bad)
    # out may be x itself; any other overlap of the two batches is refused
    a = list(good)
    a[19] = C.c_void_p(ptr.value + 16)
    assert h.vfx_loudness_limit_f32(*a) == _lib.EINVAL
    a = list(good)
    a[3], a[1], a[19], a[20] = 2, 64, ptr, 128
    assert h.vfx_loudness_limit_f32(*a) == _lib.EINVAL
    assert h.vfx_launch_count() == before
