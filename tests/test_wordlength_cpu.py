"""Word-length reduction without a device: the numpy specification (wordlength.py) -- split-equals-whole, saturation, the
statistics of the two dithers -- the ``_Output`` record, ``audio_io.save_pcm`` (24-bit WAV, FLAC at both depths), the C-ABI
binding of vfx_quantize_rows_f32, the CLI flags and the public signatures."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from voicefixer_amd import _lib, api, audio_io, flac, wordlength

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SATURATION = np.array([1.0, -1.0, 1.5, -1.5, np.nan, np.inf, -np.inf], np.float32)


@pytest.mark.parametrize("kind", ["tpdf", "hp"])
@pytest.mark.parametrize("bits", [16, 24])
def test_a_row_in_two_pieces_equals_the_whole_row(kind, bits):
    rng = np.random.default_rng(11)
    x = (0.2 * rng.standard_normal(5000)).astype(np.float32)
    whole, clipped, peak = wordlength.quantize_ref(x, bits, kind, seed=9, channel=2)
    assert whole.dtype == np.int32 and whole.shape == x.shape
    for cut in (1, 2, 3, 1237):
        a, ca, pa = wordlength.quantize_ref(x[:cut], bits, kind, seed=9, channel=2)
        b, cb, pb = wordlength.quantize_ref(x[cut:], bits, kind, seed=9, n0=cut, channel=2)
        assert np.array_equal(np.concatenate([a, b]), whole), (kind, cut)
        assert ca + cb == clipped and max(pa, pb) == peak
    d = wordlength.dither(kind, 0, 5000, 2, 9)
    for cut in (1, 2, 3, 1237):
        assert np.array_equal(wordlength.dither(kind, cut, 5000 - cut, 2, 9), d[cut:])
    # the counter's second word: a row that crosses block 2^32 equals its two pieces as well
    n0 = 2 ** 34 - 6
    d = wordlength.dither(kind, n0, 12, 0, 9)
    assert np.array_equal(np.concatenate([wordlength.dither(kind, n0, 5, 0, 9), wordlength.dither(kind, n0 + 5, 7, 0, 9)]), d)
    assert len(set(d.tolist())) == 12


def test_dither_depends_on_channel_and_seed_and_is_bounded():
    for kind in ("tpdf", "hp"):
        base = wordlength.dither(kind, 0, 4096, 0, 0)
        assert np.all(np.abs(base) < 1.0) and np.all(base * 2.0 ** 24 == np.rint(base * 2.0 ** 24))
        assert not np.array_equal(base, wordlength.dither(kind, 0, 4096, 1, 0))
        assert not np.array_equal(base, wordlength.dither(kind, 0, 4096, 0, 1))
        assert not np.array_equal(base, wordlength.dither(kind, 0, 4096, 0, 2 ** 63 + 5))
        assert np.array_equal(base, wordlength.dither(kind, 0, 4096, 0, 0))
    assert np.array_equal(wordlength.dither("none", 5, 100, 3, 7), np.zeros(100))
    # "hp" starts with the "tpdf" value and goes on with differences of stream 0 alone
    k0 = wordlength.words(0, 64, 0, 3, 0)
    hp = wordlength.dither("hp", 0, 64, 0, 3)
    assert hp[0] == wordlength.dither("tpdf", 0, 1, 0, 3)[0]
    assert np.array_equal(hp[1:], (k0[1:] - k0[:-1]) * 2.0 ** -24)
    assert wordlength.DEPTHS == (16, 24) and wordlength.DITHERS == ("none", "tpdf", "hp")


def test_plain_rounding_keeps_the_grid_and_rounds_half_to_even():
    q = np.arange(-32768, 32768, 7, dtype=np.int64)
    got, clipped, peak = wordlength.quantize_ref((q / 32768.0).astype(np.float32), 16, "none")
    assert np.array_equal(got, q) and clipped == 0 and peak == 32768
    halves = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.49999, 0.50001], np.float64) / 32768.0
    assert wordlength.quantize_ref(halves, 16, "none")[0].tolist() == [0, 2, 2, 0, -2, -2, 0, 1]
    q24 = np.array([-(1 << 23), (1 << 23) - 1, 12345, -1], np.int64)
    got, clipped, peak = wordlength.quantize_ref((q24 / float(1 << 23)).astype(np.float64), 24, "none")
    assert np.array_equal(got, q24) and clipped == 0 and peak == 1 << 23


def test_saturation_never_wraps():
    """The vector of the issue.  Its outputs and its peak are as stated there; its count of clipped samples follows the
    definition -- the samples the clamp changed, or whose x was NaN: 1.0 (32768 -> 32767), 1.5, -1.5, NaN, +inf and -inf are six
    (-1.0 is exactly -32768 and is not changed); the issue's text says five, which no reading of its own definition gives."""
    q, clipped, peak = wordlength.quantize_ref(SATURATION, 16, "none")
    assert q.tolist() == [32767, -32768, 32767, -32768, 0, 32767, -32768]
    assert clipped == 6 and peak == 32768
    q, clipped, peak = wordlength.quantize_ref(SATURATION, 24, "none")
    assert q.tolist() == [8388607, -8388608, 8388607, -8388608, 0, 8388607, -8388608] and clipped == 6 and peak == 8388608
    for kind in ("tpdf", "hp"):         # dither moves the two full-scale samples by at most one LSB and nothing else
        q, clipped, peak = wordlength.quantize_ref(SATURATION, 16, kind, seed=5)
        assert q[[0, 2, 3, 4, 5, 6]].tolist() == [32767, 32767, -32768, 0, 32767, -32768] and q[1] in (-32768, -32767)
        assert 5 <= clipped <= 7 and peak == 32768


@pytest.mark.parametrize("kind", ["tpdf", "hp"])
def test_error_statistics_and_spectrum(kind):
    """2^18 samples of a DC input at 0, 0.3 and 0.5 LSB: the total error has no bias and a variance of 1/4 LSB^2 whatever the
    offset (what triangular dither of +-1 LSB buys), both within 5 standard errors computed from the sample; below fs / 16 lies
    1/8 of the white dither's power and (pi/8 - sin(pi/8)) / pi = 0.0032 of the high-passed one's."""
    N = 1 << 18
    for dc in (0.0, 0.3, 0.5):
        q, clipped, _ = wordlength.quantize_ref(np.full(N, dc / 32768.0, np.float64), 16, kind)
        e = q.astype(np.float64) - dc
        m, v = float(e.mean()), float(e.var())
        se_mean = float(np.sqrt(v / N))
        se_var = float(np.sqrt(np.var((e - m) ** 2) / N))
        print("%s dc %.1f LSB: mean %+.5f (se %.5f), variance %.5f (se %.5f)" % (kind, dc, m, se_mean, v, se_var))
        assert clipped == 0
        assert abs(m) <= 5 * se_mean, (kind, dc, m, se_mean)
        assert abs(v - 0.25) <= 5 * se_var, (kind, dc, v, se_var)
    d = wordlength.dither(kind, 0, N, 0, 0)
    P = np.abs(np.fft.rfft(d)) ** 2
    P[1:-1] *= 2.0                                   # (one-sided: every bin but DC and fs / 2 stands for two)
    low = float(P[:N // 16].sum() / P.sum())         # bins below fs / 16
    print("%s: share of dither power below fs/16 = %.4f, variance %.5f LSB^2" % (kind, low, d.var()))
    assert abs(d.var() - 1.0 / 6.0) < 0.003
    if kind == "hp":
        assert low < 0.01
    else:
        assert 0.11 <= low <= 0.14


def test_output_record():
    assert api._Output().kwargs() == {}
    assert api._Output(bit_depth=24).kwargs() == {"bit_depth": 24, "dither": "tpdf", "dither_seed": 0}
    kw = api._Output(loudness=-23.0, bit_depth=16, dither="hp", dither_seed=2 ** 64 - 1).kwargs()
    assert kw == {"loudness": -23.0, "peak_ceiling": -1.0, "bit_depth": 16, "dither": "hp", "dither_seed": 2 ** 64 - 1}
    assert api._Output(dither="none", dither_seed=7).kwargs() == {}          # without a depth nothing is forwarded
    # appended AFTER the nine positional parameters
    names = list(inspect.signature(api._Output.__init__).parameters)
    assert names[-3:] == ["bit_depth", "dither", "dither_seed"] and names.index("bit_depth") == 10
    for bad in (dict(bit_depth=8), dict(bit_depth=32), dict(bit_depth=True), dict(bit_depth="16"), dict(bit_depth=16.0),
                dict(dither="rect"), dict(dither=None), dict(dither=1), dict(bit_depth=16, dither="TPDF"),
                dict(dither_seed=-1), dict(dither_seed=2 ** 64), dict(dither_seed=1.0), dict(dither_seed=True)):
        with pytest.raises((ValueError, TypeError)):
            api._Output(**bad)
    with pytest.raises(ValueError):
        api._Output().quantize(None, [])                                      # a job without a depth has nothing to quantise
    vf = api.VoiceFixer.__new__(api.VoiceFixer)
    x = np.zeros(44100, np.float32)
    for call in (lambda: api.VoiceFixer.restore_inmem(vf, x, bit_depth=8),
                 lambda: api.VoiceFixer.restore_batch(vf, [x], bit_depth=16, dither="rect"),
                 lambda: next(api.VoiceFixer.restore_batches(vf, iter([]), bit_depth=24, dither_seed=-1)),
                 lambda: api.VoiceFixer.restore_folder(vf, "/nonexistent", "/nonexistent", bit_depth=20),
                 lambda: api.VoiceFixer.restore(vf, "a.wav", "b.wav", bit_depth=16, dither_seed=2 ** 64),
                 lambda: api.VoiceFixer.open_stream(vf, bit_depth=12),
                 lambda: api.quantize(x, bit_depth=None),
                 lambda: api.quantize(x, bit_depth=16, dither="shaped")):
        with pytest.raises((ValueError, TypeError)):
            call()


def test_every_public_signature_has_the_three_keywords():
    for fn in (api.VoiceFixer.restore, api.VoiceFixer.restore_inmem, api.VoiceFixer.restore_batch,
               api.VoiceFixer.restore_batches, api.VoiceFixer.restore_folder, api.VoiceFixer.open_stream):
        sig = inspect.signature(fn).parameters
        assert sig["bit_depth"].default is None and sig["dither"].default == "tpdf" and sig["dither_seed"].default == 0, fn
    sig = inspect.signature(api.VoiceFixer.restore_stream).parameters
    assert not {"bit_depth", "dither", "dither_seed"} & set(sig)
    sig = inspect.signature(api.quantize).parameters
    assert list(sig) == ["wav", "bit_depth", "dither", "dither_seed"] and sig["bit_depth"].default == 16
    import voicefixer_amd
    assert voicefixer_amd.quantize is api.quantize and "quantize" in voicefixer_amd.__all__
    assert list(inspect.signature(audio_io.save_pcm).parameters) == ["pcm", "fname", "sample_rate", "bit_depth", "channels_first"]


@pytest.mark.parametrize("nch", [1, 2, 3])
@pytest.mark.parametrize("n", [1000, 1001])
def test_save_pcm_24_bit_wav(tmp_path, nch, n):
    from scipy.io import wavfile
    rng = np.random.default_rng(nch * 10 + n)
    pcm = rng.integers(-(1 << 23), 1 << 23, size=(nch, n)).astype(np.int32)
    pcm[0, 0], pcm[-1, -1] = -(1 << 23), (1 << 23) - 1
    f = str(tmp_path / "x.wav")
    audio_io.save_pcm(pcm, f, 48000, 24, channels_first=True)
    sr, data = wavfile.read(f)
    assert sr == 48000 and data.dtype == np.int32                      # (scipy: 24-bit left-justified in int32)
    assert np.array_equal(data.reshape(n, -1) >> 8, pcm.T) and not np.any(data & 0xff)
    assert audio_io.wav_info(f) == (48000, n, n) and audio_io.wav_channels(f) == nch
    assert os.path.getsize(f) % 2 == 0
    head = open(f, "rb").read(24)
    assert int.from_bytes(head[20:22], "little") == (1 if nch <= 2 else 0xFFFE)       # WAVE_FORMAT_EXTENSIBLE past stereo
    back, _ = audio_io.load_wav_native(f, mono=False)
    assert np.array_equal(np.atleast_2d(back) * float(1 << 23), pcm.astype(np.float32))
    if nch == 1:                                                        # the shapes save_wave takes
        audio_io.save_pcm(pcm[0], f, 44100, 24)
        assert np.array_equal(wavfile.read(f)[1] >> 8, pcm[0])
        audio_io.save_pcm(pcm, f, 44100, 24)
        assert np.array_equal(wavfile.read(f)[1] >> 8, pcm[0])


def test_save_pcm_flac_and_16_bit_wav(tmp_path):
    from scipy.io import wavfile
    rng = np.random.default_rng(8)
    for bits, dtype in ((16, np.int16), (24, np.int32)):
        for nch in (1, 2, 3):
            pcm = rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), size=(nch, 5000)).astype(dtype)
            pcm[0, :2] = [-(1 << (bits - 1)), (1 << (bits - 1)) - 1]
            f = str(tmp_path / ("x%d_%d.flac" % (bits, nch)))
            audio_io.save_pcm(pcm, f, 44100, bits, channels_first=True)
            sr, back, bps = flac.read(f)
            assert (sr, bps) == (44100, bits) and np.array_equal(back, pcm.T)
            assert audio_io.wav_channels(f) == nch and audio_io.wav_info(f)[:2] == (44100, 5000)
    pcm = rng.integers(-32768, 32768, size=(2, 3001)).astype(np.int16)
    f = str(tmp_path / "x16.wav")
    audio_io.save_pcm(pcm, f, 32000, 16, channels_first=True)
    sr, back = wavfile.read(f)
    assert sr == 32000 and back.dtype == np.int16 and np.array_equal(back, pcm.T)
    with pytest.raises(ValueError):
        audio_io.save_pcm(np.array([40000], np.int32), f, 44100, 16)          # outside the depth: refused, never wrapped
    with pytest.raises(ValueError):
        audio_io.save_pcm(np.zeros(10, np.float32), f, 44100, 16)             # floats go through save_wave
    with pytest.raises(ValueError):
        audio_io.save_pcm(pcm, f, 44100, 20)
    with pytest.raises(RuntimeError):
        audio_io.save_pcm(pcm, str(tmp_path / "x.ogg"), 44100, 16)


def test_save_wave_still_truncates(tmp_path):
    """The default path is the reference's: x * 2^15 truncated toward zero, never rounded, byte for byte what it was."""
    from scipy.io import wavfile
    x = np.array([32766.6 / 32768, -32766.6 / 32768, 0.5 / 32768, -0.5 / 32768, 1.9 / 32768, -1.9 / 32768, 0.25, -1.0, 0.0,
                  0.99997], np.float32)
    want = np.array([32766, -32766, 0, 0, 1, -1, 8192, -32768, 0, 32767], np.int16)
    assert 32766.5 < float(x[0]) * 2 ** 15 < 32767.0                           # rounding would give 32767
    assert np.array_equal(audio_io.to_int16(x), want)
    f, g = str(tmp_path / "t.wav"), str(tmp_path / "want.wav")
    audio_io.save_wave(x[None], f)
    wavfile.write(g, 44100, want)
    assert open(f, "rb").read() == open(g, "rb").read()
    audio_io.save_wave(x[None], str(tmp_path / "t.flac"))
    sr, back, bps = flac.read(str(tmp_path / "t.flac"))
    assert bps == 16 and np.array_equal(back[:, 0], want)
    assert wordlength.quantize_ref(x, 16, "none")[0].tolist() == [32767, -32767, 0, 0, 2, -2, 8192, -32768, 0, 32767]


def test_entry_point_declared_mapped_and_bound():
    hdr = open(os.path.join(ROOT, "include", "vfx_hip.h")).read()
    decl = re.search(r"int vfx_quantize_rows_f32\(([^;]*)\);", hdr).group(1)
    args = [" ".join(a.split()) for a in decl.split(",")]
    assert args == ["const float* x", "int64_t x_stride", "const int32_t* n_rows", "int B", "int64_t n_max", "const int64_t* n0",
                    "const int32_t* chan", "int bits", "int dither", "uint64_t seed", "void* out", "int64_t out_stride",
                    "int32_t* result", "vfx_stream_t stream"]
    P, I, L = C.c_void_p, C.c_int, C.c_int64
    assert _lib.SIGNATURES["vfx_quantize_rows_f32"] == (I, [P, L, P, I, L, P, P, I, I, C.c_uint64, P, L, P, P])
    vmap = open(os.path.join(ROOT, "voicefixer_amd", "csrc", "vfx.map")).read()
    assert "vfx_*;" in vmap and "vfx_quantize_rows_f32" in vmap
    mk = open(os.path.join(ROOT, "voicefixer_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*vfx_wordlength\.hip", mk, re.M) and "vfx_philox.h" in mk
    # one Philox: the header both translation units include
    csrc = os.path.join(ROOT, "voicefixer_amd", "csrc")
    assert "uint4 philox4x32_10(" in open(os.path.join(csrc, "vfx_philox.h")).read()
    for f in ("vfx_train.hip", "vfx_wordlength.hip"):
        src = open(os.path.join(csrc, f)).read()
        assert '#include "vfx_philox.h"' in src and "uint4 philox4x32_10(uint4" not in src, f


def test_library_refuses_bad_arguments_without_a_device():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    h = _lib.lib()
    assert hasattr(h, "vfx_quantize_rows_f32")
    p = C.c_void_p(16)
    good = [p, 100, p, 1, 100, None, None, 16, 1, 0, p, 100, p, None]
    for i, bad in ((0, None), (2, None), (10, None), (12, None), (3, -1), (3, 65536), (4, -1), (7, 8), (7, 20), (7, 32), (8, -1),
                   (8, 3), (1, 99), (11, 99)):
        a = list(good)
        a[i] = bad
        assert h.vfx_quantize_rows_f32(*a) == _lib.EINVAL, (i, bad)
    for i in (3, 4):                    # B == 0, n_max == 0: nothing to do, nothing launched (no device is touched)
        a = list(good)
        a[i] = 0
        before = h.vfx_launch_count()
        assert h.vfx_quantize_rows_f32(*a) == 0 and h.vfx_launch_count() == before


def test_cli_flags(tmp_path, monkeypatch):
    from voicefixer_amd import __main__ as cli
    a = cli.build_parser().parse_args(["-i", "x.wav", "--bit-depth", "24", "--dither", "hp", "--dither-seed", "5"])
    assert (a.bit_depth, a.dither, a.dither_seed) == (24, "hp", 5)
    a = cli.build_parser().parse_args(["-i", "x.wav", "--bit-depth", "16"])
    assert (a.bit_depth, a.dither, a.dither_seed) == (16, "tpdf", 0)
    a = cli.build_parser().parse_args(["-i", "x.wav"])
    assert a.bit_depth is None
    for bad in (["--dither", "hp"], ["--dither-seed", "3"], ["--dither", "none", "--dither-seed", "3"], ["--bit-depth", "8"],
                ["--bit-depth", "24", "--dither", "shaped"], ["--bit-depth", "16", "--dither-seed", "-1"],
                ["--bit-depth", "16", "--dither-seed", str(2 ** 64)]):
        with pytest.raises(SystemExit):
            cli.build_parser().parse_args(["-i", "x.wav"] + bad)

    seen = []

    class Stub:
        def restore_folder(self, infolder, outfolder, **kw):
            seen.append(("folder", kw))
            kw["stats"].update(files=0, failed=[], skipped=[])
            return []

        def restore(self, **kw):
            seen.append(("file", kw))

    monkeypatch.setattr(api, "VoiceFixer", Stub)
    ind, outd = tmp_path / "in", tmp_path / "out"
    ind.mkdir()
    (ind / "a.wav").write_bytes(b"")
    three = ("bit_depth", "dither", "dither_seed")
    assert cli.main(["-ifdr", str(ind), "-ofdr", str(outd), "--silent", "--bit-depth", "24", "--dither", "hp", "--dither-seed", "5"]) == 0
    assert {k: seen[-1][1][k] for k in three} == {"bit_depth": 24, "dither": "hp", "dither_seed": 5}
    assert cli.main(["-ifdr", str(ind), "-ofdr", str(outd), "--silent"]) == 0
    assert seen[-1][0] == "folder" and not set(three) & set(seen[-1][1])
    assert cli.main(["-i", str(ind / "a.wav"), "-o", str(outd / "a.flac"), "--silent", "--bit-depth", "16"]) == 0
    assert seen[-1][0] == "file" and {k: seen[-1][1][k] for k in three} == {"bit_depth": 16, "dither": "tpdf", "dither_seed": 0}
    assert cli.main(["-i", str(ind / "a.wav"), "-o", str(outd / "a.wav"), "--silent"]) == 0
    assert seen[-1][0] == "file" and not set(three) & set(seen[-1][1])
