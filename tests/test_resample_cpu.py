"""Rate conversion without a GPU: the C ABI of the device resampler (vfx_resample_rows_f32) is declared and bound, the sum it
evaluates -- restated in float64 from the shared bank helper -- is scipy's resample_poly with resample_hq's filter, the host
resampler built on that helper did not move, and the CLI takes the new flags."""
import os
import re

import numpy as np
import pytest

from voicefixer_amd import audio_io, _lib
from conftest import GOLDEN, ROOT

# (input rate, output rate) -> (up, down, J): the conversions that matter (8 / 16 / 22.05 / 24 / 32 / 48 / 96 kHz inputs,
# 48 and 16 kHz outputs)
PAIRS = {(8000, 44100): (441, 80, 188), (16000, 44100): (441, 160, 188), (32000, 44100): (441, 320, 188),
         (22050, 44100): (2, 1, 188), (24000, 44100): (147, 80, 188), (48000, 44100): (147, 160, 205),
         (96000, 44100): (147, 320, 408), (44100, 48000): (160, 147, 188), (44100, 16000): (160, 441, 517)}


def device_sum_f64(x, up, down, bank, J, c):
    """The kernel's sum in float64: y[m] = sum_i bank[p][i] * x[lo + i], pos = c + m*down, kmax = pos // up,
    p = pos mod up, lo = kmax - J + 1, m < ceil(n * up / down), x zero outside [0, n)."""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    ny = -(-n * up // down)
    m = np.arange(ny, dtype=np.int64)
    pos = c + m * down
    kmax = pos // up
    p = pos - kmax * up
    idx = (kmax - J + 1)[:, None] + np.arange(J)[None]
    xv = np.where((idx >= 0) & (idx < n), x[np.clip(idx, 0, max(n - 1, 0))], 0.0)
    return np.sum(bank[p] * xv, axis=1)


def test_header_declares_and_lib_binds_the_entry_point():
    hdr = open(os.path.join(ROOT, "include", "vfx_hip.h")).read()
    assert re.search(r"int vfx_resample_rows_f32\(", hdr)
    assert "vfx_resample_rows_f32" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["vfx_resample_rows_f32"]
    assert len(args) == 15
    assert "vfx_resample_poly_f32" not in hdr       # (the host library's name stays the host library's)
    mk = open(os.path.join(ROOT, "voicefixer_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*vfx_resample\.hip", mk, re.M)
    assert re.search(r"^check_no_pk_fma: .*vfx_resample\.o", mk, re.M) and '"vfx_resample:."' in mk


def test_bank_layout_is_the_host_resamplers():
    """bank[p][J - 1 - j] = g[p + j * up] (zero past L): the loop of csrc_host/vfx_resample.c, and the sizes of the table."""
    for (a, b), (up, down, J) in PAIRS.items():
        assert audio_io.rate_ratio(a, b) == (up, down)
        h, g = audio_io.hq_filter(up, down)
        bank, J2, c = audio_io.hq_bank(up, down)
        L = g.shape[0]
        assert J2 == J == -(-L // up) and c == (L - 1) // 2 and bank.shape == (up, J) and bank.dtype == np.float32
        want = np.zeros((up, J), np.float32)
        for p in range(up):
            for j in range(J):
                t = p + j * up
                want[p, J - 1 - j] = g[t] if t < L else 0.0
        assert np.array_equal(bank, want), (a, b)


@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_device_sum_equals_resample_poly(pair):
    """The float64 restatement of the kernel's sum, driven by the shared helper, is scipy.signal.resample_poly with
    resample_hq's window: the alignment c and the ceil length are pinned, for n = 1, n < J and n >> J."""
    from scipy.signal import resample_poly
    up, down, J = PAIRS[pair]
    h, _ = audio_io.hq_filter(up, down)
    bank, J2, c = audio_io.polyphase_bank(h * up, up)
    assert J2 == J
    rng = np.random.default_rng(sum(pair))
    for n in (1, 2, J // 3, J - 1, 40 * J):
        x = rng.uniform(-1, 1, n)
        got = device_sum_f64(x, up, down, bank, J, c)
        want = resample_poly(x, up, down, window=h)
        assert got.shape == want.shape == (audio_io.converted_length(n, *pair),)
        assert np.max(np.abs(got - want)) <= 1e-12, (pair, n)


def test_resample_hq_is_bit_identical_to_before():
    """The host default did not move: resample_hq (now built on hq_filter) returns the bits recorded from the previous tree."""
    from voicefixer_amd import flac
    assert flac.native() is not None, "libvfx_audio.so is built by build()"
    g = np.load(os.path.join(GOLDEN, "resample_hq_host.npz"))
    for a, b in PAIRS:
        x, want = g["x_%d_%d" % (a, b)], g["y_%d_%d" % (a, b)]
        got = audio_io.resample_hq(x, a, b)
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (a, b)


def test_wav_length_is_the_converted_length(tmp_path):
    from scipy.io import wavfile
    for sr, n in ((16000, 12345), (48000, 7), (22050, 1000)):
        p = str(tmp_path / ("x%d.wav" % sr))
        wavfile.write(p, sr, np.zeros(n, np.int16))
        assert audio_io.wav_info(p) == (sr, n, n)
        assert audio_io.wav_length(p, 44100) == audio_io.converted_length(n, sr, 44100) == -(-n * 44100 // sr)
        x, sr2 = audio_io.load_wav_native(p)
        assert sr2 == sr and x.shape == (n,)


def test_rate_arguments_are_checked():
    from voicefixer_amd import api
    assert api._output_rate(None) == 44100 and api._output_rate(48000) == 48000
    for bad in (0, -16000, 44100.5, True):
        with pytest.raises(ValueError):
            api._check_rate(bad)
    assert api._row_rates(16000, 3) == [16000] * 3 and api._row_rates([8000, 44100], 2) == [8000, 44100]
    with pytest.raises(ValueError):
        api._row_rates([8000], 2)


def test_cli_parses_the_rate_flags():
    from voicefixer_amd import __main__ as cli
    a = cli.build_parser().parse_args(["-ifdr", "in"])
    assert a.output_sample_rate is None and a.resample_on_device is False
    a = cli.build_parser().parse_args(["-ifdr", "in", "--output-sample-rate", "48000", "--resample-on-device"])
    assert a.output_sample_rate == 48000 and a.resample_on_device is True
    for bad in ("0", "-8000"):
        with pytest.raises(SystemExit):
            cli.build_parser().parse_args(["-ifdr", "in", "--output-sample-rate", bad])
