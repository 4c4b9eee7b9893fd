"""Rate conversion on the MI355X (vfx_resample_rows_f32): the kernel against the float64 sum for every conversion that
matters, 64-bit positions on a long row, and the public surface -- any-rate input, chosen-rate output, mixed-rate batches,
the folder job with resample_on_device and the CLI flags -- against the host-resampled path."""
import os
import struct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import voicefixer_amd  # noqa: E402
from voicefixer_amd import audio_io, ops, _lib  # noqa: E402
from test_resample_cpu import PAIRS, device_sum_f64  # noqa: E402


@pytest.fixture(scope="module")
def vf(seeded_states):
    return voicefixer_amd.VoiceFixer.from_state(*seeded_states)


def _rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


def _ref64(x, pair):
    up, down, _ = PAIRS[pair]
    h, _ = audio_io.hq_filter(up, down)
    bank, J, c = audio_io.polyphase_bank(h * up, up)
    return device_sum_f64(x, up, down, bank, J, c)


@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_kernel_matches_float64(pair):
    """B = 4 ragged rows (one shorter than J), rows 0, 1, 3 listed, row 2 not: NaN beyond every row's end in x must not
    leak, y beyond every row's converted length and the unlisted row stay untouched (NaN), max abs error <= 2e-6 on
    unit-peak noise."""
    up, down, J = PAIRS[pair]
    rng = np.random.default_rng(up * 1000 + down)
    lens = [J // 2, 3001, 1777, 4000]
    W = max(lens) + 64
    x = np.full((4, W), np.nan, np.float32)
    for r, n in enumerate(lens):
        v = rng.uniform(-1, 1, n)
        x[r, :n] = v / np.abs(v).max()
    ny = [audio_io.converted_length(n, *pair) for n in lens]
    Wy = max(ny) + 32
    xd = torch.from_numpy(x).cuda()
    yd = torch.full((4, Wy), float("nan"), device="cuda")
    n_rows = torch.tensor(lens, dtype=torch.int32, device="cuda")
    listed = [0, 1, 3]
    before = _lib.lib().vfx_launch_count()
    ops.resample_rows(xd, n_rows, yd, up, down, row_index=torch.tensor(listed, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    assert _lib.lib().vfx_launch_count() == before + 1
    y = yd.cpu().numpy()
    worst = 0.0
    for r in listed:
        ref = _ref64(x[r, :lens[r]], pair)
        assert ref.shape == (ny[r],)
        assert np.all(np.isfinite(y[r, :ny[r]])), (pair, r)
        assert np.all(np.isnan(y[r, ny[r]:])), (pair, r)
        worst = max(worst, float(np.max(np.abs(y[r, :ny[r]] - ref))))
    assert np.all(np.isnan(y[2]))
    print("resample %s: max abs error vs float64 %.3g" % (pair, worst))
    assert worst <= 2e-6, (pair, worst)
    # bad arguments are refused, nothing is launched
    lib = _lib.lib()
    assert lib.vfx_resample_rows_f32(None, W, None, 4, None, 4, None, J, up, down, 0, None, Wy, Wy, None) == _lib.EINVAL


def test_long_row_positions_past_2_31():
    """6 minutes at 44.1 kHz -> 16 kHz: c + m * down passes 2^31 at m ~ 4.87 M; outputs beyond that and the last ones are
    checked against float64 (evaluated for those outputs only)."""
    pair = (44100, 16000)
    up, down, J = PAIRS[pair]
    n = 6 * 60 * 44100
    g = torch.Generator().manual_seed(5)
    xt = torch.rand(n, generator=g) * 2 - 1
    x = xt.numpy()
    ny = audio_io.converted_length(n, *pair)
    yd = torch.empty((1, ny), device="cuda")
    ops.resample_rows(xt[None].cuda(), torch.tensor([n], dtype=torch.int32, device="cuda"), yd, up, down)
    y = yd[0].cpu().numpy()
    h, _ = audio_io.hq_filter(up, down)
    bank, J2, c = audio_io.polyphase_bank(h * up, up)
    m0 = (2 ** 31 - c) // down + 1
    assert c + m0 * down > 2 ** 31 and m0 < ny
    for start in (m0 - 5, m0 + 400_000, ny - 300):
        m = np.arange(start, min(start + 300, ny), dtype=np.int64)
        pos = c + m * down
        kmax = pos // up
        idx = (kmax - J + 1)[:, None] + np.arange(J)[None]
        xv = np.where(idx < n, x.astype(np.float64)[np.clip(idx, 0, n - 1)], 0.0)
        ref = np.sum(bank[pos - kmax * up] * xv, axis=1)
        assert np.max(np.abs(y[m] - ref)) <= 2e-6, start


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_restore_inmem_at_16k_converts_on_the_device(vf, mode, monkeypatch):
    rng = np.random.default_rng(16)
    t = np.arange(24000) / 16000.0
    x16 = (0.05 * rng.standard_normal(24000) + 0.3 * np.sin(2 * np.pi * 220 * t)).astype(np.float32)
    kw = {"seed": 99} if mode == 2 else {}
    want = vf.restore_inmem(audio_io.resample_hq(x16, 16000, 44100), cuda=True, mode=mode, **kw)

    def no_host(*a, **k):
        raise AssertionError("the host resampler ran")
    monkeypatch.setattr(audio_io, "resample_hq", no_host)
    got = vf.restore_inmem(x16, cuda=True, mode=mode, sample_rate=16000, **kw)
    assert got.shape == want.shape
    rms = _rms(got, want)
    print("mode %d: restore_inmem(16 kHz, device conversion) vs host conversion: waveform RMS %.3g" % (mode, rms))
    assert rms <= 1e-4


def test_output_at_48k_and_the_peak_rule(vf, tmp_path):
    rng = np.random.default_rng(48)
    x = (0.1 * rng.standard_normal(60000)).astype(np.float32)
    y44 = vf.restore_inmem(x, cuda=True)
    want = audio_io.resample_hq(y44[0], 44100, 48000)
    pk = np.abs(want).max()
    want = want / pk if pk > 1 else want
    got = vf.restore_inmem(x, cuda=True, output_sample_rate=48000)
    assert got.shape == (1, audio_io.converted_length(60000, 44100, 48000))
    assert np.max(np.abs(got[0] - want)) <= 2e-6
    # a plugin vocoder that returns a full-scale square wave: the reference's peak rule leaves it alone (peak == 1), the
    # band-limited conversion overshoots 1.0 -- the converted row is scaled back, and the written PCM16 is full scale
    def square(mel):
        L = 441 * (mel.shape[2] + 6)
        return torch.from_numpy(np.where((np.arange(L) // 200) % 2 == 0, 1.0, -1.0).astype(np.float32))[None, None]
    sq44 = vf.restore_inmem(x, cuda=True, your_vocoder_func=square)
    assert np.abs(sq44).max() == 1.0
    raw = audio_io.resample_hq(sq44[0], 44100, 48000)
    assert np.abs(raw).max() > 1.0
    sq48 = vf.restore_inmem(x, cuda=True, your_vocoder_func=square, output_sample_rate=48000)
    assert np.abs(sq48).max() <= 1.0 and np.max(np.abs(sq48[0] - raw / np.abs(raw).max())) <= 2e-6
    fin, fout = str(tmp_path / "in.wav"), str(tmp_path / "out.wav")
    audio_io.save_wave(x[None], fin)
    vf.restore(fin, fout, your_vocoder_func=square, output_sample_rate=48000)
    from scipy.io import wavfile
    sr, pcm = wavfile.read(fout)
    assert sr == 48000 and pcm.dtype == np.int16 and np.abs(pcm.astype(np.int32)).max() >= 32000


def test_mixed_rate_restore_batch(vf):
    """Rows at 8, 16, 22.05, 44.1 and 48 kHz in one ragged batch (one conversion launch per rate pair) equal the same
    files restored one at a time."""
    rng = np.random.default_rng(5)
    rates = [8000, 16000, 22050, 44100, 48000, 16000]
    secs = [1.3, 1.1, 1.2, 1.0, 1.4, 1.25]
    wavs = [(0.1 * rng.standard_normal(int(s * r))).astype(np.float32) for s, r in zip(secs, rates)]
    before = _lib.lib().vfx_launch_count()
    outs = vf.restore_batch(wavs, batch_size=8, sample_rate=rates)
    batched = _lib.lib().vfx_launch_count() - before
    for w, r, o in zip(wavs, rates, outs):
        one = vf.restore_inmem(w, cuda=True, sample_rate=r)
        assert o.shape == one.shape == (1, audio_io.converted_length(len(w), r, 44100))
        assert _rms(o, one) < 2e-5
    single = (_lib.lib().vfx_launch_count() - before - batched) / len(wavs)
    assert batched < 1.5 * single                     # one ragged batch
    outs48 = vf.restore_batch(wavs, batch_size=8, sample_rate=rates, output_sample_rate=48000)
    for w, r, o, o44 in zip(wavs, rates, outs48, outs):
        assert o.shape == (1, audio_io.converted_length(o44.shape[1], 44100, 48000))
    with pytest.raises(ValueError):
        vf.restore_batch(wavs, sample_rate=rates[:2])
    with pytest.raises(NotImplementedError):
        vf.restore_stream(wavs[3], output_sample_rate=48000)


def test_restore_stream_converts_the_input_once(vf, monkeypatch):
    rng = np.random.default_rng(7)
    x16 = (0.1 * rng.standard_normal(16000 * 3)).astype(np.float32)
    want = vf.restore_stream(audio_io.resample_hq(x16, 16000, 44100), chunk_seconds=1.5, overlap_seconds=0.25)
    monkeypatch.setattr(audio_io, "resample_hq", lambda *a, **k: (_ for _ in ()).throw(AssertionError("host resampler")))
    got = vf.restore_stream(x16, chunk_seconds=1.5, overlap_seconds=0.25, sample_rate=16000)
    assert got.shape == want.shape and _rms(got, want) <= 1e-4


def _rate_folder(d):
    """8 kHz WAV, 16 kHz FLAC, 48 kHz stereo WAV, 44.1 kHz WAV, a 16 kHz WAV cut short of what its header promises, and a
    file that is no WAV at all."""
    from scipy.io import wavfile
    from voicefixer_amd import flac
    os.makedirs(d)
    rng = np.random.default_rng(3)

    def sig(n, sr):
        t = np.arange(n) / sr
        return 0.05 * rng.standard_normal(n) + 0.3 * np.sin(2 * np.pi * 180 * t)
    pcm = lambda v: np.clip(np.round(v * 32767), -32768, 32767).astype(np.int16)
    wavfile.write(os.path.join(d, "a8k.wav"), 8000, pcm(sig(9000, 8000)))
    flac.write(os.path.join(d, "b16k.flac"), pcm(sig(20000, 16000))[:, None], 16000, 16)
    wavfile.write(os.path.join(d, "c48k.wav"), 48000, pcm(np.stack([sig(60000, 48000), sig(60000, 48000)], 1)))
    wavfile.write(os.path.join(d, "d44k.wav"), 44100, pcm(sig(50000, 44100)))
    p = os.path.join(d, "e16k_trunc.wav")
    wavfile.write(p, 16000, pcm(sig(30000, 16000)))
    with open(p, "rb") as f:
        raw = f.read()
    with open(p, "wb") as f:
        f.write(raw[:44 + 2 * 21000])                 # the header still promises 30000 samples
    with open(os.path.join(d, "f_bad.wav"), "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 4) + b"JUNK")


def test_folder_job_with_device_resampling(vf, tmp_path):
    import warnings
    from scipy.io import wavfile
    ind = str(tmp_path / "in")
    _rate_folder(ind)
    ext = (".wav", ".flac")
    st_h, st_d, st_48 = {}, {}, {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        host = vf.restore_folder(ind, str(tmp_path / "host"), batch_size=8, io_threads=2, extensions=ext, stats=st_h)
        dev = vf.restore_folder(ind, str(tmp_path / "dev"), batch_size=8, io_threads=2, extensions=ext, stats=st_d,
                                resample_on_device=True)
        o48 = vf.restore_folder(ind, str(tmp_path / "o48"), batch_size=8, io_threads=2, extensions=ext, stats=st_48,
                                resample_on_device=True, output_sample_rate=48000)
    assert host == dev == o48 == ["a8k.wav", "b16k.flac", "c48k.wav", "d44k.wav", "e16k_trunc.wav"]
    assert st_h["failed"] == st_d["failed"] == st_48["failed"] and [n for n, _ in st_h["failed"]] == ["f_bad.wav"]
    assert st_h["resample_worker_s"] > 0 and st_d["resample_worker_s"] == 0.0
    for name in host:
        a, sa = audio_io.load_wav_native(str(tmp_path / "host" / name))
        b, sb = audio_io.load_wav_native(str(tmp_path / "dev" / name))
        assert sa == sb == 44100 and a.shape == b.shape, name
        assert np.max(np.abs(a - b)) * 32768 <= 2, name
        c, sc = audio_io.load_wav_native(str(tmp_path / "o48" / name))
        assert sc == 48000 and c.shape == (audio_io.converted_length(a.shape[0], 44100, 48000),), name
    assert wavfile.read(str(tmp_path / "dev" / "e16k_trunc.wav"))[1].shape[0] == audio_io.converted_length(21000, 16000, 44100)


def test_cli_device_resampling_and_output_rate(vf, seeded_states, tmp_path, monkeypatch):
    from voicefixer_amd import __main__ as cli
    vsd, rsd = seeded_states
    home = str(tmp_path / "home")              # the default constructor's checkpoint files, holding the seeded weights
    a = os.path.join(home, ".cache/voicefixer/analysis_module/checkpoints")
    v = os.path.join(home, ".cache/voicefixer/synthesis_module/44100")
    os.makedirs(a)
    os.makedirs(v)
    torch.save({"generator": vsd}, os.path.join(v, "model.ckpt-1490000_trimed.pt"))
    torch.save({"generator." + k: t for k, t in rsd.items()}, os.path.join(a, "vf.ckpt"))
    monkeypatch.setenv("HOME", home)
    ind = str(tmp_path / "in")
    _rate_folder(ind)
    os.remove(os.path.join(ind, "f_bad.wav"))
    out = str(tmp_path / "out")
    assert cli.main(["-ifdr", ind, "-ofdr", out, "--resample-on-device", "--output-sample-rate", "48000", "--silent"]) == 0
    ref = str(tmp_path / "ref")
    vf.restore_folder(ind, ref, batch_size=32, resample_on_device=True, output_sample_rate=48000)
    assert sorted(os.listdir(out)) == sorted(os.listdir(ref)) == ["a8k.wav", "c48k.wav", "d44k.wav", "e16k_trunc.wav"]
    for name in os.listdir(out):
        a, sa = audio_io.load_wav_native(os.path.join(out, name))
        b, _ = audio_io.load_wav_native(os.path.join(ref, name))
        assert sa == 48000 and a.shape == b.shape and np.max(np.abs(a - b)) * 32768 <= 1, name
    one = str(tmp_path / "one.flac")
    assert cli.main(["-i", os.path.join(ind, "a8k.wav"), "-o", one, "--resample-on-device", "--output-sample-rate", "16000",
                     "--silent"]) == 0
    y, sr = audio_io.load_wav_native(one)
    assert sr == 16000 and y.shape == (audio_io.converted_length(audio_io.converted_length(9000, 8000, 44100), 44100, 16000),)
