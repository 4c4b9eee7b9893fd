"""Loudness normalisation on the MI355X (vfx_loudness_rows_f32): the kernel against the float64 definition at every common
rate with ragged rows, the cross-workgroup state carry on a 30-minute row, the sample-peak ceiling, and the public surface --
restore_inmem / restore_batch / the folder job / the CLI with ``loudness`` -- against float32(g) times the plain output."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import voicefixer_amd  # noqa: E402
from voicefixer_amd import _lib, audio_io, loudness, ops  # noqa: E402
from test_loudness_cpu import ref_loudness  # noqa: E402

RATES = [8000, 11025, 16000, 22050, 44100, 48000]


@pytest.fixture(scope="module")
def vf(seeded_states):
    return voicefixer_amd.VoiceFixer.from_state(*seeded_states)


@pytest.fixture(scope="module")
def utterance(vf):
    rng = np.random.default_rng(21)
    t = np.arange(3 * 44100) / 44100.0
    x = (0.05 * rng.standard_normal(t.size) * (1 + np.sin(2 * np.pi * 1.5 * t)) + 0.2 * np.sin(2 * np.pi * 180 * t))
    return vf.restore_inmem(x.astype(np.float32), cuda=True)[0]


def _hum(n, fs, seed):
    """Noise plus a strong 50 Hz hum under slow amplitude modulation: exercises the high-pass state across chunks."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / fs
    return ((0.1 * rng.standard_normal(n) * (0.55 + 0.45 * np.sin(2 * np.pi * 0.4 * t)) + 0.5 * np.sin(2 * np.pi * 50 * t))
            .astype(np.float32))


def _gain(L, peak, target, ceiling=-1.0):
    if not math.isfinite(L):
        return 1.0
    return min(10.0 ** ((target - L) / 20.0), 10.0 ** (ceiling / 20.0) / peak)


@pytest.mark.parametrize("fs", RATES)
def test_kernel_matches_float64(fs, utterance):
    hop = loudness.hop_length(fs)
    rows = [_hum(int(0.35 * fs), fs, 1),                      # under 400 ms
            np.zeros(int(1.7 * fs), np.float32),               # silence
            _hum(int(6.3 * fs) + 17, fs, 2),                  # hum + noise, several spans at low rates
            utterance[: int(2.9 * fs)].copy(),                # a restored seeded utterance (read as audio at fs)
            _hum(23 * hop + 1, fs, 3)]                        # exactly k * hop + 1 samples
    lens = [len(r) for r in rows]
    W = max(lens) + 40
    x = np.full((5, W), np.nan, np.float32)                   # NaN canaries past every row end
    for r, v in enumerate(rows):
        x[r, :lens[r]] = v
    xd = torch.from_numpy(x).cuda()
    n_rows = torch.tensor(lens, dtype=torch.int32, device="cuda")
    lib = _lib.lib()
    before = lib.vfx_launch_count()
    res = ops.loudness_rows(xd, n_rows, fs, target=-20.0, ceiling_db=-1.0).cpu().numpy()   # (in place)
    got = xd.cpu().numpy()
    assert lib.vfx_launch_count() - before <= 4
    worst = 0.0
    for r in range(5):
        L, g, pk = res[r]
        want = ref_loudness(x[r, :lens[r]], fs)
        assert pk == np.abs(x[r, :lens[r]]).max(), (fs, r)
        if math.isinf(want):
            assert L == -math.inf and g == 1.0, (fs, r, L)
            assert np.array_equal(got[r, :lens[r]], x[r, :lens[r]]), (fs, r)        # untouched
        else:
            worst = max(worst, abs(L - want))
            assert abs(L - want) <= 0.005, (fs, r, L, want)
            assert g == pytest.approx(_gain(L, pk, -20.0), rel=1e-12)
            assert np.array_equal(got[r, :lens[r]], np.float32(g) * x[r, :lens[r]]), (fs, r)
        assert np.all(np.isnan(got[r, lens[r]:])), (fs, r)       # nothing written past a row end
    assert res[0, 0] == -math.inf and res[1, 0] == -math.inf
    print("loudness %d Hz: max |dL| vs float64 %.2e LU" % (fs, worst))
    # measure only: 3 launches, nothing written
    before = lib.vfx_launch_count()
    xm = torch.from_numpy(x).cuda()
    res2 = ops.loudness_rows(xm, n_rows, fs).cpu().numpy()
    assert lib.vfx_launch_count() - before == 3
    assert np.array_equal(res2[:, 0], res[:, 0]) and np.all(res2[:, 1] == 1.0)
    assert np.array_equal(xm.cpu().numpy(), x, equal_nan=True)
    # a row measured alone gives the same bits as inside the ragged batch
    alone = ops.loudness_rows(torch.from_numpy(x[3:4, :lens[3]].copy()).cuda(),
                              n_rows[3:4].clone(), fs).cpu().numpy()
    assert np.array_equal(alone[0, [0, 2]], res[3, [0, 2]])
    # bad arguments: EINVAL, nothing launched
    p = loudness.plan(fs)
    before = lib.vfx_launch_count()
    import ctypes as C
    coef = (C.c_double * 10)(*p["coef"])
    ws = torch.empty((1024,), dtype=torch.float64, device="cuda")
    out = torch.empty((5, W), device="cuda")
    args = [ops._ptr(xd), W, ops._ptr(n_rows), 5, W, coef, ops._ptr(ws), p["S"], hop, p["lookback"], -20.0, -1.0,
            ops._ptr(out), W, ops._ptr(ws), ops._ptr(ws), 8 * 1024, None]
    for i, bad in ((7, 48), (8, p["S"] - 1), (9, 0), (3, 0), (1, W - 1), (10, float("inf")), (16, 8), (12, None)):
        a = list(args)
        a[i] = bad
        assert lib.vfx_loudness_rows_f32(*a) == _lib.EINVAL, i
    assert lib.vfx_loudness_rows_f32(*args) == _lib.EINVAL               # workspace too small
    assert lib.vfx_launch_count() == before


def test_30_minute_row_at_44k():
    fs = 44100
    n = 30 * 60 * fs
    x = _hum(n, fs, 30)
    x[: 5 * fs] *= 0.01                                       # a quiet start: the gates have work to do
    res = ops.loudness_rows(torch.from_numpy(x).cuda()[None], torch.tensor([n], dtype=torch.int32, device="cuda"),
                            fs).cpu().numpy()
    want = ref_loudness(x, fs)
    print("30 min row: L %.5f LUFS, float64 %.5f, dL %.2e" % (res[0, 0], want, res[0, 0] - want))
    assert abs(res[0, 0] - want) <= 0.005


def test_ceiling_binds_on_sparse_clicks():
    fs = 44100
    x = np.zeros(5 * fs, np.float32)
    x[:: fs // 4] = 0.5
    x[1:: fs // 4] = -0.3
    xd = torch.from_numpy(x).cuda()[None].contiguous()
    res = ops.loudness_rows(xd, torch.tensor([x.size], dtype=torch.int32, device="cuda"), fs, target=-10.0,
                            ceiling_db=-1.0).cpu().numpy()
    y = xd[0].cpu().numpy()
    L, g, pk = res[0]
    assert g == pytest.approx(10 ** (-1 / 20) / 0.5, rel=1e-12) and g < 10 ** ((-10 - L) / 20)
    assert abs(float(np.abs(y).max()) - 10 ** (-1 / 20)) <= 1e-7
    assert ref_loudness(y, fs) < -10.0


def _expected(plain, target, ceiling=-1.0, fs=44100):
    L = voicefixer_amd.measure_loudness(plain, sample_rate=fs)
    return np.float32(_gain(L, float(np.abs(plain).max()), target, ceiling)) * plain


@pytest.mark.parametrize("case", ["44k", "48k", "mode1", "61s"])
def test_restore_inmem_loudness(vf, case):
    rng = np.random.default_rng(61)
    n = 61 * 44100 if case == "61s" else 3 * 44100
    x = (0.02 * rng.standard_normal(n)).astype(np.float32)
    kw = {"output_sample_rate": 48000} if case == "48k" else ({"mode": 1} if case == "mode1" else {})
    fs = 48000 if case == "48k" else 44100
    plain = vf.restore_inmem(x, cuda=True, **kw)
    got = vf.restore_inmem(x, cuda=True, loudness=-16, **kw)
    assert got.shape == plain.shape
    assert np.array_equal(got[0], _expected(plain[0], -16.0, fs=fs))
    L = ref_loudness(got[0], fs)
    limited = abs(float(np.abs(got).max()) - 10 ** (-1 / 20)) <= 1e-6
    print("restore_inmem(%s, loudness=-16): %.4f LUFS%s" % (case, L, " (ceiling)" if limited else ""))
    assert abs(L + 16.0) <= 0.01 or (limited and L < -16.0)


def test_restore_batch_loudness(vf):
    rng = np.random.default_rng(23)
    lens = [30000, 52000, 41000, 44100 * 2, 36000]
    wavs = [(a * rng.standard_normal(n)).astype(np.float32) for a, n in zip((0.01, 0.3, 0.05, 0.1, 0.2), lens)]
    plain = vf.restore_batch(wavs, batch_size=8)
    outs = vf.restore_batch(wavs, batch_size=8, loudness=-23)
    for w, p, o in zip(wavs, plain, outs):
        assert np.array_equal(o[0], _expected(p[0], -23.0))            # the row's own measurement, whatever its batch
        one = vf.restore_inmem(w, cuda=True, loudness=-23)
        assert o.shape == one.shape
        assert abs(ref_loudness(o[0], 44100) - ref_loudness(one[0], 44100)) <= 1e-3
    with pytest.raises(NotImplementedError):
        vf.restore_stream(wavs[3], loudness=-16)


def _level_folder(d, n_files=12):
    from scipy.io import wavfile
    os.makedirs(d)
    rng = np.random.default_rng(12)
    for k, db in enumerate(np.linspace(-40, -6, n_files)):
        n = int(44100 * (1.0 + 0.15 * k))
        t = np.arange(n) / 44100
        v = rng.standard_normal(n) * 0.3 + np.sin(2 * np.pi * 200 * t)
        v = v / np.abs(v).max() * 10 ** (db / 20)
        wavfile.write(os.path.join(d, "f%02d.wav" % k), 44100, np.round(v * 32767).astype(np.int16))


def _check_outputs(folder, names, stats=None):
    from scipy.io import wavfile
    rep = {n: (L0, gdb) for n, L0, gdb in stats["loudness"]} if stats is not None else {}
    for name in names:
        sr, pcm = wavfile.read(os.path.join(folder, name))
        assert sr == 44100 and pcm.dtype == np.int16
        y = pcm.astype(np.float64) / 32768.0
        L = ref_loudness(y, sr)
        limited = abs(np.abs(y).max() - 10 ** (-1 / 20)) <= 2.0 / 32768
        assert abs(L + 16.0) <= 0.05 or (limited and L < -16.0), (name, L)
        if name in rep:
            L0, gdb = rep[name]
            assert abs((L0 + gdb) - L) <= 0.05 or limited, (name, L0, gdb, L)


def test_folder_job_and_cli(vf, seeded_states, tmp_path, monkeypatch):
    ind = str(tmp_path / "in")
    _level_folder(ind)
    lib = _lib.lib()
    st0, st1 = {}, {}
    c0 = lib.vfx_launch_count()
    plain = vf.restore_folder(ind, str(tmp_path / "plain"), batch_size=32, io_threads=2, stats=st0)
    c1 = lib.vfx_launch_count()
    names = vf.restore_folder(ind, str(tmp_path / "loud"), batch_size=32, io_threads=2, stats=st1, loudness=-16)
    c2 = lib.vfx_launch_count()
    assert plain == names and len(names) == 12 and st1["failed"] == []
    assert st0["loudness"] == [] and sorted(n for n, _, _ in st1["loudness"]) == names
    assert (c2 - c1) - (c1 - c0) == 4 * st1["batches"]         # loudness=None adds no launch; with it, 4 per batch
    _check_outputs(str(tmp_path / "loud"), names, st1)
    # the CLI, with the default constructor's checkpoint files holding the seeded weights
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
    assert cli.main(["-ifdr", ind, "-ofdr", out, "--loudness", "-16", "--silent"]) == 0
    assert sorted(os.listdir(out)) == names
    _check_outputs(out, names)
    one = str(tmp_path / "one.wav")
    assert cli.main(["-i", os.path.join(ind, "f00.wav"), "-o", one, "--loudness", "-16", "--peak-ceiling", "-1",
                     "--silent"]) == 0
    _check_outputs(str(tmp_path), ["one.wav"])


def test_measure_loudness_api():
    fs = 48000
    t = np.arange(20 * fs) / fs
    x = (0.1 * np.sin(2 * np.pi * 997 * t)).astype(np.float32)
    L = voicefixer_amd.measure_loudness(x, sample_rate=fs)
    assert isinstance(L, float) and abs(L + 23.0103) <= 0.005
    Ls = voicefixer_amd.measure_loudness([x, np.zeros(100, np.float32), x[: fs * 2]], sample_rate=fs)
    assert Ls[0] == L and Ls[1] == -math.inf and abs(Ls[2] + 23.0103) <= 0.01
    assert audio_io is not None
