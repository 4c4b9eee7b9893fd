"""Mode 2 on the MI355X: the train-mode kernels (vfx_bn_stats_f32, vfx_bn_apply_f32, vfx_dropout_f32) against float64 /
the numpy specification, the train-mode restorer against the float64 restatement (tests/train_reference.py, itself pinned
against the reference's own modules by test_train_mode_cpu.py), and the API / folder contract."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import voicefixer_amd  # noqa: E402
from voicefixer_amd import audio_io, dropout, engine, ops  # noqa: E402

import train_reference as tref  # noqa: E402


@pytest.fixture(scope="module")
def vf(seeded_states):
    return voicefixer_amd.VoiceFixer.from_state(*seeded_states)


def _rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


def _map(B, C, H, lp, rows_h, rng):
    """A guarded (B,C,H*P) pitch map whose guard, spare column and rows past each row's extent hold NaN."""
    P = 1 << lp
    v = ops.guarded(B, C, H * P, P + 8, "cuda")
    v._vfx_base.fill_(float("nan"))
    x = rng.standard_normal((B, C, H, P)).astype(np.float32)
    x[..., P - 1] = np.nan
    for b, h in enumerate(rows_h):
        x[b, :, h:] = np.nan
    x[0, 0, :, :] = 1e3 + 1e-2 * x[0, 0, :, :]         # mean 1e3, std 1e-2
    v.copy_(torch.from_numpy(x.reshape(B, C, H * P)))
    rows = torch.tensor([h * P for h in rows_h], dtype=torch.int32, device="cuda")
    return ops.with_rows(v, rows), x


@pytest.mark.parametrize("lp", [1, 2, 3, 4, 5, 6, 7])
def test_bn_stats_and_apply_maps(lp):
    rng = np.random.default_rng(lp)
    B, C, H = 3, 5, 40 if lp > 1 else 6
    rows_h = [H, H // 2 + 1, 2]
    x, xh = _map(B, C, H, lp, rows_h, rng)
    P = 1 << lp
    gamma = torch.from_numpy(rng.uniform(0.5, 2, C).astype(np.float32)).cuda()
    beta = torch.from_numpy(rng.standard_normal(C).astype(np.float32)).cuda()
    sc, sh = torch.empty(B * C, device="cuda"), torch.empty(B * C, device="cuda")
    ops.bn_stats(x, H * P, lp, gamma, beta, sc, sh)
    sc2, sh2 = torch.empty_like(sc), torch.empty_like(sh)
    ops.bn_stats(x, H * P, lp, gamma, beta, sc2, sh2)
    y = ops.guarded(B, C, H * P, P + 8, "cuda")
    y._vfx_base.fill_(7.0)
    ops.bn_apply(x, y, H * P, lp, sc, sh, slope=0.01)
    torch.cuda.synchronize()
    assert torch.equal(sc, sc2) and torch.equal(sh, sh2)            # deterministic
    assert torch.isfinite(sc).all() and torch.isfinite(sh).all()    # no NaN from guard / spare column / past-extent rows
    g, be = gamma.cpu().double().numpy(), beta.cpu().double().numpy()
    yh = y.cpu().numpy().reshape(B, C, H, P)
    for b, h in enumerate(rows_h):
        reg = xh[b, :, :h, :P - 1].astype(np.float64)
        mean, var = reg.mean(axis=(1, 2)), reg.var(axis=(1, 2))
        a = g / np.sqrt(var + 1e-5)
        np.testing.assert_allclose(sc[b * C:(b + 1) * C].cpu().numpy(), a, rtol=2e-5)
        np.testing.assert_allclose(sh[b * C:(b + 1) * C].cpu().numpy(), be - mean * a, rtol=2e-4, atol=2e-4)
        want = reg * a[:, None, None] + (be - mean * a)[:, None, None]
        want = np.where(want > 0, want, 0.01 * want)
        # y = x * scale + shift in fp32: the bound grows with |x * scale| (the mean-1e3 channel cancels ~1e5 against ~1e5)
        bound = 1e-3 + 1e-4 * np.abs(want) + 4e-7 * np.abs(reg * a[:, None, None])
        assert np.all(np.abs(yh[b, :, :h, :P - 1] - want) <= bound)
        assert np.all(yh[b, :, :h, P - 1] == 0.0)                     # the structural zero column


def test_bn_stats_1d_single_channel():
    rng = np.random.default_rng(3)
    B, C, L = 3, 512, 301
    v = ops.guarded(B, C, L, 64, "cuda")
    v._vfx_base.fill_(float("nan"))
    x = rng.standard_normal((B, C, L)).astype(np.float32) * 3 + 5
    v[:, :, :L].copy_(torch.from_numpy(x))
    T = [301, 150, 65]
    for b, t in enumerate(T):
        v[b, :, t:] = float("nan")
    ops.with_rows(v, torch.tensor(T, dtype=torch.int32, device="cuda"))
    gamma, beta = torch.tensor([1.3], device="cuda"), torch.tensor([-0.2], device="cuda")
    sc, sh = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
    ops.bn_stats(v, L, 0, gamma, beta, sc, sh)
    ops.bn_apply(v, v, L, 0, sc, sh)
    torch.cuda.synchronize()
    for b, t in enumerate(T):
        reg = x[b, :, :t].astype(np.float64)
        a = 1.3 / np.sqrt(reg.var() + 1e-5)
        assert abs(sc[b].item() - a) < 2e-5 * a and abs(sh[b].item() - (-0.2 - reg.mean() * a)) < 1e-4
        np.testing.assert_allclose(v[b, :, :t].cpu().numpy(), reg * a - 0.2 - reg.mean() * a, rtol=1e-4, atol=1e-4)


def test_dropout_matches_specification():
    rng = np.random.default_rng(4)
    B, C, T = 3, 512, 77
    for seed, layer in ((0, 0), (2 ** 64 - 1, 1), (123456789012345, 0)):
        segs = [0, 5, 2]
        v = ops.guarded(B, C, T, 16, "cuda")
        x = (np.abs(rng.standard_normal((B, C, T))) + 0.5).astype(np.float32)
        x[1] *= -1
        v[:, :, :T].copy_(torch.from_numpy(x))
        k0, k1 = dropout.key_of(seed)
        rk = torch.from_numpy(np.array([[s, k0, k1] for s in segs], np.uint32).view(np.int32)).cuda()
        relu = layer == 0
        ops.dropout(v, T, rk, layer, relu=relu)
        got = v[:, :, :T].cpu().numpy()
        for b, s in enumerate(segs):
            m = dropout.mask(seed, s, layer, T).T                          # (C, T)
            want = x[b] * m
            if relu:
                want = np.maximum(want, 0)
            assert np.array_equal(got[b], want)                            # bit-exact: x2 is exact


def test_train_restorer_vs_float64_ragged(seeded_states):
    """A ragged batch T = 65 / 230 / 1001 through forward_train against the float64 restatement, and each row alone."""
    vsd, rsd = seeded_states
    pipe = engine.Pipeline(vsd, rsd, "cuda:0")
    rng = np.random.default_rng(8)
    Ts = [65, 230, 1001]
    lens = [441 * (t - 1) + 100 for t in Ts]
    wav = np.zeros((3, max(lens)), np.float32)
    for b, n in enumerate(lens):
        wav[b, :n] = 0.2 * rng.standard_normal(n)
    seed, segs = 77, [0, 3, 1]
    out = pipe.restore_train(torch.from_numpy(wav).cuda(), lens, segs, seed).cpu().numpy()
    worst = 0.0
    for b, n in enumerate(lens):
        alone = pipe.restore_train(torch.from_numpy(wav[b:b + 1, :n]).cuda(), [n], [segs[b]], seed).cpu().numpy()
        assert _rms(out[b, :n], alone[0]) < 1e-5
        with torch.no_grad():
            ref = tref.restore_segment(wav[b, :n], vsd, rsd, seed, segs[b])
        r = _rms(alone[0], ref[0])
        worst = max(worst, r)
        assert r < 1e-3, (Ts[b], r)
    print("mode-2 waveform RMS vs float64 restatement: worst %.3g" % worst)


def test_train_restorer_stages_vs_float64(seeded_states):
    """mask / unet_out / log-mel of forward_train against the restatement, relative to the stage's peak."""
    vsd, rsd = seeded_states
    pipe = engine.Pipeline(vsd, rsd, "cuda:0")
    g = torch.Generator().manual_seed(1)
    for T in (65, 300):
        mel = (torch.rand((1, T, 128), generator=g) ** 2) * 3
        k0, k1 = dropout.key_of(5)
        rk = torch.from_numpy(np.array([[0, k0, k1]], np.uint32).view(np.int32)).cuda()
        dbg = {}
        logmel, _ = pipe.restorer.forward_train(mel.cuda(), T, rk, debug=dbg)
        with torch.no_grad():
            ref = tref.restorer_forward(mel[:, None].double(), {k: v.double() for k, v in rsd.items()},
                                        tref.masks_for(5, 0, T))
        for name, got, want in (("mask", dbg["mask"].transpose(1, 2), ref["mask"][:, 0]),
                                ("unet_out", dbg["unet_out"], ref["unet_out"][:, 0]), ("logmel", logmel, ref["mel"][:, 0])):
            got = got.cpu().double()
            rel = float((got - want).abs().max() / want.abs().max())
            print("T=%d %s: max |err| / peak = %.3g" % (T, name, rel))
            assert rel < 2e-4, (T, name, rel)


def test_restore_inmem_mode2(vf):
    rng = np.random.default_rng(2)
    wav = (0.2 * rng.standard_normal(44100 * 2)).astype(np.float32)
    m0 = vf.restore_inmem(wav, mode=0)
    a = vf.restore_inmem(wav, mode=2, seed=11)
    b = vf.restore_inmem(wav, mode=2, seed=11)
    c = vf.restore_inmem(wav, mode=2, seed=12)
    assert a.shape == (1, wav.shape[0]) and np.array_equal(a, b) and not np.array_equal(a, c)
    assert np.array_equal(m0, vf.restore_inmem(wav, mode=0))       # no running statistics moved
    vf.set_math("bf16x3")
    try:
        assert np.array_equal(a, vf.restore_inmem(wav, mode=2, seed=11))   # mode 2 is fp32 whatever set_math says
    finally:
        vf.set_math("f32")
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        vf.restore_inmem(np.zeros(441 * 60, np.float32), mode=2, seed=1)              # 61 frames
    long = (0.2 * rng.standard_normal(int(44100 * 30.3))).astype(np.float32)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        vf.restore_inmem(long, mode=2, seed=1)


def test_long_input_segments_equal_separate_runs(vf):
    rng = np.random.default_rng(6)
    wav = (0.2 * rng.standard_normal(44100 * 31)).astype(np.float32)
    out = vf.restore_inmem(wav, mode=2, seed=3)
    pipe = vf._get_pipe()
    s0 = pipe.restore_train(torch.from_numpy(wav[:44100 * 30])[None].cuda(), [44100 * 30], [0], 3).cpu().numpy()
    s1 = pipe.restore_train(torch.from_numpy(wav[44100 * 30:])[None].cuda(), [44100], [1], 3).cpu().numpy()
    assert np.array_equal(out, np.concatenate([s0, s1], axis=1))


def test_folder_and_cli_mode2(vf, tmp_path):
    from voicefixer_amd import __main__ as cli
    rng = np.random.default_rng(7)
    ind, outd, single = tmp_path / "in", tmp_path / "out", tmp_path / "single"
    ind.mkdir(); single.mkdir()
    for name, n in (("a.wav", 60000), ("b.wav", 91000), ("short.wav", 22050)):
        audio_io.save_wave((0.2 * rng.standard_normal(n)).astype(np.float32)[None], str(ind / name))
    st = {}
    files = vf.restore_folder(str(ind), str(outd), mode=2, seed=7, batch_size=4, io_threads=2, stats=st)
    assert files == ["a.wav", "b.wav"] and [f for f, _ in st["failed"]] == ["short.wav"]
    from scipy.io import wavfile
    for f in files:
        vf.restore(input=str(ind / f), output=str(single / f), mode=2, seed=7)
        x1, x2 = wavfile.read(str(outd / f))[1], wavfile.read(str(single / f))[1]
        assert x1.shape == x2.shape and np.max(np.abs(x1.astype(np.int32) - x2.astype(np.int32))) <= 1
    os.remove(str(ind / "short.wav"))
    home = os.environ.get("HOME")
    api = voicefixer_amd.api
    orig = api.VoiceFixer.__init__

    def init(self, _states=None):          # the CLI builds VoiceFixer() from checkpoints: hand it the seeded states
        orig(self, _states=(vf._vocoder._state, vf._restorer_state))
    api.VoiceFixer.__init__ = init
    try:
        rc = cli.main(["-ifdr", str(ind), "-ofdr", str(tmp_path / "all"), "--mode", "all", "--seed", "7", "--silent"])
    finally:
        api.VoiceFixer.__init__ = orig
    assert rc == 0 and home == os.environ.get("HOME")
    assert sorted(os.listdir(tmp_path / "all")) == ["a-mode0.wav", "a-mode1.wav", "a-mode2.wav",
                                                    "b-mode0.wav", "b-mode1.wav", "b-mode2.wav"]
    x1 = wavfile.read(str(tmp_path / "all" / "a-mode2.wav"))[1]
    x2 = wavfile.read(str(single / "a.wav"))[1]
    assert np.max(np.abs(x1.astype(np.int32) - x2.astype(np.int32))) <= 1
