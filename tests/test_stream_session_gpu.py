"""The streaming session on the MI355X: vfx_resample_span_f32 against the whole-row kernel bit for bit (minimal windows, NaN
all around), its 64-bit positions against float64, its argument checks, vfx_xfade_f32 against numpy's float32 expression,
and VoiceFixer.open_stream against its definition -- restore_stream on the concatenated input, converted as a whole row."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import voicefixer_amd  # noqa: E402
from voicefixer_amd import api, audio_io, ops, _lib  # noqa: E402

SPAN_PAIRS = [(16000, 44100), (22050, 44100), (48000, 44100), (44100, 48000), (44100, 16000)]
PAD = 16


@pytest.fixture(scope="module")
def vf(seeded_states):
    return voicefixer_amd.VoiceFixer.from_state(*seeded_states)


def _launches():
    return _lib.lib().vfx_launch_count()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _whole_row(x, up, down):
    n = x.shape[0]
    ny = -(-n * up // down)
    yd = torch.empty((1, ny), device="cuda")
    ops.resample_rows(torch.from_numpy(x)[None].cuda(), torch.tensor([n], dtype=torch.int32, device="cuda"), yd, up, down)
    return yd[0].cpu().numpy()


def _span(x, n_total, up, down, J, c, m0, m1):
    """Outputs [m0, m1) of row x from the MINIMAL window, NaN on both sides of the window and of y; returns the outputs
    after checking the canaries and the launch count."""
    n = x.shape[0]
    lo, hi = audio_io.span_window(m0, max(m1, m0 + 1), up, down, J, c)
    g0, end = max(lo, 0), min(hi - 1, n - 1)
    assert end >= g0
    xb = np.full(end - g0 + 1 + 2 * PAD, np.nan, np.float32)
    xb[PAD:-PAD] = x[g0:end + 1]
    xd = torch.from_numpy(xb).cuda()
    cnt = m1 - m0
    yd = torch.full((max(cnt, 1) + 2 * PAD,), float("nan"), device="cuda")
    before = _launches()
    ops.resample_span(xd[PAD:-PAD], g0, n_total, up, down, m0, m1, yd[PAD:PAD + max(cnt, 1)])
    torch.cuda.synchronize()
    assert _launches() == before + (1 if cnt else 0)
    y = yd.cpu().numpy()
    assert np.all(np.isnan(y[:PAD])) and np.all(np.isnan(y[PAD + cnt:])), (m0, m1)
    assert np.all(np.isfinite(y[PAD:PAD + cnt])), (m0, m1)
    return y[PAD:PAD + cnt]


@pytest.mark.parametrize("pair", SPAN_PAIRS)
def test_span_equals_whole_row_bit_for_bit(pair):
    up, down = audio_io.rate_ratio(*pair)
    _, J, c = audio_io.hq_bank(up, down)
    rng = np.random.default_rng(up * 1000 + down)
    for n in (4000, J // 2):
        v = rng.uniform(-1, 1, n)
        x = (v / np.abs(v).max()).astype(np.float32)
        ref = _whole_row(x, up, down)
        ny = ref.shape[0]
        assert ny == audio_io.converted_length(n, *pair)
        cuts = sorted(set(int(b) for b in rng.integers(1, ny, 6)))
        one = cuts[len(cuts) // 2]
        cuts = sorted(cuts + [one, one + 1])          # [one, one): an empty span; [one, one + 1): a one-output span
        bounds = [0] + cuts + [ny]
        spans = [(a, b) for a, b in zip(bounds[:-1], bounds[1:]) if b >= a]
        assert (one, one) in spans and (one, one + 1) in spans and spans[0][0] == 0 and spans[-1][1] == ny
        assert audio_io.span_window(0, 1, up, down, J, c)[0] < 0          # the first span starts left of the row
        got = []
        for m0, m1 in spans:
            y = _span(x, n, up, down, J, c, m0, m1)
            assert np.array_equal(_bits(y), _bits(ref[m0:m1])), (pair, n, m0, m1)
            if m1 > m0 and audio_io.span_window(m0, m1, up, down, J, c)[1] <= n:       # reads nothing past the row's end
                y2 = _span(x, None, up, down, J, c, m0, m1)
                assert np.array_equal(_bits(y2), _bits(ref[m0:m1])), (pair, n, m0, m1, "end unknown")
            got.append(y)
        assert np.array_equal(_bits(np.concatenate(got)), _bits(ref))


def test_span_positions_past_2_31():
    """44.1 -> 16 kHz, outputs whose c + m * down lies beyond 2^31: only the window exists (values a function of the global
    index), the outputs are compared with the float64 sum."""
    pair = (44100, 16000)
    up, down = audio_io.rate_ratio(*pair)
    h, _ = audio_io.hq_filter(up, down)
    bank64, J, c = audio_io.polyphase_bank(h * up, up)
    m0 = 2 ** 31 // down + 7
    m1 = m0 + 512
    assert c + m0 * down > 2 ** 31
    lo, hi = audio_io.span_window(m0, m1, up, down, J, c)
    assert lo > 1.3e7 and 1500 < hi - lo < 3500
    k = np.arange(lo, hi, dtype=np.uint64)
    xw = (((k * np.uint64(2654435761)) % np.uint64(2 ** 32)).astype(np.float64) / 2.0 ** 31 - 1.0).astype(np.float32)
    yd = torch.full((512 + PAD,), float("nan"), device="cuda")
    for n_total in (None, 3 * 10 ** 9):
        yd.fill_(float("nan"))
        ops.resample_span(torch.from_numpy(xw).cuda(), lo, n_total, up, down, m0, m1, yd[:512])
        y = yd.cpu().numpy()
        assert np.all(np.isnan(y[512:]))
        m = np.arange(m0, m1, dtype=np.int64)
        pos = c + m * down
        kmax = pos // up
        idx = (kmax - J + 1)[:, None] + np.arange(J)[None] - lo
        ref = np.sum(bank64[pos - kmax * up] * xw.astype(np.float64)[idx], axis=1)
        worst = float(np.max(np.abs(y[:512] - ref)))
        print("span past 2^31 (n_total %r): max abs error vs float64 %.3g" % (n_total, worst))
        assert worst <= 2e-6


def test_span_refuses_bad_arguments_and_launches_nothing():
    pair = (16000, 44100)
    up, down = audio_io.rate_ratio(*pair)
    bank, J, c = ops.resample_bank(torch.device("cuda", torch.cuda.current_device()), up, down)
    n, m0, m1 = 4000, 3000, 3400
    lo, hi = audio_io.span_window(m0, m1, up, down, J, c)
    assert lo > 0 and hi < n
    x = torch.zeros((n,), device="cuda")
    y = torch.full((m1 - m0 + PAD,), float("nan"), device="cuda")
    fn = _lib.lib().vfx_resample_span_f32
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + 4 * off)

    def call(xp, g0, wlen, n_total, bp, J_, c_, a, b, yp):
        return fn(xp, g0, wlen, n_total, bp, J_, up, down, c_, a, b, yp, None)
    before = _launches()
    assert call(ptr(x, lo + 1), lo + 1, hi - lo - 1, n, ptr(bank), J, c, m0, m1, ptr(y)) == _lib.EINVAL     # short on the left
    assert call(ptr(x, lo), lo, hi - lo - 1, n, ptr(bank), J, c, m0, m1, ptr(y)) == _lib.EINVAL             # short on the right
    assert call(ptr(x, lo), lo, hi - lo - 1, 2 ** 63 - 1, ptr(bank), J, c, m0, m1, ptr(y)) == _lib.EINVAL
    assert call(None, lo, hi - lo, n, ptr(bank), J, c, m0, m1, ptr(y)) == _lib.EINVAL
    assert call(ptr(x, lo), lo, hi - lo, n, None, J, c, m0, m1, ptr(y)) == _lib.EINVAL
    assert call(ptr(x, lo), lo, hi - lo, n, ptr(bank), J, c, m0, m1, None) == _lib.EINVAL
    assert call(ptr(x, lo), lo, hi - lo, n, ptr(bank), J, c, m1, m0, ptr(y)) == _lib.EINVAL                 # m1 < m0
    assert call(ptr(x, lo), lo, hi - lo, n, ptr(bank), J, up * J, m0, m1, ptr(y)) == _lib.EINVAL            # c >= up * J
    assert call(ptr(x, lo), lo, hi - lo, n, ptr(bank), J, c, m0, m0, ptr(y)) == 0                           # empty: ok, no launch
    torch.cuda.synchronize()
    assert _launches() == before and bool(torch.isnan(y).all())
    assert call(ptr(x, lo), lo, hi - lo, n, ptr(bank), J, c, m0, m1, ptr(y)) == 0                           # the exact window: taken
    torch.cuda.synchronize()
    assert _launches() == before + 1 and bool((y[:m1 - m0] == 0).all()) and bool(torch.isnan(y[m1 - m0:]).all())
    with pytest.raises(_lib.VfxError):
        ops.resample_span(x[lo + 1:hi], lo + 1, n, up, down, m0, m1, y)
    xf = _lib.lib().vfx_xfade_f32
    assert xf(None, ptr(x), ptr(x), 4, ptr(y), None) == _lib.EINVAL and xf(ptr(x), ptr(x), ptr(x), -1, ptr(y), None) == _lib.EINVAL
    assert xf(ptr(x), ptr(x), ptr(x), 0, ptr(y), None) == 0 and _launches() == before + 1


@pytest.mark.parametrize("n", [1, 7, 11025])
def test_xfade_is_numpys_float32_expression(n):
    rng = np.random.default_rng(n)

    def noise():
        v = rng.standard_normal(n + PAD).astype(np.float32)
        v[rng.integers(0, n, max(n // 8, 1))] *= np.float32(1e-39)       # denormal-scale values
        v[rng.integers(0, n, max(n // 16, 1))] = 1.0
        v[rng.integers(0, n, max(n // 16, 1))] = -1.0
        return v
    a, b = noise(), noise()
    f = np.arange(n, dtype=np.float32) / max(n, 1)
    want = a[:n] * (1.0 - f) + b[:n] * f
    assert want.dtype == np.float32
    ad, bd, fd = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), torch.from_numpy(f).cuda()
    out = torch.full((n + PAD,), float("nan"), device="cuda")
    before = _launches()
    ops.xfade(ad[:n], bd[:n], fd, out[:n])
    torch.cuda.synchronize()
    assert _launches() == before + 1
    o = out.cpu().numpy()
    assert np.array_equal(_bits(o[:n]), _bits(want)) and np.all(np.isnan(o[n:]))
    assert np.array_equal(_bits(ad.cpu().numpy()), _bits(a)) and np.array_equal(_bits(bd.cpu().numpy()), _bits(b))
    ops.xfade(ad[:n], bd[:n], fd, ad[:n])                 # in place: out is tail
    o = ad.cpu().numpy()
    assert np.array_equal(_bits(o[:n]), _bits(want)) and np.array_equal(_bits(o[n:]), _bits(a[n:]))
    hd = torch.from_numpy(b).cuda()
    ops.xfade(torch.from_numpy(a).cuda()[:n], hd[:n], fd, hd[:n])             # in place: out is head (the session's use)
    o = hd.cpu().numpy()
    assert np.array_equal(_bits(o[:n]), _bits(want)) and np.array_equal(_bits(o[n:]), _bits(b[n:]))


CS, OVS = 1.5, 0.25


def _definition(vf, x, rate_in, rate_out, mode, batch_size=1):
    """Z of RestoreSession's definition (and the precondition: restore_stream at batch_size 1 is reproducible)."""
    dev = vf._get_pipe().device
    x44, (n44,) = api.convert_rows(torch.from_numpy(x)[None].to(dev), [len(x)], [rate_in])
    x44 = x44[0, :n44].cpu().numpy()
    y44 = vf.restore_stream(x44, chunk_seconds=CS, overlap_seconds=OVS, batch_size=batch_size, mode=mode)
    again = vf.restore_stream(x44, chunk_seconds=CS, overlap_seconds=OVS, batch_size=batch_size, mode=mode)
    assert np.array_equal(_bits(y44), _bits(again)), "restore_stream itself is not reproducible run to run"
    if rate_out == 44100:
        return y44, n44
    up, down = audio_io.rate_ratio(44100, rate_out)
    n = y44.shape[1]
    z = torch.empty((1, audio_io.converted_length(n, 44100, rate_out)), device=dev)
    ops.resample_rows(torch.from_numpy(y44).to(dev), torch.tensor([n], dtype=torch.int32, device=dev), z, up, down)
    return z.cpu().numpy(), n44


def _pushed(s, x, sizes):
    got, at = [], 0
    for k in list(sizes) + [len(x)]:
        got.append(s.push(x[at:at + k]))
        at = min(at + k, len(x))
    assert at == len(x)
    got.append(s.finish())
    for g in got:
        assert g.dtype == np.float32 and g.ndim == 2 and g.shape[0] == 1
    return got


@pytest.mark.parametrize("case,mode,rate_in,rate_out", [("a", 0, 44100, 44100), ("b", 1, 44100, 44100), ("c", 0, 16000, 44100),
                                                        ("d", 0, 44100, 48000), ("e", 0, 16000, 48000)])
def test_session_equals_its_definition(vf, case, mode, rate_in, rate_out):
    """~4.2 s of noise in blocks of 1, 0, 4410, 70001 samples and the rest, chunks of 1.5 s with 0.25 s of overlap, B = 1:
    the pushed results concatenate to restore_stream of the whole (converted) input, converted as a whole -- bit for bit."""
    rng = np.random.default_rng(ord(case))
    n = int(4.2 * rate_in) + 311
    x = (0.1 * rng.standard_normal(n)).astype(np.float32)
    want, n44 = _definition(vf, x, rate_in, rate_out, mode)
    chunk = 66150 - (66150 % 512 if mode == 1 else 0)
    plan = api.plan_stream_chunks(n44, chunk, 11025, 1535 if mode == 1 else 1024)
    assert len(plan) >= 3
    if mode == 1:
        assert plan[-1][1] % 512 != 0 and want.shape[1] == plan[-1][0] + 512 * (plan[-1][1] // 512) < n44
    s = vf.open_stream(chunk_seconds=CS, overlap_seconds=OVS, batch_size=1, mode=mode, sample_rate=rate_in,
                       output_sample_rate=None if rate_out == 44100 else rate_out)
    got = _pushed(s, x, [1, 0, 4410, 70001])
    z = np.concatenate(got, axis=1)
    assert z.shape == want.shape and s.position == want.shape[1]
    assert np.array_equal(_bits(z), _bits(want)), (case, float(np.max(np.abs(z - want))))


def test_session_batched_chunks_against_single(vf):
    rng = np.random.default_rng(52)
    x = (0.1 * rng.standard_normal(int(4.2 * 44100) + 311)).astype(np.float32)
    one = np.concatenate(_pushed(vf.open_stream(chunk_seconds=CS, overlap_seconds=OVS, batch_size=1), x, [1, 0, 4410, 70001]), 1)
    seen = []
    pipe = vf._get_pipe()
    restore = pipe.restore

    def spy(seg, n, *a, **k):
        seen.append(seg.shape[0])
        return restore(seg, n, *a, **k)
    pipe.restore = spy
    try:
        two = np.concatenate(_pushed(vf.open_stream(chunk_seconds=CS, overlap_seconds=OVS, batch_size=2), x, []), 1)
    finally:
        del pipe.restore
    assert 2 in seen                                       # chunks settled by one push went through the path together
    assert one.shape == two.shape
    rms = float(np.sqrt(np.mean((one.astype(np.float64) - two) ** 2)))
    print("session batch_size 2 vs 1: waveform RMS %.3g" % rms)
    assert rms < 2e-5


def test_it_streams(vf):
    rng = np.random.default_rng(6)
    n = int(4.2 * 44100) + 311
    x = (0.1 * rng.standard_normal(n)).astype(np.float32)
    chunk, ov = 66150, 11025
    planner = api.StreamPlanner(chunk, ov)
    want = vf.restore_stream(x, chunk_seconds=CS, overlap_seconds=OVS, batch_size=1)
    with vf.open_stream(chunk_seconds=CS, overlap_seconds=OVS) as s:
        got, final, first_at = [], 0, None
        for at in range(0, n, 20000):
            blk = x[at:at + 20000]
            y = s.push(blk)
            for a, length in planner.feed(len(blk)):
                final = a + length - ov                   # restore_stream's rule for a chunk that is not the last
            assert s.position == final, at
            assert np.array_equal(_bits(y), _bits(want[:, final - y.shape[1]:final]))      # no gap, no overlap
            if y.shape[1] and first_at is None:
                first_at = at
            got.append(y)
        assert first_at is not None and first_at + 20000 < n        # the first result came before the last block went in
        got.append(s.finish())
        assert s.position == n and np.array_equal(_bits(np.concatenate(got, 1)), _bits(want))
        with pytest.raises(RuntimeError):
            s.finish()
        with pytest.raises(RuntimeError):
            s.push(x[:10])
    short = vf.open_stream(chunk_seconds=CS, overlap_seconds=OVS, sample_rate=16000)
    assert short.push(x[:371]).shape == (1, 0)             # 371 samples at 16 kHz: 1023 at 44.1 kHz, under MIN_SAMPLES[0]
    before = _launches()
    with pytest.raises(ValueError):
        short.finish()
    assert _launches() == before
    with pytest.raises(RuntimeError):
        short.finish()
