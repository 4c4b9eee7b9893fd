"""Word-length reduction on the MI355X: vfx_quantize_rows_f32 and everything above it against the numpy specification
(wordlength.quantize_ref) -- as integers, without a tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import voicefixer_amd  # noqa: E402
from voicefixer_amd import _lib, api, audio_io, flac, ops, wordlength  # noqa: E402

LENS = [1, 5, 1027, 4099]
N0 = [0, 3, 2 ** 34 - 2, 1237]              # the third row crosses block 2^32 of the counter two samples in
CHAN = [0, 1, 7, 0]
N_MAX, XS, OS = 4099, 4112, 4108            # both strides beyond n_max, different from each other
SATURATION = [1.0, -1.0, 1.5, -1.5, np.nan, np.inf, -np.inf]
CS, OVS = 1.5, 0.25                         # the chunk geometry of tests/test_stream_session_gpu.py


@pytest.fixture(scope="module")
def vf(seeded_states):
    return voicefixer_amd.VoiceFixer.from_state(*seeded_states)


@pytest.fixture(scope="module")
def rows():
    """The four input rows (float32, padded with NaN to the stride: nothing behind a row's end may be read into a result)."""
    rng = np.random.default_rng(77)
    x = np.full((4, XS), np.nan, np.float32)
    for r, n in enumerate(LENS):
        x[r, :n] = 0.3 * rng.standard_normal(n)
    near = [s * (1.0 - k * 2.0 ** -e) for e in (15, 23) for k in (0.25, 0.5, 0.75, 1.0, 1.5) for s in (1.0, -1.0)]
    x[0, 0] = 1.0 - 2.0 ** -16
    x[1, :5] = SATURATION[:5]
    x[2, :7] = SATURATION
    x[2, 7:7 + len(near)] = near
    x[3, 100:107] = SATURATION
    x[3, 4099 - len(near):4099] = near                      # ... and in the last, partial group of four
    x[3, 2000:2008] = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 3.5, -3.5]) / 32768.0         # ties at 16 bits
    return x


def _launches():
    return _lib.lib().vfx_launch_count()


def _call(xd, x_stride, n_rows, B, n_max, n0, chan, bits, dither, seed, outd, out_stride, res):
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None       # noqa: E731
    rc = _lib.lib().vfx_quantize_rows_f32(P(xd), x_stride, P(n_rows), B, n_max, P(n0), P(chan), bits, dither, seed, P(outd),
                                          out_stride, P(res), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def _sentinel(bits):
    return (0x5555, torch.int16) if bits == 16 else (0x55555555, torch.int32)


@pytest.mark.parametrize("seed", [0, 2 ** 63 + 5])
@pytest.mark.parametrize("dither", [0, 1, 2])
@pytest.mark.parametrize("bits", [16, 24])
def test_kernel_equals_the_specification(rows, bits, dither, seed):
    kind = wordlength.DITHERS[dither]
    want = [wordlength.quantize_ref(rows[r, :n], bits, kind, seed=seed, n0=N0[r], channel=CHAN[r]) for r, n in enumerate(LENS)]
    assert want[2][1] >= 5 and want[3][2] == 1 << (bits - 1)
    sent, dtype = _sentinel(bits)
    xd = torch.from_numpy(rows).cuda()
    n_rows = torch.tensor(LENS, dtype=torch.int32, device="cuda")
    n0 = torch.tensor(N0, dtype=torch.int64, device="cuda")
    chan = torch.tensor(CHAN, dtype=torch.int32, device="cuda")
    out = torch.full((4, OS), sent, dtype=dtype, device="cuda")
    res = torch.full((4, 2), -7, dtype=torch.int32, device="cuda")
    before = _launches()
    assert _call(xd, XS, n_rows, 4, N_MAX, n0, chan, bits, dither, seed, out, OS, res) == 0
    assert _launches() == before + 1                      # (the clear of ``result`` is not counted: one kernel)
    got, gres = out.cpu().numpy(), res.cpu().numpy()
    for r, n in enumerate(LENS):
        assert np.array_equal(got[r, :n].astype(np.int32), want[r][0]), (r, np.flatnonzero(got[r, :n] != want[r][0])[:8])
        assert np.all(got[r, n:] == sent), r              # behind the row's own end, up to the next row
        assert gres[r].tolist() == [want[r][1], want[r][2]], (r, gres[r])
    # every row alone: the same bits (its own pointer: rows 1 and 3 start 16-byte aligned, row stride % 4 == 0)
    for r, n in enumerate(LENS):
        one = torch.full((1, OS), sent, dtype=dtype, device="cuda")
        res1 = torch.full((1, 2), -7, dtype=torch.int32, device="cuda")
        assert _call(xd[r], XS, n_rows[r:r + 1], 1, n, n0[r:r + 1], chan[r:r + 1], bits, dither, seed, one, OS, res1) == 0
        assert np.array_equal(one.cpu().numpy()[0], got[r]) and res1.cpu().numpy()[0].tolist() == gres[r].tolist(), r
    # the input one float off 16-byte alignment, the output one element off: the sample-by-sample path, identical bits
    xs = torch.full((4 * XS + 1,), float("nan"), device="cuda")
    xs[1:] = xd.reshape(-1)
    outs = torch.full((4 * OS + 1,), sent, dtype=dtype, device="cuda")
    assert xs[1:].data_ptr() % 16 == 4
    assert _call(xs[1:], XS, n_rows, 4, N_MAX, n0, chan, bits, dither, seed, outs[1:], OS, res) == 0
    assert int(outs[0]) == sent and np.array_equal(outs[1:].cpu().numpy().reshape(4, OS), got)
    assert np.array_equal(res.cpu().numpy(), gres)
    # ... and strides that are no multiple of four elements (rows 1..3 start unaligned)
    xo = torch.full((4, XS + 1), float("nan"), device="cuda")
    xo[:, :XS] = xd
    outo = torch.full((4, OS + 3), sent, dtype=dtype, device="cuda")
    assert _call(xo, XS + 1, n_rows, 4, N_MAX, n0, chan, bits, dither, seed, outo, OS + 3, res) == 0
    assert np.array_equal(outo.cpu().numpy()[:, :OS], got) and np.all(outo.cpu().numpy()[:, OS:] == sent)
    assert np.array_equal(res.cpu().numpy(), gres)
    # without n0 and chan: every row starts its file on channel 0
    assert _call(xd, XS, n_rows, 4, N_MAX, None, None, bits, dither, seed, out, OS, res) == 0
    got0 = out.cpu().numpy()
    for r, n in enumerate(LENS):
        w = wordlength.quantize_ref(rows[r, :n], bits, kind, seed=seed)
        assert np.array_equal(got0[r, :n].astype(np.int32), w[0]) and res.cpu().numpy()[r].tolist() == [w[1], w[2]], r


def test_every_alignment_of_the_start_index(rows):
    """n0 % 4 decides which words of the neighbouring blocks a thread needs, and n0 = 0 how "hp" starts: all four residues,
    on a row of more than one tile, for the three dithers."""
    x = rows[3, :4099]
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()[None]
    n_rows = torch.tensor([4099], dtype=torch.int32, device="cuda")
    for start in (0, 1, 2, 3, 4, 2 ** 34 - 1, 2 ** 34 - 1024 * 4 + 1):
        n0 = torch.tensor([start], dtype=torch.int64, device="cuda")
        for kind in wordlength.DITHERS:
            out, res = ops.quantize_rows(xd, n_rows, 16, kind, 12345, n0=n0)
            q, clipped, peak = wordlength.quantize_ref(x, 16, kind, seed=12345, n0=start)
            assert out.dtype == torch.int16 and np.array_equal(out.cpu().numpy()[0].astype(np.int32), q), (start, kind)
            assert res.cpu().numpy()[0].tolist() == [clipped, peak]


def test_more_rows_than_the_grid_has_workgroups_for(rows):
    """The launch is capped at about 2048 workgroups: with 700 rows a workgroup walks two or three of its row's five tiles, and
    the per-row counts are folded over them.  Rows r, r + 28, r + 56, ... are the same row (input, start, channel) and must come
    out the same; 28 references serve all 700."""
    B, kinds = 700, 28
    base = np.stack([np.roll(rows[3], 37 * k) for k in range(kinds)])           # (the NaN padding rolls into some rows: fine)
    base[:, N_MAX:] = np.nan
    lens = [N_MAX - 41 * k for k in range(kinds)]
    starts = [k * (2 ** 30 + 1) for k in range(kinds)]
    xd = torch.from_numpy(base).cuda().repeat(B // kinds, 1)
    n_rows = torch.tensor(lens * (B // kinds), dtype=torch.int32, device="cuda")
    n0 = torch.tensor(starts * (B // kinds), dtype=torch.int64, device="cuda")
    chan = torch.tensor([k % 8 for k in range(kinds)] * (B // kinds), dtype=torch.int32, device="cuda")
    for bits, kind in ((16, "hp"), (24, "tpdf")):
        out, res = ops.quantize_rows(xd, n_rows, bits, kind, 77, n0=n0, chan=chan)
        got, gres = out.cpu().numpy().astype(np.int32), res.cpu().numpy()
        for k in range(kinds):
            q, clipped, peak = wordlength.quantize_ref(base[k, :lens[k]], bits, kind, seed=77, n0=starts[k], channel=k % 8)
            assert np.all(got[k::kinds, :lens[k]] == q[None]), (bits, kind, k)
            assert np.all(gres[k::kinds] == np.array([clipped, peak])), (bits, kind, k, gres[k::kinds][:3], clipped, peak)


def test_kernel_refuses_bad_arguments_and_launches_nothing(rows):
    xd = torch.from_numpy(rows).cuda()
    n_rows = torch.tensor(LENS, dtype=torch.int32, device="cuda")
    out = torch.full((4, OS), 0x5555, dtype=torch.int16, device="cuda")
    res = torch.full((4, 2), -7, dtype=torch.int32, device="cuda")
    good = dict(xd=xd, x_stride=XS, n_rows=n_rows, B=4, n_max=N_MAX, n0=None, chan=None, bits=16, dither=1, seed=0, outd=out,
                out_stride=OS, res=res)
    before = _launches()
    for bad in (dict(xd=None), dict(n_rows=None), dict(outd=None), dict(res=None), dict(B=-1), dict(n_max=-1), dict(bits=8),
                dict(bits=20), dict(bits=32), dict(dither=-1), dict(dither=3), dict(x_stride=N_MAX - 1), dict(out_stride=N_MAX - 1)):
        assert _call(**dict(good, **bad)) == _lib.EINVAL, bad
    for nothing in (dict(B=0), dict(n_max=0)):
        assert _call(**dict(good, **nothing)) == 0, nothing
    assert _launches() == before
    assert np.all(out.cpu().numpy() == 0x5555) and np.all(res.cpu().numpy() == -7)
    assert _call(**good) == 0 and _launches() == before + 1                   # ... and the same arguments, unbroken, run


def test_public_quantize():
    rng = np.random.default_rng(3)
    x = (0.4 * rng.standard_normal((3, 2051))).astype(np.float32)
    x[1, :7] = SATURATION
    for bits, dtype in ((16, np.int16), (24, np.int32)):
        got = voicefixer_amd.quantize(x, bits, "hp", 9)
        assert got.shape == x.shape and got.dtype == dtype
        for c in range(3):
            assert np.array_equal(got[c].astype(np.int32), wordlength.quantize_ref(x[c], bits, "hp", seed=9, channel=c)[0]), c
    a, b = x[0, :1500], x[2]
    got = voicefixer_amd.quantize([a, b])
    assert [g.shape for g in got] == [(1500,), (2051,)] and all(g.dtype == np.int16 for g in got)
    for g, w in zip(got, (a, b)):
        assert np.array_equal(g.astype(np.int32), wordlength.quantize_ref(w, 16)[0])
    one = voicefixer_amd.quantize(a, 24, "none")
    assert one.shape == (1500,) and np.array_equal(one, wordlength.quantize_ref(a, 24, "none")[0])
    mixed = voicefixer_amd.quantize([x[:2], a], 16, "tpdf", 1)
    assert mixed[0].shape == (2, 2051) and np.array_equal(mixed[0][1].astype(np.int32),
                                                          wordlength.quantize_ref(x[1], 16, seed=1, channel=1)[0])
    assert voicefixer_amd.quantize([]) == []


def test_output_record_quantises_files_of_channels():
    rng = np.random.default_rng(4)
    x = (0.4 * rng.standard_normal((3, 2051))).astype(np.float32)
    lens = [1800, 1800, 2051]
    job = api._Output(bit_depth=24, dither="tpdf", dither_seed=6)
    xd = torch.from_numpy(x).cuda()
    pcm, res = job.quantize(xd, lens, [2, 1])
    assert pcm.dtype == torch.int32 and tuple(pcm.shape) == (3, 2051) and tuple(res.shape) == (3, 2)
    for r, (n, c) in enumerate(zip(lens, (0, 1, 0))):
        q, clipped, peak = wordlength.quantize_ref(x[r, :n], 24, "tpdf", seed=6, channel=c)
        assert np.array_equal(pcm[r, :n].cpu().numpy(), q) and res[r].tolist() == [clipped, peak], r
    assert not np.array_equal(pcm[0, :1800].cpu().numpy(), wordlength.quantize_ref(x[0, :1800], 24, "tpdf", seed=6, channel=1)[0])
    pcm, _ = job.quantize(xd, lens, None, n0=[5, 0, 2 ** 33])
    for r, (n, start) in enumerate(zip(lens, (5, 0, 2 ** 33))):
        assert np.array_equal(pcm[r, :n].cpu().numpy(), wordlength.quantize_ref(x[r, :n], 24, "tpdf", seed=6, n0=start)[0]), r
    pcm, _ = job.quantize(xd[:, ::2], [900, 900, 1000], None, n0=7)              # a view that is not contiguous
    assert np.array_equal(pcm[2, :1000].cpu().numpy(), wordlength.quantize_ref(x[2, ::2][:1000], 24, "tpdf", seed=6, n0=7)[0])


def test_restore_inmem_returns_the_float_result_quantised(vf):
    rng = np.random.default_rng(12)
    x = (0.2 * rng.standard_normal(30000)).astype(np.float32)
    y = vf.restore_inmem(x, cuda=True)
    q = vf.restore_inmem(x, cuda=True, bit_depth=16, dither="tpdf", dither_seed=3)
    assert q.dtype == np.int16 and q.shape == y.shape == (1, 30000)
    want = wordlength.quantize_ref(y[0], 16, "tpdf", seed=3)[0]
    print("restore_inmem: %d of %d samples differ from quantize_ref of the float result" % (int(np.sum(q[0] != want)), want.size))
    assert np.array_equal(q[0].astype(np.int32), want)
    q24 = vf.restore_inmem(np.stack([x, x[::-1]]), cuda=True, channels="all", bit_depth=24, dither="hp")
    y2 = vf.restore_inmem(np.stack([x, x[::-1]]), cuda=True, channels="all")
    assert q24.dtype == np.int32 and q24.shape == y2.shape == (2, 30000)
    for c in range(2):
        assert np.array_equal(q24[c], wordlength.quantize_ref(y2[c], 24, "hp", channel=c)[0]), c


def test_session_quantises_from_its_position(vf):
    rng = np.random.default_rng(21)
    x = (0.1 * rng.standard_normal(int(4.2 * 44100) + 311)).astype(np.float32)

    def pushed(s):
        got, at = [], 0
        for k in [1, 0, 4410, 70001, len(x)]:
            got.append(s.push(x[at:at + k]))
            at = min(at + k, len(x))
        got.append(s.finish())
        return got

    plain = np.concatenate(pushed(vf.open_stream(chunk_seconds=CS, overlap_seconds=OVS)), axis=1)
    s = vf.open_stream(chunk_seconds=CS, overlap_seconds=OVS, bit_depth=24, dither="hp")
    got = pushed(s)
    assert all(g.dtype == np.int32 and g.ndim == 2 and g.shape[0] == 1 for g in got)
    assert sum(g.shape[1] > 0 for g in got) >= 3 and got[0].shape == (1, 0)       # several stretches, at uneven positions
    z = np.concatenate(got, axis=1)
    assert z.shape == plain.shape and s.position == plain.shape[1]
    assert np.array_equal(z[0], wordlength.quantize_ref(plain[0], 24, "hp", n0=0)[0])
    s16 = vf.open_stream(chunk_seconds=CS, overlap_seconds=OVS, bit_depth=16)
    assert s16.push(x[:0]).dtype == np.int16 and s16.push(x[:100]).dtype == np.int16
    s16.close()


def test_folder_writes_the_depth_it_is_asked_for(vf, tmp_path):
    from scipy.io import wavfile
    rng = np.random.default_rng(31)
    ind = tmp_path / "in"
    ind.mkdir()
    mono = (0.2 * rng.standard_normal(30000)).astype(np.float32)
    stereo = (0.2 * rng.standard_normal((2, 41000))).astype(np.float32)
    audio_io.save_wave(mono[None], str(ind / "a.wav"))
    audio_io.save_wave(stereo, str(ind / "b.flac"), channels_first=True)
    both = (".wav", ".flac")
    ins = [audio_io.load_wav(str(ind / f), 44100, mono=False) for f in ("a.wav", "b.flac")]
    assert ins[0].shape == (30000,) and ins[1].shape == (2, 41000)
    st = {}
    names = vf.restore_folder(str(ind), str(tmp_path / "q"), batch_size=4, io_threads=2, extensions=both, channels="all",
                              bit_depth=24, stats=st)
    assert names == ["a.wav", "b.flac"] and st["failed"] == []
    want = vf.restore_batch(ins, batch_size=4, channels="all", bit_depth=24)
    assert [w.dtype for w in want] == [np.int32, np.int32] and [w.shape for w in want] == [(1, 30000), (2, 41000)]
    sr, a = wavfile.read(str(tmp_path / "q" / "a.wav"))
    assert sr == 44100 and a.dtype == np.int32 and np.array_equal(a >> 8, want[0][0])
    assert audio_io.wav_info(str(tmp_path / "q" / "a.wav"))[:2] == (44100, 30000)
    sr, b, bps = flac.read(str(tmp_path / "q" / "b.flac"))
    assert (sr, bps) == (44100, 24) and np.array_equal(b.T, want[1])
    assert [(n, bits) for n, bits, _, _ in st["word_length"]] == [("a.wav", 24), ("b.flac", 24)]
    for (_, _, clipped, peak_db), w in zip(st["word_length"], want):
        assert clipped == 0 and abs(peak_db - 20 * np.log10(np.abs(w).max() / 2.0 ** 23)) < 1e-9
    # the same job without a depth: the files save_wave writes from the float results, as before
    st0 = {}
    assert vf.restore_folder(str(ind), str(tmp_path / "d"), batch_size=4, io_threads=2, extensions=both, channels="all",
                             stats=st0) == names
    assert "word_length" not in st0
    floats = vf.restore_batch(ins, batch_size=4, channels="all")
    assert [f.dtype for f in floats] == [np.float32, np.float32]
    audio_io.save_wave(floats[0], str(tmp_path / "wa.wav"), channels_first=True)
    audio_io.save_wave(floats[1], str(tmp_path / "wb.flac"), channels_first=True)
    assert open(str(tmp_path / "d" / "a.wav"), "rb").read() == open(str(tmp_path / "wa.wav"), "rb").read()
    assert open(str(tmp_path / "d" / "b.flac"), "rb").read() == open(str(tmp_path / "wb.flac"), "rb").read()
    assert flac.read(str(tmp_path / "d" / "b.flac"))[2] == 16
    # restore(): file -> file at 16 bits through the device, FLAC
    vf.restore(str(ind / "a.wav"), str(tmp_path / "one.flac"), cuda=True, bit_depth=16, dither="none")
    sr, one, bps = flac.read(str(tmp_path / "one.flac"))
    y = vf.restore_inmem(ins[0], cuda=True)
    assert bps == 16 and np.array_equal(one[:, 0], wordlength.quantize_ref(y[0], 16, "none")[0])
