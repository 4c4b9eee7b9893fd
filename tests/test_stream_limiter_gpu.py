"""The fixed-gain look-ahead limiter of a streaming session on the MI355X (vfx_limit_span_f32; ops.limit_span,
voicefixer_amd.limit, open_stream(gain_db=..., limiter=True)) against the float64 reference ``ref_fixed`` of
tests/test_stream_limiter_cpu.py, and against itself: a row cut into spans, each from its minimal window, must give the bits
of the single span.

Per sample |out - ref| <= Cl (TP_BOUND max(1, gL / Cl) + (2 H + 9) 2^-24), TP_BOUND = 2e-6 max(1, max e): the bound of
tests/test_limiter_gpu.py, whose arithmetic the span kernels repeat (the trim's rounding, which it also covers, does not occur
here).  The same bound, relative, holds for min g.  Observed on the MI355X: see DESIGN.md 3.16."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import voicefixer_amd  # noqa: E402
from voicefixer_amd import _lib, loudness, ops  # noqa: E402
from test_true_peak_cpu import ref_true_peak  # noqa: E402
from test_stream_limiter_cpu import ref_fixed  # noqa: E402

PAD = 40
INT64_MAX = 2 ** 63 - 1


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _noise(rng, n, amp=0.1):
    return (amp * rng.uniform(-1, 1, n)).astype(np.float32)


def _window(N, m0, m1, H, Bk, Fw, known):
    """The minimal window [lo, hi) of the span [m0, m1) of a row of N samples."""
    lo = max(0, m0 - 2 * H - Bk)
    hi = m1 - 1 + 2 * H + Fw
    return lo, (min(N - 1, hi) if known else hi) + 1


def _span(x, fs, gain_db, m0, m1, lo, hi, known, ceiling_db=-1.0, true_peak=True, ms=3.0, shift=0, launches=3):
    """Outputs [m0, m1) from the window x[lo:hi] with NaN on both sides of the window and of ``out``; ``shift`` moves every
    global position (the data stay).  Returns (out (m1 - m0,), record (2,)); checks canaries, input and launch count."""
    buf = np.full(hi - lo + 2 * PAD, np.nan, np.float32)
    buf[PAD:PAD + hi - lo] = x[lo:hi]
    xd = torch.from_numpy(buf).cuda()
    od = torch.full((m1 - m0 + 2 * PAD,), float("nan"), device="cuda")
    lib = _lib.lib()
    c0 = lib.vfx_launch_count()
    rec = ops.limit_span(xd[PAD:PAD + hi - lo], lo + shift, len(x) + shift if known else None, fs, gain_db, m0 + shift,
                         m1 + shift, od[PAD:PAD + m1 - m0], ceiling_db, true_peak, ms)
    assert lib.vfx_launch_count() - c0 == (launches if m1 > m0 else 0)
    out = od.cpu().numpy()
    assert np.all(np.isnan(out[:PAD])) and np.all(np.isnan(out[PAD + m1 - m0:])), "out canaries"
    assert not np.any(np.isnan(out[PAD:PAD + m1 - m0]))
    assert np.array_equal(xd.cpu().numpy(), buf, equal_nan=True)
    return out[PAD:PAD + m1 - m0], rec.cpu().numpy()


def _whole(x, fs, gain_db, **kw):
    return _span(x, fs, gain_db, 0, len(x), 0, len(x), True, **kw)


def _check(what, rows, fs, gains, ceiling_db=-1.0, true_peak=True, ms=3.0):
    """Every row as ONE span against ref_fixed; the ceiling of the device output against the reference's own.  Returns the
    worst error / bound."""
    Cl = 10.0 ** (ceiling_db / 20.0)
    H = loudness.limiter_window(fs, ms)[0]
    worst, worst_abs, worst_g = 0.0, 0.0, 0.0
    for i, x in enumerate(rows):
        gain_db = gains[i % len(gains)]
        gL = 10.0 ** (gain_db / 20.0)
        got, rec = _whole(x, fs, gain_db, ceiling_db=ceiling_db, true_peak=true_peak, ms=ms)
        ref = ref_fixed(x, fs, gL, ceiling_db, ms, true_peak)
        assert ref["H"] == H
        tpb = 2e-6 * max(1.0, float(ref["e"].max()))
        tol = Cl * (tpb * max(1.0, gL / Cl) + (2 * H + 9) * 2.0 ** -24)
        err = float(np.abs(got.astype(np.float64) - ref["out"]).max())
        worst, worst_abs = max(worst, err / tol), max(worst_abs, err)
        assert err <= tol, (what, i, len(x), err, tol, int(np.abs(got - ref["out"]).argmax()))
        gerr = abs(rec[0] - ref["g"].min())
        worst_g = max(worst_g, gerr / (tol / Cl))
        assert gerr <= tol / Cl, (what, i, rec[0], ref["g"].min())
        assert rec[1] == float(np.abs(got).max()), (what, i)
        assert rec[1] <= Cl * (1 + 1e-12) + tol, (what, i, rec[1] / Cl)       # every sample under the ceiling (the reference's are)
        peak = (lambda v: ref_true_peak(v, fs)) if true_peak else (lambda v: float(np.abs(v).max()))
        ref_tp = peak(ref["out"])
        assert ref_tp <= Cl * (1 + 1e-4), (what, i, ref_tp / Cl)              # a condition on the test's own rows
        assert peak(got) <= ref_tp * (1 + tpb), (what, i, peak(got) / ref_tp)
    print("stream limiter %s: worst |out - ref| = %.2e, / bound = %.3f; min g / bound = %.3f over %d rows"
          % (what, worst_abs, worst, worst_g, len(rows)))
    return worst


def _peak_rows(rng, N, positions):
    rows = []
    for pos in positions:
        v = _noise(rng, N)
        v[pos] = -0.97 if pos % 2 else 0.97
        rows.append(v)
    return rows


def test_lengths_and_peak_positions_against_float64():
    """fs = 44100: R = 4, H = 132; output tiles of 1024 samples from m0, true-peak tiles of 1024 that start 2 samples early."""
    fs, H, T = 44100, 132, 1024
    rng = np.random.default_rng(11)
    rows = []
    for n in (1, 2, H, 2 * H + 1, T - 1, T, T + 1, 2 * T + 1, 5000):
        v = _noise(rng, n)
        v[n // 2] = 0.97
        rows.append(v)
    N = 5000
    rows += _peak_rows(rng, N, [0, N - 1] + list(range(1019, 1029)) +
                       [T - H, T - H - 1, T - 2 * H, T - 2 * H - 1, T - 2 - H, T - 2 - H - 1, T - 2 - 2 * H, T - 2 - 2 * H - 1])
    _check("44.1 kHz lengths / positions", rows, fs, [6.0, 12.0])


@pytest.mark.parametrize("fs,true_peak,ms", [(8000, True, 3.0), (96000, True, 3.0), (192000, True, 3.0), (44100, False, 3.0),
                                             (44100, True, 1.0)])
def test_rates_and_modes_against_float64(fs, true_peak, ms):
    rng = np.random.default_rng(fs + int(ms))
    H = loudness.limiter_window(fs, ms)[0]
    rows = []
    for n in (H + 3, 1025, 2 * H + 1500, 3333):
        v = _noise(rng, n)
        v[n // 4], v[n // 2], v[n - 1] = 0.97, -0.99, 0.9
        rows.append(v)
    _check("%d Hz tp=%d %g ms" % (fs, true_peak, ms), rows, fs, [6.0, 12.0], true_peak=true_peak, ms=ms)


@pytest.mark.parametrize("fs,true_peak", [(44100, True), (44100, False), (96000, True)])
def test_split_invariance_bit_for_bit(fs, true_peak):
    """The 5000-sample row cut into spans, each from its MINIMAL window between NaNs, n_total unknown wherever the ready rule
    allows the span before the end: the concatenation has the bits of the single span."""
    H, Bk, Fw = loudness.limiter_reach(fs, 3.0, true_peak)
    rng = np.random.default_rng(fs + true_peak)
    N = 5000
    x = _noise(rng, N)
    for p in (0, 700, 1023, 1024, 2 * H, 2500, 2500 + H, 4000, N - 1):
        x[p] = 0.97 if p % 2 == 0 else -0.95
    want, rec = _whole(x, fs, 6.0, true_peak=true_peak)
    cuts = sorted(set([1, 2, 1023, 1024, 1025, 2 * H, 2 * H + 1] + [int(v) for v in rng.integers(1, N, 5)]))
    got, gmin, vmax, unknown = [], 1.0, 0.0, 0
    for m0, m1 in zip([0] + cuts, cuts + [N]):
        known = m1 + 2 * H + Fw > N
        unknown += not known
        lo, hi = _window(N, m0, m1, H, Bk, Fw, known)
        o, r = _span(x, fs, 6.0, m0, m1, lo, hi, known, true_peak=true_peak)
        got.append(o)
        gmin, vmax = min(gmin, r[0]), max(vmax, r[1])
    assert unknown >= 5
    assert np.array_equal(_bits(np.concatenate(got)), _bits(want))
    assert (gmin, vmax) == (rec[0], rec[1]) and gmin < 0.6                       # exact folds


def test_position_independence():
    """An interior span gives the same bits with every global position moved beyond 2^33 (n_total unknown, the window data
    identical), whether or not the move keeps the window's 16-byte phase."""
    fs = 44100
    H, Bk, Fw = loudness.limiter_reach(fs, 3.0, True)
    rng = np.random.default_rng(3)
    x = _noise(rng, 5000)
    x[1500], x[2047], x[2900] = 0.97, -0.96, 0.99
    m0, m1 = 1400, 3100
    lo, hi = _window(5000, m0, m1, H, Bk, Fw, False)
    assert lo > 0
    a, ra = _span(x, fs, 6.0, m0, m1, lo, hi, False)
    assert np.array_equal(_bits(a), _bits(_whole(x, fs, 6.0)[0][m0:m1])) and ra[0] < 0.6
    for shift in (2 ** 33, 2 ** 33 + 1, 2 ** 40 + 1022):
        b, rb = _span(x, fs, 6.0, m0, m1, lo, hi, False, shift=shift)
        assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(ra, rb), shift


@pytest.mark.parametrize("true_peak", [True, False])
def test_exact_pass_through(true_peak):
    fs, gain_db = 44100, 6.0
    gLf = np.float32(10.0 ** (gain_db / 20.0))
    H, Bk, Fw = loudness.limiter_reach(fs, 3.0, True)
    rng = np.random.default_rng(21)
    x = _noise(rng, 5000, amp=0.12)                           # Cl / gL = 0.447: nothing near it, between the samples either
    got, rec = _whole(x, fs, gain_db, true_peak=true_peak)
    assert np.array_equal(_bits(got), _bits(gLf * x)) and rec[0] == 1.0
    x[2600] = 0.97
    got, rec = _whole(x, fs, gain_db, true_peak=true_peak)
    far = np.abs(np.arange(5000) - 2600) > 2 * H + 94
    assert np.array_equal(_bits(got[far]), _bits((gLf * x)[far])) and rec[0] < 0.5
    assert not np.array_equal(_bits(got[~far]), _bits((gLf * x)[~far]))


def test_refusals_launch_nothing():
    fs = 44100
    H, Bk, Fw = loudness.limiter_reach(fs, 3.0, True)
    bank, J, c = ops.true_peak_bank("cuda", 4)
    N = 3000
    xd = torch.zeros((N,), device="cuda")
    buf = torch.full((N + 64,), float("nan"), device="cuda")
    od = buf[:N]
    rec = torch.full((2,), 7.0, dtype=torch.float64, device="cuda")
    lib = _lib.lib()
    nb = lib.vfx_limit_span_workspace_bytes(N, H)
    assert nb > 0 and lib.vfx_limit_span_workspace_bytes(N, 0) == 0 and lib.vfx_limit_span_workspace_bytes(N, 4097) == 0
    assert lib.vfx_limit_span_workspace_bytes(-1, H) == 0
    ws = torch.empty((nb // 8 + 2,), dtype=torch.float64, device="cuda")
    P = lambda t: None if t is None else t.data_ptr()
    good = dict(xw=P(xd), g0=0, wlen=N, n_total=N, m0=0, m1=N, gain=2.0, ceiling=-1.0, H=H, bank=P(bank), J=J, R=4, c=c,
                out=P(od), rec=P(rec), ws=P(ws), nb=nb)

    def call(**kw):
        a = dict(good, **kw)
        return lib.vfx_limit_span_f32(a["xw"], a["g0"], a["wlen"], a["n_total"], a["m0"], a["m1"], C.c_double(a["gain"]),
                                      C.c_double(a["ceiling"]), a["H"], a["bank"], a["J"], a["R"], a["c"], a["out"], a["rec"],
                                      a["ws"], a["nb"], None)

    bad = [dict(wlen=N - 1),                                  # the window ends before the row does
           dict(g0=1, wlen=N - 1),                            # ... or starts behind what output 0 reads
           dict(m0=1000, m1=2000, g0=1000 - 2 * H - Bk + 1, wlen=N - (1000 - 2 * H - Bk + 1)),
           dict(m0=1000, m1=2000, n_total=INT64_MAX, wlen=2000 + 2 * H + Fw - 1),
           dict(m0=10, m1=9), dict(m0=-1), dict(m1=N + 1, wlen=N + 1), dict(g0=-1),
           dict(H=0), dict(H=4097), dict(R=3), dict(R=0), dict(bank=None), dict(J=0), dict(c=4 * J),
           dict(gain=float("nan")), dict(gain=float("inf")), dict(gain=0.0), dict(gain=-2.0),
           dict(ceiling=float("nan")), dict(ceiling=float("inf")),
           dict(nb=nb - 16), dict(ws=P(ws) + 8), dict(ws=None), dict(rec=None), dict(xw=None), dict(out=None),
           dict(out=P(xd) + 4 * (N - 1)), dict(out=P(xd))]
    c0 = lib.vfx_launch_count()
    for kw in bad:
        assert call(**kw) == -1, kw                           # VFX_EINVAL
    assert call(m0=500, m1=500) == 0                          # an empty span: VFX_OK, nothing launched
    assert call(m0=N, m1=N, g0=0, wlen=0) == 0
    torch.cuda.synchronize()
    assert lib.vfx_launch_count() == c0
    assert bool(torch.isnan(buf).all()) and rec.cpu().tolist() == [7.0, 7.0]
    assert ops.limit_span(xd, 0, N, fs, 6.0, 5, 5, od).cpu().tolist() == [1.0, 0.0] and lib.vfx_launch_count() == c0
    assert call() == 0 and call(R=1, bank=None) == 0          # (the good call is one)
    torch.cuda.synchronize()
    assert lib.vfx_launch_count() == c0 + 6 and not bool(torch.isnan(od).any()) and bool(torch.isnan(buf[N:]).all())
    with pytest.raises(_lib.VfxError):
        ops.limit_span(xd[:100], 0, N, fs, 6.0, 0, 50, od)
    with pytest.raises(ValueError):
        ops.limit_span(xd, 0, N, fs, None, 0, 50, od)


# ---- the session and the public function ---------------------------------------------------------------------------------------

CS, OVS = 1.5, 0.25
SIZES = [1, 0, 4410, 70001]
_Z = {}


@pytest.fixture(scope="module")
def vf(seeded_states):
    return voicefixer_amd.VoiceFixer.from_state(*seeded_states)


def _pushed(s, x):
    got, at = [], 0
    for k in SIZES + [len(x)]:
        got.append(s.push(x[at:at + k]))
        at = min(at + k, len(x))
        assert s.position == sum(g.shape[1] for g in got)
    got.append(s.finish())
    return np.concatenate(got, axis=1)


def _open(vf, rate_out, **kw):
    return vf.open_stream(chunk_seconds=CS, overlap_seconds=OVS, output_sample_rate=None if rate_out == 44100 else rate_out, **kw)


def _plain(vf, rate_out):
    """(x, Z, gain_db): Z is the plain session's output, the gain puts its true peak 6 dB above the ceiling."""
    if rate_out not in _Z:
        rng = np.random.default_rng(rate_out)
        x = (0.1 * rng.standard_normal(int(4.2 * 44100) + 311)).astype(np.float32)
        s = _open(vf, rate_out)
        Z = _pushed(s, x)
        assert s.limiter_stats is None and Z.dtype == np.float32
        Cl = 10.0 ** (-1.0 / 20.0)
        _Z[rate_out] = (x, Z, float(20.0 * np.log10(Cl / ref_true_peak(Z[0], rate_out)) + 6.0))
    return _Z[rate_out]


@pytest.mark.parametrize("rate_out", [44100, 48000])
def test_session_equals_limit_of_the_plain_output(vf, rate_out):
    x, Z, gain_db = _plain(vf, rate_out)
    st = {}
    want = voicefixer_amd.limit(Z[0], gain_db, true_peak=True, sample_rate=rate_out, stats=st)
    assert want.shape == Z[0].shape and st["max_reduction_db"] > 5.99 and st["peak_out_db"] <= -1.0 + 3e-4
    s = _open(vf, rate_out, gain_db=gain_db, limiter=True, true_peak=True)
    got = _pushed(s, x)
    assert got.shape == Z.shape and s.position == Z.shape[1]
    assert np.array_equal(_bits(got[0]), _bits(want))
    assert s.limiter_stats == st
    st2 = {}
    assert np.array_equal(_bits(voicefixer_amd.limit(Z[0], gain_db, true_peak=True, sample_rate=rate_out, stats=st2, _span=4096)),
                          _bits(want)) and st2 == st
    both = voicefixer_amd.limit([Z[0, :5000], Z[0]], gain_db, true_peak=True, sample_rate=rate_out, stats=st2)
    assert np.array_equal(_bits(both[1]), _bits(want)) and st2["max_reduction_db"][1] == st["max_reduction_db"]
    # 16 bit: integer for integer, nothing at full scale -- while the same gain alone saturates
    s = _open(vf, rate_out, gain_db=gain_db, limiter=True, true_peak=True, bit_depth=16, dither_seed=5)
    q = _pushed(s, x)
    assert q.dtype == np.int16 and np.array_equal(q[0], voicefixer_amd.quantize(want, 16, "tpdf", 5))
    assert int(np.abs(q.astype(np.int32)).max()) < 32767
    loud = voicefixer_amd.quantize(np.float32(10.0 ** (gain_db / 20.0)) * Z[0], 16, "tpdf", 5)
    assert int(np.abs(loud.astype(np.int32)).max()) >= 32767


@pytest.mark.parametrize("rate_out", [44100, 48000])
def test_session_gain_alone_and_no_gain(vf, rate_out):
    x, Z, gain_db = _plain(vf, rate_out)
    lib = _lib.lib()
    c0 = lib.vfx_launch_count()
    s = _open(vf, rate_out, gain_db=gain_db)
    got = _pushed(s, x)
    c1 = lib.vfx_launch_count()
    assert s.limiter_stats is None
    assert np.array_equal(_bits(got), _bits(np.float32(10.0 ** (gain_db / 20.0)) * Z))
    s = _open(vf, rate_out, gain_db=None, limiter=False)
    assert np.array_equal(_bits(_pushed(s, x)), _bits(Z))      # today's path: the same bits and the same launches
    assert lib.vfx_launch_count() - c1 == c1 - c0
