"""The streaming loudness leveller on the MI355X (vfx_level_span_f32; ops.level_span, voicefixer_amd.level,
open_stream(leveller=...)) against the float64 specification of voicefixer_amd/loudness.py (leveller_energies, leveller_gains,
level_reference), and against itself: a row cut into spans, fed in blocks or placed elsewhere in memory gives the same bits.

Bounds.  Anchors: |G_device - G_spec| <= 0.002 dB -- twice the 0.001 LU DESIGN.md 3.10 reports for the same fp32
filter on whole files (a 3 s window averages less) -- under the condition, asserted on the specification, that every anchor's
l_q is at least 0.5 LU away from the gate, so that no hold can flip between fp32 and fp64.  Samples:
|out - ref| <= (10^(0.002 / 20) - 1 + 4 * 2^-24) |ref|: the anchor bound as a ratio, and one rounding each for a_q, the
difference, the product and the sum of the interpolation and for the final product being placed differently around a gain
that differs -- four of them cover it.  Observed on the MI355X: see DESIGN.md 3.17."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import voicefixer_amd  # noqa: E402
from voicefixer_amd import _lib, api, loudness, ops  # noqa: E402

PAD = 40
INT64_MAX = 2 ** 63 - 1
ANCHOR_DB = 0.002
SAMPLE_REL = 10.0 ** (ANCHOR_DB / 20.0) - 1.0 + 4 * 2.0 ** -24
_SPEC = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _steps(rng, n, fs, levels=(0.02, 0.2, 0.005, 0.08)):
    """Noise whose level steps every 0.7 s."""
    x = rng.standard_normal(n)
    seg = int(0.7 * fs)
    for i in range(0, n, seg):
        x[i:i + seg] *= levels[(i // seg) % len(levels)]
    return x.astype(np.float32)


def _gap(rng, fs, n):
    """2 s of noise, 4 s of digital silence, noise to the end."""
    x = (0.05 * rng.standard_normal(n)).astype(np.float32)
    x[2 * fs:6 * fs] = 0.0
    return x


def _spec(key, x, fs, T, mg, gate):
    """The float64 specification of a row, computed once; the 0.5 LU condition is asserted here."""
    if key not in _SPEC:
        st = {}
        ref = loudness.level_reference(x, fs, T, mg, gate, stats=st)
        l = st["l"]
        assert np.all(np.abs(l[np.isfinite(l)] - gate) >= 0.5), (key, "an anchor within 0.5 LU of the gate")
        _SPEC[key] = (ref, st)
    return _SPEC[key]


def _run(x, fs, T, mg=12.0, gate=-50.0, cuts=(), xoff=0, ooff=0, each=None):
    """The row through ops.level_span in the spans [0, c1), [c1, c2), ... [ck, N) from a window that holds the whole row at
    ``xoff`` floats past a 16-byte boundary, NaN around it and around ``out`` (``ooff`` floats past a boundary).  Returns
    (out, state); ``each(m1, state)`` is called after every span."""
    N = len(x)
    buf = np.full(N + 2 * PAD + 4, np.nan, np.float32)
    buf[PAD + xoff:PAD + xoff + N] = x
    xd = torch.from_numpy(buf).cuda()
    od = torch.full((N + 2 * PAD + 4,), float("nan"), device="cuda")
    state = torch.full((loudness.LEVELLER_STATE,), 7.0, dtype=torch.float64, device="cuda")   # (m0 = 0 initialises it)
    lib = _lib.lib()
    edges = [0] + [c for c in cuts if 0 < c < N] + [N]
    for m0, m1 in zip(edges[:-1], edges[1:]):
        c0 = lib.vfx_launch_count()
        ops.level_span(xd[PAD + xoff:PAD + xoff + N], 0, N, fs, T, m0, m1, od[PAD + ooff + m0:PAD + ooff + m1], state, mg, gate)
        assert 2 <= lib.vfx_launch_count() - c0 <= 3
        if each is not None:
            each(m1, state.cpu().numpy())
    out = od.cpu().numpy()
    assert np.all(np.isnan(out[:PAD + ooff])) and np.all(np.isnan(out[PAD + ooff + N:])), "out canaries"
    assert not np.any(np.isnan(out[PAD + ooff:PAD + ooff + N]))
    assert np.array_equal(xd.cpu().numpy(), buf, equal_nan=True)
    st = state.cpu().numpy()
    assert st[6] == 0.0
    return out[PAD + ooff:PAD + ooff + N], st


def _against_spec(key, x, fs, T, mg=12.0, gate=-50.0):
    """One call over the whole row against the specification's samples and counts; the row again in spans of one quarter, which
    leaves every anchor's G in the state in turn, against the specification's anchors.  Returns the worst anchor error (dB) and
    the worst sample error over the bound."""
    hop, N = loudness.hop_length(fs), len(x)
    ref, sp = _spec(key, x, fs, T, mg, gate)
    got, st = _run(x, fs, T, mg, gate)
    Q = N // hop
    assert (int(st[2]), int(st[3])) == (Q + 1, int(sp["held"].sum())) == (sp["anchors"], sp["gated"]), key
    G = np.full(Q + 1, np.nan)

    def each(m1, s):
        na = int(s[2])
        assert na == loudness.leveller_counts(m1, hop, Q)[0]
        G[na - 1] = s[4]
        if na == 2:
            G[0] = 20.0 * np.log10(s[8])

    cut, _ = _run(x, fs, T, mg, gate, cuts=range(hop, N, hop), each=each)
    assert np.array_equal(_bits(cut), _bits(got)), key
    assert not np.any(np.isnan(G))
    aerr = float(np.abs(G - sp["G"]).max())
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    tol = SAMPLE_REL * np.abs(ref.astype(np.float64))
    serr = float((err / np.maximum(tol, 1e-300)).max()) if N else 0.0
    print("leveller %s: N = %d, worst |G - spec| = %.2e dB (bound %.0e), worst sample error / bound = %.3f; G in [%.2f, %.2f], "
          "%d of %d gated" % (key, N, aerr, ANCHOR_DB, serr, st[0], st[1], int(st[3]), int(st[2])))
    assert aerr <= ANCHOR_DB, (key, aerr, int(np.abs(G - sp["G"]).argmax()))
    assert np.all(err <= tol), (key, serr, int((err - tol).argmax()))
    assert abs(st[0] - sp["min_gain_db"]) <= ANCHOR_DB and abs(st[1] - sp["max_gain_db"]) <= ANCHOR_DB
    return aerr, serr


def test_lengths_against_the_float64_specification():
    """fs = 8000, hop = 800: a row shorter than a quarter, exactly one, around the first unclipped look-ahead, every window
    clipped (29 hop + 5), clipped at both ends and unclipped between (45 hop + 17)."""
    fs, hop = 8000, 800
    rng = np.random.default_rng(5)
    for n in (hop - 1, hop, 11 * hop - 1, 11 * hop + 1, 29 * hop + 5, 45 * hop + 17):
        x = _steps(rng, n, fs)
        _against_spec("steps-%d" % n, x, fs, -20.0)
        if n < hop:
            got, st = _run(x, fs, -20.0)
            assert np.array_equal(_bits(got), _bits(x)) and (st[2], st[3], st[4]) == (1.0, 1.0, 0.0)


def test_gap_and_clamps_against_the_float64_specification():
    fs, hop = 8000, 800
    rng = np.random.default_rng(6)
    x = _gap(rng, fs, 80 * hop + 3)
    _against_spec("gap", x, fs, -20.0)
    sp = _spec("gap", x, fs, -20.0, 12.0, -50.0)[1]
    assert sp["held"].sum() >= 10 and not sp["held"][:15].any()            # the hold is exercised, behind valid anchors
    quiet = (0.0008 * rng.standard_normal(45 * hop + 17)).astype(np.float32)     # about -62 LUFS: wants far more than 12 dB
    _against_spec("max-clamp", quiet, fs, -16.0, 12.0, -69.0)
    assert np.all(_spec("max-clamp", quiet, fs, -16.0, 12.0, -69.0)[1]["G"] == 12.0)
    loud = (0.3 * rng.standard_normal(45 * hop + 17)).astype(np.float32)         # about -10 LUFS against a target of -60
    _against_spec("cut-clamp", loud, fs, -60.0, 0.0, -70.0)
    assert np.all(_spec("cut-clamp", loud, fs, -60.0, 0.0, -70.0)[1]["G"] == -40.0)


@pytest.mark.parametrize("fs", [44100, 48000, 192000])
def test_rates_against_the_float64_specification(fs):
    rng = np.random.default_rng(fs)
    x = _steps(rng, int(1.5 * fs) + 13, fs)
    _against_spec("steps-%d Hz" % fs, x, fs, -23.0)


@pytest.mark.parametrize("fs,n", [(8000, 64003), (44100, 66163)])
def test_split_invariance_bit_for_bit(fs, n):
    """``level`` in spans of 1237, hop, hop + 1 and 2^22 outputs, and a _SpanLeveller fed in blocks of 1, 4410, 7, 70001, ...
    samples: the same bits and the same record."""
    hop = loudness.hop_length(fs)
    rng = np.random.default_rng(n)
    x = _gap(rng, fs, n) if fs == 8000 else _steps(rng, n, fs)
    want, st = None, None
    for span in (1 << 22, 1237, hop, hop + 1):
        s = {}
        got = voicefixer_amd.level(x, -20.0, sample_rate=fs, stats=s, _span=span)
        if want is None:
            want, st = got, s
            assert st["anchors"] == n // hop + 1 and st["max_gain_db"] > st["min_gain_db"]
            whole, dst = _run(x, fs, -20.0)                    # ... which is one call over the whole row
            assert np.array_equal(_bits(whole), _bits(want))
            assert (dst[0], dst[1], dst[2], dst[3]) == (st["min_gain_db"], st["max_gain_db"], st["anchors"], st["gated"])
        assert np.array_equal(_bits(got), _bits(want)) and s == st, span
    lv = api._SpanLeveller(fs, -20.0)
    xd = torch.from_numpy(x).cuda()
    parts, at, i, held = [], 0, 0, 0
    while at < n:
        k = (1, 4410, 7, 70001)[i % 4]
        parts.append(lv.feed(xd[at:at + k]))
        at, i = min(at + k, n), i + 1
        held = max(held, lv.win.numel() - k)
    parts.append(lv.finish("cuda"))
    assert np.array_equal(_bits(torch.cat(parts).cpu().numpy()), _bits(want)) and lv.stats() == st
    assert held <= 33 * hop                          # O(3.3 s) of samples beyond a block, whatever was pushed


def test_position_independence():
    """The same row from windows at different offsets of a larger buffer (not all of them aligned to 16 bytes), into outputs at
    different offsets: the same bits, the same state."""
    fs = 44100
    rng = np.random.default_rng(9)
    x = _steps(rng, 66163, fs)
    want, st = _run(x, fs, -20.0)
    for xoff, ooff in ((1, 0), (2, 3), (3, 1), (0, 2)):
        got, s = _run(x, fs, -20.0, xoff=xoff, ooff=ooff, cuts=(30001,))
        assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(s, st), (xoff, ooff)


def test_short_rows_come_back_as_they_are():
    for fs in (8000, 44100):
        hop = loudness.hop_length(fs)
        x = _steps(np.random.default_rng(fs), hop - 1, fs)
        s = {}
        assert np.array_equal(_bits(voicefixer_amd.level(x, -16.0, sample_rate=fs, stats=s)), _bits(x))
        assert s == {"min_gain_db": 0.0, "max_gain_db": 0.0, "anchors": 1, "gated": 1}
    both = voicefixer_amd.level([x, np.zeros(0, np.float32)], -16.0, sample_rate=44100, stats=s)
    assert np.array_equal(_bits(both[0]), _bits(x)) and both[1].shape == (0,) and s["anchors"] == [1, 0]


def test_refusals_launch_nothing():
    fs, hop = 8000, 800
    N = 30 * hop
    p = loudness.leveller_plan(fs)
    xd = torch.zeros((N,), device="cuda")
    buf = torch.full((N + 64,), float("nan"), device="cuda")
    od = buf[:N]
    state = torch.full((loudness.LEVELLER_STATE,), 7.0, dtype=torch.float64, device="cuda")
    mpow = torch.from_numpy(p["mpow"]).cuda()
    coef = (C.c_double * 10)(*[float(v) for v in p["coef"]])
    bad_coef = (C.c_double * 10)(*([float("nan")] + [float(v) for v in p["coef"][1:]]))
    lib = _lib.lib()
    nb = lib.vfx_level_span_workspace_bytes(N, hop)
    assert nb > 0 and lib.vfx_level_span_workspace_bytes(-1, hop) == 0 and lib.vfx_level_span_workspace_bytes(N, 399) == 0
    assert lib.vfx_level_span_workspace_bytes(N, 19201) == 0 and lib.vfx_level_span_workspace_bytes(2 ** 30 + 1, hop) == 0
    ws = torch.empty((nb // 8 + 2,), dtype=torch.float64, device="cuda")
    P = lambda t: None if t is None else t.data_ptr()
    good = dict(xw=P(xd), g0=0, wlen=N, n_total=N, m0=0, m1=N, fs=fs, coef=coef, mpow=P(mpow), S=p["S"], T=-16.0, mg=12.0,
                gate=-50.0, state=P(state), out=P(od), ws=P(ws), nb=nb)

    def call(**kw):
        a = dict(good, **kw)
        return lib.vfx_level_span_f32(a["xw"], a["g0"], a["wlen"], a["n_total"], a["m0"], a["m1"], a["fs"], a["coef"], a["mpow"],
                                      a["S"], C.c_double(a["T"]), C.c_double(a["mg"]), C.c_double(a["gate"]), a["state"],
                                      a["out"], a["ws"], a["nb"], None)

    bad = [dict(wlen=N - 1),                                  # a short window: the last quarter's region ends behind it
           dict(m0=0, m1=5 * hop, wlen=15 * hop - 1),         # ... the look-ahead of anchor 5 reads quarter 14
           dict(m0=15 * hop, m1=16 * hop, g0=15 * hop + 1, wlen=N - 15 * hop - 1),     # ... starts behind the first output
                      dict(n_total=INT64_MAX, m1=20 * hop + 1),          # beyond the ready bound (30 - 10) hop with the end unknown
           dict(n_total=INT64_MAX, m1=N),
           dict(fs=192001), dict(fs=384000), dict(fs=3999), dict(S=p["S"] + 32), dict(S=0),
           dict(mg=40.5), dict(mg=-0.1), dict(mg=float("nan")), dict(T=0.0), dict(T=-70.5), dict(T=float("nan")),
           dict(gate=-16.0), dict(gate=-71.0), dict(gate=float("nan")), dict(coef=bad_coef),
           dict(m0=10, m1=9), dict(m0=-1), dict(m1=N + 1, wlen=N + 1), dict(g0=-1),
           dict(nb=nb - 256), dict(ws=P(ws) + 8), dict(ws=None), dict(state=None), dict(xw=None), dict(out=None), dict(mpow=None),
           dict(coef=None), dict(out=P(xd) + 4 * (N - 1)), dict(out=P(xd))]
    c0 = lib.vfx_launch_count()
    for kw in bad:
        assert call(**kw) == -1, kw                           # VFX_EINVAL
    assert call(m0=500, m1=500) == 0                          # an empty span: VFX_OK, nothing launched
    torch.cuda.synchronize()
    assert lib.vfx_launch_count() == c0
    assert bool(torch.isnan(buf).all()) and state.cpu().tolist() == [7.0] * loudness.LEVELLER_STATE
    assert call(n_total=INT64_MAX, m1=20 * hop) == 0                           # (three launches)
    assert call(m0=20 * hop, out=P(od) + 4 * 20 * hop) == 0                    # (two: no quarter is new)
    torch.cuda.synchronize()
    assert lib.vfx_launch_count() == c0 + 5 and not bool(torch.isnan(od).any()) and bool(torch.isnan(buf[N:]).all())
    assert state.cpu().tolist()[2:7] == [31.0, 31.0, 0.0, 30.0, 0.0]             # silence: every anchor gated, the gain held at 0
    assert call(m0=5 * hop, m1=6 * hop, out=P(od) + 4 * 5 * hop) == 0     # out of order: memory-safe, and the state says so
    assert state.cpu().tolist()[6] == 1.0
    for kw in (dict(max_gain_db=41.0), dict(gate=-10.0), dict(max_gain_db=True)):
        with pytest.raises(ValueError):
            ops.level_span(xd, 0, N, fs, -16.0, 0, N, od, state, **kw)
    with pytest.raises(ValueError):
        ops.level_span(xd, 0, N, 384000, -16.0, 0, N, od, state)
    with pytest.raises(_lib.VfxError):
        ops.level_span(xd[:100], 0, N, fs, -16.0, 0, 50, od, state)


# ---- the session ----------------------------------------------------------------------------------------------------------------

CS, OVS = 1.5, 0.25
SIZES = [1, 0, 4410, 7, 70001]
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
    """(x, Z): Z is the output of the session without a leveller; the input's level steps, so the gain has to move."""
    if rate_out not in _Z:
        rng = np.random.default_rng(rate_out)
        x = _steps(rng, 5 * 44100 + 311, 44100, levels=(0.1, 0.01, 0.05))
        s = _open(vf, rate_out)
        Z = _pushed(s, x)
        assert s.leveller_stats is None and Z.dtype == np.float32
        _Z[rate_out] = (x, Z)
    return _Z[rate_out]


@pytest.mark.parametrize("rate_out", [44100, 48000])
def test_session_equals_level_of_the_plain_output(vf, rate_out):
    x, Z = _plain(vf, rate_out)
    st = {}
    want = voicefixer_amd.level(Z[0], -20.0, sample_rate=rate_out, stats=st)
    assert want.shape == Z[0].shape and st["anchors"] == Z.shape[1] // loudness.hop_length(rate_out) + 1
    assert st["gated"] < st["anchors"] and not np.array_equal(want, Z[0])
    s = _open(vf, rate_out, leveller=-20)
    got = _pushed(s, x)
    assert got.shape == Z.shape and s.position == Z.shape[1]
    assert np.array_equal(_bits(got[0]), _bits(want))
    assert s.leveller_stats == st and s.limiter_stats is None
    # the limiter behind it, without a gain: at 0 dB
    lst = {}
    lim = voicefixer_amd.limit(want, gain_db=0.0, true_peak=True, sample_rate=rate_out, stats=lst)
    s = _open(vf, rate_out, leveller=-20, limiter=True, true_peak=True)
    got = _pushed(s, x)
    assert np.array_equal(_bits(got[0]), _bits(lim)) and s.leveller_stats == st and s.limiter_stats == lst
    # ... and the word length behind both
    s = _open(vf, rate_out, leveller=-20, limiter=True, true_peak=True, bit_depth=16, dither_seed=5)
    q = _pushed(s, x)
    assert q.dtype == np.int16 and np.array_equal(q[0], voicefixer_amd.quantize(lim, 16, "tpdf", 5))
    assert s.leveller_stats == st
    # a fixed gain follows the leveller
    s = _open(vf, rate_out, leveller=-20, gain_db=-3.0)
    assert np.array_equal(_bits(_pushed(s, x)[0]), _bits(np.float32(10.0 ** (-3.0 / 20.0)) * want))
