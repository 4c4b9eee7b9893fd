"""The streaming loudness leveller on the host: the argument checks of ``level`` and ``open_stream(leveller=...)``, and the float64
specification of voicefixer_amd/loudness.py (leveller_energies, leveller_gains, level_reference) against what it
is defined to be: the truncated warm-up against the whole-row filter, the steady state, the hold, the clamps and the ready rule."""
import numpy as np
import pytest
from scipy.signal import lfilter

import voicefixer_amd
from voicefixer_amd import VoiceFixer, loudness


def _vf():
    return VoiceFixer.__new__(VoiceFixer)       # (no weights, no device: the checks come before either)


def test_exports_and_constants():
    assert "level" in voicefixer_amd.__all__ and callable(voicefixer_amd.level)
    assert (loudness.LEVELLER_WARMUP, loudness.LEVELLER_BEHIND, loudness.LEVELLER_AHEAD, loudness.LEVELLER_MAX_CUT) == (2, 20, 10, 40.0)
    assert [loudness.leveller_ready(n, 800) for n in (0, 7999, 8000, 8799, 8800, 9599, 9600)] == [0, 0, 0, 0, 800, 800, 1600]
    assert loudness.leveller_counts(0, 800) == (0, 0) and loudness.leveller_counts(1, 800) == (2, 11)
    assert loudness.leveller_counts(800, 800) == (2, 11) and loudness.leveller_counts(801, 800) == (3, 12)
    assert loudness.leveller_counts(801, 800, 5) == (3, 5) and loudness.leveller_counts(10 ** 6, 800, 5) == (6, 5)
    assert loudness.leveller_counts(5, 800, 0) == (1, 0)
    for fs in (4000, 8000, 44100, 48000, 192000):
        p = loudness.leveller_plan(fs)
        assert p["S"] % 32 == 0 and 256 * p["S"] >= 3 * p["hop"] > 256 * (p["S"] - 32) and p["mpow"].shape == (8, 4, 4)
        M = np.linalg.matrix_power(loudness.transition(fs), p["S"])
        assert np.allclose(p["mpow"][3], np.linalg.matrix_power(M, 8), rtol=1e-9, atol=1e-300)


@pytest.mark.parametrize("kw", [dict(target=0.0), dict(target=-70.5), dict(target=None), dict(target=True), dict(target="-16"),
                                dict(target=float("nan")), dict(max_gain_db=-0.5), dict(max_gain_db=40.5), dict(max_gain_db=True),
                                dict(max_gain_db=None), dict(gate=-16.0), dict(gate=-10.0), dict(gate=-70.5), dict(gate=False),
                                dict(sample_rate=192001), dict(sample_rate=768000), dict(sample_rate=True), dict(stats=[]),
                                dict(_span=0)])
def test_level_refuses_before_the_device(kw):
    with pytest.raises(ValueError):
        voicefixer_amd.level(np.zeros(100, np.float32), **kw)


def test_level_refuses_a_matrix():
    with pytest.raises(ValueError):
        voicefixer_amd.level(np.zeros((2, 100), np.float32))


@pytest.mark.parametrize("kw", [dict(leveller=0.0), dict(leveller=-71), dict(leveller=True), dict(leveller="-16"),
                                dict(leveller=-16, leveller_max_gain_db=41), dict(leveller=-16, leveller_max_gain_db=-1),
                                dict(leveller=-16, leveller_max_gain_db=False), dict(leveller=-16, leveller_gate=-16),
                                dict(leveller=-16, leveller_gate=-71), dict(leveller=-16, leveller_gate=True),
                                dict(leveller=-16, output_sample_rate=384000)])
def test_open_stream_refuses_before_the_device(kw):
    with pytest.raises(ValueError):
        _vf().open_stream(**kw)


def test_open_stream_accepts_a_leveller():
    s = _vf().open_stream(leveller=-16, limiter=True)
    assert s._lev is not None and s._lim is not None and s._lim.gain_db == 0.0 and s._gain is None
    assert s.leveller_stats == {"min_gain_db": 0.0, "max_gain_db": 0.0, "anchors": 0, "gated": 0}
    s = _vf().open_stream(leveller=-23.0, leveller_max_gain_db=6, leveller_gate=-60, gain_db=3.0, limiter=True, output_sample_rate=48000)
    assert (s._lev.target, s._lev.max_gain_db, s._lev.gate, s._lev.hop, s._lim.gain_db) == (-23.0, 6.0, -60.0, 4800, 3.0)
    assert _vf().open_stream().leveller_stats is None and _vf().open_stream(leveller=-16).limiter_stats is None
    with pytest.raises(NotImplementedError):
        _vf().open_stream(limiter=True)                       # without a gain and without a leveller: as before
    with pytest.raises(NotImplementedError):
        _vf().restore_stream(np.zeros(50000, np.float32), limiter=True)
    with pytest.raises(TypeError):
        _vf().restore_stream(np.zeros(50000, np.float32), leveller=-16)


def _whole_row_quarters(x, fs):
    """The quarter sums of ONE filter over the whole row (float64, the fp32-rounded coefficients)."""
    c = loudness.coefficients(fs).astype(np.float32).astype(np.float64)
    y = lfilter(c[5:8], [1.0, c[8], c[9]], lfilter(c[0:3], [1.0, c[3], c[4]], np.asarray(x, np.float64)))
    hop = loudness.hop_length(fs)
    Q = len(x) // hop
    return np.array([float(np.dot(y[q * hop:(q + 1) * hop], y[q * hop:(q + 1) * hop])) for q in range(Q)])


@pytest.mark.parametrize("fs", [8000, 44100, 192000])
def test_truncated_warm_up_against_the_whole_row_filter(fs):
    """Largest relative difference seen: see DESIGN.md 3.17; the transition powers predict < 1e-15, the bound leaves seven
    decades, so only a wrong region fails it."""
    rng = np.random.default_rng(fs)
    n = int(1.2 * fs) + 17
    x = 0.1 * rng.standard_normal(n) + 0.3                    # (an offset: the high-pass has something to forget)
    x[: n // 3] *= 30.0                                       # a loud start, so that what is truncated is not small
    E = loudness.leveller_energies(x, fs)
    W = _whole_row_quarters(x, fs)
    assert E.shape == W.shape == (n // loudness.hop_length(fs),)
    rel = float(np.abs(E / W - 1.0).max())
    print("leveller truncation at %d Hz: largest relative difference of E_q = %.2e" % (fs, rel))
    assert rel < 1e-9
    assert np.array_equal(E[:3], W[:3])                       # the regions of the first three quarters start at 0: the same filter


def test_steady_state():
    fs, T = 8000, -18.0
    hop = loudness.hop_length(fs)
    x = 0.1 * np.sin(2 * np.pi * 997.0 * np.arange(8 * fs) / fs)
    E = loudness.leveller_energies(x, fs)
    r = loudness.leveller_gains(E, len(x), fs, T)
    Q = len(x) // hop
    W = _whole_row_quarters(x, fs)
    for q in range(20, Q - 9):                                # the unclipped windows
        l = -0.691 + 10.0 * np.log10(W[q - 20:q + 10].sum() / (30.0 * hop))
        assert abs(r["G"][q] - (T - l)) < 1e-9 and abs(r["l"][q] - l) < 1e-9 and not r["held"][q]
    # 997 Hz at -20 dBFS peak: -23.0 dBFS RMS, K-weighting ~ +0.0 dB at 1 kHz... the gain is that of a sine of this level
    assert abs(r["G"][40] - (T - (-0.691 + 10 * np.log10(0.005) + 0.0))) < 0.8
    assert np.all(r["a"] == np.float32(10.0 ** (r["G"] / 20.0)))


def test_gating_holds_the_gain():
    fs = 8000
    hop = loudness.hop_length(fs)
    rng = np.random.default_rng(1)
    x = 0.05 * rng.standard_normal(9 * fs)
    x[3 * fs:7 * fs] = 0.0                                    # a 4 s gap
    st = {}
    y = loudness.level_reference(x, fs, -20.0, stats=st)
    g = st["held"]
    first = int(np.argmax(g))
    assert 30 < first <= 51 and g[first:60].all() and not g[:first].any() and not g[62:].any()
    assert np.all(st["G"][g] == st["G"][first - 1]) and np.all(st["a"][g] == st["a"][first - 1])
    lo, hi = first * hop, 60 * hop
    assert np.array_equal(y[lo:hi], (x[lo:hi].astype(np.float32) * st["a"][first]))     # a constant gain through the hold
    assert st["anchors"] == 91 and st["gated"] == g.sum()
    # nothing valid yet: the gain held is G_{-1} = 0 dB
    z = np.zeros(3 * fs)
    z[2 * fs:] = 0.05 * rng.standard_normal(fs)
    r = loudness.leveller_gains(loudness.leveller_energies(z, fs), len(z), fs, -20.0)
    assert r["held"][:10].all() and np.all(r["G"][:10] == 0.0) and np.all(r["a"][:10] == 1.0) and not r["held"][12]


def test_both_clamps_are_reached():
    fs = 8000
    rng = np.random.default_rng(2)
    quiet = 0.0008 * rng.standard_normal(4 * fs)
    r = loudness.leveller_gains(loudness.leveller_energies(quiet, fs), len(quiet), fs, -16.0, 12.0, -69.0)
    assert not r["held"].any() and np.all(r["G"] == 12.0) and np.all(-16.0 - r["l"] > 30.0)
    r = loudness.leveller_gains(loudness.leveller_energies(quiet, fs), len(quiet), fs, -16.0, 40.0, -69.0)
    assert np.all(r["G"] == 40.0)
    loud = 0.3 * rng.standard_normal(4 * fs)
    r = loudness.leveller_gains(loudness.leveller_energies(loud, fs), len(loud), fs, -60.0, 0.0, -70.0)
    assert not r["held"].any() and np.all(r["G"] == -40.0) and np.all(-60.0 - r["l"] < -45.0)
    assert np.all(r["a"] == np.float32(0.01))


def test_short_rows_and_the_tail():
    fs = 8000
    rng = np.random.default_rng(3)
    x = (0.1 * rng.standard_normal(799)).astype(np.float32)
    st = {}
    assert np.array_equal(loudness.level_reference(x, fs, stats=st), x) and (st["anchors"], st["gated"]) == (1, 1)
    assert loudness.level_reference(np.zeros(0, np.float32), fs).shape == (0,)
    x = (0.1 * rng.standard_normal(5 * 800 + 300)).astype(np.float32)
    y = loudness.level_reference(x, fs, -30.0, stats=st)
    a = st["a"]
    assert a.shape == (6,) and np.array_equal(y[4000:], x[4000:] * a[5])       # behind the last complete quarter: a_Q
    assert np.array_equal(y[0:4000:800], x[0:4000:800] * a[:5])               # at an anchor: its own gain
    t = 800 + 123
    f = np.float32(123) / np.float32(800)
    assert y[t] == x[t] * np.float32(a[1] + np.float32(np.float32(a[2] - a[1]) * f))


@pytest.mark.parametrize("n_known", [0, 799, 8800, 8801, 12345, 20000, 36017])
def test_ready_rule_by_brute_force(n_known):
    """Whatever follows the first n_known samples -- other data, or the end of the row -- the outputs below leveller_ready are
    the same bits."""
    fs, hop, N = 8000, 800, 45 * 800 + 17
    rng = np.random.default_rng(4)
    x = (rng.standard_normal(N) * np.repeat([0.02, 0.3, 0.004, 0.1, 0.05], N // 5 + 1)[:N]).astype(np.float32)
    ready = loudness.leveller_ready(n_known, hop)
    assert ready == max(0, (n_known // hop - 10) * hop)
    want = loudness.level_reference(x, fs, -20.0)[:ready]
    other = x.copy()
    other[n_known:] = (0.5 * rng.standard_normal(N - n_known)).astype(np.float32)
    longer = np.concatenate([x[:n_known], np.zeros(7000, np.float32)])
    for v in (other, x[:n_known], longer):
        got = loudness.level_reference(v, fs, -20.0)[:ready]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if ready + hop <= n_known and n_known < N:                # ... and the rule is tight: the next quarter does depend on it
        assert not np.array_equal(loudness.level_reference(other, fs, -20.0)[:ready + hop], loudness.level_reference(x, fs, -20.0)[:ready + hop])
