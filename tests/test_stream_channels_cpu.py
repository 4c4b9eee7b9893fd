"""Every channel in a streaming session on the host: the float64 specifications of the LINKED limiter
(``ref_fixed_linked``, here) and of the linked leveller (loudness.leveller_energies_linked / level_reference_linked), their
ready rules for C > 1, the bookkeeping of a ``channels="all"`` session with the device replaced by host stand-ins, the argument
rules and the public surface.  No GPU."""
import inspect
import os
import re

import numpy as np
import pytest
from scipy.ndimage import minimum_filter1d

import voicefixer_amd
from voicefixer_amd import _lib, api, loudness
from test_limiter_cpu import ref_envelope, ref_window
from test_stream_limiter_cpu import ref_fixed
from test_stream_session_cpu import _FakeVF, host_ops  # noqa: F401  (host_ops: the fixture of the session's stand-ins)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ref_fixed_linked(X, fs, gL, ceiling_db=-1.0, ms=3.0, true_peak=True):
    """F_C in float64 on a programme X (C, N): the steps of ``ref_fixed`` on ONE envelope e[n] = max_c e_c[n].  A dict with
    ``out`` (C, N), ``e``, ``c``, ``m``, ``g`` (N,) and ``H``."""
    X = np.asarray(X, np.float64)
    C, N = X.shape
    Cl = 10.0 ** (ceiling_db / 20.0)
    H, w = ref_window(fs, ms)
    if N == 0:
        z = np.zeros(0)
        return dict(out=np.zeros((C, 0)), e=z, c=z, m=z, g=z, H=H)
    e = np.max(np.stack([ref_envelope(X[c], fs, true_peak) for c in range(C)]), axis=0)
    c = np.where(e > 0, np.minimum(1.0, Cl / (gL * np.where(e > 0, e, 1.0))), 1.0)
    m = minimum_filter1d(c, size=2 * H + 1, mode="constant", cval=1.0)
    d = np.pad(1.0 - m, H, mode="edge")                       # m[clamp(n + k, 0, N - 1)]
    g = 1.0 - np.convolve(d, w, mode="valid")
    return dict(out=gL * g[None] * X, e=e, c=c, m=m, g=g, H=H)


def _row(rng, n, peaks, amp=0.1):
    x = amp * rng.uniform(-1, 1, n)
    for p in peaks:
        if 0 <= p < n:
            x[p] = 0.97 if p % 2 == 0 else -0.93
    return x.astype(np.float32)


def _steps(rng, n, fs, levels=(0.02, 0.2, 0.005, 0.08)):
    x = rng.standard_normal(n)
    seg = int(0.7 * fs)
    for i in range(0, n, seg):
        x[i:i + seg] *= levels[(i // seg) % len(levels)]
    return x.astype(np.float32)


# ---- the specifications, exact -----------------------------------------------------------------------------------------------

def test_linked_leveller_specification_exact():
    fs, hop = 8000, 800
    rng = np.random.default_rng(1)
    N = 33 * hop + 5
    x, y = _steps(rng, N, fs), _steps(rng, N, fs, levels=(0.1, 0.01, 0.3))
    E = loudness.leveller_energies(x, fs)
    assert np.array_equal(loudness.leveller_energies_linked(x[None], fs), E)                    # C = 1: 0 + 1 E
    st1, stm = {}, {}
    mono = loudness.level_reference(x, fs, -20.0, stats=stm)
    one = loudness.level_reference_linked(x[None], fs, -20.0, stats=st1)
    assert one.shape == (1, N) and np.array_equal(one[0].view(np.uint32), mono.view(np.uint32))
    assert np.array_equal(st1["a"], stm["a"]) and st1["gated"] == stm["gated"] and st1["anchors"] == N // hop + 1
    # two identical channels at 0.5 each: 0.5 E + 0.5 E = E in float64
    st = {}
    two = loudness.level_reference_linked(np.stack([x, x]), fs, -20.0, weights=[0.5, 0.5], stats=st)
    assert np.array_equal(st["a"], stm["a"]) and np.array_equal(st["G"], stm["G"])
    assert np.array_equal(two[0].view(np.uint32), mono.view(np.uint32)) and np.array_equal(two[1], two[0])
    # weights [1, 0]: the gains of channel 0 alone, applied to both
    st = {}
    both = loudness.level_reference_linked(np.stack([x, y]), fs, -20.0, weights=[1.0, 0.0], stats=st)
    assert np.array_equal(st["a"], stm["a"]) and np.array_equal(both[0].view(np.uint32), mono.view(np.uint32))
    assert np.array_equal(both[1].view(np.uint32), loudness.leveller_apply(y, stm["a"], hop).view(np.uint32))
    # the default weights are BS.1770-4's: two channels sum, and the sum is the ascending one
    E2 = loudness.leveller_energies_linked(np.stack([x, y]), fs)
    assert np.array_equal(E2, (0.0 + 1.0 * E) + 1.0 * loudness.leveller_energies(y, fs))
    six = np.stack([x, y, x, y, x, y])
    w = loudness.channel_weights(6)
    assert w[3] == 0.0
    want = np.zeros(N // hop)
    for c in range(6):
        want = want + w[c] * loudness.leveller_energies(six[c], fs)
    assert np.array_equal(loudness.leveller_energies_linked(six, fs), want)
    for bad in (x, np.zeros((9, N)), np.zeros((2, 2, 8))):
        with pytest.raises(ValueError):
            loudness.leveller_energies_linked(bad, fs)
    with pytest.raises(ValueError):
        loudness.leveller_energies_linked(np.stack([x, y]), fs, [1.0])


@pytest.mark.parametrize("fs,true_peak", [(44100, True), (8000, True), (44100, False)])
def test_linked_limiter_specification_exact(fs, true_peak):
    rng = np.random.default_rng(fs + true_peak)
    H, Bk, Fw = loudness.limiter_reach(fs, 3.0, true_peak)
    N = 8 * H + 700
    x = _row(rng, N, [3 * H + 100])
    mono = ref_fixed(x, fs, 2.0, -1.0, 3.0, true_peak)
    one = ref_fixed_linked(x[None], fs, 2.0, -1.0, 3.0, true_peak)
    assert np.array_equal(one["out"][0], mono["out"]) and np.array_equal(one["g"], mono["g"])     # C = 1
    same = ref_fixed_linked(np.stack([x, x, x]), fs, 2.0, -1.0, 3.0, true_peak)
    assert all(np.array_equal(same["out"][c], mono["out"]) for c in range(3))                    # identical channels
    # a peak in channel 1 only reduces channel 0 around it, with the same g
    quiet = _row(rng, N, [])
    pair = ref_fixed_linked(np.stack([quiet, x]), fs, 2.0, -1.0, 3.0, true_peak)
    alone = ref_fixed(quiet, fs, 2.0, -1.0, 3.0, true_peak)
    assert np.all(alone["g"] == 1.0) and pair["g"].min() < 0.6
    assert np.array_equal(pair["out"][0], 2.0 * pair["g"] * quiet.astype(np.float64))
    assert np.array_equal(pair["out"][1], 2.0 * pair["g"] * x.astype(np.float64))
    near = np.abs(np.arange(N) - (3 * H + 100)) <= H
    assert np.all(np.abs(pair["out"][0][near]) < np.abs(alone["out"][near]) + (quiet[near] == 0))
    far = np.abs(np.arange(N) - (3 * H + 100)) > 2 * H + max(Bk, Fw) + 1
    assert np.array_equal(pair["out"][0][far], alone["out"][far])
    # min_c (e_c > thr ? thr / e_c : 1) is the c of the linked envelope
    Cl = 10.0 ** (-1.0 / 20.0)
    cc = [np.where(ref_envelope(v, fs, true_peak) > Cl / 2.0, (Cl / 2.0) / np.maximum(ref_envelope(v, fs, true_peak), 1e-300), 1.0)
          for v in (quiet, x)]
    e = pair["e"]
    assert np.array_equal(np.minimum(cc[0], cc[1]), np.where(e > Cl / 2.0, (Cl / 2.0) / np.maximum(e, 1e-300), 1.0))


# ---- the ready rules are unchanged for C > 1 -----------------------------------------------------------------------------------

@pytest.mark.parametrize("fs,true_peak", [(8000, True), (44100, True), (44100, False)])
def test_limiter_ready_rule_for_two_channels(fs, true_peak):
    """Truncating the programme at n_known changes no output of either channel below limiter_ready(n_known), whatever arrives
    later in either channel: exact float64 equality."""
    rng = np.random.default_rng(fs)
    H, Bk, Fw = loudness.limiter_reach(fs, 3.0, true_peak)
    N = 7 * H + 900
    X = np.stack([_row(rng, N, [0, 2 * H + 50, 4 * H + 200, N - 1]), _row(rng, N, [H, 4 * H + 3, N - H])])
    full = ref_fixed_linked(X, fs, 2.0, -1.0, 3.0, true_peak)["out"]
    for n_known in [1, 2, 2 * H + Fw, 2 * H + Fw + 1, 4 * H + 3 + 2 * H + Fw, 4 * H + 4 + 2 * H + Fw, N - 1, N] + \
            [int(v) for v in rng.integers(1, N, 6)]:
        r = loudness.limiter_ready(n_known, H, Fw)
        part = ref_fixed_linked(X[:, :n_known], fs, 2.0, -1.0, 3.0, true_peak)["out"]
        assert np.array_equal(part[:, :r], full[:, :r]), (n_known, r)
    # ... and the rule is not slack: a peak in the first unknown sample of the OTHER channel changes output ready(n_known)
    n_known = 3 * H + 17
    X = np.stack([_row(rng, N, []), _row(rng, N, [n_known])])
    r = loudness.limiter_ready(n_known, H, 0)
    full = ref_fixed_linked(X, fs, 2.0, true_peak=False)["out"]
    part = ref_fixed_linked(X[:, :n_known], fs, 2.0, true_peak=False)["out"]
    assert np.array_equal(part[:, :r], full[:, :r]) and part[0, r] != full[0, r]


def test_leveller_ready_rule_for_two_channels():
    fs, hop = 8000, 800
    rng = np.random.default_rng(4)
    N = 40 * hop + 123
    X = np.stack([_steps(rng, N, fs), _steps(rng, N, fs, levels=(0.3, 0.004, 0.05))])
    full = loudness.level_reference_linked(X, fs, -20.0)
    for n_known in (1, hop, 10 * hop, 11 * hop - 1, 11 * hop, 11 * hop + 1, 25 * hop + 7, N - 1, N):
        r = loudness.leveller_ready(n_known, hop)
        assert r == max(0, (n_known // hop - 10) * hop)
        Y = X[:, :n_known].copy()
        part = loudness.level_reference_linked(Y, fs, -20.0)
        assert np.array_equal(part[:, :r].view(np.uint32), full[:, :r].view(np.uint32)), n_known
    # the first quarter the rule withholds does depend on what comes, in EITHER channel
    n_known = 25 * hop
    r = loudness.leveller_ready(n_known, hop)
    Y = X.copy()
    Y[1, n_known:n_known + hop] *= 30.0
    other = loudness.level_reference_linked(Y, fs, -20.0)
    assert np.array_equal(other[:, :r].view(np.uint32), full[:, :r].view(np.uint32))
    assert not np.array_equal(other[0, r:r + hop], full[0, r:r + hop])


# ---- bookkeeping: the device replaced by host stand-ins -------------------------------------------------------------------------

BLOCKS = [1, 0, 4410, 7, 70001]


class _LimitRows:
    """ops.limit_span_rows on the host: knows the whole-programme result and checks every call's window, order and ready rule."""

    def __init__(self, Z, fs, gain_db, ceiling_db, true_peak, ms):
        self.Z = np.asarray(Z, np.float32)
        self.args = (fs, gain_db, ceiling_db, true_peak, ms)
        ref = ref_fixed_linked(self.Z, fs, 10.0 ** (gain_db / 20.0), ceiling_db, ms, true_peak)
        self.out, self.g = ref["out"].astype(np.float32), ref["g"]
        self.H, self.Bk, self.Fw = loudness.limiter_reach(fs, ms, true_peak)
        self.calls, self.beyond, self.done = 0, 0, 0

    def __call__(self, xw, g0, n_total, rate, gain_db, m0, m1, out, ceiling_db=-1.0, true_peak=False, lookahead_ms=3.0):
        import torch
        assert (rate, gain_db, ceiling_db, true_peak, lookahead_ms) == self.args
        C, N = self.Z.shape
        assert xw.dim() == 2 and xw.shape[0] == C and out.shape[0] == C and out.shape[1] >= m1 - m0
        assert (xw.shape[1] <= 1 or xw.stride(1) == 1) and (out.shape[1] <= 1 or out.stride(1) == 1)
        win = xw.numpy()
        assert g0 >= 0 and g0 + win.shape[1] <= N
        assert np.array_equal(win.view(np.uint32), self.Z[:, g0:g0 + win.shape[1]].view(np.uint32)), "the window holds other samples"
        assert m0 == self.done and m0 < m1 <= N
        if n_total is None:
            assert m1 <= loudness.limiter_ready(g0 + win.shape[1], self.H, self.Fw)
        else:
            assert n_total == N
        lo, hi = max(0, m0 - 2 * self.H - self.Bk), min(N - 1 if n_total is not None else 2 ** 62, m1 - 1 + 2 * self.H + self.Fw)
        assert g0 <= lo and hi < g0 + win.shape[1], "the window does not cover the span"
        self.calls += 1
        self.beyond = max(self.beyond, m0 - g0)                # what the window keeps behind the first output
        self.done = m1
        out[:, :m1 - m0] = torch.from_numpy(self.out[:, m0:m1])
        return torch.tensor([float(np.float32(self.g[m0:m1].min())), float(np.abs(self.out[:, m0:m1]).max())], dtype=torch.float64)


class _LevelRows:
    """ops.level_span_rows on the host: halves every channel; checks order, ready rule, window, the one state, the weights."""

    def __init__(self, Z, fs, weights):
        self.Z, self.hop, self.weights = np.asarray(Z, np.float32), loudness.hop_length(fs), weights
        self.calls, self.done, self.beyond, self.states = 0, 0, 0, set()

    def __call__(self, xw, g0, n_total, rate, target, m0, m1, out, state, max_gain_db=12.0, gate=-50.0, weights=None):
        C, N = self.Z.shape
        assert xw.dim() == 2 and xw.shape[0] == C and out.shape == (C, m1 - m0) and weights == self.weights
        win = xw.numpy()
        assert np.array_equal(win.view(np.uint32), self.Z[:, g0:g0 + win.shape[1]].view(np.uint32)), "the window holds other samples"
        assert m0 == self.done and m0 < m1 <= N and g0 <= m0 and m1 <= g0 + win.shape[1]
        if n_total is None:
            assert m1 <= loudness.leveller_ready(g0 + win.shape[1], self.hop)
        else:
            assert n_total == N
        ne0, ne1 = loudness.leveller_counts(m0, self.hop, None if n_total is None else N // self.hop)[1], \
            loudness.leveller_counts(m1, self.hop, None if n_total is None else N // self.hop)[1]
        if ne1 > ne0:
            assert g0 <= max(0, (ne0 - 2) * self.hop) and ne1 * self.hop <= g0 + win.shape[1], "a new quarter's region is not there"
        self.states.add(state.data_ptr())
        self.beyond = max(self.beyond, m0 - g0)
        out.copy_(0.5 * xw[:, m0 - g0:m1 - g0])
        state[2] += 1
        self.calls, self.done = self.calls + 1, m1


def _run_session(x, rate_in, rate_out, **kw):
    s = api.VoiceFixer.open_stream(_FakeVF(), 1.5, 0.25, 1, 0, None, rate_in, None if rate_out == 44100 else rate_out, **kw)
    got, at, pos = [], 0, []
    n = x.shape[-1]
    for k in BLOCKS + [n]:
        blk = x[..., at:at + k]
        at = min(at + k, n)
        got.append(s.push(blk))
        assert got[-1].ndim == 2 and s.position == sum(g.shape[1] for g in got)
        pos.append(s.position)
    got.append(s.finish())
    assert all(g.shape[0] == got[0].shape[0] for g in got)
    return s, np.concatenate(got, axis=1), pos


@pytest.mark.parametrize("C,rate_in,rate_out", [(2, 44100, 48000), (3, 16000, 44100)])
def test_session_bookkeeping_with_every_channel(host_ops, monkeypatch, C, rate_in, rate_out):  # noqa: F811
    """The path restores every row on its own here, so channel c of the channels="all" session must be the mono session on
    channel c, bit for bit; the linked stages are stand-ins that know the whole-programme result and check every call."""
    import torch
    from voicefixer_amd import ops
    rng = np.random.default_rng(C)
    n = 80000 if rate_in == 44100 else 75000
    x = (0.3 * rng.standard_normal((C, n)) * np.array([1.0, 0.3, 0.1])[:C, None]).astype(np.float32)
    monos = [_run_session(x[c], rate_in, rate_out)[1] for c in range(C)]
    s0, Z, pos0 = _run_session(x, rate_in, rate_out, channels="all")
    assert Z.shape == (C, monos[0].shape[1]) and Z.dtype == np.float32 and s0.position == Z.shape[1]
    assert s0.limiter_stats is None and s0.leveller_stats is None
    for c in range(C):
        assert np.array_equal(Z[c].view(np.uint32), monos[c][0].view(np.uint32)), c
    assert any(0 < p < Z.shape[1] for p in pos0)
    # "mix" / "first": the mono session on the reduced input
    assert np.array_equal(_run_session(x, rate_in, rate_out, channels="first")[1].view(np.uint32), monos[0].view(np.uint32))
    mixed = _run_session(x.mean(axis=0, dtype=np.float32), rate_in, rate_out)[1]
    got = _run_session(x, rate_in, rate_out, channels="mix")[1]
    assert got.shape == mixed.shape and np.array_equal(got.view(np.uint32), mixed.view(np.uint32))
    assert np.array_equal(_run_session(x[0], rate_in, rate_out, channels="mix")[1].view(np.uint32), monos[0].view(np.uint32))
    # the linked limiter behind a gain
    gain_db = 20.0 * np.log10(0.7 / np.abs(Z).max()) + 6.0
    lim = _LimitRows(Z, rate_out, gain_db, -3.0, True, 2.0)
    monkeypatch.setattr(ops, "limit_span_rows", lim)
    monkeypatch.setattr(ops, "limit_span", None)              # (a programme never goes through the mono launchers)
    s1, got, pos1 = _run_session(x, rate_in, rate_out, channels="all", gain_db=gain_db, limiter=True, peak_ceiling=-3.0,
                                 true_peak=True, limiter_lookahead_ms=2.0)
    assert got.shape == Z.shape and np.array_equal(got.view(np.uint32), lim.out.view(np.uint32))
    late = 2 * lim.H + lim.Fw
    assert all(b == max(a - late, 0) for a, b in zip(pos0, pos1))
    assert lim.calls >= 3 and lim.beyond <= 2 * lim.H + lim.Bk             # per channel: what F_C reads behind an output
    assert s1.limiter_stats == {"max_reduction_db": -loudness.to_db(float(np.float32(lim.g.min()))) + 0.0,
                                "peak_out_db": loudness.to_db(float(np.abs(lim.out).max()))}
    assert s1.limiter_stats["max_reduction_db"] > 1.0 and s1.leveller_stats is None
    # the gain alone: float32(gL) Z
    s2, got2, pos2 = _run_session(x, rate_in, rate_out, channels="all", gain_db=gain_db)
    assert pos2 == pos0 and np.array_equal(got2.view(np.uint32), (np.float32(10.0 ** (gain_db / 20.0)) * Z).view(np.uint32))
    # the linked leveller (one state, the session's weights), the limiter at 0 dB behind it, 16 bit behind both
    weights = [1.0, 0.5, 0.0][:C]
    lev = _LevelRows(Z, rate_out, weights)
    lim = _LimitRows(0.5 * Z, rate_out, 0.0, -1.0, False, 3.0)
    monkeypatch.setattr(ops, "level_span_rows", lev)
    monkeypatch.setattr(ops, "level_span", None)
    monkeypatch.setattr(ops, "limit_span_rows", lim)
    monkeypatch.setattr(ops, "level_state", lambda device: torch.zeros((loudness.LEVELLER_STATE,), dtype=torch.float64))
    s3, got3, pos3 = _run_session(x, rate_in, rate_out, channels="all", channel_weights=weights, leveller=-20.0, limiter=True)
    hop = loudness.hop_length(rate_out)
    assert np.array_equal(got3.view(np.uint32), lim.out.view(np.uint32)) and len(lev.states) == 1
    assert lev.beyond <= 2 * hop and lev.calls >= 3                        # the window starts two quarters before a new one
    assert s3.leveller_stats["anchors"] == lev.calls and s3.limiter_stats["peak_out_db"] == loudness.to_db(float(np.abs(lim.out).max()))
    ready = [loudness.limiter_ready(loudness.leveller_ready(p, hop), lim.H, lim.Fw) for p in pos0]
    assert pos3[:-1] == ready[:-1] and s3.position == Z.shape[1]

    from voicefixer_amd import wordlength

    def quantize_rows(xq, n_rows, bit_depth, dither, seed, n0=None, chan=None, out=None):
        rows = [wordlength.quantize_ref(xq[r].numpy(), bit_depth, dither, seed, n0=0 if n0 is None else int(n0[r]),
                                        channel=0 if chan is None else int(chan[r]))[0] for r in range(xq.shape[0])]
        return torch.from_numpy(np.stack(rows)), None

    monkeypatch.setattr(ops, "quantize_rows", quantize_rows)
    lev.calls, lev.done, lim.calls, lim.done = 0, 0, 0, 0
    q = _run_session(x, rate_in, rate_out, channels="all", channel_weights=weights, leveller=-20.0, limiter=True, bit_depth=16,
                     dither_seed=5)[1]
    want = np.stack([wordlength.quantize_ref(lim.out[c], 16, "tpdf", 5, channel=c, n0=0)[0] for c in range(C)])
    assert q.dtype == np.int16 and np.array_equal(q, want)


# ---- argument rules, before the device ------------------------------------------------------------------------------------------

def test_argument_rules_come_before_the_device():
    vf = api.VoiceFixer.__new__(api.VoiceFixer)               # (no device, no weights: the checks come first)
    opened = lambda **kw: api.VoiceFixer.open_stream(vf, **kw)
    for bad in ("stereo", 2, True, ["all"]):
        with pytest.raises(ValueError):
            opened(channels=bad)
    for ch in (None, "mix", "first"):                         # weights weigh a programme's channels
        with pytest.raises(ValueError, match="channel_weights"):
            opened(channels=ch, channel_weights=[1.0, 1.0])
    for bad in ("11", [], [1.0] * 9, [1.0, -1.0], [1.0, float("nan")], [1.0, "a"], 1.0):
        with pytest.raises(ValueError):
            opened(channels="all", channel_weights=bad)
    # channels=None: today's behaviour, the ValueError for a 2-D block included
    s = opened()
    with pytest.raises(ValueError):
        s.push(np.zeros((2, 100), np.float32))
    assert s.push(np.zeros(0, np.float32)).shape == (1, 0)
    # "all": (C, k) blocks of one C in 1..8
    s = opened(channels="all", channel_weights=[1.0, 0.5], leveller=-20.0, limiter=True)
    with pytest.raises(ValueError):
        s.push(np.zeros(100, np.float32))                     # a 1-D block
    with pytest.raises(ValueError):
        s.push(np.zeros((9, 100), np.float32))
    with pytest.raises(ValueError):
        s.push(np.zeros((0, 100), np.float32))
    with pytest.raises(ValueError):
        s.push(np.zeros((2, 2, 100), np.float32))
    with pytest.raises(ValueError, match="channel_weights"):
        s.push(np.zeros((3, 0), np.float32))                  # two weights, three channels
    assert s.push(np.zeros((2, 0), np.float32)).shape == (2, 0) and s.position == 0      # fixes C, needs no device
    for bad in (np.zeros((3, 10), np.float32), np.zeros((1, 10), np.float32), np.zeros(10, np.float32)):
        with pytest.raises(ValueError):
            s.push(bad)
    assert s.limiter_stats == {"max_reduction_db": 0.0, "peak_out_db": -np.inf} and s.leveller_stats["anchors"] == 0
    with pytest.raises(ValueError):                           # under MIN_SAMPLES per channel: refused before anything is launched
        s.finish()
    with pytest.raises(RuntimeError):
        s.push(np.zeros((2, 10), np.float32))
    s = opened(channels="all", bit_depth=16)
    assert s.push(np.zeros((8, 0), np.float32)).dtype == np.int16
    with pytest.raises(ValueError):
        opened(channels="all").finish()                       # nothing pushed at all
    for ch in ("mix", "first"):
        s = opened(channels=ch)
        assert s.push(np.zeros((2, 0), np.float32)).shape == (1, 0) and s.push(np.zeros(0, np.float32)).shape == (1, 0)
        with pytest.raises(ValueError):
            s.push(np.zeros((9, 10), np.float32))
        with pytest.raises(ValueError):
            s.push(np.zeros((2, 2, 10), np.float32))
    with pytest.raises(NotImplementedError):
        opened(channels="all", mode=2)
    with pytest.raises(NotImplementedError):                  # the limiter still needs a gain or a leveller
        opened(channels="all", limiter=True)
    # limit / level
    x2 = np.zeros((2, 10), np.float32)
    for fn in (voicefixer_amd.limit, voicefixer_amd.level):
        with pytest.raises(ValueError):
            fn(x2)                                            # without channels a 2-D array still raises
        for bad in ("mix", "first", "both", 2):
            with pytest.raises(ValueError):
                fn(x2, channels=bad)
        with pytest.raises(ValueError):
            fn(np.zeros((9, 10), np.float32), channels="all")
        with pytest.raises(ValueError):
            fn(np.zeros((2, 2, 10), np.float32), channels="all")
        assert fn([], channels="all") == []
    with pytest.raises(ValueError, match="channel_weights"):
        voicefixer_amd.level(np.zeros(10, np.float32), channel_weights=[1.0])
    with pytest.raises(ValueError):
        voicefixer_amd.level(x2, channels="all", channel_weights=[1.0])
    with pytest.raises(ValueError):
        voicefixer_amd.level([x2, np.zeros((3, 10), np.float32)], channels="all", channel_weights=[1.0, 1.0])
    with pytest.raises(NotImplementedError):                  # restore_stream is unchanged and still refuses
        api.VoiceFixer.restore_stream(vf, np.zeros(44100, np.float32), limiter=True)
    assert "channels" not in inspect.signature(api.VoiceFixer.restore_stream).parameters


def test_new_keywords_are_last():
    p = inspect.signature(api.RestoreSession.__init__).parameters
    assert list(p)[-2:] == ["channels", "channel_weights"] and p["channels"].default is None and p["channel_weights"].default is None
    # open_stream's named parameters stay the mono session's (tests/test_multichannel_cpu.py pins that): the two keywords come
    # behind all of them, by keyword only, and go to RestoreSession; nothing else does
    p = inspect.signature(api.VoiceFixer.open_stream).parameters
    assert list(p)[-1] == "programme" and p["programme"].kind is inspect.Parameter.VAR_KEYWORD
    assert sorted(list(p)[1:-1]) == sorted(k for k in inspect.signature(api.RestoreSession.__init__).parameters
                                           if k not in ("self", "vf", "channels", "channel_weights"))
    vf = api.VoiceFixer.__new__(api.VoiceFixer)
    s = api.VoiceFixer.open_stream(vf, channels="all", channel_weights=[1.0, 1.0])
    assert s._channels == "all" and s._weights == [1.0, 1.0]
    assert api.VoiceFixer.open_stream(vf)._channels is None
    for bad in (dict(channel="all"), dict(channels="all", weights=[1.0])):
        with pytest.raises(TypeError, match="unexpected keyword"):
            api.VoiceFixer.open_stream(vf, **bad)
    p = inspect.signature(voicefixer_amd.limit).parameters
    assert list(p)[-2:] == ["_span", "channels"] and p["channels"].default is None
    p = inspect.signature(voicefixer_amd.level).parameters
    assert list(p)[-3:] == ["_span", "channels", "channel_weights"] and p["channels"].default is None
    assert p["channel_weights"].default is None


def test_entry_points_declared_mapped_and_bound():
    header = open(os.path.join(ROOT, "include", "vfx_hip.h")).read()
    vmap = open(os.path.join(ROOT, "voicefixer_amd", "csrc", "vfx.map")).read()
    assert re.search(r"global:\s*vfx_\*;", vmap)
    for name, nargs in (("vfx_limit_span_rows_workspace_bytes", 3), ("vfx_limit_span_rows_f32", 21),
                        ("vfx_level_span_rows_workspace_bytes", 3), ("vfx_level_span_rows_f32", 22)):
        m = re.search(r"\b(?:int|size_t) %s\(([^;]*)\);" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
    from voicefixer_amd import ops
    assert list(inspect.signature(ops.limit_span_rows).parameters) == list(inspect.signature(ops.limit_span).parameters)
    assert list(inspect.signature(ops.level_span_rows).parameters) == list(inspect.signature(ops.level_span).parameters) + ["weights"]
    mk = open(os.path.join(ROOT, "voicefixer_amd", "csrc", "Makefile")).read()
    src = open(os.path.join(ROOT, "voicefixer_amd", "csrc", "vfx_loudness.hip")).read()
    for stage in ("limit", "level"):                          # one file per stage defines the mono and the linked entry point
        inc = "vfx_%s_span.inc" % stage
        assert inc in mk and '#include "%s"' % inc in src
        body = open(os.path.join(ROOT, "voicefixer_amd", "csrc", inc)).read()
        for entry in ("vfx_%s_span_f32" % stage, "vfx_%s_span_rows_f32" % stage):
            assert re.search(r'extern "C" int %s\(' % entry, body), entry
        assert not os.path.exists(os.path.join(ROOT, "voicefixer_amd", "csrc", "vfx_%s_span_rows.inc" % stage))


def test_span_stage_carries_a_programme():
    """The stage contract for (C, k): concatenated, dropped and counted along the last axis."""
    import torch
    from voicefixer_amd import stream

    class Toy(stream._SpanStage):
        def _ready(self, n):
            return max(0, n - 5)

        def _run(self, a, e, n_total, y):
            assert self.win.dim() == 2 and y.shape == (self.win.shape[0], e - a) and self.g0 <= max(a - 3, 0)
            last = 2 ** 62 if n_total is None else n_total - 1
            m = torch.arange(a, e)
            y.copy_(self.win[:, (m - 3).clamp(min=0) - self.g0] + 2.0 * self.win[:, (m + 5).clamp(max=last) - self.g0])

        def _keep(self, m1):
            return m1 - 3

    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.integers(-99, 99, (3, 1000)).astype(np.float32))
    m = np.arange(1000)
    want = x.numpy()[:, np.clip(m - 3, 0, None)] + 2.0 * x.numpy()[:, np.clip(m + 5, None, 999)]
    assert np.array_equal(Toy(7).whole(x).numpy(), want)
    st, got, at = Toy(64), [], 0
    for cpos in (1, 1, 400, 407, 1000):
        got.append(st.feed(x[:, at:cpos]))
        at = cpos
        assert st.n_in == at and st.m_done == max(0, at - 5) and st.win.shape[0] == 3 and st.win.shape[1] <= 9 + 600
    got.append(st.finish("cpu"))
    assert np.array_equal(torch.cat(got, dim=1).numpy(), want) and st.m_done == 1000
    st = Toy()
    st.rows = 2
    assert st.finish("cpu").shape == (2, 0)
