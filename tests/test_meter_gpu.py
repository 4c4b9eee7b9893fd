"""The streaming loudness meter on the device (csrc/vfx_meter_span.inc: vfx_meter_span_rows_f32, vfx_meter_report_f32;
ops.meter_span_rows / meter_report; ``LoudnessMeter``; ``open_stream(meter=True)``) against a float64
specification written out here, against the whole-row report, across splits bit for bit, at its refusals and inside a session.

Bounds: the loudness figures within 0.005 LU, the range within 0.01 LU, the true peak within 2e-6 max(1,
ref); the sample peak and, against ``measure_true_peak``, the true peak bit for bit.  Condition of every comparison of a gated
figure, asserted on the reference before the device is touched: no block lies within 0.05 LU of a gate it is tested against."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
from scipy.signal import lfilter, upfirdn

import voicefixer_amd
from voicefixer_amd import _lib, audio_io, loudness, ops

pytestmark = pytest.mark.gpu

INT64_MAX = 2 ** 63 - 1
LU, LRA_LU, TP_REL, MARGIN = 0.005, 0.01, 2e-6, 0.05
LOUD = ("integrated", "max_momentary", "max_short_term", "momentary", "short_term")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


# ---- the float64 specification, written out ---------------------------------------------------------------------------------------

def _lufs(z):
    return -0.691 + 10.0 * math.log10(z) if z > 0.0 else -math.inf


def ref_energies(X, fs, w):
    """E_q = sum_c w_c E_{q,c}: a float64 lfilter over [max(0, (q - 2) hop), (q + 1) hop) from zero state, fp32-rounded coefficients."""
    c = loudness.coefficients(fs).astype(np.float32).astype(np.float64)
    hop = (fs + 5) // 10
    E = np.zeros(X.shape[1] // hop)
    for ch in range(X.shape[0]):
        x = X[ch].astype(np.float64)
        e = np.zeros_like(E)
        for q in range(E.shape[0]):
            r0 = max(0, (q - 2) * hop)
            y = lfilter(c[5:8], [1.0, c[8], c[9]], lfilter(c[0:3], [1.0, c[3], c[4]], x[r0:(q + 1) * hop]))[q * hop - r0:]
            e[q] = float(np.dot(y, y))
        E = E + np.float64(w[ch]) * e
    return E


def ref_true_peak(X, fs, final=True):
    """max(P, max |y|) in float64: upfirdn with the project's interpolator; final=False: the values of the samples below N - Fw."""
    N = X.shape[1]
    P = float(np.abs(X).max()) if N else 0.0
    R = 4 if fs < 96000 else (2 if fs < 192000 else 1)
    if R == 1 or N == 0:
        return P, P
    g = audio_io.hq_filter(R, 1)[1].astype(np.float64)
    c = (g.size - 1) // 2
    Fw = c // R
    m1 = R * N if final else max(0, min(R * N, R * (N - Fw + c // R) - c))
    tp = P
    for ch in range(X.shape[0]):
        y = upfirdn(g, X[ch].astype(np.float64), up=R)[c:c + m1]
        if y.size:
            tp = max(tp, float(np.abs(y).max()))
    return P, tp


def ref_meter(X, fs, w=None, final=True):
    """(figures, margin): the nine figures (peaks linear) and the least distance of a block from a gate it is tested against."""
    X = np.asarray(X, np.float32)
    X = X[None] if X.ndim == 1 else X
    w = loudness.channel_weights(X.shape[0]) if w is None else w
    hop = (fs + 5) // 10
    E = ref_energies(X, fs, w)
    Q = E.shape[0]
    z = np.array([(E[j] + E[j + 1] + E[j + 2] + E[j + 3]) / (4.0 * hop) for j in range(max(Q - 3, 0))])
    st = np.array([float(sum(E[j:j + 30].tolist())) / (30.0 * hop) for j in range(max(Q - 29, 0))])
    lz, ls = np.array([_lufs(v) for v in z]), np.array([_lufs(v) for v in st])
    margin = math.inf
    L = -math.inf
    if z.size:
        margin = min(margin, float(np.abs(lz + 70.0).min()))
        g1 = lz > -70.0
        if g1.any():
            gr = _lufs(z[g1].mean()) - 10.0
            margin = min(margin, float(np.abs(lz[g1] - gr).min()))
            g2 = g1 & (lz > gr)
            if g2.any():
                L = _lufs(z[g2].mean())
    lra = 0.0
    if st.size:
        margin = min(margin, float(np.abs(ls + 70.0).min()))
        g1 = ls > -70.0
        if g1.any():
            gr = _lufs(st[g1].mean()) - 20.0
            margin = min(margin, float(np.abs(ls[g1] - gr).min()))
            s = np.sort(st[g1 & (ls > gr)])
            n = s.size
            if n:
                lra = _lufs(s[((n - 1) * 95 + 50) // 100]) - _lufs(s[((n - 1) + 5) // 10])
    P, TP = ref_true_peak(X, fs, final)
    fig = {"integrated": L, "loudness_range": lra, "max_momentary": float(lz.max()) if z.size else -math.inf,
           "max_short_term": float(ls.max()) if st.size else -math.inf, "sample_peak": P, "true_peak": TP,
           "momentary": float(lz[-1]) if z.size else -math.inf, "short_term": float(ls[-1]) if st.size else -math.inf,
           "seconds": X.shape[1] / float(fs)}
    return fig, margin


def _close(got, want, bound):
    return got == want if math.isinf(want) or math.isinf(got) else abs(got - want) <= bound


def _lin(db):
    return 0.0 if db == -math.inf else 10.0 ** (db / 20.0)


def _check_figures(what, got, want, k=1.0):
    """``got``: a dict with peaks in dB (the public form); ``want``: the reference's, peaks linear."""
    for key in LOUD:
        print("%s %s: %.6f (reference %.6f)" % (what, key, got[key], want[key]))
        assert _close(got[key], want[key], k * LU), (what, key, got[key], want[key])
    print("%s loudness_range: %.6f (reference %.6f)" % (what, got["loudness_range"], want["loudness_range"]))
    assert abs(got["loudness_range"] - want["loudness_range"]) <= k * LRA_LU, (what, got["loudness_range"], want["loudness_range"])
    tp = _lin(got["true_peak"])
    print("%s true peak: %.9g (reference %.9g), sample peak %.9g" % (what, tp, want["true_peak"], _lin(got["sample_peak"])))
    assert abs(tp - want["true_peak"]) <= k * TP_REL * max(1.0, want["true_peak"]), (what, tp, want["true_peak"])
    assert got["seconds"] == want["seconds"]


# ---- signals ------------------------------------------------------------------------------------------------------------------------

def _steps(rng, n, fs, levels):
    """Noise whose level steps every 1.1 s through ``levels``."""
    seg = int(1.1 * fs)
    a = np.array([levels[(i // seg) % len(levels)] for i in range(n)])
    return (a * rng.standard_normal(n)).astype(np.float32)


def _signal(fs, N, Cn, seed, levels=(0.1, 0.03, 0.2)):
    rng = np.random.default_rng(seed)
    X = np.stack([_steps(rng, N, fs, levels[c % len(levels):] + levels[:c % len(levels)]) for c in range(Cn)])
    return X[0] if Cn == 1 else X


def _stepped_40s():
    """40 s at 8 kHz: 10 s stretches 26 dB apart, so that the loudness range is well defined."""
    rng = np.random.default_rng(11)
    a = np.repeat([0.01, 0.2, 0.02, 0.1], 80000)
    return (a * rng.standard_normal(320000)).astype(np.float32)


HOP8 = 800
CASES = {
    "8k-no-quarter": (8000, lambda: _signal(8000, HOP8 - 1, 1, 1)),
    "8k-no-block": (8000, lambda: _signal(8000, 3 * HOP8 + 5, 1, 2)),
    "8k-one-block": (8000, lambda: _signal(8000, 4 * HOP8, 1, 3)),
    "8k-33-quarters": (8000, lambda: _signal(8000, 33 * HOP8 + 17, 1, 4)),
    "8k-40s-stepped": (8000, _stepped_40s),
    "44k": (44100, lambda: _signal(44100, 4 * 44100, 1, 5)),
    "48k": (48000, lambda: _signal(48000, 4 * 48000, 1, 6)),
    "96k": (96000, lambda: _signal(96000, 144000, 1, 7)),
    "192k": (192000, lambda: _signal(192000, 288000, 1, 8)),
    "8k-stereo": (8000, lambda: _signal(8000, 33 * HOP8 + 17, 2, 9)),
    "8k-5.1": (8000, lambda: _signal(8000, 33 * HOP8 + 17, 6, 10)),
}
_DONE = {}


def _report_dict(rep, n, fs):
    v = rep.cpu().numpy()
    assert v[9] == 0.0 and not np.isnan(v).any(), v
    return {"integrated": float(v[0]), "loudness_range": float(v[1]), "max_momentary": float(v[2]), "max_short_term": float(v[3]),
            "sample_peak": loudness.to_db(v[4]), "true_peak": loudness.to_db(v[5]), "momentary": float(v[6]),
            "short_term": float(v[7]), "seconds": n / float(fs)}, v


def _case(name):
    """The case's signal, its reference (margin asserted BEFORE the device is touched) and the device's figures from ONE call."""
    if name not in _DONE:
        fs, make = CASES[name]
        X = make()
        want, margin = ref_meter(X, fs)
        print("%s: margin to the nearest gate %.3f LU" % (name, margin))
        assert margin >= MARGIN, (name, margin)
        N, hop = X.shape[-1], loudness.hop_length(fs)
        xd = torch.from_numpy(X).cuda()
        state, qlog = ops.meter_state(xd.device), torch.zeros((max(N // hop, 1),), dtype=torch.float64, device="cuda")
        ops.meter_span_rows(xd, 0, N, fs, 0, N, state, qlog)
        got, raw = _report_dict(ops.meter_report(state, qlog, fs), N, fs)
        assert raw[8] == N // hop and state.cpu().tolist()[2:5] == [N // hop, N, 0.0]
        _DONE[name] = (fs, X, want, got)
    return _DONE[name]


@pytest.mark.parametrize("name", list(CASES))
def test_against_the_float64_specification(name):
    fs, X, want, got = _case(name)
    host = loudness.meter_reference(X, fs)                    # the module's specification is the one written out above
    for key in LOUD + ("loudness_range",):
        assert _close(host[key], want[key], 1e-9), (key, host[key], want[key])
    assert abs(_lin(host["true_peak"]) - want["true_peak"]) <= 1e-12 and host["seconds"] == want["seconds"]
    _check_figures(name, got, want)
    assert got["sample_peak"] == loudness.to_db(float(np.abs(X).max()))                  # bit for bit
    assert got["true_peak"] == voicefixer_amd.measure_true_peak(X, fs)                   # the whole-row kernel's maximum, bit for bit
    if name == "8k-no-quarter":
        assert got["integrated"] == got["momentary"] == -math.inf
    if name == "8k-no-block":
        assert got["integrated"] == got["max_momentary"] == got["max_short_term"] == -math.inf and got["loudness_range"] == 0.0
    if name == "8k-40s-stepped":
        assert want["loudness_range"] > 15.0


@pytest.mark.parametrize("name", list(CASES))
def test_agrees_with_the_whole_row_report(name):
    """Both lie within one bound of the same float64 value: within two of each other."""
    fs, X, want, got = _case(name)
    whole = voicefixer_amd.loudness_report(X, fs)
    for key in ("integrated", "max_momentary", "max_short_term"):
        print("%s %s: meter %.6f, whole row %.6f" % (name, key, got[key], whole[key]))
        assert _close(got[key], whole[key], 2 * LU), (key, got[key], whole[key])
    assert abs(got["loudness_range"] - whole["loudness_range"]) <= 2 * LRA_LU
    assert got["sample_peak"] == whole["sample_peak"] and got["true_peak"] == whole["true_peak"]


# ---- the span form: windows with canaries, any split -------------------------------------------------------------------------------

PAD = 37


class _Meter:
    """A meter whose state and log sit between NaN canaries; ``span`` feeds [m0, m1) from the smallest window the header allows,
    copied ``off`` floats behind a 16-byte boundary into NaN, the rows ``gap`` floats apart."""

    def __init__(self, X, fs, weights=None, qcap=None):
        self.X = X[None] if X.ndim == 1 else X
        self.fs, self.hop, self.w = fs, loudness.hop_length(fs), weights
        self.N = self.X.shape[1]
        self.R, self.Bk, self.Fw = loudness.meter_reach(fs)
        self.qcap = self.N // self.hop + 3 if qcap is None else qcap
        self.sbuf = torch.full((16 + loudness.METER_STATE + 16,), float("nan"), dtype=torch.float64, device="cuda")
        self.qbuf = torch.full((8 + self.qcap + 8,), float("nan"), dtype=torch.float64, device="cuda")
        self.state, self.qlog = self.sbuf[16:16 + loudness.METER_STATE], self.qbuf[8:8 + self.qcap]
        self.done = 0            # (the caller's: where its next span starts)

    def window(self, m0, m1, known):
        lo, hi = max(0, m0 - self.Bk), (min(self.N - 1, m1 - 1 + self.Fw) if known else m1 - 1 + self.Fw)
        q0, q1 = m0 // self.hop, m1 // self.hop
        if q1 > q0:
            lo, hi = min(lo, max(0, q0 - 2) * self.hop), max(hi, q1 * self.hop - 1)
        return lo, hi

    def span(self, m0, m1, known=True, off=0, gap=0, short=(0, 0)):
        lo, hi = self.window(m0, m1, known)
        lo, hi = lo + short[0], hi - short[1]
        Cn, wlen = self.X.shape[0], hi - lo + 1
        stride = wlen + gap
        buf = torch.full((4 * ((PAD + 3) // 4) + off + Cn * stride + PAD,), float("nan"), device="cuda")
        base = 4 * ((PAD + 3) // 4) + off
        view = buf[base:].as_strided((Cn, wlen), (stride, 1))
        view.copy_(torch.from_numpy(np.ascontiguousarray(self.X[:, lo:hi + 1])))
        ops.meter_span_rows(view, lo, self.N if known else None, self.fs, m0, m1, self.state, self.qlog, self.w)
        assert int(torch.isnan(buf).sum()) == buf.numel() - Cn * wlen           # every canary around every row stays

    def result(self):
        rep = ops.meter_report(self.state, self.qlog, self.fs)
        torch.cuda.synchronize()
        sb, qb = self.sbuf.cpu().numpy(), self.qbuf.cpu().numpy()
        Q = self.N // self.hop
        assert np.isnan(sb[:16]).all() and np.isnan(sb[16 + loudness.METER_STATE:]).all() and not np.isnan(sb[16:32]).any()
        assert np.isnan(qb[:8]).all() and np.isnan(qb[8 + Q:]).all() and not np.isnan(qb[8:8 + Q]).any()
        r = rep.cpu().numpy()
        assert not np.isnan(r).any() and r[9] == 0.0
        return _bits(sb[16:32]), _bits(qb[8:8 + Q]), _bits(r)


def _same(a, b, what):
    for u, v, part in zip(a, b, ("state", "log", "report")):
        assert np.array_equal(u, v), (what, part)


def _cuts(N, step):
    return list(range(0, N, step)) + [N]


def _pushed_meter(X, fs, sizes, channels=None, each=None):
    m = voicefixer_amd.LoudnessMeter(fs, channels=channels)
    at, n, mids = 0, X.shape[-1], []
    for k in list(sizes) + [n]:
        m.push(X[..., at:at + k])
        at = min(at + k, n)
        if each is not None:
            mids.append((at, m.report()))
    fin = m.finish()
    assert fin == m.report()                                   # (still readable, the same figures)
    Q = n // loudness.hop_length(fs)
    tap = m._tap
    rep = ops.meter_report(tap.state, tap.qlog, fs).cpu().numpy()
    return (_bits(tap.state.cpu().numpy()), _bits(tap.qlog[:Q].cpu().numpy()), _bits(rep)), fin, mids


SIZES = [1, 0, 4410, 7, 70001]


@pytest.mark.parametrize("fs,Cn", [(8000, 1), (8000, 2), (44100, 1), (44100, 2)])
def test_split_invariance_bit_for_bit(fs, Cn):
    N = 100017
    X = _signal(fs, N, Cn, 20 + Cn)
    hop = loudness.hop_length(fs)
    one = _Meter(X, fs)
    one.span(0, N)
    want = one.result()
    for what, cuts, known in (("one quarter", _cuts(N, hop), True), ("1237 samples", _cuts(N, 1237), False)):
        m = _Meter(X, fs)
        for a, b in zip(cuts[:-1], cuts[1:]):
            last = b == N
            if not known and not last and b > N - m.Fw:       # (the end is unknown: only what is ready)
                continue
            m.span(m.done, b, known or last)
            m.done = b
        _same(m.result(), want, what)
    for off in (1, 2, 3):                                     # windows off a 16-byte boundary; a stride that moves channel 1 again
        m = _Meter(X, fs)
        for b in (5 * hop + 3, 9 * hop, N):
            m.span(m.done, b, b == N, off=off, gap=off + 2)
            m.done = b
        _same(m.result(), want, "window %d floats off" % off)
    got, fin, _ = _pushed_meter(X, fs, SIZES, "all" if Cn > 1 else None)
    _same(got, want, "LoudnessMeter")
    again, fin2, mids = _pushed_meter(X, fs, SIZES, "all" if Cn > 1 else None, each=True)
    _same(again, want, "LoudnessMeter with a report after every push")
    assert fin2 == fin and len(mids) == len(SIZES) + 1
    if fs == 8000:                                            # every mid-stream report against the specification of the prefix
        Xp = X[None] if X.ndim == 1 else X
        refs = [(n, ref_meter(Xp[:, :n], fs, final=False)) for n, _ in mids]
        for n, (want_n, margin) in refs:
            assert margin >= MARGIN, (n, margin)
        for (n, got_n), (_, (want_n, _)) in zip(mids, refs):
            _check_figures("after %d samples" % n, got_n, want_n)
            assert got_n["sample_peak"] == loudness.to_db(float(np.abs(Xp[:, :n]).max())) if n else got_n["sample_peak"] == -math.inf


def test_out_of_order_sets_the_flag_and_stays_inside():
    fs, hop = 8000, 800
    X = _signal(fs, 12 * hop, 1, 30)
    m = _Meter(X, fs)
    m.span(0, 4 * hop)
    m.span(5 * hop, 7 * hop)                                  # a gap: quarters 5, 6 are written, quarter 4 never is
    m.span(7 * hop, 12 * hop)                                 # the flag is sticky
    rep = ops.meter_report(m.state, m.qlog, fs).cpu().numpy()
    sb, qb = m.sbuf.cpu().numpy(), m.qbuf.cpu().numpy()
    assert rep[9] == 1.0 and sb[16 + 4] == 1.0 and np.isnan(sb[:16]).all() and np.isnan(sb[32:]).all()
    assert np.isnan(qb[:8]).all() and np.isnan(qb[8 + 4]) and np.isnan(qb[8 + 12:]).all() and not np.isnan(qb[8 + 5:8 + 12]).any()
    tap = voicefixer_amd.LoudnessMeter(fs)
    tap.push(X)
    tap._tap.state[4] = 1.0
    with pytest.raises(_lib.VfxError):
        tap.report()


def test_refusals_launch_nothing():
    fs, hop = 8000, 800
    N = 30 * hop
    p = loudness.leveller_plan(fs)
    bank, J, c = ops.true_peak_bank(torch.device("cuda"), 4)
    R, Bk, Fw = loudness.meter_reach(fs)
    xd = torch.zeros((2 * N,), device="cuda")
    state = torch.full((loudness.METER_STATE,), 7.0, dtype=torch.float64, device="cuda")
    qcap = 30
    qlog = torch.full((qcap + 4,), 7.0, dtype=torch.float64, device="cuda")
    report = torch.full((10,), 7.0, dtype=torch.float64, device="cuda")
    mpow = torch.from_numpy(p["mpow"]).cuda()
    coef = (C.c_double * 10)(*[float(v) for v in p["coef"]])
    bad_coef = (C.c_double * 10)(*([float("nan")] + [float(v) for v in p["coef"][1:]]))
    W = lambda *v: (C.c_double * len(v))(*v)
    lib = _lib.lib()
    nb = lib.vfx_meter_span_workspace_bytes(N, hop, 2)
    assert nb > lib.vfx_meter_span_workspace_bytes(N, hop, 1) > 0
    for bad in ((-1, hop, 2), (N, 399, 2), (N, 19201, 2), (2 ** 30 + 1, hop, 2), (N, hop, 0), (N, hop, 9)):
        assert lib.vfx_meter_span_workspace_bytes(*bad) == 0
    assert lib.vfx_meter_report_workspace_bytes(-1) == 0 and lib.vfx_meter_report_workspace_bytes(100) >= 800
    ws = torch.empty((nb // 8 + 2,), dtype=torch.float64, device="cuda")
    P = lambda t: None if t is None else t.data_ptr()
    good = dict(xw=P(xd), ws_=N, C=2, w=W(1.0, 1.0), g0=0, wlen=N, n_total=N, m0=0, m1=N, fs=fs, coef=coef, mpow=P(mpow), S=p["S"],
                bank=P(bank), J=J, R=4, c=c, state=P(state), qlog=P(qlog), qcap=qcap, ws=P(ws), nb=nb)

    def call(**kw):
        a = dict(good, **kw)
        return lib.vfx_meter_span_rows_f32(a["xw"], a["ws_"], a["C"], a["w"], a["g0"], a["wlen"], a["n_total"], a["m0"], a["m1"],
                                           a["fs"], a["coef"], a["mpow"], a["S"], a["bank"], a["J"], a["R"], a["c"], a["state"],
                                           a["qlog"], a["qcap"], a["ws"], a["nb"], None)

    m0, m1 = 10 * hop + 5, 20 * hop + 5                       # a span inside: reads [m0 - Bk .. m1 - 1 + Fw], quarters from 8 hop
    inner = dict(m0=m0, m1=m1, g0=8 * hop, wlen=m1 + Fw - 8 * hop)
    assert min(m0 - Bk, 8 * hop) == 8 * hop
    bad = [dict(wlen=N - 1),                                  # the last sample is missing
           dict(inner, wlen=inner["wlen"] - 1), dict(inner, g0=8 * hop + 1, wlen=inner["wlen"] - 1),      # one sample short at each end
           dict(m0=m0, m1=m0 + 10, g0=m0 - Bk + 1, wlen=N - (m0 - Bk + 1)),                               # ... of the taps behind
           dict(n_total=INT64_MAX, m1=N - Fw + 1), dict(n_total=INT64_MAX, m1=N),                         # past the ready bound
           dict(qcap=29), dict(qcap=-1), dict(m1=N - 1, qcap=28),                                         # nq(m1) == qcap + 1
           dict(fs=192001), dict(fs=3999), dict(S=p["S"] + 32), dict(S=0), dict(coef=bad_coef),
           dict(m0=10, m1=9), dict(m0=-1), dict(m1=N + 1, wlen=N + 1, ws_=N + 1), dict(g0=-1), dict(wlen=-1),
           dict(nb=nb - 256), dict(ws=P(ws) + 8), dict(ws=None), dict(state=None), dict(qlog=None), dict(xw=None), dict(mpow=None),
           dict(coef=None), dict(state=P(state) + 4), dict(qlog=P(qlog) + 4),
           dict(C=0), dict(C=9), dict(w=None), dict(w=W(1.0, -0.5)), dict(w=W(1.0, float("nan"))), dict(w=W(float("inf"), 1.0)),
           dict(ws_=N - 1),
           dict(R=3), dict(R=0), dict(bank=None), dict(J=0), dict(J=2049), dict(c=-1), dict(c=4 * J)]
    c0 = lib.vfx_launch_count()
    for kw in bad:
        assert call(**kw) == -1, kw                           # VFX_EINVAL
    assert call(m0=500, m1=500) == 0                          # an empty span: VFX_OK, nothing launched
    rws = torch.empty((64,), dtype=torch.float64, device="cuda")
    rgood = dict(state=P(state), qlog=P(qlog), hop=hop, report=P(report), ws=P(rws), nb=8 * 64)
    rcall = lambda **kw: (lambda a: lib.vfx_meter_report_f32(a["state"], a["qlog"], a["hop"], a["report"], a["ws"], a["nb"], None))(
        dict(rgood, **kw))
    for kw in (dict(state=None), dict(qlog=None), dict(report=None), dict(ws=None), dict(hop=399), dict(hop=19201),
               dict(report=P(state)), dict(report=P(state) + 8 * 15), dict(report=P(report) + 4), dict(ws=P(rws) + 4)):
        assert rcall(**kw) == -1, kw
    torch.cuda.synchronize()
    assert lib.vfx_launch_count() == c0
    assert state.cpu().tolist() == [7.0] * loudness.METER_STATE and qlog.cpu().tolist() == [7.0] * (qcap + 4)
    assert report.cpu().tolist() == [7.0] * 10
    assert call(n_total=INT64_MAX, m1=N - Fw) == 0            # (three launches)
    assert call(m0=N - Fw, m1=N - 3) == 0                     # (two: no quarter is new)
    assert call(m0=N - 3) == 0                                # (three: the last quarter)
    assert rcall() == 0
    torch.cuda.synchronize()
    assert lib.vfx_launch_count() == c0 + 9
    assert state.cpu().tolist() == [0.0, 0.0, 30.0, float(N)] + [0.0] * 12 and qlog.cpu().tolist() == [0.0] * 30 + [7.0] * 4
    r = report.cpu().tolist()                                 # silence
    assert r[0] == r[2] == r[3] == r[6] == r[7] == -math.inf and r[1] == r[4] == r[5] == r[9] == 0.0 and r[8] == 30.0
    state2 = state.clone()
    state2[2] = 65.0                                          # more quarters than the workspace holds: flag 2, an empty log's figures
    assert rcall(state=P(state2)) == 0
    r = report.cpu().tolist()
    assert r[9] == 2.0 and r[8] == 0.0 and r[0] == -math.inf
    x2 = xd.view(2, N)
    for kw in (dict(weights=[1.0]), dict(weights=[1.0, -1.0]), dict(true_peak=1)):
        with pytest.raises(ValueError):
            ops.meter_span_rows(x2, 0, N, fs, 0, N, state, qlog, **kw)
    with pytest.raises(ValueError):
        ops.meter_span_rows(x2, 0, N, 192001, 0, N, state, qlog)
    with pytest.raises(_lib.VfxError):
        ops.meter_span_rows(x2[:, :100], 0, N, fs, 0, 50, state, qlog)


# ---- the session --------------------------------------------------------------------------------------------------------------------

CS, OVS = 1.5, 0.25


@pytest.fixture(scope="module")
def vf(seeded_states):
    return voicefixer_amd.VoiceFixer.from_state(*seeded_states)


def _blocks(s, x, sizes=SIZES):
    got, at, n = [], 0, x.shape[-1]
    for k in list(sizes) + [n]:
        got.append(s.push(x[..., at:at + k]))
        at = min(at + k, n)
    got.append(s.finish())
    return got


def _open(vf, rate_out, **kw):
    return vf.open_stream(chunk_seconds=CS, overlap_seconds=OVS, sample_rate=44100,
                          output_sample_rate=None if rate_out == 44100 else rate_out, **kw)


CONFIGS = {"plain": {}, "levelled": dict(leveller=-20, limiter=True, true_peak=True), "all": dict(channels="all")}


@pytest.mark.parametrize("rate_out", [44100, 48000])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_session_meter_is_a_tap(vf, rate_out, config):
    kw = CONFIGS[config]
    x = _signal(44100, 5 * 44100 + 311, 2, 40, levels=(0.1, 0.01, 0.05))
    x = x if config == "all" else x[0]
    s0 = _open(vf, rate_out, **kw)
    plain = _blocks(s0, x)
    assert s0.loudness_report is None
    s1 = _open(vf, rate_out, meter=True, **kw)
    mid = None
    metered = []
    at = 0
    for k in SIZES + [x.shape[-1]]:
        metered.append(s1.push(x[..., at:at + k]))
        at = min(at + k, x.shape[-1])
        mid = s1.loudness_report                              # (readable at any time; changes nothing: the bits below)
    metered.append(s1.finish())
    assert len(metered) == len(plain)
    for a, b in zip(metered, plain):                          # bit for bit AND block for block
        assert a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(_bits(a), _bits(b))
    Z = np.concatenate(plain, axis=1)
    assert mid["seconds"] <= Z.shape[1] / rate_out
    m = voicefixer_amd.LoudnessMeter(rate_out, channels="all" if config == "all" else None)
    m.push(Z if config == "all" else Z[0])
    want = m.finish()
    got = s1.loudness_report                                  # after finish (and close): the final figures
    print("session %s -> %d Hz: %r" % (config, rate_out, got))
    assert got == want and list(got) == list(loudness.METER_KEYS) and got["seconds"] == Z.shape[1] / rate_out
    assert got["integrated"] > -70.0 and got["true_peak"] >= got["sample_peak"] > -math.inf
    if config == "levelled":
        assert abs(got["integrated"] - (-20.0)) < 3.0        # the leveller's target, loosely: the meter sees what it did
        s2 = _open(vf, rate_out, meter=True, bit_depth=16, **kw)
        pcm = _blocks(s2, x)
        assert pcm[-1].dtype == np.int16 and sum(b.shape[1] for b in pcm) == Z.shape[1]
        assert s2.loudness_report == want                     # the float signal ahead of the word-length reduction
