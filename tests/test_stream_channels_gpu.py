"""Every channel in a streaming session on the MI355X: the linked span kernels (vfx_limit_span_rows_f32,
vfx_level_span_rows_f32; ops.limit_span_rows / level_span_rows) against the float64 specifications (``ref_fixed_linked`` of
tests/test_stream_channels_cpu.py, loudness.level_reference_linked) and against themselves -- a programme cut into spans, with
padded rows and misaligned windows, must give the bits of the single span -- and the ``channels="all"`` session against
``limit`` / ``level`` / ``quantize`` of its plain (C, N) output.

Bounds.  Limiter: |out - ref| <= Cl (TP_BOUND max(1, gL / Cl) + (2 H + 9) 2^-24), TP_BOUND = 2e-6 max(1, max e) with the LINKED
e, and the same bound, relative, for min g: the formula of tests/test_stream_limiter_gpu.py unchanged (the kernels repeat its
arithmetic on a maximum of envelopes, and a maximum adds no rounding).  Leveller: anchors 0.002 dB under the asserted condition
that every l_q is >= 0.5 LU from the gate, samples SAMPLE_REL |ref|: the bounds of tests/test_leveller_gpu.py (the weighted sum of C
energies adds C roundings of 2^-53 each).  Session: every channel within 2e-5 rms of the mono session on that channel, the bound
tests/test_multichannel_gpu.py holds restore_inmem(channels="all") to.  Observed on the MI355X: see DESIGN.md 3.18."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import voicefixer_amd  # noqa: E402
from voicefixer_amd import _lib, loudness, ops  # noqa: E402
from test_true_peak_cpu import ref_true_peak  # noqa: E402
from test_stream_channels_cpu import ref_fixed_linked  # noqa: E402

PAD = 40
INT64_MAX = 2 ** 63 - 1
ANCHOR_DB = 0.002
SAMPLE_REL = 10.0 ** (ANCHOR_DB / 20.0) - 1.0 + 4 * 2.0 ** -24


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _noise(rng, shape, amp=0.1):
    return (amp * rng.uniform(-1, 1, shape)).astype(np.float32)


def _steps(rng, n, fs, levels=(0.02, 0.2, 0.005, 0.08)):
    x = rng.standard_normal(n)
    seg = int(0.7 * fs)
    for i in range(0, n, seg):
        x[i:i + seg] *= levels[(i // seg) % len(levels)]
    return x.astype(np.float32)


def _rows_in(X, lo, hi, gap, off):
    """X[:, lo:hi] as a device (C, hi - lo) view of a NaN buffer: rows ``gap`` floats apart beyond their length, the first one
    ``off`` floats past a 16-byte boundary.  Returns (view, buffer, host copy of the buffer)."""
    Cn, wlen = X.shape[0], hi - lo
    stride = wlen + gap
    buf = np.full(PAD + 4 + Cn * stride + PAD, np.nan, np.float32)
    for c in range(Cn):
        buf[PAD + off + c * stride:PAD + off + c * stride + wlen] = X[c, lo:hi]
    d = torch.from_numpy(buf).cuda()
    assert d.data_ptr() % 16 == 0
    return torch.as_strided(d, (Cn, wlen), (stride, 1), PAD + off), d, buf


def _rows_out(Cn, n, gap, off):
    stride = n + gap
    d = torch.full((PAD + 4 + Cn * stride + PAD,), float("nan"), device="cuda")
    return torch.as_strided(d, (Cn, n), (stride, 1), PAD + off), d


def _taken(view, buf, Cn, n, gap, off):
    """The (C, n) outputs of a ``_rows_out`` buffer; everything around them must still be NaN."""
    host = buf.cpu().numpy()
    stride = n + gap
    mask = np.zeros(host.shape, bool)
    for c in range(Cn):
        mask[PAD + off + c * stride:PAD + off + c * stride + n] = True
    assert np.all(np.isnan(host[~mask])), "the guards around out"
    out = view.cpu().numpy()
    assert not np.any(np.isnan(out))
    return out


# ---- the linked limiter ---------------------------------------------------------------------------------------------------------

def _window(N, m0, m1, H, Bk, Fw, known):
    lo = max(0, m0 - 2 * H - Bk)
    hi = m1 - 1 + 2 * H + Fw
    return lo, (min(N - 1, hi) if known else hi) + 1


def _lspan(X, fs, gain_db, m0, m1, lo, hi, known, ceiling_db=-1.0, true_peak=True, ms=3.0, shift=0, gap=0, xoff=0, ooff=0):
    """Outputs [m0, m1) of every channel from the windows X[:, lo:hi]; NaN between the rows, around the windows and around out."""
    xv, xd, xhost = _rows_in(X, lo, hi, gap, xoff)
    ov, od = _rows_out(X.shape[0], m1 - m0, gap, ooff)
    lib = _lib.lib()
    c0 = lib.vfx_launch_count()
    rec = ops.limit_span_rows(xv, lo + shift, X.shape[1] + shift if known else None, fs, gain_db, m0 + shift, m1 + shift, ov,
                              ceiling_db, true_peak, ms)
    assert lib.vfx_launch_count() - c0 == (3 if m1 > m0 else 0)          # whatever the span and C
    out = _taken(ov, od, X.shape[0], m1 - m0, gap, ooff)
    assert np.array_equal(xd.cpu().numpy(), xhost, equal_nan=True)
    return out, rec.cpu().numpy()


def _lwhole(X, fs, gain_db, **kw):
    return _lspan(X, fs, gain_db, 0, X.shape[1], 0, X.shape[1], True, **kw)


def _lcheck(what, progs, fs, gains, ceiling_db=-1.0, true_peak=True, ms=3.0):
    Cl = 10.0 ** (ceiling_db / 20.0)
    H = loudness.limiter_window(fs, ms)[0]
    worst, worst_g = 0.0, 0.0
    for i, X in enumerate(progs):
        gain_db = gains[i % len(gains)]
        gL = 10.0 ** (gain_db / 20.0)
        got, rec = _lwhole(X, fs, gain_db, ceiling_db=ceiling_db, true_peak=true_peak, ms=ms)
        ref = ref_fixed_linked(X, fs, gL, ceiling_db, ms, true_peak)
        assert ref["H"] == H
        tpb = 2e-6 * max(1.0, float(ref["e"].max()))
        tol = Cl * (tpb * max(1.0, gL / Cl) + (2 * H + 9) * 2.0 ** -24)
        err = float(np.abs(got.astype(np.float64) - ref["out"]).max())
        gerr = abs(rec[0] - ref["g"].min())
        worst, worst_g = max(worst, err / tol), max(worst_g, gerr / (tol / Cl))
        print("linked limiter %s [%d] C = %d N = %d: |out - ref| / bound = %.3f, min g / bound = %.3f"
              % (what, i, X.shape[0], X.shape[1], err / tol, gerr / (tol / Cl)))
        assert err <= tol, (what, i, X.shape, err, tol)
        assert gerr <= tol / Cl, (what, i, rec[0], ref["g"].min())
        assert rec[1] == float(np.abs(got).max()), (what, i)
        assert rec[1] <= Cl * (1 + 1e-12) + tol, (what, i, rec[1] / Cl)
    print("linked limiter %s: worst |out - ref| / bound = %.3f, min g / bound = %.3f over %d programmes" % (what, worst, worst_g, len(progs)))
    return worst


def _peaked(rng, Cn, N, silent=None):
    """Noise with single peaks at 0, N - 1, 1023, 1024 (where they exist), each in another channel; ``silent``: a channel of zeros."""
    X = _noise(rng, (Cn, N))
    if silent is not None:
        X[silent] = 0.0
    loud = [c for c in range(Cn) if c != silent]
    for i, p in enumerate(sorted({0, N - 1, 1023, 1024})):
        if 0 <= p < N:
            X[loud[i % len(loud)], p] = 0.97 if i % 2 == 0 else -0.95
    return X


@pytest.mark.parametrize("Cn", [2, 3])
def test_limiter_lengths_and_peak_positions_against_float64(Cn):
    fs, H = 44100, 132
    rng = np.random.default_rng(Cn)
    progs = []
    for N in (1, 2 * H + 1, 1025, 5000):
        progs += [_peaked(rng, Cn, N), _peaked(rng, Cn, N, silent=Cn - 1)]
    _lcheck("44.1 kHz C = %d" % Cn, progs, fs, [6.0, 12.0])


@pytest.mark.parametrize("fs,true_peak", [(8000, True), (96000, True), (192000, True), (44100, False)])
def test_limiter_rates_and_modes_against_float64(fs, true_peak):
    rng = np.random.default_rng(fs + true_peak)
    H = loudness.limiter_window(fs, 3.0)[0]
    N = 2 * H + 1500
    X = _noise(rng, (2, N))
    X[0, N // 4], X[1, N // 2], X[0, N - 1], X[1, 0] = 0.97, -0.99, 0.9, 0.95
    _lcheck("%d Hz tp=%d" % (fs, true_peak), [X], fs, [6.0], true_peak=true_peak)


@pytest.mark.parametrize("true_peak", [True, False])
def test_limiter_one_channel_is_the_mono_kernel(true_peak):
    fs = 44100
    rng = np.random.default_rng(7)
    x = _noise(rng, 5000)
    x[0], x[1023], x[2600], x[4999] = 0.97, -0.95, 0.99, 0.9
    xd = torch.from_numpy(x).cuda()
    want = torch.empty_like(xd)
    rec = ops.limit_span(xd, 0, 5000, fs, 6.0, 0, 5000, want, -1.0, true_peak, 3.0).cpu().numpy()
    got, r = _lwhole(x[None], fs, 6.0, true_peak=true_peak)
    assert np.array_equal(_bits(got[0]), _bits(want.cpu().numpy())) and np.array_equal(r, rec) and r[0] < 0.6
    # an interior span with the end unknown
    H, Bk, Fw = loudness.limiter_reach(fs, 3.0, true_peak)
    lo, hi = _window(5000, 900, 3000, H, Bk, Fw, False)
    part = torch.empty((2100,), device="cuda")
    rec = ops.limit_span(xd[lo:hi], lo, None, fs, 6.0, 900, 3000, part, -1.0, true_peak, 3.0).cpu().numpy()
    got, r = _lspan(x[None], fs, 6.0, 900, 3000, lo, hi, False, true_peak=true_peak, xoff=1, ooff=3)
    assert np.array_equal(_bits(got[0]), _bits(part.cpu().numpy())) and np.array_equal(r, rec)


@pytest.mark.parametrize("true_peak", [True, False])
def test_limiter_exact_pass_through(true_peak):
    fs, gain_db = 44100, 6.0
    gLf = np.float32(10.0 ** (gain_db / 20.0))
    H = loudness.limiter_reach(fs, 3.0, True)[0]
    rng = np.random.default_rng(21)
    X = _noise(rng, (3, 5000), amp=0.12)                      # Cl / gL = 0.447: nothing near it, between the samples either
    got, rec = _lwhole(X, fs, gain_db, true_peak=true_peak)
    assert np.array_equal(_bits(got), _bits(gLf * X)) and rec[0] == 1.0
    X[1, 2600] = 0.97                                         # a peak in channel 1 only: every channel is reduced around it
    got, rec = _lwhole(X, fs, gain_db, true_peak=true_peak)
    far = np.abs(np.arange(5000) - 2600) > 2 * H + 94
    assert np.array_equal(_bits(got[:, far]), _bits((gLf * X)[:, far])) and rec[0] < 0.5
    for c in range(3):
        assert not np.array_equal(_bits(got[c, ~far]), _bits((gLf * X)[c, ~far])), c
    near = np.abs(np.arange(5000) - 2600) <= H
    ratio = got[:, near].astype(np.float64) / (np.float64(gLf) * X[:, near])
    assert np.abs(ratio / ratio[1] - 1.0).max() < 3e-7       # the same g in every channel (two fp32 roundings apart)


@pytest.mark.parametrize("true_peak", [True, False])
def test_limiter_split_invariance_bit_for_bit(true_peak):
    """A 5000-sample C = 2 programme cut into spans, each from its MINIMAL windows, rows apart (NaN between them), windows and
    outputs 1, 2, 3 floats off a 16-byte boundary, n_total unknown wherever the ready rule allows."""
    fs = 44100
    H, Bk, Fw = loudness.limiter_reach(fs, 3.0, true_peak)
    rng = np.random.default_rng(40 + true_peak)
    N = 5000
    X = _noise(rng, (2, N))
    for i, p in enumerate((0, 700, 1023, 1024, 2 * H, 2500, 2500 + H, 4000, N - 1)):
        X[i % 2, p] = 0.97 if p % 2 == 0 else -0.95
    want, rec = _lwhole(X, fs, 6.0, true_peak=true_peak)
    cuts = sorted(set([1, 1023, 1024, 1025, 2 * H, 2 * H + 1] + [int(v) for v in rng.integers(1, N, 3)]))
    got, gmin, vmax, unknown = [], 1.0, 0.0, 0
    for i, (m0, m1) in enumerate(zip([0] + cuts, cuts + [N])):
        known = m1 + 2 * H + Fw > N
        unknown += not known
        lo, hi = _window(N, m0, m1, H, Bk, Fw, known)
        o, r = _lspan(X, fs, 6.0, m0, m1, lo, hi, known, true_peak=true_peak, gap=(0, 5, 7, 6)[i % 4], xoff=(i + 1) % 4,
                      ooff=(i + 2) % 4)
        got.append(o)
        gmin, vmax = min(gmin, r[0]), max(vmax, r[1])
    assert unknown >= 5
    assert np.array_equal(_bits(np.concatenate(got, axis=1)), _bits(want))
    assert (gmin, vmax) == (rec[0], rec[1]) and gmin < 0.6                       # exact folds


def test_limiter_position_independence():
    fs = 44100
    H, Bk, Fw = loudness.limiter_reach(fs, 3.0, True)
    rng = np.random.default_rng(3)
    X = _noise(rng, (2, 5000))
    X[0, 1500], X[1, 2047], X[0, 2900] = 0.97, -0.96, 0.99
    m0, m1 = 1400, 3100
    lo, hi = _window(5000, m0, m1, H, Bk, Fw, False)
    a, ra = _lspan(X, fs, 6.0, m0, m1, lo, hi, False)
    assert np.array_equal(_bits(a), _bits(_lwhole(X, fs, 6.0)[0][:, m0:m1])) and ra[0] < 0.6
    for shift in (2 ** 33, 2 ** 33 + 1):
        b, rb = _lspan(X, fs, 6.0, m0, m1, lo, hi, False, shift=shift, gap=3)
        assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(ra, rb), shift


def test_limiter_refusals_launch_nothing():
    fs = 44100
    H, Bk, Fw = loudness.limiter_reach(fs, 3.0, True)
    bank, J, c = ops.true_peak_bank("cuda", 4)
    N = 3000
    xd = torch.zeros((2 * N,), device="cuda")
    buf = torch.full((2 * N + 64,), float("nan"), device="cuda")
    rec = torch.full((2,), 7.0, dtype=torch.float64, device="cuda")
    lib = _lib.lib()
    nb = lib.vfx_limit_span_rows_workspace_bytes(N, H, 2)
    assert nb > 0 and nb == lib.vfx_limit_span_workspace_bytes(N, H) == lib.vfx_limit_span_rows_workspace_bytes(N, H, 8)
    for bad in ((N, 0, 2), (N, 4097, 2), (-1, H, 2), (N, H, 0), (N, H, 9)):
        assert lib.vfx_limit_span_rows_workspace_bytes(*bad) == 0
    ws = torch.empty((nb // 8 + 2,), dtype=torch.float64, device="cuda")
    P = lambda t: None if t is None else t.data_ptr()
    good = dict(xw=P(xd), ws_=N, C=2, g0=0, wlen=N, n_total=N, m0=0, m1=N, gain=2.0, ceiling=-1.0, H=H, bank=P(bank), J=J, R=4, c=c,
                out=P(buf), os_=N, rec=P(rec), ws=P(ws), nb=nb)

    def call(**kw):
        a = dict(good, **kw)
        return lib.vfx_limit_span_rows_f32(a["xw"], a["ws_"], a["C"], a["g0"], a["wlen"], a["n_total"], a["m0"], a["m1"],
                                           C.c_double(a["gain"]), C.c_double(a["ceiling"]), a["H"], a["bank"], a["J"], a["R"],
                                           a["c"], a["out"], a["os_"], a["rec"], a["ws"], a["nb"], None)

    bad = [dict(wlen=N - 1), dict(g0=1, wlen=N - 1),          # what vfx_limit_span_f32 refuses ...
           dict(m0=1000, m1=2000, g0=1000 - 2 * H - Bk + 1, wlen=N - (1000 - 2 * H - Bk + 1)),
           dict(m0=1000, m1=2000, n_total=INT64_MAX, wlen=2000 + 2 * H + Fw - 1),
           dict(m0=10, m1=9), dict(m0=-1), dict(m1=N + 1, wlen=N + 1, ws_=N + 1), dict(g0=-1),
           dict(H=0), dict(H=4097), dict(R=3), dict(R=0), dict(bank=None), dict(J=0), dict(c=4 * J),
           dict(gain=float("nan")), dict(gain=float("inf")), dict(gain=0.0), dict(gain=-2.0),
           dict(ceiling=float("nan")), dict(ceiling=float("inf")),
           dict(nb=nb - 16), dict(ws=P(ws) + 8), dict(ws=None), dict(rec=None), dict(xw=None), dict(out=None),
           dict(C=0), dict(C=9), dict(C=-1),                  # ... and what the rows add
           dict(ws_=N - 1), dict(os_=N - 1), dict(ws_=-N), dict(os_=0),
           dict(out=P(xd) + 4 * (2 * N - 1)), dict(out=P(xd)), dict(out=P(xd) + 4 * N),
           dict(out=P(xd) - 4 * (2 * N - 1)), dict(C=1, out=P(xd) + 4 * (N - 1))]
    c0 = lib.vfx_launch_count()
    for kw in bad:
        assert call(**kw) == -1, kw                           # VFX_EINVAL
    assert call(m0=500, m1=500) == 0                          # an empty span: VFX_OK, nothing launched
    torch.cuda.synchronize()
    assert lib.vfx_launch_count() == c0
    assert bool(torch.isnan(buf).all()) and rec.cpu().tolist() == [7.0, 7.0]
    assert call() == 0 and call(R=1, bank=None) == 0 and call(C=1, out=P(xd) + 4 * N) == 0     # (good calls are good)
    torch.cuda.synchronize()
    assert lib.vfx_launch_count() == c0 + 9 and not bool(torch.isnan(buf[:2 * N]).any()) and bool(torch.isnan(buf[2 * N:]).all())
    x2 = xd.view(2, N)
    o2 = buf[:2 * N].view(2, N)
    with pytest.raises(_lib.VfxError):
        ops.limit_span_rows(x2[:, :100], 0, N, fs, 6.0, 0, 50, o2)
    with pytest.raises(_lib.VfxError):
        ops.limit_span_rows(x2, 0, N, fs, 6.0, 0, N, o2[:, :N - 1])
    with pytest.raises(ValueError):
        ops.limit_span_rows(x2, 0, N, fs, None, 0, 50, o2)
    with pytest.raises(ValueError):
        ops.limit_span_rows(torch.zeros((9, 10), device="cuda"), 0, 10, fs, 6.0, 0, 10, torch.zeros((9, 10), device="cuda"))
    assert ops.limit_span_rows(x2, 0, N, fs, 6.0, 5, 5, o2).cpu().tolist() == [1.0, 0.0]


# ---- the linked leveller --------------------------------------------------------------------------------------------------------

_SPEC = {}


def _spec(key, X, fs, T, weights, mg=12.0, gate=-50.0):
    if key not in _SPEC:
        st = {}
        ref = loudness.level_reference_linked(X, fs, T, mg, gate, weights, stats=st)
        l = st["l"]
        assert np.all(np.abs(l[np.isfinite(l)] - gate) >= 0.5), (key, "an anchor within 0.5 LU of the gate")
        _SPEC[key] = (ref, st)
    return _SPEC[key]


def _vrun(X, fs, T, weights=None, mg=12.0, gate=-50.0, cuts=(), gap=0, xoff=0, ooff=0, each=None):
    """The programme through ops.level_span_rows in the spans [0, c1), ... [ck, N) from windows that hold the whole rows."""
    Cn, N = X.shape
    xv, xd, xhost = _rows_in(X, 0, N, gap, xoff)
    ov, od = _rows_out(Cn, N, gap, ooff)
    state = torch.full((loudness.LEVELLER_STATE,), 7.0, dtype=torch.float64, device="cuda")      # (m0 = 0 initialises it)
    lib = _lib.lib()
    edges = [0] + [c for c in cuts if 0 < c < N] + [N]
    for m0, m1 in zip(edges[:-1], edges[1:]):
        c0 = lib.vfx_launch_count()
        ops.level_span_rows(xv, 0, N, fs, T, m0, m1, ov[:, m0:m1], state, mg, gate, weights)
        assert 2 <= lib.vfx_launch_count() - c0 <= 3
        if each is not None:
            each(m1, state.cpu().numpy())
    out = _taken(ov, od, Cn, N, gap, ooff)
    assert np.array_equal(xd.cpu().numpy(), xhost, equal_nan=True)
    st = state.cpu().numpy()
    assert st[6] == 0.0
    return out, st


def _against_spec(key, X, fs, T, weights=None):
    hop, N = loudness.hop_length(fs), X.shape[1]
    ref, sp = _spec(key, X, fs, T, weights)
    got, st = _vrun(X, fs, T, weights)
    Q = N // hop
    assert (int(st[2]), int(st[3])) == (Q + 1, int(sp["held"].sum())) == (sp["anchors"], sp["gated"]), key
    G = np.full(Q + 1, np.nan)

    def each(m1, s):
        na = int(s[2])
        assert na == loudness.leveller_counts(m1, hop, Q)[0]
        G[na - 1] = s[4]
        if na == 2:
            G[0] = 20.0 * np.log10(s[8])

    cut, cst = _vrun(X, fs, T, weights, cuts=range(hop, N, hop), gap=5, xoff=1, ooff=2, each=each)
    assert np.array_equal(_bits(cut), _bits(got)) and np.array_equal(cst, st), key
    assert not np.any(np.isnan(G))
    aerr = float(np.abs(G - sp["G"]).max())
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    tol = SAMPLE_REL * np.abs(ref.astype(np.float64))
    serr = float((err / np.maximum(tol, 1e-300)).max())
    print("linked leveller %s: C = %d N = %d, worst |G - spec| = %.2e dB (bound %.0e), worst sample error / bound = %.3f; G in "
          "[%.2f, %.2f], %d of %d gated" % (key, X.shape[0], N, aerr, ANCHOR_DB, serr, st[0], st[1], int(st[3]), int(st[2])))
    assert aerr <= ANCHOR_DB, (key, aerr, int(np.abs(G - sp["G"]).argmax()))
    assert np.all(err <= tol), (key, serr)
    assert abs(st[0] - sp["min_gain_db"]) <= ANCHOR_DB and abs(st[1] - sp["max_gain_db"]) <= ANCHOR_DB
    return got, st


@pytest.mark.parametrize("Cn", [2, 6])
def test_leveller_against_the_float64_specification(Cn):
    """fs = 8000, hop = 800: every window clipped (29 hop + 5), clipped at both ends and unclipped between (45 hop + 17); C = 6
    with the Table 4 weights, whose LFE weight is zero."""
    fs, hop = 8000, 800
    rng = np.random.default_rng(50 + Cn)
    lv = [(0.02, 0.2, 0.005, 0.08), (0.1, 0.01, 0.05, 0.3), (0.05, 0.05, 0.2, 0.01)]
    assert Cn != 6 or loudness.channel_weights(6)[3] == 0.0
    for n in (29 * hop + 5, 45 * hop + 17):
        X = np.stack([_steps(rng, n, fs, lv[c % 3]) for c in range(Cn)])
        _against_spec("steps-%d-%d" % (Cn, n), X, fs, -20.0)


def test_leveller_44k_against_the_float64_specification():
    fs = 44100
    rng = np.random.default_rng(44)
    n = int(1.5 * fs) + 13
    X = np.stack([_steps(rng, n, fs), _steps(rng, n, fs, (0.1, 0.01, 0.05))])
    _against_spec("steps-44k", X, fs, -23.0)


def test_leveller_exact():
    fs, hop = 8000, 800
    rng = np.random.default_rng(60)
    N = 33 * hop + 17
    x, y = _steps(rng, N, fs), _steps(rng, N, fs, (0.1, 0.01, 0.3))
    xd = torch.from_numpy(x).cuda()
    want = torch.empty_like(xd)
    mst = torch.full((loudness.LEVELLER_STATE,), 7.0, dtype=torch.float64, device="cuda")
    ops.level_span(xd, 0, N, fs, -20.0, 0, N, want, mst)
    want, mst = want.cpu().numpy(), mst.cpu().numpy()
    assert mst[1] > mst[0]
    # C = 1 (weight 1): the bits and the state of the mono kernels
    got, st = _vrun(x[None], fs, -20.0)
    assert np.array_equal(_bits(got[0]), _bits(want)) and np.array_equal(st, mst)
    # weights [1, 0]: the a_q of the mono call on channel 0, applied to both
    got, st = _vrun(np.stack([x, x[::-1].copy()]), fs, -20.0, weights=[1.0, 0.0])
    assert np.array_equal(_bits(got[0]), _bits(want)) and np.array_equal(st, mst)
    rev = x[::-1].copy()
    lone = torch.empty_like(xd)
    ops.level_span(torch.from_numpy(rev).cuda(), 0, N, fs, -20.0, 0, N, lone, torch.zeros_like(torch.from_numpy(mst)).cuda())
    assert not np.array_equal(_bits(got[1]), _bits(lone.cpu().numpy()))         # (channel 1 follows channel 0's gain, not its own)
    got, st = _vrun(np.stack([x, x]), fs, -20.0, weights=[1.0, 0.0])
    assert np.array_equal(_bits(got[1]), _bits(want)) and np.array_equal(_bits(got[0]), _bits(want))
    got, st = _vrun(np.stack([x, x]), fs, -20.0, weights=[0.5, 0.5])            # 0.5 E + 0.5 E = E
    assert np.array_equal(_bits(got[1]), _bits(want)) and np.array_equal(st, mst)
    # spans of one quarter and of hop + 1, rows apart, windows and outputs off a 16-byte boundary
    X = np.stack([x, y, rev])
    whole, wst = _vrun(X, fs, -20.0)
    for k, (step, gap, xoff, ooff) in enumerate(((hop, 3, 1, 2), (hop + 1, 5, 2, 3), (hop + 1, 2, 3, 1))):
        got, st = _vrun(X, fs, -20.0, cuts=range(step, N, step), gap=gap, xoff=xoff, ooff=ooff)
        assert np.array_equal(_bits(got), _bits(whole)) and np.array_equal(st, wst), k


def test_leveller_refusals_launch_nothing():
    fs, hop = 8000, 800
    N = 30 * hop
    p = loudness.leveller_plan(fs)
    xd = torch.zeros((2 * N,), device="cuda")
    buf = torch.full((2 * N + 64,), float("nan"), device="cuda")
    state = torch.full((loudness.LEVELLER_STATE,), 7.0, dtype=torch.float64, device="cuda")
    mpow = torch.from_numpy(p["mpow"]).cuda()
    coef = (C.c_double * 10)(*[float(v) for v in p["coef"]])
    bad_coef = (C.c_double * 10)(*([float("nan")] + [float(v) for v in p["coef"][1:]]))
    W = lambda *v: (C.c_double * len(v))(*v)
    lib = _lib.lib()
    nb = lib.vfx_level_span_rows_workspace_bytes(N, hop, 2)
    assert nb > lib.vfx_level_span_workspace_bytes(N, hop) > 0
    for bad in ((-1, hop, 2), (N, 399, 2), (N, 19201, 2), (2 ** 30 + 1, hop, 2), (N, hop, 0), (N, hop, 9)):
        assert lib.vfx_level_span_rows_workspace_bytes(*bad) == 0
    ws = torch.empty((nb // 8 + 2,), dtype=torch.float64, device="cuda")
    P = lambda t: None if t is None else t.data_ptr()
    good = dict(xw=P(xd), ws_=N, C=2, w=W(1.0, 1.0), g0=0, wlen=N, n_total=N, m0=0, m1=N, fs=fs, coef=coef, mpow=P(mpow), S=p["S"],
                T=-16.0, mg=12.0, gate=-50.0, state=P(state), out=P(buf), os_=N, ws=P(ws), nb=nb)

    def call(**kw):
        a = dict(good, **kw)
        return lib.vfx_level_span_rows_f32(a["xw"], a["ws_"], a["C"], a["w"], a["g0"], a["wlen"], a["n_total"], a["m0"], a["m1"],
                                           a["fs"], a["coef"], a["mpow"], a["S"], C.c_double(a["T"]), C.c_double(a["mg"]),
                                           C.c_double(a["gate"]), a["state"], a["out"], a["os_"], a["ws"], a["nb"], None)

    bad = [dict(wlen=N - 1), dict(m0=0, m1=5 * hop, wlen=15 * hop - 1),          # what vfx_level_span_f32 refuses ...
           dict(m0=15 * hop, m1=16 * hop, g0=15 * hop + 1, wlen=N - 15 * hop - 1),
           dict(n_total=INT64_MAX, m1=20 * hop + 1), dict(n_total=INT64_MAX, m1=N),
           dict(fs=192001), dict(fs=3999), dict(S=p["S"] + 32), dict(S=0),
           dict(mg=40.5), dict(mg=-0.1), dict(mg=float("nan")), dict(T=0.0), dict(T=-70.5), dict(T=float("nan")),
           dict(gate=-16.0), dict(gate=-71.0), dict(gate=float("nan")), dict(coef=bad_coef),
           dict(m0=10, m1=9), dict(m0=-1), dict(m1=N + 1, wlen=N + 1, ws_=N + 1), dict(g0=-1),
           dict(nb=nb - 256), dict(ws=P(ws) + 8), dict(ws=None), dict(state=None), dict(xw=None), dict(out=None), dict(mpow=None),
           dict(coef=None),
           dict(C=0), dict(C=9), dict(w=None), dict(w=W(1.0, -0.5)), dict(w=W(1.0, float("nan"))), dict(w=W(float("inf"), 1.0)),
           dict(ws_=N - 1), dict(os_=N - 1), dict(os_=0),     # ... and what the rows add
           dict(out=P(xd) + 4 * (2 * N - 1)), dict(out=P(xd)), dict(out=P(xd) + 4 * N), dict(out=P(xd) - 4 * (2 * N - 1))]
    c0 = lib.vfx_launch_count()
    for kw in bad:
        assert call(**kw) == -1, kw                           # VFX_EINVAL
    assert call(m0=500, m1=500) == 0                          # an empty span: VFX_OK, nothing launched
    torch.cuda.synchronize()
    assert lib.vfx_launch_count() == c0
    assert bool(torch.isnan(buf).all()) and state.cpu().tolist() == [7.0] * loudness.LEVELLER_STATE
    assert call(n_total=INT64_MAX, m1=20 * hop, os_=N) == 0                     # (three launches)
    assert call(m0=20 * hop, out=P(buf) + 4 * 20 * hop) == 0                    # (two: no quarter is new)
    torch.cuda.synchronize()
    assert lib.vfx_launch_count() == c0 + 5 and not bool(torch.isnan(buf[:2 * N]).any()) and bool(torch.isnan(buf[2 * N:]).all())
    assert state.cpu().tolist()[2:7] == [31.0, 31.0, 0.0, 30.0, 0.0]             # silence: every anchor gated, the gain held at 0
    x2, o2 = xd.view(2, N), buf[:2 * N].view(2, N)
    for kw in (dict(max_gain_db=41.0), dict(gate=-10.0), dict(weights=[1.0]), dict(weights=[1.0, -1.0])):
        with pytest.raises(ValueError):
            ops.level_span_rows(x2, 0, N, fs, -16.0, 0, N, o2, state, **kw)
    with pytest.raises(_lib.VfxError):
        ops.level_span_rows(x2[:, :100], 0, N, fs, -16.0, 0, 50, o2, state)


# ---- the session and the public functions -----------------------------------------------------------------------------------------

CS, OVS = 1.5, 0.25
SIZES = [1, 0, 4410, 7, 70001]
_Z = {}


@pytest.fixture(scope="module")
def vf(seeded_states):
    return voicefixer_amd.VoiceFixer.from_state(*seeded_states)


def _pushed(s, x, sizes=SIZES):
    got, at, n = [], 0, x.shape[-1]
    for k in list(sizes) + [n]:
        got.append(s.push(x[..., at:at + k]))
        at = min(at + k, n)
        assert s.position == sum(g.shape[1] for g in got)
    got.append(s.finish())
    return np.concatenate(got, axis=1)


def _open(vf, rate_in, rate_out, **kw):
    return vf.open_stream(chunk_seconds=CS, overlap_seconds=OVS, sample_rate=rate_in,
                          output_sample_rate=None if rate_out == 44100 else rate_out, **kw)


def _input(rate_in):
    rng = np.random.default_rng(rate_in)
    n = (5 * 44100 + 311) * rate_in // 44100 if rate_in != 44100 else 5 * 44100 + 311
    return np.stack([_steps(rng, n, rate_in, levels=(0.1, 0.01, 0.05)), _steps(rng, n, rate_in, levels=(0.02, 0.2, 0.005, 0.08))])


def _plain(vf, rate_in, rate_out):
    """(x (2, n), Z (2, N), the two mono sessions' outputs): stepped levels that differ between the channels."""
    key = (rate_in, rate_out)
    if key not in _Z:
        x = _input(rate_in)
        s = _open(vf, rate_in, rate_out, channels="all")
        Z = _pushed(s, x)
        assert s.limiter_stats is None and s.leveller_stats is None and Z.dtype == np.float32 and s.position == Z.shape[1]
        monos = [_pushed(_open(vf, rate_in, rate_out), x[c]) for c in range(2)]
        _Z[key] = (x, Z, monos)
    return _Z[key]


def _rms(v):
    return float(np.sqrt(np.mean(np.square(v.astype(np.float64)))))


@pytest.mark.parametrize("rate_in,rate_out", [(44100, 44100), (44100, 48000), (16000, 44100)])
def test_session_restores_every_channel(vf, rate_in, rate_out):
    x, Z, monos = _plain(vf, rate_in, rate_out)
    assert Z.shape == (2, monos[0].shape[1])
    again = _pushed(_open(vf, rate_in, rate_out, channels="all"), x, sizes=[30000, 3, 0, 100000])
    assert np.array_equal(_bits(again), _bits(Z))             # another block split: the same bits
    for c in range(2):
        d = _rms(Z[c] - monos[c][0])
        print("session %d -> %d Hz channel %d: rms of the difference to the mono session = %.3e (bound 2e-5), rms = %.3e"
              % (rate_in, rate_out, c, d, _rms(Z[c])))
        assert d <= 2e-5, (c, d)
    # "mix" / "first": the mono session, bit for bit
    assert np.array_equal(_bits(_pushed(_open(vf, rate_in, rate_out, channels="first"), x)), _bits(monos[0]))
    mixed = _pushed(_open(vf, rate_in, rate_out), x.mean(axis=0, dtype=np.float32))
    assert np.array_equal(_bits(_pushed(_open(vf, rate_in, rate_out, channels="mix"), x)), _bits(mixed))


@pytest.mark.parametrize("rate_in,rate_out", [(44100, 44100), (44100, 48000)])
def test_session_linked_stages_equal_the_public_functions(vf, rate_in, rate_out):
    x, Z, monos = _plain(vf, rate_in, rate_out)
    st = {}
    want = voicefixer_amd.level(Z, -20.0, sample_rate=rate_out, stats=st, channels="all")
    assert want.shape == Z.shape and st["anchors"] == Z.shape[1] // loudness.hop_length(rate_out) + 1
    assert st["gated"] < st["anchors"] and st["max_gain_db"] > st["min_gain_db"]
    s = _open(vf, rate_in, rate_out, channels="all", leveller=-20)
    got = _pushed(s, x)
    assert got.shape == Z.shape and np.array_equal(_bits(got), _bits(want)) and s.leveller_stats == st and s.limiter_stats is None
    st2 = {}
    assert np.array_equal(_bits(voicefixer_amd.level(Z, -20.0, sample_rate=rate_out, stats=st2, _span=4099, channels="all")),
                          _bits(want)) and st2 == st
    # the link keeps the balance between the channels; two mono levellers move it
    bal = lambda v: _rms(v[0]) / _rms(v[1])
    lone = np.concatenate([_pushed(_open(vf, rate_in, rate_out, leveller=-20), x[c]) for c in range(2)])
    print("balance: linked %.3e, two mono sessions %.3e" % (abs(bal(got) / bal(Z) - 1.0), abs(bal(lone) / bal(Z) - 1.0)))
    assert abs(bal(lone) / bal(Z) - 1.0) > 1e-3
    # leveller + limiter (at 0 dB)
    lst = {}
    lim = voicefixer_amd.limit(want, gain_db=0.0, true_peak=True, sample_rate=rate_out, stats=lst, channels="all")
    s = _open(vf, rate_in, rate_out, channels="all", leveller=-20, limiter=True, true_peak=True)
    got = _pushed(s, x)
    assert np.array_equal(_bits(got), _bits(lim)) and s.leveller_stats == st and s.limiter_stats == lst
    # ... and 16 bit behind both: quantize of the (2, N) array, integer for integer
    s = _open(vf, rate_in, rate_out, channels="all", leveller=-20, limiter=True, true_peak=True, bit_depth=16, dither_seed=5)
    q = _pushed(s, x)
    assert q.dtype == np.int16 and q.shape == Z.shape and np.array_equal(q, voicefixer_amd.quantize(lim, 16, "tpdf", 5))
    # a gain and the limiter without a leveller
    Cl = 10.0 ** (-1.0 / 20.0)
    gain_db = float(20.0 * np.log10(Cl / max(ref_true_peak(Z[c], rate_out) for c in range(2))) + 6.0)
    lst = {}
    lim = voicefixer_amd.limit(Z, gain_db, true_peak=True, sample_rate=rate_out, stats=lst, channels="all")
    assert lst["max_reduction_db"] > 5.9 and lst["peak_out_db"] <= -1.0 + 3e-4
    s = _open(vf, rate_in, rate_out, channels="all", gain_db=gain_db, limiter=True, true_peak=True)
    got = _pushed(s, x)
    assert np.array_equal(_bits(got), _bits(lim)) and s.limiter_stats == lst
    # the gain alone: float32(gL) Z, and the balance stays
    s = _open(vf, rate_in, rate_out, channels="all", gain_db=gain_db)
    got = _pushed(s, x)
    assert np.array_equal(_bits(got), _bits(np.float32(10.0 ** (gain_db / 20.0)) * Z))
    assert abs(bal(got) / bal(Z) - 1.0) <= 1e-6
    assert voicefixer_amd.limit(np.zeros((3, 0), np.float32), channels="all").shape == (3, 0)
