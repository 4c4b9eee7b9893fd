"""The fixed-gain look-ahead limiter of a streaming session (loudness.py) on the host: the float64 reference
``ref_fixed`` and its properties, the ready rule, the bookkeeping of ``_SpanLimiter`` and of the session with a numpy stand-in
for ops.limit_span, the argument rules and the public surface.  No GPU."""
import inspect
import os
import re

import numpy as np
import pytest
from scipy.ndimage import minimum_filter1d

import voicefixer_amd
from voicefixer_amd import _lib, api, loudness
from test_limiter_cpu import ref_envelope, ref_window
from test_stream_session_cpu import _FakeVF, host_ops  # noqa: F401  (host_ops: the fixture of the session's stand-ins)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ref_fixed(x, fs, gL, ceiling_db=-1.0, ms=3.0, true_peak=True):
    """F in float64 on one row (N,): ``ref_limit`` of tests/test_limiter_cpu.py without the bound test and without the trim.
    A dict with ``out``, ``e``, ``c``, ``m``, ``g`` (N,) and ``H``."""
    x = np.asarray(x, np.float64)
    N = x.size
    Cl = 10.0 ** (ceiling_db / 20.0)
    H, w = ref_window(fs, ms)
    if N == 0:
        z = np.zeros(0)
        return dict(out=z, e=z, c=z, m=z, g=z, H=H)
    e = ref_envelope(x, fs, true_peak)
    c = np.where(e > 0, np.minimum(1.0, Cl / (gL * np.where(e > 0, e, 1.0))), 1.0)
    m = minimum_filter1d(c, size=2 * H + 1, mode="constant", cval=1.0)
    d = np.pad(1.0 - m, H, mode="edge")                       # m[clamp(n + k, 0, N - 1)]
    g = 1.0 - np.convolve(d, w, mode="valid")
    return dict(out=gL * g * x, e=e, c=c, m=m, g=g, H=H)


def _row(rng, n, peaks, amp=0.1):
    x = amp * rng.uniform(-1, 1, n)
    for p in peaks:
        if 0 <= p < n:
            x[p] = 0.97 if p % 2 == 0 else -0.93
    return x.astype(np.float32)


@pytest.mark.parametrize("fs,true_peak", [(8000, True), (44100, True), (96000, True), (192000, True), (44100, False)])
@pytest.mark.parametrize("gL", [2.0, 4.0])
def test_reference_properties(fs, true_peak, gL):
    rng = np.random.default_rng(fs % 1000 + int(gL))
    H, Bk, Fw = loudness.limiter_reach(fs, 3.0, true_peak)
    N = 8 * H + 700
    x = _row(rng, N, [3 * H + 100])
    Cl = 10.0 ** (-1.0 / 20.0)
    ref = ref_fixed(x, fs, gL, -1.0, 3.0, true_peak)
    assert ref["H"] == H
    hot = np.flatnonzero(ref["e"] > Cl / gL)
    assert hot.size and hot.min() >= 3 * H + 100 - Fw - 1 and hot.max() <= 3 * H + 100 + Bk + 1
    far = np.ones(N, bool)                                    # no sample within 2 H + reach exceeds Cl / gL
    for p in np.flatnonzero(np.abs(x) > Cl / gL):
        far[max(p - 2 * H - Fw - 1, 0):p + 2 * H + Bk + 2] = False
    assert far.sum() > N // 3
    assert np.array_equal(ref["out"][far], gL * x.astype(np.float64)[far]) and np.all(ref["g"][far] == 1.0)
    assert np.abs(ref["out"]).max() <= Cl * (1 + 1e-12)
    assert np.all(ref["g"] <= ref["c"] + 1e-15) and ref["g"].min() < 0.6
    # a row that nowhere exceeds the threshold is a plain product
    q = _row(rng, N, [], amp=0.9 * Cl / gL / 1.5)
    assert np.array_equal(ref_fixed(q, fs, gL, -1.0, 3.0, False)["out"], gL * q.astype(np.float64))


def test_limiter_reach_and_ready():
    assert loudness.limiter_reach(44100, 3.0, True) == (132, 94, 93)
    assert loudness.limiter_reach(8000, 3.0, True) == (24, 94, 93)
    assert loudness.limiter_reach(96000, 3.0, True) == (288, 94, 93)
    assert loudness.limiter_reach(192000, 3.0, True) == (576, 0, 0)
    assert loudness.limiter_reach(44100, 3.0, False) == (132, 0, 0)
    assert loudness.limiter_reach(44100, 1.0, True)[0] == 44
    assert loudness.limiter_ready(0, 132, 93) == 0 and loudness.limiter_ready(357, 132, 93) == 0
    assert loudness.limiter_ready(358, 132, 93) == 1 and loudness.limiter_ready(10 ** 12, 1, 0) == 10 ** 12 - 2
    with pytest.raises(ValueError):
        loudness.limiter_reach(768000, 10.0, False)           # 7680 samples
    with pytest.raises(ValueError):
        loudness.limiter_reach(44100, 3.0, 1)


@pytest.mark.parametrize("fs", [8000, 44100, 96000])
@pytest.mark.parametrize("true_peak", [True, False])
def test_ready_rule(fs, true_peak):
    """Truncating the row at n_known changes no output below limiter_ready(n_known): exact float64 equality."""
    rng = np.random.default_rng(fs)
    H, Bk, Fw = loudness.limiter_reach(fs, 3.0, true_peak)
    N = 7 * H + 900
    x = _row(rng, N, [0, H, 2 * H + 50, 4 * H + 3, 4 * H + 200, N - 1, N - H])
    full = ref_fixed(x, fs, 2.0, -1.0, 3.0, true_peak)["out"]
    for n_known in [1, 2, 2 * H + Fw, 2 * H + Fw + 1, 2 * H + Fw + 2, 4 * H + 3 + 2 * H + Fw, 4 * H + 4 + 2 * H + Fw,
                    N - 1, N] + [int(v) for v in rng.integers(1, N, 6)]:
        r = loudness.limiter_ready(n_known, H, Fw)
        assert r == max(0, n_known - 2 * H - Fw)
        part = ref_fixed(x[:n_known], fs, 2.0, -1.0, 3.0, true_peak)["out"]
        assert np.array_equal(part[:r], full[:r]), (n_known, r)
    assert np.array_equal(ref_fixed(x[:N], fs, 2.0, -1.0, 3.0, true_peak)["out"], full)      # at the end all N are final


@pytest.mark.parametrize("fs", [8000, 44100, 96000])
def test_ready_rule_is_not_slack(fs):
    """The first output the rule withholds does depend on what comes: a peak at position 0 with a higher one behind it, and
    n_known = 1 (output 0 = limiter_ready(1) changes); in the sample-peak mode, a peak in the first unknown sample changes
    output limiter_ready(n_known) for any n_known."""
    rng = np.random.default_rng(fs + 1)
    H, Bk, Fw = loudness.limiter_reach(fs, 3.0, True)
    x = _row(rng, 6 * H + 400, [])
    x[0], x[1] = 0.9, 0.97
    assert loudness.limiter_ready(1, H, Fw) == 0
    full, part = ref_fixed(x, fs, 2.0)["out"], ref_fixed(x[:1], fs, 2.0)["out"]
    assert part[0] != full[0]
    n_known = 3 * H + 17
    x = _row(rng, 6 * H + 400, [n_known])
    r = loudness.limiter_ready(n_known, H, 0)
    full, part = ref_fixed(x, fs, 2.0, true_peak=False)["out"], ref_fixed(x[:n_known], fs, 2.0, true_peak=False)["out"]
    assert np.array_equal(part[:r], full[:r]) and part[r] != full[r]


# ---- bookkeeping: ops.limit_span replaced by a stand-in that knows the whole-row result ---------------------------------------

class _StandIn:
    def __init__(self, row, fs, gain_db, ceiling_db, true_peak, ms):
        self.row = np.asarray(row, np.float32)
        self.args = (fs, gain_db, ceiling_db, true_peak, ms)
        ref = ref_fixed(self.row, fs, 10.0 ** (gain_db / 20.0), ceiling_db, ms, true_peak)
        self.out, self.g = ref["out"].astype(np.float32), ref["g"]
        self.H, self.Bk, self.Fw = loudness.limiter_reach(fs, ms, true_peak)
        self.calls, self.window, self.done = 0, 0, 0

    def __call__(self, xw, g0, n_total, rate, gain_db, m0, m1, out, ceiling_db=-1.0, true_peak=False, lookahead_ms=3.0):
        import torch
        assert (rate, gain_db, ceiling_db, true_peak, lookahead_ms) == self.args
        N = self.row.size
        win = xw.numpy()
        assert g0 >= 0 and g0 + win.size <= N
        assert np.array_equal(win.view(np.uint32), self.row[g0:g0 + win.size].view(np.uint32)), "the window holds other samples"
        assert m0 == self.done and m0 < m1 <= N
        if n_total is None:                                   # only what the ready rule allows, from the samples in the window
            assert m1 <= loudness.limiter_ready(g0 + win.size, self.H, self.Fw)
        else:
            assert n_total == N
        lo, hi = max(0, m0 - 2 * self.H - self.Bk), min(N - 1 if n_total is not None else 2 ** 62, m1 - 1 + 2 * self.H + self.Fw)
        assert g0 <= lo and hi < g0 + win.size, "the window does not cover the span"
        self.calls += 1
        self.window = max(self.window, win.size)
        self.done = m1
        out[:m1 - m0] = torch.from_numpy(self.out[m0:m1])
        return torch.tensor([float(np.float32(self.g[m0:m1].min())), float(np.abs(self.out[m0:m1]).max())], dtype=torch.float64)


@pytest.mark.parametrize("fs,true_peak,ms", [(8000, True, 3.0), (44100, True, 3.0), (96000, True, 1.0), (44100, False, 3.0)])
def test_span_limiter_bookkeeping(monkeypatch, fs, true_peak, ms):
    import torch
    from voicefixer_amd import ops
    rng = np.random.default_rng(fs + 7)
    H, Bk, Fw = loudness.limiter_reach(fs, ms, true_peak)
    reach = 2 * H + Fw
    for N, cuts in [(9 * H + 1500, None), (reach - 5, [3]), (reach + 40, [reach + 38]), (5 * H + 700, [1, 2, 5 * H + 690]),
                    (1, []), (4000, [1999, 2000, 2000])]:
        x = _row(rng, N, [0, N // 3, N // 3 + H, N - 1])
        stand = _StandIn(x, fs, 6.0, -2.0, true_peak, ms)
        monkeypatch.setattr(ops, "limit_span", stand)
        lim = api._SpanLimiter(fs, 6.0, -2.0, true_peak, ms)
        if cuts is None:                                      # random blocks, some shorter than the reach, some empty-handed
            cuts = sorted(int(v) for v in rng.integers(0, N, 14))
        got, at = [], 0
        for cpos in list(cuts) + [N]:
            blk = torch.from_numpy(x[at:cpos].copy())
            at = max(at, cpos)
            if blk.numel():
                got.append(lim.feed(blk).numpy())
                assert lim.m_done == loudness.limiter_ready(at, H, Fw) == sum(g.size for g in got)
        got.append(lim.finish("cpu").numpy())
        got = np.concatenate(got)
        assert got.size == N and np.array_equal(got.view(np.uint32), stand.out.view(np.uint32))
        assert stand.window <= 4 * H + Bk + Fw + 1 + max(np.diff([0] + list(cuts) + [N]).max(), 1)
        st = lim.stats()
        assert st["max_reduction_db"] == -loudness.to_db(float(np.float32(stand.g.min()))) + 0.0
        assert st["peak_out_db"] == loudness.to_db(float(np.abs(stand.out).max()))
    lim = api._SpanLimiter(44100, 0.0)
    assert lim.finish("cpu").numel() == 0 and lim.stats() == {"max_reduction_db": 0.0, "peak_out_db": -np.inf}


@pytest.mark.parametrize("rate_in,rate_out", [(44100, 44100), (44100, 48000), (16000, 48000)])
def test_session_bookkeeping_with_the_limiter(host_ops, monkeypatch, rate_in, rate_out):  # noqa: F811
    """Everything the session adds around the limiter -- the stage order, what it keeps, when an output is final, the
    position, the stats -- with the path, the converters and the limiter replaced by host stand-ins."""
    from voicefixer_amd import ops
    rng = np.random.default_rng(rate_in + rate_out)
    cs, ovs = 0.16, 0.03
    n = int(0.55 * rate_in) + 77
    x = (0.3 * rng.standard_normal(n)).astype(np.float32)
    blocks = [1, 0, 441, 7001, 3, 2500] + [1000] * 40

    def run(**kw):
        s = api.VoiceFixer.open_stream(_FakeVF(), cs, ovs, 1, 0, None, rate_in, None if rate_out == 44100 else rate_out, **kw)
        got, at, pos = [], 0, []
        for k in blocks:
            got.append(s.push(x[at:at + k]))
            at += len(x[at:at + k])
            assert s.position == sum(g.shape[1] for g in got)
            pos.append(s.position)
        got.append(s.finish())
        return s, np.concatenate(got, axis=1), pos

    s0, Z, pos0 = run()
    assert s0.limiter_stats is None and Z.dtype == np.float32
    gain_db = 20.0 * np.log10(0.7 / np.abs(Z).max()) + 6.0
    stand = _StandIn(Z[0], rate_out, gain_db, -3.0, True, 2.0)
    monkeypatch.setattr(ops, "limit_span", stand)
    s1, got, pos1 = run(gain_db=gain_db, limiter=True, peak_ceiling=-3.0, true_peak=True, limiter_lookahead_ms=2.0)
    assert got.shape == Z.shape and s1.position == Z.shape[1]
    assert np.array_equal(got.view(np.uint32), stand.out[None].view(np.uint32))
    late = 2 * stand.H + stand.Fw                             # the limiter's latency, and nothing more
    assert all(b == max(a - late, 0) for a, b in zip(pos0, pos1)) and any(0 < b < Z.shape[1] for b in pos1)
    assert stand.calls >= 3 and stand.window < 16000
    assert s1.limiter_stats == {"max_reduction_db": -loudness.to_db(float(np.float32(stand.g.min()))) + 0.0,
                                "peak_out_db": loudness.to_db(float(np.abs(stand.out).max()))}
    assert s1.limiter_stats["max_reduction_db"] > 1.0
    # the gain alone: float32(gL) Z, no limiter call
    calls = stand.calls
    s2, got2, pos2 = run(gain_db=gain_db)
    assert stand.calls == calls and pos2 == pos0 and s2.limiter_stats is None
    assert np.array_equal(got2.view(np.uint32), (np.float32(10.0 ** (gain_db / 20.0)) * Z).view(np.uint32))


def test_argument_rules_come_before_the_device():
    vf = api.VoiceFixer.__new__(api.VoiceFixer)               # (no device, no weights: the checks come first)
    opened = lambda **kw: api.VoiceFixer.open_stream(vf, **kw)
    with pytest.raises(NotImplementedError, match="gain_db"):
        opened(limiter=True)
    for bad in (1, "yes", None):
        with pytest.raises(ValueError):
            opened(limiter=bad)
        with pytest.raises(ValueError):
            opened(limiter=bad, gain_db=3.0)
    for bad in (True, "3", float("nan"), float("inf"), 60.5, -61):
        with pytest.raises(ValueError):
            opened(gain_db=bad)
        with pytest.raises(ValueError):
            opened(gain_db=bad, limiter=True)
    for kw in (dict(peak_ceiling=0.5), dict(peak_ceiling=-21), dict(true_peak=1), dict(limiter_lookahead_ms=0.05),
               dict(limiter_lookahead_ms=11), dict(peak_ceiling=float("nan"))):
        with pytest.raises(ValueError):                      # validated always, used only with the limiter
            opened(**kw)
        with pytest.raises(ValueError):
            opened(gain_db=0.0, limiter=True, **kw)
    with pytest.raises(ValueError):                          # H = 4410 at the output rate
        opened(gain_db=0.0, limiter=True, limiter_lookahead_ms=10.0, output_sample_rate=441000)
    opened(limiter_lookahead_ms=10.0, output_sample_rate=441000)      # (not used without the limiter)
    s = opened(gain_db=-3.0)
    assert s.limiter_stats is None and s.position == 0
    s = opened(gain_db=60, limiter=True, peak_ceiling=-20, true_peak=True, limiter_lookahead_ms=0.1, output_sample_rate=48000)
    assert s.limiter_stats == {"max_reduction_db": 0.0, "peak_out_db": -np.inf}
    assert s.push(np.zeros(0, np.float32)).shape == (1, 0)
    for fn in (loudness.check_gain,):
        assert fn(None) is None and fn(-60) == -60.0 and fn(np.float32(1.5)) == 1.5
    # the module-level function
    for kw in (dict(gain_db=None), dict(gain_db=True), dict(peak_ceiling=1.0), dict(true_peak=None), dict(lookahead_ms=0.0),
               dict(sample_rate=0), dict(stats=[]), dict(_span=0)):
        with pytest.raises(ValueError):
            voicefixer_amd.limit(np.zeros(10, np.float32), **kw)
    with pytest.raises(ValueError):
        voicefixer_amd.limit(np.zeros((2, 10), np.float32))
    assert voicefixer_amd.limit([]) == []


def test_signature_defaults_and_order():
    for fn in (api.VoiceFixer.open_stream, api.RestoreSession.__init__):
        p = inspect.signature(fn).parameters
        names = list(p)
        assert p["gain_db"].default is None and p["limiter"].default is False
        assert p["peak_ceiling"].default == -1.0 and p["true_peak"].default is False and p["limiter_lookahead_ms"].default == 3.0
        assert names.index("gain_db") == names.index("dither_seed") + 1                     # appended: positional callers keep working
        assert names[names.index("gain_db"):names.index("gain_db") + 3] == ["gain_db", "peak_ceiling", "true_peak"]
    names = list(inspect.signature(api.VoiceFixer.open_stream).parameters)
    assert names[1:14] == ["chunk_seconds", "overlap_seconds", "batch_size", "mode", "your_vocoder_func", "sample_rate",
                           "output_sample_rate", "limiter", "limiter_lookahead_ms", "bit_depth", "dither", "dither_seed", "gain_db"]
    p = inspect.signature(voicefixer_amd.limit).parameters
    assert [(k, v.default) for k, v in p.items()][:7] == [("x", inspect.Parameter.empty), ("gain_db", 0.0), ("peak_ceiling", -1.0),
                                                          ("true_peak", False), ("lookahead_ms", 3.0), ("sample_rate", 44100),
                                                          ("stats", None)]
    assert "limit" in voicefixer_amd.__all__ and voicefixer_amd.limit is api.limit
    with pytest.raises(NotImplementedError):                  # restore_stream is unchanged and still refuses
        api.VoiceFixer.restore_stream(api.VoiceFixer.__new__(api.VoiceFixer), np.zeros(44100, np.float32), limiter=True)


def test_entry_points_declared_mapped_and_bound():
    header = open(os.path.join(ROOT, "include", "vfx_hip.h")).read()
    vmap = open(os.path.join(ROOT, "voicefixer_amd", "csrc", "vfx.map")).read()
    assert re.search(r"global:\s*vfx_\*;", vmap) and "vfx_limit_span_f32" in vmap and "vfx_limit_span_workspace_bytes" in vmap
    for name, nargs in (("vfx_limit_span_workspace_bytes", 2), ("vfx_limit_span_f32", 18)):
        m = re.search(r"\b%s\(([^;]*)\);" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
    from voicefixer_amd import ops
    assert list(inspect.signature(ops.limit_span).parameters) == ["xw", "g0", "n_total", "rate", "gain_db", "m0", "m1", "out",
                                                                  "ceiling_db", "true_peak", "lookahead_ms"]
    mk = open(os.path.join(ROOT, "voicefixer_amd", "csrc", "Makefile")).read()
    assert "vfx_limit_span.inc" in mk
    assert '#include "vfx_limit_span.inc"' in open(os.path.join(ROOT, "voicefixer_amd", "csrc", "vfx_loudness.hip")).read()


# ---- limit() and level(): the row runner on the host ---------------------------------------------------------------------------

@pytest.mark.parametrize("fs", [8000, 44100])
@pytest.mark.parametrize("span", [977, 1 << 22])
def test_limit_and_level_rows_on_the_host(monkeypatch, fs, span):
    """``limit`` and ``level`` with the device replaced by the CPU and the launchers by stand-ins: every row goes through a fresh
    stage as a whole, in runs of ``_span`` outputs that come in order with the row's end known, and the stats arrive as scalars
    for one array and as lists for a list."""
    import torch
    from voicefixer_amd import ops
    monkeypatch.setattr(api, "_device", lambda: torch.device("cpu"))
    rng = np.random.default_rng(fs + span % 1000)
    H, Bk, Fw = loudness.limiter_reach(fs, 3.0, True)
    for N in (1, 2 * H + Fw - 5, 9 * H + 1500):
        x = _row(rng, N, [0, N // 3, N // 3 + H, N - 1])
        runs = -(-N // span)
        for as_list in (False, True):
            stand, ends = _StandIn(x, fs, 6.0, -2.0, True, 3.0), []

            def limit_span(xw, g0, n_total, *a, stand=stand, ends=ends, **kw):
                ends.append(n_total)
                return stand(xw, g0, n_total, *a, **kw)

            monkeypatch.setattr(ops, "limit_span", limit_span)
            st = {}
            got = voicefixer_amd.limit([x] if as_list else x, 6.0, -2.0, True, 3.0, fs, st, span)
            want = {"max_reduction_db": -loudness.to_db(float(np.float32(stand.g.min()))) + 0.0,
                    "peak_out_db": loudness.to_db(float(np.abs(stand.out).max()))}
            if as_list:
                assert isinstance(got, list) and len(got) == 1 and st == {k: [v] for k, v in want.items()}
                got = got[0]
            else:
                assert st == want
            assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), stand.out.view(np.uint32))
            assert stand.calls == runs and stand.done == N and ends == [N] * runs      # (in order: the stand-in asserts m0 == done)

        calls = {"state": 0, "span": 0, "m1": 0}

        def level_state(device):
            calls["state"] += 1
            return torch.zeros((loudness.LEVELLER_STATE,), dtype=torch.float64, device=device)

        def level_span(xw, g0, n_total, rate, target, m0, m1, out, state, max_gain_db=12.0, gate=-50.0):
            assert (n_total, rate, target, max_gain_db, gate) == (N, fs, -20.0, 6.0, -60.0)
            assert m0 == calls["m1"] and m0 < m1 <= N and m1 - m0 <= span and g0 <= m0 and m1 <= g0 + xw.numel()
            out[:m1 - m0] = xw[m0 - g0:m1 - g0]
            state[2] += 1
            calls["span"], calls["m1"] = calls["span"] + 1, m1

        monkeypatch.setattr(ops, "level_state", level_state)
        monkeypatch.setattr(ops, "level_span", level_span)
        for as_list in (False, True):
            calls.update(state=0, span=0, m1=0)
            st = {}
            got = voicefixer_amd.level([x] if as_list else x, -20.0, 6.0, -60.0, fs, st, span)
            want = {"min_gain_db": 0.0, "max_gain_db": 0.0, "anchors": runs, "gated": 0}
            if as_list:
                assert isinstance(got, list) and len(got) == 1 and st == {k: [v] for k, v in want.items()}
                got = got[0]
            else:
                assert st == want
            assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), x.view(np.uint32))
            assert calls == {"state": 1, "span": runs, "m1": N}
    calls.update(state=0, span=0, m1=0)
    st = {}
    assert voicefixer_amd.level(np.zeros(0, np.float32), -20.0, 6.0, -60.0, fs, st, span).shape == (0,)
    assert calls == {"state": 0, "span": 0, "m1": 0} and st == {"min_gain_db": 0.0, "max_gain_db": 0.0, "anchors": 0, "gated": 0}
    st = {}
    assert voicefixer_amd.level([], -20.0, 6.0, -60.0, fs, st, span) == [] and st["anchors"] == []
    monkeypatch.setattr(ops, "limit_span", None)                 # (an empty row makes no call)
    st = {}
    assert voicefixer_amd.limit(np.zeros(0, np.float32), 6.0, -2.0, True, 3.0, fs, st, span).shape == (0,)
    assert st == {"max_reduction_db": 0.0, "peak_out_db": -np.inf}
    assert voicefixer_amd.limit([], stats=st) == [] and st == {"max_reduction_db": [], "peak_out_db": []}
