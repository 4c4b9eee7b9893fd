"""The streaming session without a GPU: the C ABI of the span resampler and the cross-fade is declared and bound, the two
window helpers agree with brute force, StreamPlanner returns plan_stream_chunks whatever the block sizes, and the argument
errors of open_stream / push come before any device work."""
import os
import re

import numpy as np
import pytest

from voicefixer_amd import api, audio_io, _lib
from conftest import ROOT


def test_header_declares_and_lib_binds_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "vfx_hip.h")).read()
    assert re.search(r"int vfx_resample_span_f32\(const float\* xw, int64_t g0, int64_t wlen, int64_t n_total,", hdr)
    assert re.search(r"int vfx_xfade_f32\(const float\* tail, const float\* head, const float\* fade, int64_t n,", hdr)
    assert len(_lib.SIGNATURES["vfx_resample_span_f32"][1]) == 13
    assert len(_lib.SIGNATURES["vfx_xfade_f32"][1]) == 6
    src = open(os.path.join(ROOT, "voicefixer_amd", "csrc", "vfx_resample.hip")).read()
    assert "resample_span_kernel" in src and "xfade_kernel" in src


def test_ready_outputs_and_span_window_against_brute_force():
    rng = np.random.default_rng(11)
    for _ in range(300):
        up, down, J = int(rng.integers(1, 40)), int(rng.integers(1, 40)), int(rng.integers(1, 30))
        c = int(rng.integers(0, up * J))
        kmax = lambda m: (c + m * down) // up
        for avail in [0, 1, 2] + [int(v) for v in rng.integers(0, 400, 6)]:
            m = 0
            while kmax(m) < avail:
                m += 1
            assert audio_io.ready_outputs(avail, up, down, c) == m, (up, down, c, avail)
        m0 = int(rng.integers(0, 500))
        m1 = m0 + int(rng.integers(1, 60))
        lo, hi = audio_io.span_window(m0, m1, up, down, J, c)
        reads = [k for m in range(m0, m1) for k in range(kmax(m) - J + 1, kmax(m) + 1)]
        assert (lo, hi) == (min(reads), max(reads) + 1), (up, down, J, c, m0, m1)
    # the real filters: a span's window is J samples for one output, and outputs are ready one filter half late
    for pair in ((16000, 44100), (44100, 48000), (44100, 16000)):
        up, down = audio_io.rate_ratio(*pair)
        _, J, c = audio_io.hq_bank(up, down)
        lo, hi = audio_io.span_window(7, 8, up, down, J, c)
        assert hi - lo == J
        assert audio_io.ready_outputs(0, up, down, c) == 0
        assert audio_io.ready_outputs(10 ** 6, up, down, c) <= audio_io.converted_length(10 ** 6, *pair)


def _fed(n, chunk, overlap, min_tail, cuts):
    p = api.StreamPlanner(chunk, overlap, min_tail)
    got, at = [], 0
    for b in [min(b, n) for b in cuts] + [n]:
        got += p.feed(b - at)
        at = b
    assert p.known == n
    return got + p.finish()


def test_stream_planner_equals_plan_stream_chunks():
    rng = np.random.default_rng(3)
    for _ in range(1500):
        overlap = int(rng.integers(0, 300))
        chunk = overlap + 1025 + int(rng.integers(0, 3000))
        min_tail = int(rng.choice([1024, 1535]))
        n = int(rng.integers(0, 6 * chunk))
        cuts = sorted(int(v) for v in rng.integers(0, n + 1, int(rng.integers(0, 8))))
        assert _fed(n, chunk, overlap, min_tail, cuts) == api.plan_stream_chunks(n, chunk, overlap, min_tail), \
            (n, chunk, overlap, min_tail, cuts)


@pytest.mark.parametrize("min_tail", [1024, 1535])
def test_stream_planner_on_the_merge_boundary(min_tail):
    chunk, overlap = 5000, 700
    hop = chunk - overlap
    for k in (1, 2, 4):                      # the tail behind chunk k is exactly mergeable / one sample too long to merge
        for extra in (0, 1):
            n = k * hop + overlap + min_tail + extra
            want = api.plan_stream_chunks(n, chunk, overlap, min_tail)
            assert len(want) == k + extra and want[-1][0] + want[-1][1] == n
            for cuts in ([], [1], [n - 1], [n], [hop, 2 * hop], list(range(0, n, 997))):
                assert _fed(n, chunk, overlap, min_tail, cuts) == want, (n, cuts)
    for n in (0, 1, 1025, chunk - 1, chunk, chunk + 1, chunk + min_tail, chunk + min_tail + 1):      # n <= chunk and just past it
        for cuts in ([], [n // 2], list(range(0, n, 313))):
            assert _fed(n, chunk, overlap, min_tail, cuts) == api.plan_stream_chunks(n, chunk, overlap, min_tail)
    p = api.StreamPlanner(chunk, overlap, min_tail)
    assert p.feed(chunk + min_tail) == [] and p.feed(1) == [(0, chunk)]      # settled by the first sample past the merge range
    p.finish()
    with pytest.raises(RuntimeError):
        p.finish()
    with pytest.raises(RuntimeError):
        p.feed(1)
    with pytest.raises(ValueError):
        api.StreamPlanner(2000, 1000)


def test_argument_errors_come_before_the_device():
    vf = api.VoiceFixer.__new__(api.VoiceFixer)     # (no device, no weights: the checks come first)
    opened = lambda **kw: api.VoiceFixer.open_stream(vf, **kw)
    for bad in (0, -16000, 44100.5, True):
        with pytest.raises(ValueError):
            opened(sample_rate=bad)
        with pytest.raises(ValueError):
            opened(output_sample_rate=bad)
    with pytest.raises(ValueError):
        opened(chunk_seconds=1.0, overlap_seconds=1.0)
    with pytest.raises(ValueError):
        opened(chunk_seconds=(11025 + 1024) / 44100.0, overlap_seconds=0.25)      # chunk == overlap + 1024
    with pytest.raises(NotImplementedError):
        opened(mode=2)
    with pytest.raises(ValueError):
        opened(mode=3)
    with pytest.raises(ValueError):
        opened(batch_size=0)
    s = opened(chunk_seconds=1.5, overlap_seconds=0.25, sample_rate=16000, output_sample_rate=48000)
    assert isinstance(s, api.RestoreSession) and s.position == 0
    with pytest.raises(ValueError):
        s.push(np.zeros((2, 100), np.float32))
    with pytest.raises(ValueError):
        s.push(np.float32(0.5))
    assert s.push(np.zeros(0, np.float32)).shape == (1, 0)      # an empty block needs no device either
    with pytest.raises(ValueError):              # under MIN_SAMPLES: refused before anything is launched
        s.finish()
    with pytest.raises(RuntimeError):
        s.finish()
    with pytest.raises(RuntimeError):
        s.push(np.zeros(10, np.float32))
    with opened() as s2:
        pass
    with pytest.raises(RuntimeError):
        s2.push(np.zeros(10, np.float32))


def test_restore_stream_still_refuses_an_output_rate():
    vf = api.VoiceFixer.__new__(api.VoiceFixer)
    with pytest.raises(NotImplementedError):
        api.VoiceFixer.restore_stream(vf, np.zeros(44100, np.float32), output_sample_rate=48000)


# ---- the session's bookkeeping on the host: the device launchers replaced by numpy stand-ins ------------------------------

def _poly_outputs(x_at, n_total, up, down, m0, m1):
    """Outputs [m0, m1) of the polyphase sum, one fixed float64 evaluation per output: x_at(idx) returns the samples at
    global indices idx (inside [0, n_total))."""
    bank, J, c = audio_io.hq_bank(up, down)
    m = np.arange(m0, m1, dtype=np.int64)
    pos = c + m * down
    kmax = pos // up
    idx = (kmax - J + 1)[:, None] + np.arange(J)[None]
    ok = (idx >= 0) & (idx < n_total)
    xv = np.zeros(idx.shape, np.float64)
    xv[ok] = x_at(idx[ok])
    return np.sum(bank[pos - kmax * up].astype(np.float64) * xv, axis=1).astype(np.float32)


class _FakePipe:
    device = "cpu"

    def __init__(self):
        self.shapes = []

    def run_checked(self, fn):
        return fn()

    def restore(self, seg, n, vocoder=None):
        """A stand-in for the path: depends on the sample, on its place in the chunk and on the chunk's length."""
        import torch
        self.shapes.append((seg.shape[0], n))
        t = torch.arange(n, dtype=torch.float32) / n
        return torch.tanh(3.0 * seg[:, :n]) * (0.5 + 0.4 * t) + 0.01 * torch.cos(7.0 * t)


class _FakeVF:
    _check_mode = staticmethod(api.VoiceFixer._check_mode)
    _restore_segments = staticmethod(api.VoiceFixer._restore_segments)

    def __init__(self):
        self.pipe = _FakePipe()

    def _get_pipe(self):
        return self.pipe


@pytest.fixture
def host_ops(monkeypatch):
    import torch
    from voicefixer_amd import ops
    calls = {"span": 0, "xfade": 0, "window": 0}

    def resample_rows(x, n_rows, y, up, down, ny_max=None, row_index=None):
        for r in range(x.shape[0]):
            n = int(n_rows[r])
            row = x[r].numpy().astype(np.float64)
            ny = -(-n * up // down)
            y[r, :ny] = torch.from_numpy(_poly_outputs(lambda i: row[i], n, up, down, 0, ny))

    def resample_span(xw, g0, n_total, up, down, m0, m1, y):
        _, J, c = audio_io.hq_bank(up, down)
        n = 2 ** 63 - 1 if n_total is None else n_total
        lo, hi = audio_io.span_window(m0, m1, up, down, J, c)
        assert max(lo, 0) >= g0 and min(hi - 1, n - 1) < g0 + xw.numel(), "the window does not cover the span"
        win = xw.numpy().astype(np.float64)
        calls["span"] += 1
        calls["window"] = max(calls["window"], xw.numel())
        y[:m1 - m0] = torch.from_numpy(_poly_outputs(lambda i: win[i - g0], n, up, down, m0, m1))

    def xfade(tail, head, fade, out):
        calls["xfade"] += 1
        a, b, f = tail.numpy().copy(), head.numpy().copy(), fade.numpy()
        assert np.array_equal(f, np.arange(len(f), dtype=np.float32) / max(len(f), 1))
        out.copy_(torch.from_numpy(a * (1.0 - f) + b * f))

    def hf_cut(wav, N, ratio=0.95):
        return 0.9 * wav[:, :512 * (N // 512)], None

    monkeypatch.setattr(ops, "resample_rows", resample_rows)
    monkeypatch.setattr(ops, "resample_span", resample_span)
    monkeypatch.setattr(ops, "xfade", xfade)
    monkeypatch.setattr(ops, "hf_cut", hf_cut)
    return calls


@pytest.mark.parametrize("mode,rate_in,rate_out,batch", [(0, 44100, 44100, 1), (1, 44100, 44100, 1), (0, 16000, 44100, 1),
                                                          (0, 44100, 48000, 1), (1, 16000, 48000, 1), (0, 48000, 16000, 3)])
def test_session_bookkeeping_equals_restore_stream(host_ops, mode, rate_in, rate_out, batch):
    """With the path and the launchers replaced by host stand-ins (one fixed evaluation per output sample, so a span and a
    whole row agree to the bit by construction), everything the session adds -- what it keeps of the input, when a chunk is
    settled, the in-place cross-fade, what is final, the windows it hands to the converters -- must reproduce
    restore_stream on the concatenated input followed by a whole-row conversion, bit for bit."""
    import torch
    rng = np.random.default_rng(100 * mode + rate_in % 97)
    cs, ovs = 0.16, 0.03                                   # 7056-sample chunks (mode 1: 6656), 1323 samples of overlap
    n = int(0.55 * rate_in) + 77
    x = (0.3 * rng.standard_normal(n)).astype(np.float32)
    vf = _FakeVF()
    xt = torch.from_numpy(x)[None]
    x44, (n44,) = api.convert_rows(xt, [n], [rate_in])
    y44 = api.VoiceFixer.restore_stream(vf, x44[0, :n44].numpy(), cs, ovs, batch, mode)
    n_chunks = sum(b for b, _ in vf.pipe.shapes)
    assert n_chunks >= 3 and (mode == 0 or y44.shape[1] < n44)
    if rate_out == 44100:
        want = y44
    else:
        up, down = audio_io.rate_ratio(44100, rate_out)
        want = torch.empty((1, audio_io.converted_length(y44.shape[1], 44100, rate_out)))
        from voicefixer_amd import ops
        ops.resample_rows(torch.from_numpy(y44), [y44.shape[1]], want, up, down)
        want = want.numpy()
    shapes_ref, vf.pipe.shapes = vf.pipe.shapes, []
    s = api.VoiceFixer.open_stream(vf, cs, ovs, batch, mode, None, rate_in, None if rate_out == 44100 else rate_out)
    got, at, early = [], 0, False
    for k in [1, 0, 441, 7001, 3, 2500] + [1000] * 40:
        blk = x[at:at + k]
        at += len(blk)
        got.append(s.push(blk))
        assert got[-1].dtype == np.float32 and got[-1].ndim == 2 and s.position == sum(g.shape[1] for g in got)
        early = early or (at < n and got[-1].shape[1] > 0)
    assert at == n and early
    got.append(s.finish())
    got = np.concatenate(got, axis=1)
    assert got.shape == want.shape and s.position == want.shape[1]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if batch == 1:
        assert vf.pipe.shapes == shapes_ref
    if rate_in != 44100 or rate_out != 44100:              # the windows stay a filter length plus a block, not the file
        assert 0 < host_ops["window"] < 12000 and host_ops["span"] >= 3
    assert host_ops["xfade"] == n_chunks - 1               # one cross-fade per chunk boundary


# ---- the contract of a span stage (stream._SpanStage), on a toy operator ---------------------------------------------------

def _toy_stage(d, b, span):
    """Output m = x[m - b] + 2 x[m + d] (indices clipped to the row): ``d`` samples late, reading ``b`` samples behind itself."""
    import torch
    from voicefixer_amd import stream

    class Toy(stream._SpanStage):
        def __init__(self):
            super().__init__(span)
            self.calls, self.window, self.at = 0, 0, 0     # (at: the output the next call starts with)

        def _ready(self, n):
            return max(0, n - d)

        def _run(self, a, e, n_total, y):
            assert a == self.at and a < e and y.numel() == e - a        # in order, no output twice, no empty call
            assert self.span is None or e - a <= self.span
            last = 2 ** 62 if n_total is None else n_total - 1
            lo, hi = max(a - b, 0), min(e - 1 + d, last)
            assert self.g0 <= lo and hi < self.g0 + self.win.numel(), "the window does not cover the span"
            m = torch.arange(a, e)
            y.copy_(self.win[(m - b).clamp(min=0) - self.g0] + 2.0 * self.win[(m + d).clamp(max=last) - self.g0])
            self.calls += 1
            self.window = max(self.window, self.win.numel())
            self.at = e

        def _keep(self, m1):
            return m1 - b

    return Toy()


@pytest.mark.parametrize("d,b", [(0, 0), (5, 3), (40, 17)])
@pytest.mark.parametrize("span", [None, 7, 1 << 22])
def test_span_stage_contract(d, b, span):
    import torch
    rng = np.random.default_rng(1000 * d + b)
    for n in sorted({1, d, d + 1, 1000}):
        x = torch.from_numpy(rng.integers(-1000, 1000, n).astype(np.float32))
        m = np.arange(n)
        want = x.numpy()[np.clip(m - b, 0, None)] + 2.0 * x.numpy()[np.clip(m + d, None, max(n - 1, 0))]
        whole_stage = _toy_stage(d, b, span)
        whole = whole_stage.whole(x)
        assert whole.dtype == torch.float32 and np.array_equal(whole.numpy(), want) and whole_stage.m_done == n
        assert whole_stage.calls == (0 if n == 0 else 1 if span is None else -(-n // span))
        for trial in range(5):
            # random cuts (equal ones: empty blocks); the last trial opens with one sample and an empty block
            cuts = sorted(int(v) for v in rng.integers(0, n + 1, int(rng.integers(0, 9))))
            if trial == 4:
                cuts = sorted([min(1, n), min(1, n), n // 2])
            st = _toy_stage(d, b, span)
            got, at, empty_handed, largest = [], 0, 0, 0
            for cpos in cuts + ([n] if n else []):
                blk = x[at:cpos].clone()
                at, largest = cpos, max(largest, blk.numel())
                got.append(st.feed(blk))
                empty_handed += got[-1].numel() == 0
                assert st.n_in == at and st.m_done == st._ready(at) == sum(g.numel() for g in got)
                assert st.win.numel() <= d + b + 1 + largest
            got.append(st.finish("cpu"))
            assert st.m_done == n
            got = torch.cat(got)
            assert np.array_equal(got.numpy(), want) and np.array_equal(got.numpy(), whole.numpy())     # once each, in order
            assert st.window <= d + b + 1 + largest
            calls = st.calls
            st.release()
            assert st.win is None and st.calls == calls and st.m_done == n       # what the stage recorded outlives the window
            assert trial < 4 or empty_handed > 0
    never = _toy_stage(d, b, span)
    y = never.finish("cpu")
    assert y.shape == (0,) and y.dtype == torch.float32 and never.calls == 0 and never.m_done == 0
