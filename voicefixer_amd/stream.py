"""The overlap-add streaming mode: the chunk plan (``plan_stream_chunks``, ``StreamPlanner``), the stages that work on a row
that arrives in pieces (``_SpanStage``, its three subclasses and the meter that taps them) and the push-style session that chains them
(``RestoreSession``; ``LoudnessMeter``, the meter on its own).  ``api`` imports this module and re-exports its names; what this module needs of ``api``
it imports inside the functions that need it."""
import numpy as np
import torch

from . import audio_io
from ._lib import VfxError


def plan_stream_chunks(n, chunk, overlap, min_tail=1024):
    """Chunk starts / lengths of the overlap-add streaming mode: chunks of ``chunk`` samples every
    ``chunk - overlap`` samples; the last one is shorter.  A tail that would be too short to restore
    (<= overlap + ``min_tail`` samples: one cross-fade plus the reflect pad of the STFT; mode 1 passes 1535 because its
    pre-filter first shortens a chunk to 512 * (len // 512) samples) is merged into its predecessor."""
    if chunk <= overlap + 1024 or overlap < 0:
        raise ValueError("chunk must exceed overlap + 1024 samples")
    hop = chunk - overlap
    plan = []
    start = 0
    while True:
        length = min(chunk, n - start)
        plan.append([start, length])
        if start + length >= n:
            break
        start += hop
    if len(plan) > 1 and plan[-1][1] <= overlap + min_tail:
        last = plan.pop()
        plan[-1][1] = last[0] + last[1] - plan[-1][0]
    return [tuple(c) for c in plan]


def _check_stream_mode(mode, what):
    """The overlap-add modes (``restore_stream``, ``open_stream``) take modes 0 and 1."""
    if mode == 2:
        raise NotImplementedError("%s: mode=2 is not built -- its per-segment statistics have no overlap-add form" % what)
    if mode not in (0, 1):
        raise ValueError("mode must be 0, 1 or 2")


def _stream_geometry(chunk_seconds, overlap_seconds, mode):
    """(chunk, overlap, min_tail) in 44.1 kHz samples of the overlap-add modes.  Mode 1's pre-filter returns 512 * (len // 512)
    samples, so its chunks are a multiple of 512 long (every full chunk keeps its length) and its shortest tail is 1535
    (``plan_stream_chunks``)."""
    chunk, overlap = int(round(chunk_seconds * 44100)), int(round(overlap_seconds * 44100))
    if mode == 1:
        chunk -= chunk % 512
    return chunk, overlap, 1535 if mode == 1 else 1024


class StreamPlanner:
    """``plan_stream_chunks`` for a waveform whose length is not known yet: ``feed(n_new)`` announces ``n_new`` more
    samples and returns the chunks (start, length) that are settled now, ``finish()`` the rest.  Everything returned,
    concatenated, is ``plan_stream_chunks(n, chunk, overlap, min_tail)`` of the final n, whatever the block sizes.
    ``plan_stream_chunks`` merges a tail of <= overlap + min_tail samples into its predecessor, so the chunk at ``start``
    is settled at length ``chunk`` only once MORE than start + chunk + min_tail samples are known: that is the latency of
    a streaming session."""

    def __init__(self, chunk, overlap, min_tail=1024):
        if chunk <= overlap + 1024 or overlap < 0:
            raise ValueError("chunk must exceed overlap + 1024 samples")
        self.chunk, self.overlap, self.min_tail = int(chunk), int(overlap), int(min_tail)
        self.known = 0       # samples announced so far
        self.start = 0       # start of the first chunk not yet returned
        self.finished = False

    def feed(self, n_new):
        if self.finished:
            raise RuntimeError("StreamPlanner: feed after finish")
        if n_new < 0:
            raise ValueError("StreamPlanner: a negative number of samples")
        self.known += int(n_new)
        out = []
        while self.known > self.start + self.chunk + self.min_tail:
            out.append((self.start, self.chunk))
            self.start += self.chunk - self.overlap
        return out

    def finish(self):
        if self.finished:
            raise RuntimeError("StreamPlanner: finish called twice")
        self.finished = True
        rest = plan_stream_chunks(self.known - self.start, self.chunk, self.overlap, self.min_tail)
        return [(self.start + a, length) for a, length in rest]


LIMIT_SPAN = 1 << 22      # outputs per ops.limit_span call of a ``_SpanLimiter``: bounds the scratch, changes no bit
LEVEL_SPAN = 1 << 22      # outputs per ops.level_span call of a ``_SpanLeveller``: bounds the scratch, changes no bit


class _SpanStage:
    """ONE row that arrives in pieces, through an operator whose output m is a function of the row's samples around m:
    ``feed`` takes the next samples (device (k,)) and returns the outputs that became final with them, ``finish`` the rest
    with the row's end known, ``whole`` all outputs of a row that is there at once.  Kept between calls: ``win``, the
    samples [g0, g0 + wlen) of the row that later outputs still read, ``n_in``, the samples fed, and ``m_done``, the outputs
    returned.  The row may be a PROGRAMME of C channels: C rows of one length that arrive together -- ``feed``,
    ``finish`` and ``whole`` then take and return (C, k), the window is (C, wlen), everything is concatenated, dropped and cloned
    along the last axis, and ``n_in`` / ``m_done`` count samples per channel.  A subclass says what its operator needs:

        _ready(n)                 how many outputs are final once n samples of a row of unknown length are known
        _length(n)                how many outputs a row of n samples has (n, unless the stage changes the rate)
        _run(a, b, n_total, y)    outputs [a, b), b > a, from ``win`` / ``g0`` into y (b - a,) -- (C, b - a), rows of unit
                                  stride, for a programme: its one ops.*_span call (n_total: the row's length, None
                                  while it is unknown)
        _keep(m1)                 the first sample that outputs from m1 on still read (may be negative)

    ``span``: the most outputs one ``_run`` call is given (None: no bound)."""

    def __init__(self, span=None):
        self.span = span
        self.win = None      # device (wlen,) or (C, wlen): samples [g0, g0 + wlen) of the row
        self.rows = None     # C once a programme has been fed (None: one row, 1-D)
        self.g0 = 0
        self.n_in = 0        # samples fed
        self.m_done = 0      # outputs returned

    def _length(self, n):
        return n

    def feed(self, x):
        self.win = x if self.win is None else torch.cat([self.win, x], dim=-1)
        self.rows = x.shape[0] if x.dim() == 2 else None
        self.n_in += x.shape[-1]
        return self._emit(self._ready(self.n_in), None)

    def finish(self, device):
        if self.win is None:
            return torch.empty((0,) if self.rows is None else (self.rows, 0), dtype=torch.float32, device=device)
        return self._emit(self._length(self.n_in), self.n_in)

    def whole(self, x):
        """All outputs of the complete row ``x`` (device (n,) or (C, n)), which serves as the window as it is: the end is known
        from the first call on."""
        self.win, self.g0, self.n_in = x, 0, x.shape[-1]
        self.rows = x.shape[0] if x.dim() == 2 else None
        return self._emit(self._length(self.n_in), self.n_in)

    def release(self):
        """Drop the window; what the subclass has recorded stays readable."""
        self.win = None

    def _emit(self, m1, n_total):
        m0, m1 = self.m_done, max(m1, self.m_done)
        y = torch.empty(tuple(self.win.shape[:-1]) + (m1 - m0,), dtype=torch.float32, device=self.win.device)
        step = self.span or max(m1 - m0, 1)
        for a in range(m0, m1, step):                     # (no outputs: no call)
            b = min(a + step, m1)
            self._run(a, b, n_total, y[..., a - m0:b - m0])
        self.m_done = m1
        # drop what no later output reads (one sample always stays: a window is never empty)
        keep = min(max(self._keep(m1), 0), self.n_in - 1)
        if keep > self.g0:
            self.win = self.win[..., keep - self.g0:].clone()
            self.g0 = keep
        return y


class _SpanConverter(_SpanStage):
    """Rate conversion (ops.resample_span): final are the outputs that read nothing beyond what has arrived
    (audio_io.ready_outputs); a row of n samples has ceil(n * up / down) of them.  Every output has the bits of
    ops.resample_rows on the whole row.  The window holds at most J + down / up + 1 samples beyond a block.  A programme is
    converted channel by channel: a row of a contiguous (C, wlen) window is a window."""

    def __init__(self, rate_in, rate_out):
        super().__init__()
        self.up, self.down = audio_io.rate_ratio(rate_in, rate_out)
        _, self.J, self.c = audio_io.hq_bank(self.up, self.down)

    def _ready(self, n):
        return audio_io.ready_outputs(n, self.up, self.down, self.c)

    def _length(self, n):
        return -(-n * self.up // self.down)

    def _run(self, a, b, n_total, y):
        from . import ops
        if self.win.dim() == 2:
            for c in range(self.win.shape[0]):
                ops.resample_span(self.win[c], self.g0, n_total, self.up, self.down, a, b, y[c])
            return
        ops.resample_span(self.win, self.g0, n_total, self.up, self.down, a, b, y)

    def _keep(self, m1):
        return audio_io.span_window(m1, m1 + 1, self.up, self.down, self.J, self.c)[0]     # output m1 starts at lo(m1)


class _SpanLimiter(_SpanStage):
    """The fixed-gain look-ahead limiter F (loudness.py; ops.limit_span): final are the outputs of
    loudness.limiter_ready.  Every output has the bits of one span over the whole row.  Output m reads from m - 2 H - Bk on, so
    the window holds at most 4 H + Bk + Fw + 1 samples beyond a block.  Kept as well: the calls' records {min g, max |out|} --
    device scalars, folded exactly (min and max) and read by ``stats()`` only.  A programme goes through the LINKED limiter
    (ops.limit_span_rows): one gain curve from the envelope over all channels, one record."""

    def __init__(self, rate, gain_db, peak_ceiling=-1.0, true_peak=False, lookahead_ms=3.0, span=None):
        from . import loudness
        super().__init__(LIMIT_SPAN if span is None else int(span))
        self.rate, self.gain_db, self.ceiling, self.true_peak, self.ms = rate, gain_db, peak_ceiling, true_peak, lookahead_ms
        self.H, self.Bk, self.Fw = loudness.limiter_reach(rate, lookahead_ms, true_peak)
        self.recs = []       # device float64 (2,) each: {min g, max |out|} of the calls so far, folded when read

    def _ready(self, n):
        from . import loudness
        return loudness.limiter_ready(n, self.H, self.Fw)

    def _run(self, a, b, n_total, y):
        from . import ops
        run = ops.limit_span_rows if self.win.dim() == 2 else ops.limit_span
        self.recs.append(run(self.win, self.g0, n_total, self.rate, self.gain_db, a, b, y, self.ceiling, self.true_peak, self.ms))
        if len(self.recs) >= 256:                             # (bounded, whatever the session's length)
            self.recs = [self._fold()]

    def _keep(self, m1):
        return m1 - 2 * self.H - self.Bk

    def _fold(self):
        r = torch.stack(self.recs)
        return torch.stack([r[:, 0].min(), r[:, 1].max()])

    def stats(self):
        """{"max_reduction_db", "peak_out_db"} over what has been returned (reads the device record: the one synchronisation)."""
        from . import loudness
        if len(self.recs) > 1:
            self.recs = [self._fold()]
        gmin, peak = (float(v) for v in self.recs[0].cpu().numpy()) if self.recs else (1.0, 0.0)
        return {"max_reduction_db": -loudness.to_db(gmin) + 0.0, "peak_out_db": loudness.to_db(peak)}


class _SpanLeveller(_SpanStage):
    """The loudness leveller (loudness.py; ops.level_span): final are the outputs of loudness.leveller_ready.
    Every output has the bits of one call over the whole row.  The window starts at the first output not yet returned or, if
    that is earlier, at the region of the next quarter to be measured, two quarters before it: fewer than 11 quarters, 1.1 s,
    beyond a block (the energies behind them live in the device state).  Kept as well: that state with the record, created by
    the first output -- nothing touches the device before -- and read by ``stats()`` only.  A programme goes through the LINKED
    leveller (ops.level_span_rows): the quarter energies summed over the channels with ``weights``
    (loudness.channel_weights), one gain for all channels, still ONE state."""

    def __init__(self, rate, target, max_gain_db=12.0, gate=-50.0, span=None, weights=None):
        from . import loudness
        super().__init__(LEVEL_SPAN if span is None else int(span))
        self.target, self.max_gain_db, self.gate = loudness.check_leveller(target, max_gain_db, gate, rate)
        self.rate, self.hop = int(rate), loudness.hop_length(rate)
        self.weights = weights     # (of a programme; checked against its channel count by whoever knows it)
        self.state = None    # device float64 (loudness.LEVELLER_STATE,)

    def _ready(self, n):
        from . import loudness
        return loudness.leveller_ready(n, self.hop)

    def _run(self, a, b, n_total, y):
        from . import ops
        if self.state is None:
            self.state = ops.level_state(self.win.device)
        if self.win.dim() == 2:
            ops.level_span_rows(self.win, self.g0, n_total, self.rate, self.target, a, b, y, self.state, self.max_gain_db,
                                self.gate, self.weights)
            return
        ops.level_span(self.win, self.g0, n_total, self.rate, self.target, a, b, y, self.state, self.max_gain_db, self.gate)

    def _keep(self, m1):
        from . import loudness
        return min(m1, (loudness.leveller_counts(m1, self.hop)[1] - loudness.LEVELLER_WARMUP) * self.hop)

    def stats(self):
        """{"min_gain_db", "max_gain_db", "anchors", "gated"} over what has been returned (reads the device state: the one
        synchronisation); zeros before the first anchor."""
        if self.state is None:
            return {"min_gain_db": 0.0, "max_gain_db": 0.0, "anchors": 0, "gated": 0}
        v = self.state[:7].cpu().numpy()
        if v[6] != 0.0:
            raise VfxError("leveller: the spans of a row did not come in order")
        return {"min_gain_db": float(v[0]), "max_gain_db": float(v[1]), "anchors": int(v[2]), "gated": int(v[3])}


class _SpanMeter(_SpanStage):
    """The streaming loudness meter (loudness.py; ops.meter_span_rows / ops.meter_report) on ``_SpanStage``'s
    window bookkeeping.  A TAP, not a stage: ``feed`` and ``finish`` return nothing, and what is fed goes on to whoever delivers
    it, neither delayed nor altered.  A session feeds it its final FLOAT signal: behind the output converter, the leveller and
    the limiter (or the fixed gain), ahead of the word-length reduction.  It meters what it can -- up to loudness.meter_ready: the
    interpolated values of a sample read Fw samples ahead -- and keeps the rest in its own window, which starts at
    loudness.meter_keep: Bk samples behind the first sample not yet metered or, if that is earlier, two quarters before the next
    quarter to be measured; fewer than 3 quarters, 0.3 s, beyond a block.  Kept as well: the device state (16 float64) and the
    log of the quarter energies, 8 bytes per 100 ms per programme (288 KB per hour), grown by doubling between calls -- the one
    thing of a session that grows with its length.  A programme (C, k) is metered with ``weights`` (loudness.channel_weights)."""

    QLOG0 = 1024             # quarters of the first log (102 s)

    def __init__(self, rate, weights=None, span=None):
        from . import loudness
        super().__init__(LEVEL_SPAN if span is None else int(span))
        loudness.check_meter(True, rate)
        self.rate, self.hop = int(rate), loudness.hop_length(rate)
        self.R, self.Bk, self.Fw = loudness.meter_reach(rate)
        self.weights = weights
        self.state = None    # device float64 (loudness.METER_STATE,)
        self.qlog = None     # device float64 (capacity,)
        self.final = False   # the end has been metered

    def _ready(self, n):
        from . import loudness
        return loudness.meter_ready(n, self.Fw)

    def _keep(self, m1):
        from . import loudness
        return loudness.meter_keep(m1, self.hop, self.Bk)

    def _room(self, quarters, device):
        """State and log on ``device``, the log with room for ``quarters``."""
        from . import ops
        if self.state is None:
            self.state = ops.meter_state(device)
            self.qlog = torch.zeros((self.QLOG0,), dtype=torch.float64, device=device)
        if quarters > self.qlog.numel():
            grown = torch.zeros((max(quarters, 2 * self.qlog.numel()),), dtype=torch.float64, device=device)
            grown[:self.qlog.numel()] = self.qlog
            self.qlog = grown

    def _run(self, a, b, n_total, y=None):
        from . import ops
        self._room(b // self.hop, self.win.device)
        ops.meter_span_rows(self.win, self.g0, n_total, self.rate, a, b, self.state, self.qlog, self.weights)

    def _emit(self, m1, n_total):
        m0, m1 = self.m_done, max(m1, self.m_done)
        for a in range(m0, m1, self.span):                # (nothing to meter: no call)
            self._run(a, min(a + self.span, m1), n_total)
        self.m_done = m1
        self.final = n_total is not None
        keep = min(self._keep(m1), self.n_in - 1)
        if keep > self.g0:
            self.win = self.win[..., keep - self.g0:].clone()
            self.g0 = keep

    def finish(self, device=None):
        if self.win is not None:
            self._emit(self.n_in, self.n_in)
        self.final = True

    def report(self):
        """The dict of loudness.METER_KEYS over what has been fed (reads the device report: the one synchronisation).  Before
        ``finish``: the figures of loudness.meter_reference(..., final=False) -- the samples fed but not yet metered (fewer than
        Fw) and the quarter they may complete are folded into a COPY of the state by the sample-peak form of the span call
        (they count for the sample peak and for their quarter; their interpolated values are not known yet); the quarter is
        written where the next call writes the same bits.  After it: the final figures.  VfxError if the spans did not come in order."""
        from . import loudness, ops
        out = {"integrated": -np.inf, "loudness_range": 0.0, "max_momentary": -np.inf, "max_short_term": -np.inf,
               "sample_peak": -np.inf, "true_peak": -np.inf, "momentary": -np.inf, "short_term": -np.inf,
               "seconds": self.n_in / float(self.rate)}
        if self.win is None and self.state is None:       # (nothing has been fed, or it was dropped before anything was metered)
            return out
        state = self.state
        if not self.final and self.win is not None and self.n_in > self.m_done:
            self._room(self.n_in // self.hop, self.win.device)
            state = self.state.clone()
            ops.meter_span_rows(self.win, self.g0, None, self.rate, self.m_done, self.n_in, state, self.qlog, self.weights,
                                true_peak=False)
        v = ops.meter_report(state, self.qlog, self.rate).cpu().numpy()
        if v[9] != 0.0:
            raise VfxError("meter: the spans of a row did not come in order" if v[9] == 1.0 else
                           "meter: the state does not belong to this log")
        out.update(integrated=float(v[0]), loudness_range=float(v[1]), max_momentary=float(v[2]), max_short_term=float(v[3]),
                   sample_peak=loudness.to_db(v[4]), true_peak=loudness.to_db(v[5]), momentary=float(v[6]), short_term=float(v[7]))
        return out


class RestoreSession:
    """``VoiceFixer.open_stream``: the overlap-add long-form mode as a push-style session on the device.

        s = vf.open_stream(chunk_seconds=30.0, overlap_seconds=1.0, sample_rate=16000, output_sample_rate=48000)
        y = s.push(block)        # float32 (k,) at sample_rate, any k >= 0 -> float32 numpy (1, j) at the output rate, j >= 0
        y = s.finish()           # the rest; afterwards push / finish raise RuntimeError
        s.position               # output samples delivered so far

    Definition: with X the concatenation of all pushed blocks, X44 its whole-row conversion to 44.1 kHz (``convert_rows``),
    Y44 = ``restore_stream(X44, chunk_seconds, overlap_seconds, batch_size, mode)`` and Z = Y44 converted as a whole row to
    the output rate by ops.resample_rows (Z = Y44 at 44.1 kHz), the results of all ``push`` calls and of ``finish``
    concatenate to Z.  NO second peak rule is applied to a converted output (``convert_output`` applies one to whole
    files): a stretch leaves before the file's peak exists, so a converted stretch may overshoot 1.0 slightly.
    Four stages, all on the device and on the current stream: the input converter (ops.resample_span on the samples that
    future outputs still read; a copy at 44.1 kHz), the chunker (``StreamPlanner``; settled chunks of equal length go
    through the path in groups of up to ``batch_size``), the stitcher (ops.xfade of the previous chunk's last ``overlap``
    samples with the next chunk's head) and the output converter (the input converter again, fed with the final 44.1 kHz
    stretches, which therefore never visit the host).  Held between calls: the 44.1 kHz samples from the next chunk's
    start on, one overlap, two filter windows -- O(chunk + the largest block), whatever has been pushed.  A chunk is
    settled once more than chunk + min_tail samples (1024; mode 1: 1535) beyond its start are known at 44.1 kHz: the
    session's latency.  Loudness normalisation to a TARGET and a trim need the whole file and are not offered here; a FIXED gain (``gain_db``) is, alone or followed by the fixed-gain look-ahead limiter (``limiter=True``;
    loudness.py) under ``peak_ceiling`` at the output rate, carried across stretches like the converters and
    2 H + 93 samples late; ``limiter_stats`` is then {"max_reduction_db", "peak_out_db"} over what has been delivered (None
    without a limiter).  The limiter bounds every sample by the ceiling, the inter-sample peak only approximately: lower
    ``peak_ceiling`` for a margin.  The word-length reduction (``bit_depth``) is offered too: its dither is a function of a
    sample's position, not of the file.  A loudness target without the whole file is the LEVELLER's (``leveller=T`` LUFS,
    ``leveller_max_gain_db``, ``leveller_gate``; loudness.py; ``voicefixer_amd.level`` on the whole output, bit
    for bit): a gain that follows the loudness of the 3 s around every 100 ms anchor, carried across stretches like the
    converters and less than 1.1 s late; with it ``limiter=True`` needs no ``gain_db`` (the limiter then runs at 0 dB) and
    ``leveller_stats`` is {"min_gain_db", "max_gain_db", "anchors", "gated"} (None without a leveller).  The stages behind the
    stitcher, a chain of ``_SpanStage``: output converter, leveller, limiter (or the gain alone); then word length, host.
    ``channels="all"`` (default None: the session above, a 2-D block raises): every block is float32 (C, k), C in
    1..8 fixed by the first block (another C, a 1-D block or more than 8 channels: ValueError before the device is touched), and
    ``push`` / ``finish`` return (C, j); ``position`` counts samples per channel.  Each channel has its own input converter,
    cross-fade and output converter; a settled chunk goes through the path as C adjacent rows of one batch (``batch_size`` keeps
    counting chunks).  The leveller and the limiter are the LINKED ones (ops.level_span_rows: the quarter energies summed over the
    channels with ``channel_weights`` -- loudness.channel_weights(C), BS.1770-4 Table 4 by default; needs channels="all" -- and
    ops.limit_span_rows: one envelope, the maximum over the channels): one gain curve per programme, so the balance between the
    channels stays -- ``level(Z, ..., channels="all")`` and ``limit(..., channels="all")`` of the plain (C, N) output Z, bit for bit,
    with one stats record per programme; the fixed gain alone is float32(gL) y; ``bit_depth`` gives ``quantize`` of the (C, N)
    array (channel c draws the dither of channel c).  ``meter=True``: a loudness meter taps the session's final
    float signal -- behind the output converter, the leveller and the limiter or the gain, ahead of the word-length reduction -- and
    ``loudness_report`` says what was delivered (integrated, momentary, short-term, LRA, sample and true peak), at any time; it
    neither delays nor alters a sample, and holds 8 bytes per 100 ms of the programme (288 KB per hour), the one thing here that grows
    with the session's length, and less than 0.3 s of samples.  With channels="all" the channels weigh ``channel_weights``; "mix" /
    "first" / None meter the mono signal.  Every channel is within 2e-5 rms of the mono session on it, not its bits: the
    path's bits depend on the batch's composition.  "mix" / "first": a (C, k) block is averaged (float32 mean) / cut to channel 0
    on the host and the session is the mono one.  Held: O(C (chunk + the largest block)).
    Every argument is checked in the constructor, before the device is touched.
    A context manager; leaving it without ``finish`` discards what is pending."""

    def __init__(self, vf, chunk_seconds=30.0, overlap_seconds=1.0, batch_size=1, mode=0, your_vocoder_func=None,
                 sample_rate=44100, output_sample_rate=None, bit_depth=None, dither="tpdf", dither_seed=0, gain_db=None,
                 peak_ceiling=-1.0, true_peak=False, limiter=False, limiter_lookahead_ms=3.0, leveller=None,
                 leveller_max_gain_db=12.0, leveller_gate=-50.0, meter=False, channels=None, channel_weights=None):
        from . import loudness as ld
        from .api import _Output, _check_rate, _output_rate
        _check_stream_mode(mode, "open_stream")
        self._channels = ld.check_channels(channels)
        if channel_weights is not None:
            if self._channels != "all":
                raise ValueError('open_stream: channel_weights weigh the channels of a programme and need channels="all"')
            if isinstance(channel_weights, (str, bytes)) or not isinstance(channel_weights, (list, tuple, np.ndarray)) \
                    or not 1 <= len(channel_weights) <= ld.MAX_CHANNELS:
                raise ValueError("channel_weights must be a list of 1..8 numbers >= 0, one per channel (got %r)" % (channel_weights,))
            channel_weights = ld.channel_weights(len(channel_weights), channel_weights)
        self._weights = channel_weights
        self._C = None           # channels="all": the channel count, fixed by the first block
        self._word = _Output(bit_depth=bit_depth, dither=dither, dither_seed=dither_seed)     # (checks the three)
        self._dtype = {None: np.float32, 16: np.int16, 24: np.int32}[self._word.bit_depth]
        self._rate_in, self._rate_out = _check_rate(sample_rate), _output_rate(output_sample_rate)
        gain_db, peak_ceiling, true_peak = ld.check_gain(gain_db), ld.check_ceiling(peak_ceiling), ld.check_true_peak(true_peak)
        limiter, limiter_lookahead_ms = ld.check_limiter(limiter, limiter_lookahead_ms)
        if limiter and gain_db is None and leveller is None:
            raise NotImplementedError("open_stream: the limiter behind a loudness target is not built -- it follows a whole-file "
                                      "measurement; give a fixed gain (gain_db=...) or a leveller (leveller=...) for the "
                                      "session's fixed-gain limiter, or use restore_inmem or restore_folder")
        self._gain = None if gain_db is None else float(np.float32(10.0 ** (gain_db / 20.0)))
        # (check_leveller: ValueError for an output rate above 192 kHz too; nothing touches the device before the first stretch)
        self._lev = (_SpanLeveller(self._rate_out, leveller, leveller_max_gain_db, leveller_gate, weights=channel_weights)
                     if leveller is not None else None)
        # (limiter_reach: ValueError for a look-ahead outside [1, 4096] samples at the output rate; behind a leveller and
        # without a gain the limiter runs at 0 dB)
        self._lim = (_SpanLimiter(self._rate_out, 0.0 if gain_db is None else gain_db, peak_ceiling, true_peak,
                                  limiter_lookahead_ms) if limiter else None)
        for r in (self._rate_in, self._rate_out):
            if r != 44100 and max(audio_io.rate_ratio(r, 44100)) > audio_io.DEVICE_MAX_RATIO:
                raise ValueError("open_stream: the device resampler does not take the ratio of %d Hz to 44100 Hz" % r)
        if isinstance(batch_size, bool) or int(batch_size) != batch_size or batch_size < 1:
            raise ValueError("batch_size must be a positive integer")
        chunk, ov, min_tail = _stream_geometry(chunk_seconds, overlap_seconds, mode)
        self._planner = StreamPlanner(chunk, ov, min_tail)     # (ValueError: chunk <= overlap + 1024)
        self._vf, self._mode, self._voc, self._batch, self._ov = vf, mode, your_vocoder_func, int(batch_size), ov
        self._conv_in = _SpanConverter(self._rate_in, 44100) if self._rate_in != 44100 else None
        conv_out = _SpanConverter(44100, self._rate_out) if self._rate_out != 44100 else None
        self._stages = [s for s in (conv_out, self._lev, self._lim) if s is not None]      # behind the stitcher, in this order
        # (check_meter: ValueError for an output rate above 192 kHz; a tap on what _deliver is about to hand over)
        self._meter = _SpanMeter(self._rate_out, channel_weights) if ld.check_meter(meter) else None
        self._n_in = 0           # samples pushed
        self._buf = None         # device (k,) -- (C, k) with channels="all", here and below: 44.1 kHz samples [b0, b0 + k)
        self._b0 = 0
        self._tail = None        # device (ov,): the previous chunk's stitched last ``ov`` samples
        self._fade = None        # device (ov,): restore_stream's fade-in ramp, uploaded once
        self._closed = False
        self.position = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def close(self):
        """Drop what is pending (nothing more is delivered); ``push`` and ``finish`` raise afterwards."""
        self._closed = True
        self._buf = self._tail = self._fade = self._conv_in = None
        for stage in self._stages + ([self._meter] if self._meter is not None else []):
            stage.release()          # (the records stay: limiter_stats, leveller_stats and loudness_report outlive the session)

    @property
    def limiter_stats(self):
        """{"max_reduction_db": -20 log10(min g), "peak_out_db": 20 log10(max |out|)} over what has been delivered -- exact folds,
        the values of one call over the whole row -- or None without a limiter."""
        return None if self._lim is None else self._lim.stats()

    @property
    def leveller_stats(self):
        """{"min_gain_db", "max_gain_db", "anchors", "gated"} of the leveller over what has been delivered -- exact folds, the
        values of ``level`` over the whole output -- or None without a leveller."""
        return None if self._lev is None else self._lev.stats()

    @property
    def loudness_report(self):
        """What the session has delivered, in EBU R 128 terms (``meter=True``; None without a meter): the dict of
        ``voicefixer_amd.loudness_report`` -- ``integrated``, ``loudness_range``, ``max_momentary``, ``max_short_term``,
        ``sample_peak``, ``true_peak`` -- plus the live ``momentary`` and ``short_term`` (the last 400 ms / 3 s) and ``seconds``,
        over the FLOAT signal ahead of the word-length reduction.  Readable at any time (one synchronisation): before ``finish``
        the figures of loudness.meter_reference(..., final=False) -- the true peak is 93 samples late --, after it the final ones;
        still readable after ``close``.  VfxError if the meter's spans did not come in order."""
        return None if self._meter is None else self._meter.report()

    @torch.no_grad()
    def push(self, block):
        """The next ``block`` (float32 (k,), k >= 0, at the session's input rate) -> the output that became final with it:
        float32 numpy (1, j) at the output rate, j >= 0.  With channels="all": (C, k) -> (C, j), C in 1..8 the same for every
        block; with "mix" / "first" a (C, k) block is averaged / cut to channel 0 first."""
        if self._closed:
            raise RuntimeError("RestoreSession: push after finish / close")
        block = self._as_block(np.asarray(block, dtype=np.float32))
        if block.shape[-1] == 0:
            return np.zeros((self._C or 1, 0), self._dtype)
        pipe = self._vf._get_pipe()
        x = torch.from_numpy(np.ascontiguousarray(block)).to(pipe.device)
        self._n_in += block.shape[-1]
        if self._conv_in is not None:
            x = self._conv_in.feed(x)
        self._buf = x if self._buf is None else torch.cat([self._buf, x], dim=-1)
        return self._deliver(pipe, self._restore(pipe, self._planner.feed(x.shape[-1]), False), False)

    def _as_block(self, block):
        """A pushed array under the session's ``channels``: (k,) for the mono session, (C, k) with "all" (ValueError otherwise,
        before the device is touched)."""
        from . import loudness as ld
        if self._channels == "all":
            if block.ndim != 2:
                raise ValueError('push: with channels="all" a block is a (channels, k) array (got shape %r)' % (block.shape,))
            C = ld.check_channel_count(int(block.shape[0]))
            if self._C is None:
                if self._weights is not None:
                    ld.channel_weights(C, self._weights)         # (ValueError: another number of weights)
                self._C = C
            elif C != self._C:
                raise ValueError("push: this session has %d channels (got a block of shape %r)" % (self._C, block.shape))
            return block
        if self._channels is not None and block.ndim == 2:
            ld.check_channel_count(int(block.shape[0]))
            return block.mean(axis=0, dtype=np.float32) if self._channels == "mix" else block[0]
        if block.ndim != 1:
            raise ValueError("push: a block is a 1-D array of samples (got shape %r)" % (block.shape,))
        return block

    @torch.no_grad()
    def finish(self):
        """The rest of the output, float32 numpy (1, j); the session is closed afterwards.  ValueError, nothing launched,
        when fewer 44.1 kHz samples than ``VoiceFixer.MIN_SAMPLES[mode]`` were pushed."""
        if self._closed:
            raise RuntimeError("RestoreSession: finish called twice (or after close)")
        from .api import VoiceFixer
        try:
            n44 = audio_io.converted_length(self._n_in, self._rate_in, 44100)
            if n44 < VoiceFixer.MIN_SAMPLES[self._mode]:
                raise ValueError("RestoreSession: %d samples at 44.1 kHz were pushed, mode %d needs at least %d"
                                 % (n44, self._mode, VoiceFixer.MIN_SAMPLES[self._mode]))
            pipe = self._vf._get_pipe()
            n_new = 0
            if self._conv_in is not None:
                x = self._conv_in.finish(pipe.device)
                self._buf = torch.cat([self._buf, x], dim=-1)
                n_new = x.shape[-1]
            plan = self._planner.feed(n_new) + self._planner.finish()
            return self._deliver(pipe, self._restore(pipe, plan, True), True)
        finally:
            self.close()

    def _restore(self, pipe, plan, at_end):
        """The settled chunks ``plan`` through the path and the stitcher; returns their final 44.1 kHz stretches (device)."""
        from . import ops
        from .api import VoiceFixer
        ov, out, i, C = self._ov, [], 0, self._C
        while i < len(plan):
            length = plan[i][1]
            grp = [c for c in plan[i:i + self._batch] if c[1] == length]
            if C is None:
                seg = torch.stack([self._buf[a - self._b0:a - self._b0 + length] for a, _ in grp])
            else:                       # a chunk of C channels: C adjacent rows of the batch
                seg = torch.cat([self._buf[:, a - self._b0:a - self._b0 + length] for a, _ in grp])
            res = pipe.run_checked(lambda: VoiceFixer._restore_segments(pipe, seg, length, self._mode, self._voc))
            got = res.shape[1]          # == length in mode 0; 512 * (length // 512) in mode 1
            for k, (a, _) in enumerate(grp):
                y = res[k] if C is None else res[k * C:(k + 1) * C]
                if a > 0 and ov > 0:    # cross-fade with what the previous chunk left in the overlap, in place
                    if C is None:
                        ops.xfade(self._tail, y[:ov], self._fade, y[:ov])
                    else:
                        for c in range(C):
                            ops.xfade(self._tail[c], y[c, :ov], self._fade, y[c, :ov])
                last = at_end and i + k == len(plan) - 1
                if last:
                    out.append(y)
                else:
                    out.append(y[..., :got - ov])
                    if ov > 0:
                        if self._fade is None:
                            self._fade = torch.from_numpy(np.arange(ov, dtype=np.float32) / max(ov, 1)).to(pipe.device)
                        self._tail = y[..., got - ov:].clone()
            i += len(grp)
        # the next chunk starts at the planner's start: nothing before it is read again
        if not at_end and self._planner.start > self._b0:
            self._buf = self._buf[..., self._planner.start - self._b0:].clone()
            self._b0 = self._planner.start
        return out

    def _deliver(self, pipe, stretches, at_end):
        """Final 44.1 kHz stretches -> the host, through the session's stages, the fixed gain when there is one and no limiter
        and, with a ``bit_depth``, the word-length reduction: sample k of what is delivered has the absolute index position + k."""
        for stage in self._stages:
            stretches = [stage.feed(y) for y in stretches if y.numel()]
            if at_end:
                stretches.append(stage.finish(pipe.device))
        if self._gain is not None and self._lim is None:
            stretches = [y * self._gain for y in stretches]      # (float32(gL) y: one rounding per sample)
        if not stretches:
            if at_end and self._meter is not None:
                self._meter.finish()
            return np.zeros((self._C or 1, 0), self._dtype)
        y = stretches[0] if len(stretches) == 1 else torch.cat(stretches, dim=-1)
        if self._meter is not None:                          # (a tap: y goes on as it is)
            if y.shape[-1] > 0:
                self._meter.feed(y)
            if at_end:
                self._meter.finish()
        if self._C is None:
            y = y[None]
        if self._word.bit_depth is not None and y.shape[1] > 0:     # (a row's channel is its index: quantize of the (C, N) array)
            y, _ = self._word.quantize(y.contiguous(), [y.shape[1]] * y.shape[0], None if self._C is None else [self._C],
                                       self.position)
        y = y.cpu().numpy().astype(self._dtype, copy=False)
        self.position += y.shape[1]
        return y


class LoudnessMeter:
    """The streaming loudness meter of a session (``open_stream(meter=True)``; loudness.py) for any audio, with no
    VoiceFixer: EBU R 128 figures of a signal that arrives in blocks, on the device, without keeping it.

        m = LoudnessMeter(sample_rate=48000)
        m.push(block)            # float32 (k,), any k >= 0
        m.report()               # the dict below over what has been pushed, at any time; the true peak is 93 samples late
        m.finish()               # the final dict; afterwards push raises RuntimeError, report keeps answering

    The dict: ``integrated`` (LUFS), ``loudness_range`` (LU), ``max_momentary``, ``max_short_term`` (LUFS), ``sample_peak`` (dBFS),
    ``true_peak`` (dBTP) -- the keys and, within the bounds of DESIGN.md 3.10 / 3.11, the values of ``loudness_report`` on the
    concatenation, the true peak bit for bit -- plus ``momentary`` and ``short_term`` (the last 400 ms / 3 s; -inf with less) and
    ``seconds``.  The figures do not depend on the block sizes, in any bit.  ``channels``: None -- blocks are (k,) -- or "all":
    blocks are (C, k), C in 1..8 fixed by the first block, ONE programme weighted by ``channel_weights`` (default
    loudness.channel_weights(C), BS.1770-4 Table 4; needs channels="all"); "mix" / "first": a (C, k) block is averaged / cut to
    channel 0 on the host, as a session does, and metered as one channel.  ``sample_rate``: 4 kHz to 192 kHz (ValueError).  Held:
    less than 0.3 s of samples beyond a block and 8 bytes per 100 ms pushed.  Every argument is checked in the constructor, before
    the device is touched.  A context manager."""

    def __init__(self, sample_rate=44100, channels=None, channel_weights=None):
        from . import loudness as ld
        ld.check_meter(True, sample_rate)
        self._channels = ld.check_channels(channels)
        if channel_weights is not None:
            if self._channels != "all":
                raise ValueError('LoudnessMeter: channel_weights weigh the channels of a programme and need channels="all"')
            if isinstance(channel_weights, (str, bytes)) or not isinstance(channel_weights, (list, tuple, np.ndarray)) \
                    or not 1 <= len(channel_weights) <= ld.MAX_CHANNELS:
                raise ValueError("channel_weights must be a list of 1..8 numbers >= 0, one per channel (got %r)" % (channel_weights,))
            channel_weights = ld.channel_weights(len(channel_weights), channel_weights)
        self._weights = channel_weights
        self._C = None
        self._tap = _SpanMeter(int(sample_rate), channel_weights)
        self._closed = False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def close(self):
        """Drop the samples held; ``push`` and ``finish`` raise afterwards, ``report`` keeps answering."""
        self._closed = True
        self._tap.release()

    @torch.no_grad()
    def push(self, block):
        """Meter the next ``block``: float32 (k,), k >= 0 -- (C, k) with channels="all"; returns nothing."""
        if self._closed:
            raise RuntimeError("LoudnessMeter: push after finish / close")
        from .api import _device
        block = RestoreSession._as_block(self, np.asarray(block, dtype=np.float32))
        if block.shape[-1]:
            self._tap.feed(torch.from_numpy(np.ascontiguousarray(block)).to(_device()))

    def report(self):
        """The dict over what has been pushed so far (one synchronisation); before ``finish`` the true peak covers the samples
        whose interpolated values are complete (loudness.meter_reference(..., final=False))."""
        return self._tap.report()

    @torch.no_grad()
    def finish(self):
        """The final dict: the end of the signal is known; the meter is closed afterwards."""
        if self._closed:
            raise RuntimeError("LoudnessMeter: finish called twice (or after close)")
        self._tap.finish()
        self.close()
        return self._tap.report()
