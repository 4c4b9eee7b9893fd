"""Drop-in Python surface of the reference for the restore / vocoder path.

    from voicefixer_amd import VoiceFixer, Vocoder          # == from voicefixer import ...

``VoiceFixer`` mirrors voicefixer/base.py:10-146 and ``Vocoder`` mirrors
voicefixer/vocoder/base.py:10-77: same constructor behaviour (checkpoint locations and the
"Error 0"/"Error 1" RuntimeErrors), same method names, argument meaning and return types, the
``your_vocoder_func`` plugin hook (base.py:126-129) and the 30 s hard-cut segmentation
(base.py:117-137).  Everything between the waveform going in and the waveform coming out runs
in libvfx_hip on the MI355X; there is NO CPU implementation behind this API:

  * ``cuda=True``  -> tensors returned on the HIP device where the reference would return CUDA tensors;
  * ``cuda=False`` -> same kernels, results copied back to host tensors (the reference would
    compute on the CPU; numerically equivalent within the parity tolerance).  Without a visible
    device either setting raises -- nothing silently falls back.
  * ``mode=0`` and ``mode=1`` (``remove_higher_frequency`` pre-filter, base.py:87-104, run on the
    device by ``vfx_hf_cut_f32``).  ``mode=2`` (train-mode BatchNorm/Dropout, base.py:114-115) needs
    ``seed=``: its dropout masks are then a documented function of the seed (dropout.py), so mode 2 is
    reproducible; without a seed it raises NotImplementedError, as the unseeded form is not built.
"""
import os

import numpy as np
import torch
import torch.nn as nn

from . import audio_io, engine, weights
from ._lib import VfxError
# the overlap-add streaming mode lives in stream.py; its names stay reachable here
from .stream import (LEVEL_SPAN, LIMIT_SPAN, LoudnessMeter, RestoreSession, StreamPlanner, _SpanConverter,  # noqa: F401
                     _SpanLeveller, _SpanLimiter, _SpanMeter, _check_stream_mode, _stream_geometry, plan_stream_chunks)

SEG_LENGTH = 44100 * 30  # voicefixer/base.py:117

ANALYSIS_CKPT = ".cache/voicefixer/analysis_module/checkpoints/vf.ckpt"
VOCODER_CKPT = ".cache/voicefixer/synthesis_module/44100/model.ckpt-1490000_trimed.pt"


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("Error: no HIP device found; voicefixer_amd has no CPU fallback "
                           "(the reference raises 'You set cuda=True but no cuda device found.' here)")
    return torch.device("cuda", torch.cuda.current_device())


def _load_vocoder_state(path):
    ckpt = torch.load(path, map_location="cpu")
    return ckpt["generator"]  # voicefixer/vocoder/base.py:26-27


def _load_restorer_state(path):
    """vf.ckpt is a flat state dict of restorer.model.VoiceFixer; the engine needs the
    ``generator.*`` (denoiser + unet) entries (voicefixer/base.py:23-29 key filter)."""
    sd = torch.load(path, map_location="cpu")
    if "state_dict" in sd and not any(k.startswith("generator.") for k in sd):
        sd = sd["state_dict"]
    out = {k[len("generator."):]: v for k, v in sd.items() if k.startswith("generator.")}
    voc = {k[len("vocoder.model."):]: v for k, v in sd.items() if k.startswith("vocoder.model.")}
    return out, (voc or None)  # vf.ckpt may overwrite the vocoder weights


def plan_batches(sorted_lengths, batch_size, ragged_ratio=0.5, ragged=True, rows=None):
    """Cut a list of ASCENDING sample counts into batches: ("ragged", [positions]) for runs of utterances of
    1025..SEG_LENGTH samples whose shortest member has >= ragged_ratio of the frames (1 + n // 441) of the longest
    (Pipeline.restore_rows), ("samples", [positions]) for runs of exactly equal length otherwise (files of several
    segments, plugin vocoders, too-short files -- the last raise in the pipeline as the reference does).
    ``rows`` (multichannel files): how many batch rows every item takes -- its channel count; a batch then holds at most
    ``batch_size`` ROWS and never splits an item (ValueError when an item alone has more rows than ``batch_size``)."""
    if rows is not None:
        if len(rows) != len(sorted_lengths):
            raise ValueError("plan_batches: %d row counts for %d items" % (len(rows), len(sorted_lengths)))
        if rows and max(rows) > batch_size:
            raise ValueError("batch_size (%d) is smaller than the largest channel count (%d): the channels of a file share "
                             "one batch" % (batch_size, max(rows)))
    plan = []
    i, n_items = 0, len(sorted_lengths)
    while i < n_items:
        n0 = sorted_lengths[i]
        j = i + 1
        used = 1 if rows is None else rows[i]
        if ragged and 1025 <= n0 <= SEG_LENGTH:
            t0 = 1 + n0 // 441
            while (j < n_items and used + (1 if rows is None else rows[j]) <= batch_size and sorted_lengths[j] <= SEG_LENGTH and
                   t0 >= ragged_ratio * (1 + sorted_lengths[j] // 441)):
                used += 1 if rows is None else rows[j]
                j += 1
            plan.append(("ragged", list(range(i, j))))
        else:
            while j < n_items and used + (1 if rows is None else rows[j]) <= batch_size and sorted_lengths[j] == n0:
                used += 1 if rows is None else rows[j]
                j += 1
            plan.append(("samples", list(range(i, j))))
        i = j
    return plan


def _check_rate(rate, what="sample_rate"):
    if isinstance(rate, bool) or int(rate) != rate or int(rate) <= 0:
        raise ValueError("%s must be a positive integer number of samples per second (got %r)" % (what, rate))
    return int(rate)


def _output_rate(output_sample_rate):
    """None (the default: 44.1 kHz, nothing converted) or a positive rate."""
    return 44100 if output_sample_rate is None else _check_rate(output_sample_rate, "output_sample_rate")


def _row_rates(sample_rate, n):
    """One input rate per row from an int or a list."""
    if isinstance(sample_rate, (list, tuple, np.ndarray)):
        if len(sample_rate) != n:
            raise ValueError("sample_rate: %d rates for %d rows" % (len(sample_rate), n))
        return [_check_rate(r) for r in sample_rate]
    return [_check_rate(sample_rate)] * n


def convert_rows(seg, lens, rates, rate_out=44100):
    """Rate conversion of device rows on the device (ops.resample_rows): row r of ``seg`` (B, >= max lens) holds lens[r]
    samples at rates[r]; returns (B, max ny) rows at ``rate_out`` and their lengths ny = ceil(lens * up / down)
    (audio_io.converted_length).  ONE launch per distinct rate pair (its rows listed by index); rows already at
    ``rate_out`` are copied.  Nothing is converted, and ``seg`` itself is returned, when every row is at ``rate_out``."""
    from . import ops
    lens, rates = [int(n) for n in lens], [int(r) for r in rates]
    if all(r == rate_out for r in rates):
        return seg, lens
    if max(lens) > seg.shape[1] or seg.stride(-1) != 1:
        raise ValueError("convert_rows: rows of %d samples in a buffer of width %d" % (max(lens), seg.shape[1]))
    B, dev = seg.shape[0], seg.device
    new = [audio_io.converted_length(n, r, rate_out) for n, r in zip(lens, rates)]
    y = torch.empty((B, max(max(new), 1)), dtype=torch.float32, device=dev)
    n_rows = torch.tensor(lens, dtype=torch.int32).to(dev, non_blocking=True)
    for sr in sorted(set(rates)):
        rows = [r for r in range(B) if rates[r] == sr]
        if sr == rate_out:
            for r in rows:
                y[r, :lens[r]] = seg[r, :lens[r]]
            continue
        up, down = audio_io.rate_ratio(sr, rate_out)
        idx = None if len(rows) == B else torch.tensor(rows, dtype=torch.int32).to(dev, non_blocking=True)
        ops.resample_rows(seg, n_rows, y, up, down, row_index=idx)
    return y, new


def convert_output(full, lens, rate_out):
    """Restored 44.1 kHz device rows -> ``rate_out`` on the device, then the reference's peak rule once more on every
    converted row (base.py:131-133: a row whose peak exceeds 1 is divided by its peak -- band-limited conversion of a
    peak-normalised row can overshoot, and audio_io.to_int16 would then skip its 2^15 scaling).  Returns (rows, lengths)."""
    from . import ops
    if rate_out == 44100:
        return full, list(lens)
    y, new = convert_rows(full if full.stride(-1) == 1 else full.contiguous(), lens, [44100] * len(lens), rate_out)
    B, dev = y.shape[0], y.device
    out = torch.empty_like(y)
    ny_rows = torch.tensor(new, dtype=torch.int32).to(dev, non_blocking=True)
    peak_ws = torch.empty((B,), dtype=torch.int32, device=dev)
    ops.post_rows(y, y.shape[1], out, ny_rows, max(new), peak_ws, ly_rows=ny_rows)
    return out, new


def apply_loudness(full, lens, rate, target, peak_ceiling=-1.0, true_peak=False):
    """Loudness normalisation of device rows (ops.loudness_rows, BS.1770-4 integrated loudness): row r of ``full`` holds
    lens[r] samples at ``rate``; each is scaled by float32(g), g = min(10^((target - L)/20), 10^(peak_ceiling/20) / peak)
    (a SAMPLE-peak ceiling; g = 1 when L = -inf: silence or under 400 ms).  Returns (rows, device float64 (B, 3) of
    {L before, g, peak}); ``target`` None returns (full, None) and launches nothing.
    ``true_peak=True``: ``peak_ceiling`` is read as dBTP -- the gain is limited by the TRUE peak (loudness.py) -- and the
    result is (B, 4) of {L before, g, sample peak, true peak}."""
    from . import loudness, ops
    target, peak_ceiling = loudness.check_target(target), loudness.check_ceiling(peak_ceiling)
    true_peak = loudness.check_true_peak(true_peak)
    if target is None:
        return full, None
    x = full if full.stride(-1) == 1 else full.contiguous()
    n_rows = torch.tensor([int(n) for n in lens], dtype=torch.int32).to(x.device, non_blocking=True)
    out = torch.empty_like(x)
    if true_peak:
        res = ops.loudness_rows(x, n_rows, rate, target, peak_ceiling, out=out, true_peak=True)
    else:
        res = ops.loudness_rows(x, n_rows, rate, target, peak_ceiling, out=out)
    return out, res


def apply_loudness_groups(full, lens, groups, rate, target, peak_ceiling=-1.0, true_peak=False, channel_weights=None):
    """``apply_loudness`` for PROGRAMMES of several channels (ops.loudness_groups; loudness.py): the rows of ``full`` are
    ``groups`` = [C_0, C_1, ...] adjacent channels per programme, all rows of one programme lens[r] samples long; ONE
    loudness, one peak and one float32 gain per programme, so the balance between its channels is kept.  Returns (rows,
    device float64 (G, 4) of {L before, g, sample peak, true peak}); without ``true_peak`` the ceiling is a sample-peak one
    and the fourth value repeats the sample peak.  ``channel_weights``: one list for every programme (all of one channel
    count then), default loudness.channel_weights."""
    from . import loudness, ops
    target, peak_ceiling = loudness.check_target(target), loudness.check_ceiling(peak_ceiling)
    true_peak = loudness.check_true_peak(true_peak)
    if target is None:
        return full, None
    weights = None if channel_weights is None else [w for g in groups for w in loudness.channel_weights(g, channel_weights)]
    x = full if full.stride(-1) == 1 else full.contiguous()
    out = torch.empty_like(x)
    res = ops.loudness_groups(x, [int(n) for n in lens], groups, rate, target, peak_ceiling, out=out, weights=weights,
                              true_peak=true_peak)
    return out, res


def apply_limiter(full, lens, rate, target, peak_ceiling=-1.0, true_peak=False, lookahead_ms=3.0, groups=None,
                  channel_weights=None):
    """``apply_loudness`` / ``apply_loudness_groups`` with the look-ahead peak limiter in place of the static ceiling
    (ops.loudness_limit; loudness.py): rows that the target would push past the ceiling get a gain curve that looks
    ``lookahead_ms`` ahead, one curve per programme of ``groups`` adjacent channels.  Returns (rows, device float64 (G or B, 8)
    of {L before, gL, sample peak, true peak, bound, min g, trim, peak after})."""
    from . import loudness, ops
    target, peak_ceiling = loudness.check_target(target), loudness.check_ceiling(peak_ceiling)
    true_peak = loudness.check_true_peak(true_peak)
    if target is None:
        raise ValueError("limiter=True needs a loudness target")
    loudness.limiter_window(rate, lookahead_ms)
    x = full if full.stride(-1) == 1 else full.contiguous()
    out = torch.empty_like(x)
    if groups is not None:
        weights = None if channel_weights is None else [w for g in groups for w in loudness.channel_weights(g, channel_weights)]
        res = ops.loudness_limit(x, [int(n) for n in lens], rate, target, peak_ceiling, true_peak, lookahead_ms, out=out,
                                 groups=groups, weights=weights)
    else:
        n_rows = torch.tensor([int(n) for n in lens], dtype=torch.int32).to(x.device, non_blocking=True)
        res = ops.loudness_limit(x, n_rows, rate, target, peak_ceiling, true_peak, lookahead_ms, out=out)
    return out, res


def _check_limiter(limiter, lookahead_ms):
    from . import loudness
    return loudness.check_limiter(limiter, lookahead_ms)[0]


def _check_channels(channels):
    from . import loudness
    return loudness.check_channels(channels)


class _Output:
    """What happens to restored rows before they leave the device: the output rate, the loudness target with its ceiling
    and channel weights, mode 2's seed, and the word length they leave at.  Built ONCE per public call from its keywords -- the
    checks are made here, before anything touches the device -- and handed down as it is.  ``kwargs()`` is the one place that
    knows which keywords a ``restore_batches`` call is given, ``finish()`` the one tail of the float device stage and
    ``quantize()``, after it, the reduction to ``bit_depth``-bit PCM (None, the default: float32 rows leave, as ever)."""
    __slots__ = ("rate_out", "loudness", "peak_ceiling", "true_peak", "channel_weights", "seed", "limiter",
                 "limiter_lookahead_ms", "bit_depth", "dither", "dither_seed")

    def __init__(self, output_sample_rate=None, loudness=None, peak_ceiling=-1.0, true_peak=False, channel_weights=None,
                 mode=0, seed=None, limiter=False, limiter_lookahead_ms=3.0, bit_depth=None, dither="tpdf", dither_seed=0):
        from . import dropout, loudness as ld, wordlength
        self.bit_depth = wordlength.check_bit_depth(bit_depth, allow_none=True)
        self.dither, self.dither_seed = wordlength.check_dither(dither), dropout.check_seed(dither_seed)
        self.rate_out = _output_rate(output_sample_rate)
        self.true_peak = ld.check_true_peak(true_peak)
        self.loudness, self.peak_ceiling = ld.check_target(loudness), ld.check_ceiling(peak_ceiling)
        self.limiter, self.limiter_lookahead_ms = ld.check_limiter(limiter, limiter_lookahead_ms)
        if self.limiter:
            if self.loudness is None:
                raise ValueError("limiter=True needs a loudness target (loudness=...)")
            ld.limiter_window(self.rate_out, self.limiter_lookahead_ms)
        if channel_weights is not None:
            if isinstance(channel_weights, (str, bytes)) or not isinstance(channel_weights, (list, tuple, np.ndarray)) \
                    or not 1 <= len(channel_weights) <= ld.MAX_CHANNELS:
                raise ValueError("channel_weights must be a list of 1..8 numbers >= 0, one per channel (got %r)" % (channel_weights,))
            ld.channel_weights(len(channel_weights), channel_weights)
        self.channel_weights = channel_weights
        self.seed = seed if mode == 2 else None     # (modes 0 and 1 ignore a seed: VoiceFixer._check_mode)

    def check_channel_counts(self, counts):
        """``channel_weights`` is one list for every file of the call: each must have that many channels."""
        if self.channel_weights is not None and any(c != len(self.channel_weights) for c in counts):
            raise ValueError("channel_weights: %d weights, but the input has %r channel(s)"
                             % (len(self.channel_weights), sorted(set(counts))))

    def kwargs(self):
        """The keywords that differ from ``restore_batches``' defaults and nothing else: a default job forwards none (a
        stand-in for the device stage takes ``(batches, your_vocoder_func, streams, mode)`` only)."""
        kw = {} if self.seed is None else {"seed": self.seed}
        if self.rate_out != 44100:
            kw["output_sample_rate"] = self.rate_out
        if self.loudness is not None:
            kw.update(loudness=self.loudness, peak_ceiling=self.peak_ceiling)
            if self.true_peak:
                kw.update(true_peak=True)
            if self.channel_weights is not None:
                kw["channel_weights"] = self.channel_weights
            if self.limiter:
                kw.update(limiter=True, limiter_lookahead_ms=self.limiter_lookahead_ms)
        if self.bit_depth is not None:
            kw.update(bit_depth=self.bit_depth, dither=self.dither, dither_seed=self.dither_seed)
        return kw

    def finish(self, full, lens, groups=None):
        """Restored 44.1 kHz device rows -> (rows, lengths, loudness results or None): ``convert_output`` when the rate differs,
        then, with a target, ONE linked gain per file of ``groups`` adjacent channels (``apply_loudness_groups``) or, without
        ``groups``, one gain per row (``apply_loudness``)."""
        if self.rate_out != 44100:
            full, lens = convert_output(full, lens, self.rate_out)
        res = None
        if self.limiter:
            full, res = apply_limiter(full, lens, self.rate_out, self.loudness, self.peak_ceiling, self.true_peak,
                                      self.limiter_lookahead_ms, groups, self.channel_weights)
        elif self.loudness is not None and groups is not None:
            full, res = apply_loudness_groups(full, lens, groups, self.rate_out, self.loudness, self.peak_ceiling,
                                              self.true_peak, self.channel_weights)
        elif self.loudness is not None:
            full, res = apply_loudness(full, lens, self.rate_out, self.loudness, self.peak_ceiling, self.true_peak)
        return full, lens, res

    def quantize(self, full, lens, groups=None, n0=None):
        """The rows ``finish()`` returned -> (PCM rows, device int32 (B, 2) of {clipped samples, max |q|}): int16 rows at
        ``bit_depth`` 16, int32 rows at 24, quantised on the device with the job's dither (ops.quantize_rows; wordlength.py).  A
        row's channel is its index within its file of ``groups`` adjacent rows (0 without groups); ``n0`` (one int, or one per
        row; default 0) is the absolute index of the rows' first sample in their file -- a streaming session passes its position."""
        from . import ops, wordlength
        if self.bit_depth is None:
            raise ValueError("_Output.quantize: the job has no bit_depth")
        x = full if full.stride(-1) == 1 else full.contiguous()
        B, dev = x.shape[0], x.device
        if len(lens) != B:
            raise ValueError("_Output.quantize: %d lengths for %d rows" % (len(lens), B))
        n_rows = torch.tensor([int(n) for n in lens], dtype=torch.int32).to(dev, non_blocking=True)
        chan = None
        if groups is not None:
            chans = [c for g in groups for c in range(int(g))]
            if len(chans) != B or max(chans, default=0) >= wordlength.MAX_CHANNELS:
                raise ValueError("_Output.quantize: groups %r do not describe %d rows of 1..8 channels" % (list(groups), B))
            if any(chans):
                chan = torch.tensor(chans, dtype=torch.int32).to(dev, non_blocking=True)
        start = None
        if n0 is not None:
            first = [wordlength.check_position(n0)] * B if isinstance(n0, (int, np.integer)) else \
                [wordlength.check_position(v) for v in n0]
            if len(first) != B:
                raise ValueError("_Output.quantize: %d positions for %d rows" % (len(first), B))
            if any(first):
                start = torch.tensor(first, dtype=torch.int64).to(dev, non_blocking=True)
        return ops.quantize_rows(x, n_rows, self.bit_depth, self.dither, self.dither_seed, start, chan)


class _Batch:
    """One item of ``restore_batches``: ``tag`` one entry per FILE, ``host`` the staging rows, ``lens`` / ``rates`` per ROW
    (``rates`` None: 44.1 kHz), ``groups`` the channel count of every file (None: one row each).  The tuple of 4, 5 or 6
    fields stays what callers and stand-ins see (``parse`` / ``as_item``); the code in between works on this."""
    __slots__ = ("tag", "kind", "host", "lens", "rates", "groups")

    def __init__(self, tag, kind, host, lens, rates=None, groups=None):
        self.tag, self.kind, self.host, self.lens, self.rates, self.groups = tag, kind, host, lens, rates, groups

    @classmethod
    def parse(cls, item):
        """A checked record from a tuple as ``restore_batches`` documents it."""
        if len(item) not in (4, 5, 6):
            raise ValueError("restore_batches: item must be (tag, kind, host, lens) or (tag, kind, host, lens, rates) or "
                             "(tag, kind, host, lens, rates or None, groups)")
        b = cls(*item)
        b.lens = lens = list(b.lens)
        b.rates = rates = None if b.rates is None else _row_rates(b.rates, len(lens))
        if b.groups is not None:
            b.groups = groups = [int(g) for g in b.groups]
            starts = b.starts()
            if min(groups, default=0) < 1 or max(groups) > 8 or starts[-1] != len(lens) or \
                    any(len(set(lens[a:z])) != 1 for a, z in zip(starts[:-1], starts[1:])) or \
                    (rates is not None and any(len(set(rates[a:z])) != 1 for a, z in zip(starts[:-1], starts[1:]))):
                raise ValueError("restore_batches: groups must be one channel count (1..8) per tag, summing to the rows, the "
                                 "rows of a file adjacent, of one length and one rate")
        if b.kind not in ("ragged", "samples") or len(lens) != b.host.shape[0] or max(lens) > b.host.shape[1]:
            raise ValueError("restore_batches: item must be (tag, 'ragged' | 'samples', host (B, >= max(lens)), lens (B))")
        return b

    def starts(self):
        """File r has the rows starts()[r] .. starts()[r + 1]."""
        if self.groups is None:
            return list(range(len(self.tag) + 1))
        return np.concatenate([[0], np.cumsum(self.groups)]).tolist()

    def as_item(self):
        """The shortest tuple that carries the content."""
        item = (self.tag, self.kind, self.host, self.lens)
        if self.groups is not None:
            return item + (self.rates, self.groups)
        return item if self.rates is None else item + (self.rates,)

    def files(self):
        """One single-file batch per tag: that file's rows of ``host``, cut to its own length."""
        starts = self.starts()
        for r, (a, z) in enumerate(zip(starts[:-1], starts[1:])):
            a, z = int(a), int(z)
            yield _Batch(self.tag[r:r + 1], self.kind, self.host[a:z, :max(int(self.lens[a]), 1)], list(self.lens[a:z]),
                         None if self.rates is None else list(self.rates[a:z]), None if self.groups is None else [z - a])


def _as_programme(x, channels, what):
    """A waveform argument under ``channels``: -> (float32 (C, N), multi).  None: a 1-D array as it is (a 2-D one raises: it
    used to be misread); "mix" / "first": a 2-D array is averaged / cut to channel 0; "all": every channel."""
    from . import loudness
    x = np.asarray(x, dtype=np.float32)
    if x.ndim == 2 and channels is None:
        raise ValueError('%s: a 2-D array of shape %r needs channels= -- channels="all" restores every channel of a '
                         '(channels, N) array, "mix" / "first" take their average / the first' % (what, x.shape))
    if x.ndim not in (1, 2):
        raise ValueError("%s: a waveform is (N,) or (channels, N) (got shape %r)" % (what, x.shape))
    if x.ndim == 2:
        loudness.check_channel_count(x.shape[0])
        if channels == "mix":
            x = x.mean(axis=0, dtype=np.float32)
        elif channels == "first":
            x = x[0]
    if channels == "all":
        return (x[None] if x.ndim == 1 else x), True
    return x[None], False


def _stage_programmes(wav, channel_weights):
    """One array or a list mixing (N,) and (C, N) arrays -> None when every array is 1-D and no weights are given (the
    per-row path measures them), else (single, padded device rows, row lengths, channel counts, row weights or None)."""
    from . import loudness
    single = not isinstance(wav, (list, tuple))
    items = [np.asarray(w, dtype=np.float32) for w in ([wav] if single else wav)]
    if channel_weights is None and all(w.ndim != 2 for w in items):
        return None
    for w in items:
        if w.ndim not in (1, 2):
            raise ValueError("a waveform is (N,) or (channels, N) (got shape %r)" % (w.shape,))
    items = [w[None] if w.ndim == 1 else w for w in items]
    groups = [loudness.check_channel_count(w.shape[0]) for w in items]
    weights = None if channel_weights is None else [v for g in groups for v in loudness.channel_weights(g, channel_weights)]
    if not items:
        return single, None, [], [], weights
    lens = [w.shape[1] for w in items for _ in range(w.shape[0])]
    host = np.zeros((len(lens), max(max(lens), 1)), np.float32)
    r = 0
    for w in items:
        host[r:r + w.shape[0], :w.shape[1]] = w
        r += w.shape[0]
    return single, torch.from_numpy(host).to(_device()), lens, groups, weights


def _stage_rows(wav):
    """One array or a list of them -> (single, padded device rows (B, >= 1), device int32 lengths, lengths)."""
    single = not isinstance(wav, (list, tuple))
    wavs = [np.asarray(w, dtype=np.float32).reshape(-1) for w in ([wav] if single else wav)]
    if not wavs:
        return single, None, None, []
    dev = _device()
    lens = [len(w) for w in wavs]
    host = np.zeros((len(wavs), max(max(lens), 1)), np.float32)
    for r, w in enumerate(wavs):
        host[r, :len(w)] = w
    return single, torch.from_numpy(host).to(dev), torch.tensor(lens, dtype=torch.int32).to(dev), lens


def _measure(wav, sample_rate, channel_weights, rows, groups, pick):
    """The staging and dispatch the three measurements share: ``groups(x, lens, counts, weights)`` when an input is 2-D or
    weights are given (every array one programme), else ``rows(x, n_rows)`` (every array one row); ``pick`` turns a line of
    the float64 result into what the caller returns for that array."""
    from . import loudness
    loudness.plan(sample_rate)
    prog = _stage_programmes(wav, channel_weights)
    if prog is not None:
        single, x, lens, counts, weights = prog
        res = groups(x, lens, counts, weights) if counts else None
    else:
        single, x, n_rows, lens = _stage_rows(wav)
        res = rows(x, n_rows) if lens else None
    if res is None:
        return []
    out = [pick(v) for v in res.cpu().numpy()]
    return out[0] if single else out


def measure_true_peak(wav, sample_rate=44100, channel_weights=None):
    """True peak in dBTP (after ITU-R BS.1770-4 Annex 2; loudness.py has the definition) of a float32 array (N,) -- or of
    every array of a list, in one device call -- measured on the device.  -inf: an all-zero or empty array.
    A (C, N) array is a programme of C channels: its true peak is the largest over the channels (``channel_weights``
    is accepted as by ``measure_loudness``; the peaks do not depend on it)."""
    from . import loudness, ops
    return _measure(wav, sample_rate, channel_weights,
                    lambda x, n_rows: ops.loudness_rows(x, n_rows, sample_rate, true_peak=True),
                    lambda x, lens, counts, weights: ops.loudness_groups(x, lens, counts, sample_rate, weights=weights),
                    lambda v: loudness.to_db(v[3]))


def loudness_report(wav, sample_rate=44100, channel_weights=None):
    """EBU R 128 figures of a float32 array (N,) -- or of every array of a list, in one device call -- all computed on the
    device (ops.loudness_report_rows; loudness.py has the definitions): a dict (a list of dicts) with ``integrated``
    (LUFS), ``loudness_range`` (LU), ``max_momentary`` and ``max_short_term`` (LUFS), ``sample_peak`` (dBFS) and
    ``true_peak`` (dBTP).  -inf: nothing to measure (silence, too short a row); the range is then 0.0.
    A (C, N) array is ONE programme of C channels (ops.loudness_report_groups): one set of figures, the channels weighted by
    ``channel_weights`` (default loudness.channel_weights(C)); lists may mix (N,) and (C, N) arrays."""
    from . import loudness, ops
    return _measure(wav, sample_rate, channel_weights,
                    lambda x, n_rows: ops.loudness_report_rows(x, n_rows, sample_rate),
                    lambda x, lens, counts, weights: ops.loudness_report_groups(x, lens, counts, sample_rate, weights=weights),
                    lambda v: {"integrated": float(v[0]), "loudness_range": float(v[1]), "max_momentary": float(v[2]),
                               "max_short_term": float(v[3]), "sample_peak": loudness.to_db(v[4]),
                               "true_peak": loudness.to_db(v[5])})


def measure_loudness(wav, sample_rate=44100, channel_weights=None):
    """Integrated loudness (ITU-R BS.1770-4) in LUFS of a float32 array (N,) -- or of every array of a list,
    in one device call -- measured on the device.  -inf: nothing above the gates (silence, or under 400 ms).
    A (C, N) array is ONE programme of C channels (1..8; loudness.py): one loudness, the channels weighted by
    ``channel_weights`` (a list of C numbers >= 0; default loudness.channel_weights(C), BS.1770-4 Table 4).  Two identical
    channels read 3.01 LU above the same signal as one channel.  Lists may mix (N,) and (C, N) arrays."""
    from . import ops
    return _measure(wav, sample_rate, channel_weights,
                    lambda x, n_rows: ops.loudness_rows(x, n_rows, sample_rate),
                    lambda x, lens, counts, weights: ops.loudness_groups(x, lens, counts, sample_rate, weights=weights),
                    lambda v: float(v[0]))


def quantize(wav, bit_depth=16, dither="tpdf", dither_seed=0):
    """Word-length reduction of a float array (N,) -- or of every array of a list, in one device call -- to ``bit_depth``-bit
    PCM (16: int16, 24: int32) on the device: rounded to nearest, saturating, with the seeded dither ``dither`` ("tpdf",
    "hp" or "none"; wordlength.py has the definition, ``wordlength.quantize_ref`` gives the same integers).  A (C, N) array is
    a file of C channels (1..8): channel c draws the dither of channel c.  Every array starts at sample 0.  Lists may mix (N,)
    and (C, N) arrays; what comes back has the shapes that went in."""
    from . import wordlength
    job = _Output(bit_depth=wordlength.check_bit_depth(bit_depth), dither=dither, dither_seed=dither_seed)
    single = not isinstance(wav, (list, tuple))
    items = [np.asarray(w, dtype=np.float32) for w in ([wav] if single else wav)]
    for w in items:
        if w.ndim not in (1, 2) or (w.ndim == 2 and not 1 <= w.shape[0] <= wordlength.MAX_CHANNELS):
            raise ValueError("a waveform is (N,) or (channels, N) with 1..8 channels (got shape %r)" % (w.shape,))
    if not items:
        return []
    rows = [w[None] if w.ndim == 1 else w for w in items]
    groups = [w.shape[0] for w in rows]
    lens = [w.shape[1] for w in rows for _ in range(w.shape[0])]
    host = np.zeros((len(lens), max(max(lens), 1)), np.float32)
    r = 0
    for w in rows:
        host[r:r + w.shape[0], :w.shape[1]] = w
        r += w.shape[0]
    pcm, _ = job.quantize(torch.from_numpy(host).to(_device()), lens, groups)
    pcm = pcm.cpu().numpy()
    out, r = [], 0
    for w, v in zip(items, rows):
        q = pcm[r:r + v.shape[0], :v.shape[1]].copy()
        out.append(q[0] if w.ndim == 1 else q)
        r += v.shape[0]
    return out[0] if single else out


def _span_rows(what, x, stage, stats, _span, channels=None):
    """``limit`` and ``level``: one float32 array (N,) -- or every array of a list, each row on its own -- through a fresh
    ``stage(span)`` (a stream._SpanStage) as a whole row on the device.  ``stats`` (a dict or None) receives the stage's
    ``stats()``: scalars for one array, lists of one value per row for a list.  With ``channels="all"`` a (C, N) array, C in
    1..8, is ONE programme through the stage (the linked form) and comes back (C, N); ``stage(span, C)`` is
    then called with its channel count.  Everything is checked before the device is touched."""
    if stats is not None and not isinstance(stats, dict):
        raise ValueError("stats must be a dict or None")
    span = None if _span is None else int(_span)
    if span is not None and span < 1:
        raise ValueError("_span must be positive")
    single = not isinstance(x, (list, tuple))
    items = [np.asarray(w, dtype=np.float32) for w in ([x] if single else x)]
    from . import loudness as ld
    if ld.check_channels(channels) not in (None, "all"):
        raise ValueError('%s: channels must be None or "all" (got %r)' % (what, channels))
    for w in items:
        if w.ndim == 2 and channels == "all":
            ld.check_channel_count(int(w.shape[0]))
        elif w.ndim != 1:
            raise ValueError("%s: a row is a 1-D array of samples (got shape %r)" % (what, w.shape))
    if channels == "all":
        for c in sorted({w.shape[0] for w in items if w.ndim == 2}):
            stage(span, c)                                           # (ValueError: weights for another channel count)
    outs, recs = [], []
    dev = _device() if items else None
    for w in items:
        st = stage(span) if w.ndim == 1 else stage(span, w.shape[0])
        if w.ndim == 2 and w.shape[1] == 0:                          # (a window is never empty)
            outs.append(w.copy())
        else:
            outs.append(st.whole(torch.from_numpy(np.ascontiguousarray(w)).to(dev)).cpu().numpy())
        recs.append(st.stats())
    if stats is not None:
        for key in (recs[0] if recs else stage(span).stats()):      # (an empty list reports its keys too)
            stats[key] = recs[0][key] if single else [r[key] for r in recs]
    return outs[0] if single else outs


def limit(x, gain_db=0.0, peak_ceiling=-1.0, true_peak=False, lookahead_ms=3.0, sample_rate=44100, stats=None, _span=None,
          channels=None):
    """The fixed-gain look-ahead limiter F (loudness.py) on the device: a float32 array (N,) at ``sample_rate``
    -- or every array of a list, each row on its own -- is multiplied by 10^(gain_db/20) and a gain curve that looks
    ``lookahead_ms`` ahead holds every sample under ``peak_ceiling`` (dBFS; with ``true_peak=True`` the envelope includes the
    interpolated values between the samples).  Nothing is measured and nothing is trimmed afterwards: this is what a streaming
    session (``open_stream(gain_db=..., limiter=True)``) applies, bit for bit, and the inter-sample peak of the result is bounded
    only approximately -- lower ``peak_ceiling`` for a margin.  Where no sample within reach is above the ceiling the output is
    float32(gL) x exactly.  ``stats``: a dict that receives {"max_reduction_db", "peak_out_db"} (lists of one value per row
    when a list went in).  A row is processed in spans of at most 2^22 outputs; the bits do not depend on the span.
    ``channels="all"``: a (C, N) array (or each (C, N) array of a list) is ONE programme of C channels through the LINKED limiter
    (DESIGN.md 3.18): one envelope, the maximum over the channels, one gain curve for all of them, one record -- what a session
    with channels="all" applies, bit for bit.  Without it a 2-D array raises ValueError."""
    from . import loudness as ld
    gain_db = ld.check_gain(gain_db)
    if gain_db is None:
        raise ValueError("limit: gain_db must be a number (0.0: the limiter alone)")
    peak_ceiling, true_peak = ld.check_ceiling(peak_ceiling), ld.check_true_peak(true_peak)
    rate = _check_rate(sample_rate)
    ld.limiter_reach(rate, lookahead_ms, true_peak)      # (ValueError: a look-ahead outside [1, 4096] samples)
    return _span_rows("limit", x, lambda span, C=None: _SpanLimiter(rate, gain_db, peak_ceiling, true_peak, lookahead_ms, span),
                      stats, _span, channels)


def level(x, target=-16.0, max_gain_db=12.0, gate=-50.0, sample_rate=44100, stats=None, _span=None, channels=None,
          channel_weights=None):
    """The streaming loudness leveller (loudness.py) on the device: a float32 array (N,) at ``sample_rate`` (at
    most 192 kHz) -- or every array of a list, each row on its own -- is multiplied by a slowly moving gain that brings the
    loudness of the 3 s around every 100 ms anchor to ``target`` LUFS: at most ``max_gain_db`` up ([0, 40] dB) and 40 dB down,
    held wherever that loudness is not above ``gate`` (LUFS, in [-70, target)), so that pauses are not pumped up.  This is what a
    streaming session (``open_stream(leveller=target)``) applies, bit for bit.  A row shorter than 100 ms comes back as it is.
    ``stats``: a dict that receives {"min_gain_db", "max_gain_db", "anchors", "gated"} (lists of one value per row when a list
    went in).  A row is processed in spans of at most 2^22 outputs; the bits do not depend on the span.
    ``channels="all"``: a (C, N) array (or each (C, N) array of a list) is ONE programme of C channels through the LINKED leveller
    (DESIGN.md 3.18): the loudness is BS.1770-4's over the channels, weighted by ``channel_weights`` (C numbers >= 0; default
    loudness.channel_weights(C); needs channels="all"), and one gain multiplies every channel -- what a session with
    channels="all" applies, bit for bit.  Without it a 2-D array raises ValueError."""
    from . import loudness as ld
    rate = _check_rate(sample_rate)
    target, max_gain_db, gate = ld.check_leveller(target, max_gain_db, gate, rate)
    if channel_weights is not None and channels != "all":
        raise ValueError('level: channel_weights weigh the channels of a programme and need channels="all"')

    def stage(span, C=None):
        weights = None if C is None or channel_weights is None else ld.channel_weights(C, channel_weights)
        return _SpanLeveller(rate, target, max_gain_db, gate, span, weights)

    return _span_rows("level", x, stage, stats, _span, channels)


class Vocoder(nn.Module):
    """44.1 kHz TFGAN-style universal vocoder (voicefixer/vocoder/base.py)."""

    def __init__(self, sample_rate=44100, _state=None):
        super().__init__()
        if sample_rate != 44100:
            raise RuntimeError("Error: Vocoder currently only support 44100 samplerate.")  # config.py:28-31
        self.rate = sample_rate
        if _state is None:
            path = os.path.join(os.path.expanduser("~"), VOCODER_CKPT)
            if not os.path.exists(path):
                raise RuntimeError(
                    "Error 1: The checkpoint for synthesis module / vocoder (model.ckpt-1490000_trimed) is not "
                    "found in ~/.cache/voicefixer/synthesis_module/44100. There is no network in this build; "
                    "place the Zenodo file there (https://zenodo.org/record/5600188).")
            _state = _load_vocoder_state(path)
        self._state = _state
        self._engine = None

    @classmethod
    def from_state(cls, state):
        """Build from an in-memory generator state dict (either weight-norm key style)."""
        return cls(44100, _state=state)

    def _get_engine(self):
        if self._engine is None:
            self._engine = engine.VocoderEngine(self._state, _device(), getattr(self, "math", "f32"))
        return self._engine

    def set_math(self, math):
        """"f32" (default, exact) or "bf16x3" (opt-in split-bf16 products, see VoiceFixer.set_math)."""
        if math not in ("f32", "bf16x3"):
            raise ValueError("math must be 'f32' or 'bf16x3'")
        self.math = math
        if self._engine is not None:
            self._engine.set_math(math)

    def forward(self, mel, cuda=False):
        """mel: [B, 1, T, 128] linear, non-normalised -> [B, 1, 441*(T + T%2 + 4)]."""
        assert mel.size()[-1] == 128
        eng = self._get_engine()
        dev = eng.device
        m = mel.detach().to(dev, torch.float32)[:, 0].contiguous()
        T = m.shape[1]
        wav, L = eng.run_f16_checked(lambda: eng.forward(m, T))
        out = wav[:, :, :L]
        return out if cuda else out.cpu()

    __call__ = forward  # usable directly as ``your_vocoder_func`` (with the default cuda=False)

    def oracle(self, fpath, out_path, cuda=False):
        """wav file -> ground-truth mel (librosa-style STFT + slaney HTK mel) -> vocoder -> wav file
        (voicefixer/vocoder/base.py:58-77); only the file decode/encode runs on the host."""
        from . import ops
        wav = audio_io.load_wav(fpath, self.rate, mono=False)
        if wav.ndim == 2:
            wav = np.ascontiguousarray(wav[0])  # read_wave(fpath)[..., 0]: the FIRST channel, not a down-mix (vocoder/base.py:61)
        eng = self._get_engine()
        w = torch.from_numpy(wav)[None].to(eng.device)
        N = w.shape[1]
        mel, T = ops.oracle_mel(w, N)            # wav/max|wav| -> |STFT| -> slaney mel, on the device
        Tc = T + T % 2 + 4
        cond = ops.guarded(1, 128, Tc, engine.G_TILE, eng.device)
        ops.mel_to_cond_plain(mel, cond, T)      # amp_to_db - 20, normalize, pre()
        wav_re, L = eng.run_f16_checked(lambda: eng.forward_cond(cond, Tc))
        audio_io.save_wave((wav_re[:, 0, :L] * 2 ** 15).cpu().numpy(), out_path, sample_rate=self.rate)


class _RestorerHandle(nn.Module):
    """What reference callers reach through ``VoiceFixer._model`` (voicefixer/base.py:13,109; test/streamlit.py:40-42 does
    ``list(vf._model.parameters())[0].is_cuda`` and ``vf._model = vf._model.to(device)``): an ``nn.Module`` with a
    ``vocoder`` attribute whose call is the restorer's forward ``(sp, mel_noisy) -> {"mel": log-mel, ...}``
    (restorer/model.py:102-120, 395-405).  The weights live in the engine's packed HIP buffers, so ``.to()`` only moves
    the one placeholder parameter that makes ``parameters()`` non-empty; compute always runs on the MI355X."""

    def __init__(self, owner):
        super().__init__()
        object.__setattr__(self, "_owner", owner)   # (not a sub-module: no cycle in nn.Module's registry)
        self.placeholder = nn.Parameter(torch.zeros(1), requires_grad=False)
        super().train(False)                        # base.py:30: the reference puts the restorer in eval mode at load time

    @property
    def vocoder(self):
        return self._owner._vocoder

    def train(self, mode=True):
        """nn.Module.train() recurses into children, so ``vf.train()`` / ``vf.eval()`` on the owning VoiceFixer (or any
        wrapper that toggles modes) must not raise here: the flag is stored, and asking for a forward pass in train mode
        (the reference's mode 2, base.py:115) is what fails."""
        return super().train(mode)

    @torch.no_grad()
    def forward(self, sp, mel_orig):
        """mel_orig: [B, 1, T, 128] linear mel -> {"mel": log10 of the restored mel [B, 1, T, 128], "clean", "noisy"};
        ``sp`` is ignored exactly as in the reference (restorer/model.py:102: the argument is unused)."""
        if self.training:
            raise NotImplementedError("mode 2 (BatchNorm / Dropout in train mode, base.py:115) is nondeterministic and "
                                      "not built; call .eval() first")
        assert mel_orig.size()[-1] == 128
        pipe = self._owner._get_pipe()
        m = mel_orig.detach().to(pipe.device, torch.float32)[:, 0].contiguous()
        dbg = {}
        logmel, _ = pipe.restorer.forward(m, m.shape[1], debug=dbg)
        pipe.check()
        out = {"mel": logmel[:, None], "noisy": mel_orig,
               "clean": (dbg["mask"].transpose(1, 2) * m)[:, None]}
        out["unet_out"] = out["lstm_out"] = dbg["unet_out"][:, None]
        dev = self.placeholder.device
        return {k: (v if v.device == dev else v.to(dev)) for k, v in out.items()}


class BatchSourceError(RuntimeError):
    """The iterator that FEEDS ``_restore_batches_isolated`` raised (staging allocation, decode planning): not a fault of a
    device batch, so no row-by-row re-issue can recover it -- the batches already issued are finished first, then this
    is raised; ``restore_folder`` records every file it never got to as failed."""


class VoiceFixer(nn.Module):
    """General speech restoration, inference path (voicefixer/base.py)."""

    def __init__(self, _states=None):
        super().__init__()
        if _states is None:
            path = os.path.join(os.path.expanduser("~"), ANALYSIS_CKPT)
            if not os.path.exists(path):
                raise RuntimeError(
                    "Error 0: The checkpoint for analysis module (vf.ckpt) is not found in "
                    "~/.cache/voicefixer/analysis_module/checkpoints. There is no network in this build; "
                    "place the Zenodo file there (https://zenodo.org/record/5600188/files/vf.ckpt).")
            restorer_state, voc_override = _load_restorer_state(path)
            vocoder = Vocoder(44100)
            if voc_override:
                merged = dict(weights.normalise_vocoder_keys(vocoder._state))
                merged.update(weights.normalise_vocoder_keys(voc_override))
                vocoder = Vocoder.from_state(merged)
        else:
            vocoder_state, restorer_state = _states
            vocoder = Vocoder.from_state(vocoder_state)
        self._vocoder = vocoder
        self._restorer_state = restorer_state
        self._pipe = None
        self._model = _RestorerHandle(self)   # the reference's attribute name (base.py:13); see _RestorerHandle
        self.math = "f32"       # "bf16x3": opt-in fast contraction arithmetic (set_math)
        self.segment_batch = 8  # 30 s segments of one long input restored per launch (~1.3 GB of HBM each)

    @classmethod
    def from_state(cls, vocoder_state, restorer_state):
        """Build from in-memory state dicts (restorer keys without the ``generator.`` prefix)."""
        return cls(_states=(vocoder_state, restorer_state))

    def _get_pipe(self):
        if self._pipe is None:
            dev = _device()
            self._pipe = engine.Pipeline(self._vocoder._state, self._restorer_state, dev, self.math)
            self._vocoder._engine = self._pipe.vocoder
        return self._pipe

    def set_math(self, math):
        """Contraction arithmetic of the convolution family (extension; the reference is fp32 only).
        "f32" (default): exact fp32 products on the fp32 MFMA.  "bf16x3": every fp32 operand is split into
        two bf16 terms and x*w is evaluated as xh*wh + xh*wl + xl*wh on the bf16 MFMA with fp32 accumulation
        (per-product relative error <= 2^-16; end-to-end waveform difference ~2e-6 RMS, the size of an fp32
        summation-order change, against the 1e-3 parity bound).  (The engine's "f16" arithmetic, DESIGN.md 3.7, is not
        offered here: it is not yet faster than either.)"""
        if math not in ("f32", "bf16x3"):
            raise ValueError("math must be 'f32' or 'bf16x3'")
        self.math = math
        if self._pipe is not None:
            self._pipe.set_math(math)

    def enable_graphs(self, max_shapes=4, max_batch=4):
        """Extension: replay a captured HIP graph for repeated (batch <= max_batch, length) shapes (single utterances of
        one length, the equal-length chunks of ``restore_stream``); bit-identical results, see engine.Pipeline."""
        self._get_pipe().enable_graphs(max_shapes, max_batch)

    def _load_wav(self, path, sample_rate, threshold=0.95):
        return audio_io.load_wav(path, sample_rate)

    @staticmethod
    def _check_mode(mode, seed=None):
        """Modes 0 and 1 always (``seed`` is ignored); mode 2 (train-mode BatchNorm + Dropout) only with a seed."""
        if mode in (0, 1):
            return
        if mode == 2:
            if seed is None:
                raise NotImplementedError(
                    "mode=2 (train-mode BatchNorm + Dropout) draws unseeded dropout masks in the reference; here it needs "
                    "seed= (an int in [0, 2**64)), which makes its masks reproducible")
            from . import dropout
            dropout.check_seed(seed)
            return
        raise ValueError("mode must be 0, 1 or 2")

    @torch.no_grad()
    def restore_inmem(self, wav_10k, cuda=False, mode=0, your_vocoder_func=None, seed=None, sample_rate=44100,
                      output_sample_rate=None, loudness=None, peak_ceiling=-1.0, true_peak=False, channels=None,
                      channel_weights=None, limiter=False, limiter_lookahead_ms=3.0, bit_depth=None, dither="tpdf",
                      dither_seed=0):
        """wav_10k: float32 numpy (N,) at 44.1 kHz -> float32 numpy (1, N).
        30 s hard-cut segments, no overlap, concatenated (voicefixer/base.py:117-138).
        ``sample_rate`` (extension): the rate of ``wav_10k``; any other rate than 44.1 kHz is converted ON THE DEVICE
        (ops.resample_rows, the filter of audio_io.resample_hq) before the path runs, to ceil(N * 44100 / sample_rate)
        samples.  ``output_sample_rate`` (extension, default 44.1 kHz): the restored waveform is converted on the device
        to that rate and the peak rule is applied once more to the converted waveform (``convert_output``).
        ``mode=2`` with ``seed`` (int in [0, 2**64)): the restorer in train mode -- batch statistics per segment, seeded
        dropout (dropout.py; segment s of the file draws the masks of (seed, s)); always fp32.  A segment of <= 64 frames
        (< 28224 samples: a short file, or the short tail of a long one) raises ValueError, as the reference does.
        ``loudness`` (extension, LUFS in [-70, 0)): the whole output, after the peak rule and any output rate conversion, is
        normalised on the device to that integrated loudness (ITU-R BS.1770-4), limited by the SAMPLE-peak ceiling
        ``peak_ceiling`` (dBFS in [-20, 0]): one fp32 gain for the file (``apply_loudness``).  None (default): unchanged.
        ``true_peak=True`` (extension): ``peak_ceiling`` is read as dBTP, the gain is limited by the file's TRUE peak at the
        output rate (measured on the device between the samples: loudness.py, EBU R 128's ceiling).
        ``limiter=True`` (extension; needs ``loudness``): where the target would push the file past ``peak_ceiling``, a
        look-ahead peak limiter takes the place of the one static gain (``apply_limiter``; loudness.py): the gain dips
        around the peaks only, ``limiter_lookahead_ms`` (0.1..10, default 3) ahead of them, and the rest of the file reaches
        the target.  The ceiling is a true-peak one with ``true_peak=True``, else a sample-peak one; with ``channels="all"``
        the gain curve is one per file.  A file the ceiling does not bind is written exactly as without the limiter.
        ``channels="all"`` (extension): ``wav_10k`` is (C, N), 1 <= C <= 8, and (C, N') comes back: the model is mono, so
        every channel goes through the path as ``restore_inmem(wav_10k[c])`` does -- the same segment cuts, mode-1 cut, seed,
        rate conversions and peak rule per channel -- with the same segment of all channels in ONE batch; ``loudness`` is
        then ONE linked gain for the file (BS.1770-4's sum over the channels weighted by ``channel_weights``, default
        loudness.channel_weights(C); the largest peak over the channels: ``apply_loudness_groups``), which keeps the
        balance between the channels.  "mix" / "first": a (C, N) input is averaged / cut to its first channel and restored
        as one.  None (default): a 2-D input raises ValueError (it used to be misread as one long row).
        ``bit_depth`` (extension; 16 or 24): the finished output -- after every stage above -- is reduced ON THE DEVICE to PCM of
        that word length and comes back as int16 / int32 of the same shape: rounded to nearest, saturating, with the dither
        ``dither`` ("tpdf", the default: white triangular dither of +-1 LSB; "hp": the same amplitude, high-passed; "none") drawn
        from ``dither_seed`` (an int in [0, 2**64)) as a function of the sample's index and channel (wordlength.py), so a call
        can be repeated.  None (default): float32 comes back, and ``audio_io.save_wave`` truncates it as the reference does."""
        self._check_mode(mode, seed)
        rate_in = _check_rate(sample_rate)
        job = _Output(output_sample_rate, loudness, peak_ceiling, true_peak, channel_weights, mode, seed, limiter,
                      limiter_lookahead_ms, bit_depth, dither, dither_seed)
        wav, multi = _as_programme(wav_10k, _check_channels(channels), "restore_inmem")     # (C, n); C = 1 unless channels="all"
        C = wav.shape[0]
        job.check_channel_counts([C])
        pipe = self._get_pipe()
        n = wav.shape[1]
        src = None           # the input converted to 44.1 kHz on the device (when it arrives at another rate)
        if rate_in != 44100:
            x = torch.from_numpy(np.ascontiguousarray(wav)).to(pipe.device)
            y, ns = convert_rows(x, [n] * C, [rate_in] * C)
            n = ns[0]
            src = y[:, :n]
        # Segment boundaries exactly as the reference's while-loop (base.py:117-120,137): full 30 s
        # segments, then a shorter tail.  Segments are independent in mode 0 (no carried state), so all
        # full segments of a long file go through the path as ONE batch (the reference runs them one
        # by one); the hard cuts and their positions are unchanged.
        bounds = []
        break_point = SEG_LENGTH
        while break_point < n + SEG_LENGTH:
            lo = break_point - SEG_LENGTH
            bounds.append((lo, min(break_point, n)))
            break_point += SEG_LENGTH
        full = [b for b in bounds if b[1] - b[0] == SEG_LENGTH]
        tail = [b for b in bounds if b[1] - b[0] != SEG_LENGTH]

        per = max(1, self.segment_batch // C)      # segments per batch: row s * C + c is channel c of the batch's segment s

        def run():
            res = []
            for i in range(0, len(full), per):
                grp = full[i:i + per]
                if src is None:
                    seg = torch.from_numpy(np.stack([wav[c, a:b] for a, b in grp for c in range(C)])).to(pipe.device)
                else:
                    seg = torch.stack([src[c, a:b] for a, b in grp for c in range(C)])
                out = self._restore_segments(pipe, seg, SEG_LENGTH, mode, your_vocoder_func, seed,
                                             [s for s in range(i, i + len(grp)) for _ in range(C)])
                res.extend(out[k * C:(k + 1) * C] for k in range(len(grp)))
            for a, b in tail:
                if src is None:
                    seg = torch.from_numpy(np.ascontiguousarray(wav[:, a:b])).to(pipe.device)
                else:
                    seg = src[:, a:b].contiguous()
                res.append(self._restore_segments(pipe, seg, b - a, mode, your_vocoder_func, seed, [len(full)] * C))
            out = torch.cat(res, -1)
            out, ms, _ = job.finish(out, [out.shape[-1]] * C, [C] if multi else None)
            if job.bit_depth is not None:
                out, _ = job.quantize(out, ms, [C] if multi else None)
            return out[:, :ms[0]].cpu().numpy()  # (synchronises)

        return pipe.run_checked(run)   # (device error flags are read here; a missed GRU hand-off re-runs the call)

    @staticmethod
    def _restore_segments(pipe, seg, n, mode, your_vocoder_func, seed=None, segments=None):
        """One batch of equal-length segments through the path; mode 1 first shortens every segment to
        512*(n//512) samples by the device-side high-frequency cut (base.py:121-122); mode 2 runs the train-mode
        restorer, row b being segment ``segments[b]`` of its file."""
        if mode == 2:
            return pipe.restore_train(seg, [n] * seg.shape[0], list(segments), seed, your_vocoder_func)
        if mode == 1:
            from . import ops
            seg, _ = ops.hf_cut(seg, n, 0.95)
            n = seg.shape[1]
        return pipe.restore(seg, n, your_vocoder_func)

    def _streams(self, streams):
        """The SAME stream objects on every call: torch's caching allocator keeps one block pool per stream, so fresh
        streams per call (torch hands them out round-robin from 32) would strand a batch's worth of HBM in a new pool
        each time until the allocator has to flush everything (measured: a 5x slower call after ~6 calls)."""
        pipe = self._get_pipe()
        if not hasattr(self, "_stream_pool"):
            self._stream_pool = []
        while len(self._stream_pool) < max(1, int(streams)):
            self._stream_pool.append(torch.cuda.Stream(device=pipe.device))
        return self._stream_pool[:max(1, int(streams))]

    def _issue_batch(self, pipe, stream, batch, mode, your_vocoder_func, job):
        """Queue ONE batch (a ``_Batch``) on ``stream``: H2D of its pinned staging tensor, (rate conversion of rows at other rates
        than 44.1 kHz,) the launch sequence, the tail ``job`` (an ``_Output``) asks for -- (conversion to the output rate,)
        (loudness normalisation,) (word-length reduction) -- D2H of the result (float32, or PCM with ``bit_depth``) and of the
        loudness and word-length results into pinned tensors, an event.  Nothing here waits for the device."""
        from . import ops
        kind, host, lens, rates, seed = batch.kind, batch.host, batch.lens, batch.rates, job.seed
        if rates is not None and all(r == 44100 for r in rates):
            rates = None
        lens_native = lens
        if rates is not None:
            lens = [audio_io.converted_length(n, r, 44100) for n, r in zip(lens, rates)]
        if kind == "ragged" and your_vocoder_func is not None:
            raise ValueError("restore_batches: a plugin vocoder takes 'samples' batches (equal lengths); plan_batches(ragged=False) cuts them")
        if kind == "samples" and min(lens) != max(lens):
            raise ValueError("restore_batches: a 'samples' batch holds rows of ONE length")
        with torch.cuda.stream(stream):
            seg = host.to(pipe.device, non_blocking=True)
            if rates is not None:       # rows staged at their own rates: converted to 44.1 kHz here, one launch per rate pair
                seg, lens = convert_rows(seg, lens_native, rates)
            if kind == "ragged":
                if mode == 1:
                    if min(lens) < 1536:
                        raise VfxError("mode 1 shortens a file to 512 * (n // 512) samples: %d samples leave too few for the "
                                       "reflect-padded STFT (needs > 1024 after the cut)" % min(lens))
                    new_lens = [512 * (n // 512) for n in lens]
                    # (rows are written in place into ONE buffer of exactly the width the longest cut row needs; what lies behind a
                    # row's own end is never read -- every kernel takes the per-row lengths -- so it is not cleared)
                    cut = torch.empty((len(lens), max(new_lens)), dtype=torch.float32, device=seg.device)
                    done = {}
                    for r in range(len(lens)):           # the cut-off is a per-file quantity (base.py:87-104);
                        if r in done:                    # rows of EQUAL length share one launch (vfx_hf_cut_f32 takes B rows)
                            continue
                        same = [q for q in range(r, len(lens)) if lens[q] == lens[r]]
                        if same == list(range(r, r + len(same))):
                            y, _ = ops.hf_cut(seg[r:r + len(same), :lens[r]], lens[r], 0.95)
                            cut[r:r + len(same), :y.shape[1]] = y
                        else:
                            for q in same:
                                y, _ = ops.hf_cut(seg[q:q + 1, :lens[q]], lens[q], 0.95)
                                cut[q, :y.shape[1]] = y[0]
                        for q in same:
                            done[q] = True
                    lens = new_lens
                    seg = cut
                # (a ragged batch holds files of at most 30 s: every row is segment 0 of its file)
                full = pipe.restore_train(seg, lens, [0] * len(lens), seed) if mode == 2 else pipe.restore_rows(seg, lens)
                lens_out = lens
            else:
                n = lens[0]
                parts = [self._restore_segments(pipe, seg[:, s0:s0 + SEG_LENGTH], min(SEG_LENGTH, n - s0), mode,
                                                your_vocoder_func, seed, [s0 // SEG_LENGTH] * len(lens))
                         for s0 in range(0, n, SEG_LENGTH)]
                full = parts[0] if len(parts) == 1 else torch.cat(parts, -1)
                lens_out = [full.shape[-1]] * len(lens)
            full, lens_out, res = job.finish(full, lens_out, batch.groups)
            loud_host = None
            if res is not None:
                loud_host = torch.empty(tuple(res.shape), dtype=torch.float64, pin_memory=True)
                loud_host.copy_(res, non_blocking=True)
            word_host = None
            if job.bit_depth is not None:
                full, qres = job.quantize(full, lens_out, batch.groups)
                word_host = torch.empty(tuple(qres.shape), dtype=torch.int32, pin_memory=True)
                word_host.copy_(qres, non_blocking=True)
            out_host = torch.empty(tuple(full.shape), dtype=full.dtype, pin_memory=True)
            out_host.copy_(full, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(stream)
        return [batch, out_host, lens_out, ev, loud_host, word_host]

    @torch.no_grad()
    def restore_batches(self, batches, your_vocoder_func=None, streams=2, mode=0, seed=None, output_sample_rate=None,
                        loudness=None, peak_ceiling=-1.0, true_peak=False, channel_weights=None, limiter=False,
                        limiter_lookahead_ms=3.0, bit_depth=None, dither="tpdf", dither_seed=0):
        """The device stage of folder inference as a GENERATOR: ``batches`` yields ``(tag, kind, host, lens)`` --
        ``host`` a pinned float32 (B, >= max(lens)) staging tensor whose row r holds ``lens[r]`` samples, ``kind``
        "ragged" (one launch sequence with per-row lengths, Pipeline.restore_rows) or "samples" (equal lengths: files
        of several 30 s segments, plugin vocoders) as ``plan_batches`` cuts them -- and the generator yields
        ``(tag, out_host, lens_out)`` in the same order, ``out_host`` a pinned (B, >= max(lens_out)) tensor.
        Batches go round-robin to ``streams`` HIP streams (the low-occupancy phases of one batch -- GRU recurrence, deep
        UNet levels -- overlap the convolutions of the next) and the host runs one batch per stream AHEAD of the device:
        H2D, the ~600 launches and the D2H of a batch are queued while earlier batches compute, so the device never waits
        for the host and the caller (restore_folder: decode / encode workers) works on other batches meanwhile.
        ``mode=2`` needs ``seed`` (restore_inmem): a row's result equals restoring that file alone with the same seed.
        An item may carry a 5th field, ``rates``: the sample rate of every row (``lens`` then counts samples at those
        rates); rows at other rates than 44.1 kHz are converted on the device before the path runs (``convert_rows``),
        and ``kind`` / the planning refer to the converted lengths.  ``output_sample_rate``: results are converted on the
        device (``convert_output``) before they cross to the host, ``lens_out`` counts samples at that rate.
        ``loudness`` / ``peak_ceiling``: every row is normalised on the device (restore_inmem) before it crosses, and the
        generator yields ``(tag, out_host, lens_out, loud_host)``, ``loud_host`` a pinned float64 (B, 3) of {LUFS before,
        gain, sample peak} per row, copied with the batch.  ``true_peak=True``: the ceiling is a true-peak one (restore_inmem)
        and ``loud_host`` is (B, 4): {LUFS before, gain, sample peak, true peak}.  ``limiter=True`` (restore_inmem): ``loud_host``
        is (B, 8): {LUFS before, gL, sample peak, true peak, bound, min g, trim, peak after} (loudness.py).
        Multichannel files: an item may carry a 6th field, ``groups`` (the 5th may then be None): one channel count (1..8) per
        tag; the channels of a file are adjacent rows of one length and rate, ``tag`` has one entry per FILE.  Every row goes
        through the path on its own; ``loudness`` is then ONE linked gain per file (``apply_loudness_groups``, weights
        ``channel_weights`` or loudness.channel_weights) and ``loud_host`` has one row per file: (G, 4).
        ``bit_depth`` / ``dither`` / ``dither_seed`` (restore_inmem): every row is reduced to PCM on the device before it crosses --
        ``out_host`` is then a pinned int16 (16) or int32 (24) tensor, half the bytes at 16 bits -- and the generator yields one
        more field, LAST (behind ``loud_host`` when that is there): a pinned int32 (B, 2) of {clipped samples, max |q|} per row.
        Every row starts at sample 0 of its file; its channel is its index within its file (``groups``).
        The two-CU GRU's error flag is read when a batch's result crosses to the host; a missed hand-off drains the
        batches in flight and re-issues them on the one-workgroup GRU kernel (Pipeline.run_checked's rule)."""
        from collections import deque
        from .engine import DeviceFlagRaised
        self._check_mode(mode, seed)
        job = _Output(output_sample_rate, loudness, peak_ceiling, true_peak, channel_weights, mode, seed, limiter,
                      limiter_lookahead_ms, bit_depth, dither, dither_seed)
        pipe = self._get_pipe()
        pool = self._streams(streams)
        main = torch.cuda.current_stream(pipe.device)
        for st in pool:
            st.wait_stream(main)
        inflight = deque()
        pipe.set_streams(len(pool))
        ok = False
        try:
            try:
                pipe.check()                  # a flag that is already set belongs to an earlier, unchecked launch (a direct
            except DeviceFlagRaised:          # pipe.restore user): check() has cleared it, and none of THIS call's work failed
                pass
            nb = 0

            def finish_oldest():
                rec = inflight[0]
                rec[3].synchronize()
                try:
                    pipe.check()
                except DeviceFlagRaised as e:
                    # which of the batches in flight raised it cannot be told: drain them all, re-issue every one of
                    # them with the fallback the flags ask for (recurrences on vfx_gru_bidir_f32: nothing to miss; f16
                    # launches in fp32), one after the other
                    torch.cuda.synchronize(pipe.device)
                    if pipe.restorer.gru_err is not None:
                        pipe.restorer.gru_err.zero_()
                    pipe.vocoder.read_f16_flag()
                    with pipe.fallback(e):
                        for q in range(len(inflight)):
                            inflight[q] = self._issue_batch(pipe, pool[0], inflight[q][0], mode, your_vocoder_func, job)
                        torch.cuda.synchronize(pipe.device)
                        pipe.check()
                    rec = inflight[0]
                inflight.popleft()
                return (rec[0].tag, rec[1], rec[2]) + ((rec[4],) if job.loudness is not None else ()) + \
                    ((rec[5],) if job.bit_depth is not None else ())

            for item in batches:
                inflight.append(self._issue_batch(pipe, pool[nb % len(pool)], _Batch.parse(item), mode, your_vocoder_func, job))
                nb += 1
                while len(inflight) > len(pool) + 1:
                    yield finish_oldest()
            while inflight:
                yield finish_oldest()
            ok = True
        finally:
            # in every case: drain the side streams and give the GRU its single-stream launch size back; when a batch
            # raised (a too-short file, an out-of-memory, a plugin vocoder error) or the caller abandoned the
            # generator, whatever the queued launches leave in the device-side error flag belongs to THIS call -- drop
            # it here so that a later, unrelated call does not inherit it
            torch.cuda.synchronize(pipe.device)
            pipe.set_streams(1)
            if not ok and pipe.restorer.gru_err is not None:
                pipe.restorer.gru_err.zero_()
            if not ok:
                pipe.vocoder.read_f16_flag()

    @torch.no_grad()
    def restore_batch(self, wavs, your_vocoder_func=None, batch_size=32, streams=2, ragged_ratio=0.5, mode=0, seed=None,
                      sample_rate=44100, output_sample_rate=None, loudness=None, peak_ceiling=-1.0, true_peak=False,
                      channels=None, channel_weights=None, limiter=False, limiter_lookahead_ms=3.0, bit_depth=None,
                      dither="tpdf", dither_seed=0):
        """Batched folder inference (not in the reference, which loops files at B=1,
        voicefixer/__main__.py:187-212): list of float32 numpy (N_i,) -> list of (1, N_i)  (mode 1: (1, 512*(N_i//512))
        per 30 s segment, as ``restore_inmem`` returns it).
        Utterances of up to 30 s go through RAGGED batches: the length-sorted list is cut into runs of up to
        ``batch_size`` files whose shortest member has at least ``ragged_ratio`` of the frames of the longest, and a run
        is ONE launch sequence in which every kernel takes the per-row lengths (Pipeline.restore_rows) -- each row is
        what restoring that utterance alone returns, the tiles past a row's end are skipped, only the buffers are
        sized for the longest row.  Longer files (several 30 s segments) and plugin vocoders are bucketed by exact
        length, one batched launch sequence per segment index.  The batches run through ``restore_batches`` (round-robin
        on ``streams`` HIP streams, pinned staging in both directions, the host one batch per stream ahead).
        ``mode=1``: every file (every 30 s segment of it) first goes through the device-side high-frequency cut
        (base.py:121-122, ``vfx_hf_cut_f32``) exactly as ``restore_inmem(mode=1)`` does it.  ``mode=2`` needs ``seed``:
        every file is restored as ``restore_inmem(mode=2, seed=seed)`` restores it.
        ``sample_rate`` (extension): the rate of the inputs, one int or a list with one rate per wav; rows are staged at
        their own rates and converted on the device (one launch per distinct rate pair and batch), the batches are
        planned by the converted lengths.  ``output_sample_rate``, ``loudness``, ``peak_ceiling``, ``true_peak``,
        ``limiter``, ``limiter_lookahead_ms``: as ``restore_inmem`` (each file is measured on its own row, whatever else its batch holds).
        ``channels="all"`` (extension): items may be (N,) or (C, N), results are (C, N').  The channels of a file are adjacent
        rows of one batch: the planning is by file, a file weighs C rows (ValueError when ``batch_size`` is smaller than the
        largest C), and ``loudness`` is one linked gain per file (``restore_inmem``; ``channel_weights`` then applies to
        every file and all must have that many channels).  "mix" / "first": (C, N) items are averaged / cut to their first
        channel first.  None (default): as before.
        ``bit_depth`` / ``dither`` / ``dither_seed``: as ``restore_inmem`` -- the results are int16 / int32 PCM of the same shapes,
        each file quantised as that call quantises it, whatever else its batch holds."""
        self._check_mode(mode, seed)
        job = _Output(output_sample_rate, loudness, peak_ceiling, true_peak, channel_weights, mode, seed, limiter,
                      limiter_lookahead_ms, bit_depth, dither, dither_seed)
        multi = _check_channels(channels) == "all"
        progs = [_as_programme(w, channels, "restore_batch")[0] for w in wavs]     # (C_i, N_i); C_i = 1 unless channels="all"
        rates = _row_rates(sample_rate, len(progs))
        counts = [w.shape[0] for w in progs]
        if multi:
            job.check_channel_counts(counts)
        native = all(r == 44100 for r in rates)
        n44 = [w.shape[1] if r == 44100 else audio_io.converted_length(w.shape[1], r, 44100) for w, r in zip(progs, rates)]
        order = sorted(range(len(progs)), key=lambda i: n44[i])
        outs = [None] * len(progs)
        plan = plan_batches([n44[k] for k in order], batch_size, ragged_ratio, ragged=your_vocoder_func is None,
                            rows=[counts[k] for k in order] if multi else None)

        def rows_of(idx):
            """(file, its first row, the row behind its last) of a batch of the files ``idx``: one row per channel."""
            row0 = 0
            for k in idx:
                yield k, row0, row0 + counts[k]
                row0 += counts[k]

        def staged():
            for kind, grp in plan:
                idx = [order[g] for g in grp]
                lens = [progs[k].shape[1] for k in idx for _ in range(counts[k])]
                # rows are padded in a PINNED staging buffer (torch caches pinned blocks) and uploaded without
                # blocking the host, so that the next batch is staged while this one's copy and kernels run
                host = torch.empty((len(lens), max(lens)), dtype=torch.float32, pin_memory=self._pin_memory())
                hv = host.numpy()
                for k, a, b in rows_of(idx):
                    hv[a:b, :progs[k].shape[1]] = progs[k]
                    hv[a:b, progs[k].shape[1]:] = 0.0
                # (only channels="all" sends the channel counts along: they are what makes the loudness gain a linked one)
                yield _Batch(idx, kind, host, lens, None if native else [rates[k] for k in idx for _ in range(counts[k])],
                             [counts[k] for k in idx] if multi else None).as_item()

        for idx, out_host, lens_out, *_ in self.restore_batches(staged(), your_vocoder_func, streams, mode, **job.kwargs()):
            ov = out_host.numpy()
            for k, a, b in rows_of(idx):
                outs[k] = ov[a:b, :lens_out[a]].copy()   # (the pinned block goes back to torch's host cache)
        return outs

    @torch.no_grad()
    def restore_stream(self, wav, chunk_seconds=30.0, overlap_seconds=1.0, batch_size=8, mode=0,
                       your_vocoder_func=None, on_chunk=None, sample_rate=44100, output_sample_rate=None, loudness=None,
                       peak_ceiling=-1.0, true_peak=False, limiter=False, limiter_lookahead_ms=3.0):
        """Long-form restoration with overlap-add (BASELINE config 5; NOT in the reference, whose 30 s segments
        are hard-cut -- ``restore_inmem`` keeps that behaviour): chunks of ``chunk_seconds`` every
        ``chunk_seconds - overlap_seconds``, each restored independently (equal-length chunks are batched),
        consecutive chunks cross-faded linearly over the overlap.  ``on_chunk(start, samples)`` is called with every
        finished stretch of output in order (bounded latency: the first call comes after the first batch).
        ``mode=1``: the high-frequency cut (base.py:121-122) runs per chunk; it returns 512 * (len // 512) samples
        aligned at the chunk's start, so the chunk length is rounded down to a multiple of 512 (every full chunk keeps
        its length) and only the last chunk loses its sub-512 tail -- the output is that much shorter, as the
        reference's mode-1 output is.  Modes 0 and 1 only: ``mode=2`` raises NotImplementedError (its per-segment
        statistics have no overlap-add form).  Returns float32 numpy (1, N').
        ``sample_rate`` (extension): the rate of ``wav``; another rate than 44.1 kHz is converted once, up front, on the
        device, and the chunks are cut from the converted waveform.  ``output_sample_rate`` other than 44.1 kHz raises
        NotImplementedError: the ``on_chunk`` stretches would need the converter's filter state across chunk boundaries; so
        does ``loudness``, and ``true_peak=True`` or ``limiter=True`` with it: the stretches leave before a whole-file measurement
        exists."""
        _check_stream_mode(mode, "restore_stream")
        rate_in = _check_rate(sample_rate)
        job = _Output(output_sample_rate, loudness, peak_ceiling, true_peak)
        if job.loudness is not None or job.true_peak or _check_limiter(limiter, limiter_lookahead_ms):
            raise NotImplementedError("restore_stream: loudness normalisation is not built -- the on_chunk stretches leave before "
                                      "the whole file has been measured; use restore_inmem or restore_folder")
        if job.rate_out != 44100:
            raise NotImplementedError("restore_stream: output_sample_rate is not built -- converting the on_chunk stretches "
                                      "would need the resampler's filter state at every chunk boundary; use restore_inmem")
        pipe = self._get_pipe()
        wav = np.asarray(wav, dtype=np.float32)
        n = wav.shape[0]
        src = None           # the input converted to 44.1 kHz on the device (when it arrives at another rate)
        if rate_in != 44100:
            x = torch.from_numpy(np.ascontiguousarray(wav))[None].to(pipe.device)
            y, (n,) = convert_rows(x, [n], [rate_in])
            src = y[0, :n]
        chunk, ov, min_tail = _stream_geometry(chunk_seconds, overlap_seconds, mode)
        plan = plan_stream_chunks(n, chunk, ov, min_tail)
        out = np.zeros((1, n), np.float32)
        fade_in = (np.arange(ov, dtype=np.float32) / max(ov, 1))[None]
        done = 0  # output is final below this sample
        n_out = n
        i = 0
        while i < len(plan):
            length = plan[i][1]
            grp = [c for c in plan[i:i + batch_size] if c[1] == length]
            if src is None:
                seg = torch.from_numpy(np.stack([wav[a:a + length] for a, _ in grp])).to(pipe.device)
            else:
                seg = torch.stack([src[a:a + length] for a, _ in grp])
            res = pipe.run_checked(lambda: self._restore_segments(pipe, seg, length, mode, your_vocoder_func).cpu().numpy())
            got = res.shape[1]          # == length in mode 0; 512 * (length // 512) in mode 1
            for (a, _), y in zip(grp, res):
                y = y[None]
                if a > 0:  # cross-fade with what the previous chunk left in the overlap
                    out[:, a:a + ov] = out[:, a:a + ov] * (1.0 - fade_in) + y[:, :ov] * fade_in
                    out[:, a + ov:a + got] = y[:, ov:]
                else:
                    out[:, :got] = y
                last = a + length >= n
                if last:
                    n_out = a + got
                final = a + got - ov if not last else n_out
                if on_chunk is not None and final > done:
                    on_chunk(done, out[:, done:final].copy())
                done = max(done, final)
            i += len(grp)
        return out[:, :n_out]

    def open_stream(self, chunk_seconds=30.0, overlap_seconds=1.0, batch_size=1, mode=0, your_vocoder_func=None,
                    sample_rate=44100, output_sample_rate=None, limiter=False, limiter_lookahead_ms=3.0, bit_depth=None,
                    dither="tpdf", dither_seed=0, gain_db=None, peak_ceiling=-1.0, true_peak=False, leveller=None,
                    leveller_max_gain_db=12.0, leveller_gate=-50.0, meter=False, **programme):
        """A push-style session of the overlap-add long-form mode (``RestoreSession``): blocks of any size go in at
        ``sample_rate``, finished stretches come out at ``output_sample_rate`` (default 44.1 kHz), nothing but the current
        chunk is held.  The results of all ``push`` calls and of ``finish``, concatenated, are what ``restore_stream``
        returns for the concatenated blocks (converted to 44.1 kHz as a whole) with the same ``chunk_seconds``,
        ``overlap_seconds``, ``batch_size`` and ``mode`` -- bit for bit at ``batch_size=1`` -- converted as a whole to the
        output rate.  Modes 0 and 1; ``mode=2`` raises NotImplementedError.  The arguments are checked here, before the
        device is touched.  ``gain_db`` (dB, [-60, 60]; default None: no level stage at all): a FIXED gain, float32(10^(gain_db/20))
        times every output sample on the device; with ``limiter=True`` as well, the fixed-gain look-ahead limiter (loudness.py,
        DESIGN.md 3.16) holds the peaks under ``peak_ceiling`` (dBFS, or dBTP with ``true_peak=True``) at the output rate, looking
        ``limiter_lookahead_ms`` ahead, which delays the output by 2 H + 93 samples; ``session.limiter_stats`` reports what it
        did.  ``peak_ceiling``, ``true_peak`` and ``limiter_lookahead_ms`` are checked always and used only there.  The limiter
        bounds every SAMPLE by the ceiling; the inter-sample peak of the gain-modulated output is bounded only approximately and a
        session cannot trim afterwards: lower ``peak_ceiling`` for a margin.  ``limiter=True`` without ``gain_db`` raises
        NotImplementedError, as ``restore_stream`` does with any limiter: a loudness TARGET needs the whole file, and a session
        never sees it (nor does it offer a trim or ``restore_stream``'s refusal lifted).  ``bit_depth`` / ``dither`` / ``dither_seed`` (restore_inmem): the stretches are reduced to PCM
        on the device, each from the session's position on, so that all of them, concatenated, are the whole output quantised
        once; ``push`` and ``finish`` then return int16 / int32 arrays.
        ``leveller`` (LUFS, [-70, 0); default None: none): the streaming loudness leveller (loudness.py) behind the
        output converter and in front of the gain / limiter stage: a slowly moving gain that brings the loudness of the 3 s
        around every 100 ms anchor of the output to this target, at most ``leveller_max_gain_db`` up ([0, 40] dB) and 40 dB down,
        held wherever that loudness is not above ``leveller_gate`` (LUFS, [-70, target)) -- what ``voicefixer_amd.level`` gives
        for the whole output, bit for bit, less than 1.1 s late; output rates up to 192 kHz.  With a leveller ``limiter=True``
        needs no ``gain_db`` (the limiter then runs at 0 dB; a ``gain_db`` follows the leveller as it follows the converter
        today); ``session.leveller_stats`` reports {"min_gain_db", "max_gain_db", "anchors", "gated"}.
        ``meter`` (default False): a streaming loudness meter (loudness.py) taps the final float signal -- behind
        converter, leveller and limiter / gain, ahead of the word-length reduction -- and ``session.loudness_report`` gives the EBU R
        128 figures of what has been delivered (``loudness_report``'s six keys, the live ``momentary`` and ``short_term``, and
        ``seconds``) at any time, also after ``finish``; it delays and alters nothing; output rates up to 192 kHz.
        Two more keywords, ``channels`` and ``channel_weights`` (both default None), are taken BY KEYWORD ONLY and handed to
        ``RestoreSession``, whose signature ends with them (any other keyword is a TypeError): the named parameters of this
        method stay the mono session's.
        ``channels`` (default None: blocks are (k,), as ever, and a 2-D block raises): "all" restores EVERY channel (DESIGN.md
        3.18) -- every block is (C, k), C in 1..8 fixed by the first one, ``push`` / ``finish`` return (C, j), a chunk goes
        through the path as C adjacent rows of one batch, and the leveller and the limiter are LINKED: one gain curve per
        programme, from the channels' energies weighted by ``channel_weights`` (C numbers >= 0; default BS.1770-4 Table 4;
        needs channels="all") and from the envelope over all channels, so the balance between the channels stays -- what
        ``level(..., channels="all")`` and ``limit(..., channels="all")`` give for the whole (C, N) output, bit for bit; the
        stats are one record per programme.  "mix" / "first": a (C, k) block is averaged / cut to channel 0 on the host and
        the session is the mono one."""
        for key in programme:
            if key not in ("channels", "channel_weights"):
                raise TypeError("open_stream() got an unexpected keyword argument %r" % key)
        return RestoreSession(self, chunk_seconds, overlap_seconds, batch_size, mode, your_vocoder_func, sample_rate,
                              output_sample_rate, bit_depth, dither, dither_seed, gain_db, peak_ceiling, true_peak, limiter,
                              limiter_lookahead_ms, leveller, leveller_max_gain_db, leveller_gate, meter, **programme)

    # shortest restorable file: the reflect-padded STFT needs > 1024 samples (mode 1: after the cut to 512 * (n // 512)); mode 2:
    # train-mode BatchNorm needs more than 64 frames (engine.check_train_frames)
    MIN_SAMPLES = {0: 1025, 1: 1536, 2: 441 * (engine.TRAIN_MIN_FRAMES - 1)}

    def _restore_batches_isolated(self, items, failed, your_vocoder_func, streams, mode, **kw):
        """``restore_batches`` with per-row fault isolation (the folder job's device stage): when a batch raises -- a
        length a kernel refuses, an allocation that does not fit, a plugin vocoder error -- the batches that were in
        flight are re-issued ROW BY ROW, every row that still fails is recorded as ``(tag, reason)`` in ``failed`` and
        the stream of batches continues; the job loses the failing file, nothing else (the reference's serial loop,
        voicefixer/__main__.py:187-212, keeps every file it finished before a bad one).  ``kw``: what ``_Output.kwargs()`` gave the
        caller, passed on to every ``restore_batches`` call as it is (none for a default job)."""
        from collections import deque
        src = iter(items)
        pending = deque()
        src_exc = []           # what the batch SOURCE raised (a generator that has raised is finished: nothing more will come)

        def feed():
            while not src_exc:
                try:
                    it = next(src)
                except StopIteration:
                    return
                except Exception as e:    # noqa: BLE001 -- not a device fault: the batches already issued finish (or are re-issued
                    src_exc.append(e)     # row by row), then the error goes to the caller, who knows which files it never saw
                    return
                pending.append(it)
                yield it

        while True:
            try:
                for rec in self.restore_batches(feed(), your_vocoder_func, streams, mode, **kw):
                    pending.popleft()
                    yield rec
                if src_exc:
                    raise BatchSourceError("the batch source failed after %s: %s" % (type(src_exc[0]).__name__, src_exc[0])) from src_exc[0]
                return
            except BatchSourceError:
                raise
            except (KeyboardInterrupt, GeneratorExit):
                raise
            except Exception as exc:    # noqa: BLE001 -- whatever the batch raised costs the rows that raise it again, alone
                bad = list(pending)
                pending.clear()
                if not bad:
                    raise
                first = "%s: %s" % (type(exc).__name__, exc)
                for it in bad:
                    for one in _Batch(*it).files():     # (a file of several channels is re-issued whole)
                        try:
                            for rec1 in self.restore_batches(iter([one.as_item()]), your_vocoder_func, streams, mode, **kw):
                                yield rec1
                        except (KeyboardInterrupt, GeneratorExit):
                            raise
                        except Exception as e1:    # noqa: BLE001
                            failed.append((one.tag[0], "%s: %s" % (type(e1).__name__, e1) if str(e1) else first))

    def restore_folder(self, infolder, outfolder, mode=0, batch_size=32, io_threads=None, your_vocoder_func=None,
                       name_suffix="", extensions=(".wav",), rank=None, world=None, streams=2, ahead=3, stats=None,
                       skip_existing=False, seed=None, output_sample_rate=None, resample_on_device=False, loudness=None,
                       peak_ceiling=-1.0, true_peak=False, channels=None, channel_weights=None, limiter=False,
                       limiter_lookahead_ms=3.0, bit_depth=None, dither="tpdf", dither_seed=0):
        """Folder inference (the reference's CLI loop, voicefixer/__main__.py:176-212: every ``*.wav`` of
        ``infolder`` -> same file name in ``outfolder``), batched, pipelined and -- with ``world`` > 1 -- sharded over
        one process per GPU (BASELINE configs[2] and [3]).

        Every rank lists the folder and reads the lengths from the file HEADERS (cheap, no decoding), so all ranks hold
        the same work list without exchanging anything; ``dist.deal_files`` deals the files longest-first to the least
        loaded rank (equal sample totals to within one file, whatever the length distribution -- NOT contiguous blocks of
        the sorted list, which would give one rank all the long files); a rank cuts ITS files, sorted by length, into
        ragged batches (``plan_batches``) and streams them: a thread pool decodes / resamples / down-mixes the files of
        the next ``ahead`` batches straight into pinned staging rows, ``restore_batches`` keeps one batch per HIP stream
        running and one more queued, and the pool encodes each finished batch to PCM16 from the pinned result --
        decode || restore || encode with the device never waiting.  No collective in the data path; every output file is
        written by exactly one rank.  ``rank`` / ``world`` default to the initialised ``torch.distributed`` group (or 0 / 1).

        A bad file costs THAT file (the reference's loop keeps every file it finished before a bad one; a batched, sharded
        job must not do worse): an unreadable header, a file too short to restore (< 1025 samples; mode 1: < 1536), a decode
        error in a worker, a row the device stage refuses (its batch is re-issued row by row) -- each is skipped, recorded
        as ``(file name, reason)`` in ``stats["failed"]`` and the job goes on; the header length only PLANS (staging
        width, dealing): a truncated file is restored at the length the decoder really returned.  Outputs are written
        to a temporary name and renamed, so a file in ``outfolder`` is always complete; ``skip_existing`` leaves files
        whose output already exists alone (resume after an interrupted job; listed in ``stats["skipped"]``).

        ``mode`` 0, 1 or 2 (2 with ``seed``, restore_batch); ``name_suffix`` goes between base name and extension (the CLI's ``-mode<k>``
        naming for ``--mode all``).  ``extensions``: which files of the folder are taken -- the reference's loop takes
        ``.wav`` only (the default, and what the CLI passes); ``(".wav", ".flac")`` adds FLAC inputs, written back as
        FLAC (the workers decode / resample / encode in libvfx_audio.so, several thousand x real time).
        ``io_threads``: decode / encode workers of this rank (default: the host's cores / (2 * world), 2..8).
        ``stats`` (optional dict) receives this rank's counters: files, audio seconds, wall seconds, summed worker
        seconds of decode and encode (decode includes the host resampling; ``resample_worker_s`` is that part alone),
        seconds the device stage waited for decoded input, ``failed``, ``skipped``.
        ``resample_on_device`` (extension, off by default): the workers only decode and down-mix; staging rows hold the
        files' own rates and the device converts every rate group of a batch to 44.1 kHz (``restore_batches``' rates
        field) -- a file whose reduced rate ratio has max(up, down) > audio_io.DEVICE_MAX_RATIO is still resampled on the
        host.  ``output_sample_rate``: outputs are converted on the device (``convert_output``) and written at that rate.
        ``loudness`` / ``peak_ceiling``: every output is normalised on the device (restore_inmem) before it is written;
        ``stats["loudness"]`` lists ``(output name, LUFS before, gain in dB)`` of the files written.  ``true_peak=True``:
        the ceiling is a true-peak one (restore_inmem) and ``stats["true_peak"]`` lists ``(output name, dBTP before, dBTP
        after)``.  ``limiter=True`` (restore_inmem): ``stats["limiter"]`` lists ``(output name, largest gain reduction in
        dB, trim in dB, peak after in dB)`` per output -- ``(name, 0.0, 0.0, peak after)`` for a file the ceiling did not bind --
        and the gain in ``stats["loudness"]`` is gL times the trim.
        ``channels`` (extension): None or "mix": files of several channels are averaged to one (the reference's
        ``librosa.load``); "first": their first channel is restored; "all": EVERY channel is restored and the output is
        written with the input's channel count (1..8; mixed counts in one folder are fine).  The count comes from the header
        at scan time; the channels of a file are adjacent rows of one batch (a file weighs C rows in the planning and C * n
        in the deal over ranks; a file with more channels than ``batch_size`` fails alone), ``loudness`` is one linked gain
        per file (``restore_inmem``) and ``stats["loudness"]`` / ``stats["true_peak"]`` keep one entry per file.
        ``bit_depth`` / ``dither`` / ``dither_seed`` (restore_inmem): the outputs are reduced to 16- or 24-bit PCM on the device,
        cross to the host as PCM and are written at that depth (``audio_io.save_pcm``: WAV or FLAC) -- the encode workers no
        longer convert anything; ``stats["word_length"]`` lists ``(output name, bits, clipped samples, peak after in dBFS)`` per
        output (a file of several channels: the sum of its rows' clipped counts, the largest of their peaks).  None (default):
        float32 rows cross and ``audio_io.save_wave`` truncates them to 16 bits, as the reference does.
        Returns the list of file names THIS rank wrote."""
        import threading
        import time
        from collections import deque
        from concurrent.futures import ThreadPoolExecutor
        from . import dist as vdist, flac
        self._check_mode(mode, seed)
        job = _Output(output_sample_rate, loudness, peak_ceiling, true_peak, channel_weights, mode, seed, limiter,
                      limiter_lookahead_ms, bit_depth, dither, dither_seed)
        rate_out = job.rate_out
        channels = _check_channels(channels)
        multi = channels == "all"
        nch = {}               # index -> rows the file takes in a batch (its channel count with channels="all", else 1)
        rank, world = vdist.rank_world(rank, world)
        if io_threads is None:
            io_threads = vdist.default_io_threads(world)
        io_threads = max(1, int(io_threads))
        min_len = self.MIN_SAMPLES[mode]
        files = sorted(f for f in os.listdir(infolder) if os.path.splitext(f)[-1] in tuple(extensions))
        os.makedirs(outfolder, exist_ok=True)
        paths = [os.path.join(infolder, f) for f in files]
        names = [("%s%s%s" % (os.path.splitext(f)[0], name_suffix, os.path.splitext(f)[1])) for f in files]
        if any(p.lower().endswith(".flac") for p in paths):
            flac.native()      # load the C codec once, before the workers race for it
        t_start = time.perf_counter()
        lock = threading.Lock()
        cnt = {"decode_s": 0.0, "encode_s": 0.0, "stall_s": 0.0, "resample_s": 0.0}
        failed = []            # (index, reason): files this rank gave up on
        real_len = {}          # index -> samples the decoder returned
        truncated = []         # (index, header length, decoded length): restored at the decoded length
        stage = {}             # resample_on_device: index -> (rate of its staging row, planned samples at that rate)

        def on_device(sr):
            return sr != 44100 and max(audio_io.rate_ratio(sr, 44100)) <= audio_io.DEVICE_MAX_RATIO

        def scan(i):
            """Planning length of file i from its header; None + reason when the header is unreadable.  A header that
            promises less than a restorable file (0 in a streamed / interrupted recording) is not believed: the file
            is decoded once to see what is really there."""
            try:
                nch[i] = audio_io.wav_channels(paths[i]) if multi else 1
                if not 1 <= nch[i] <= 8:
                    raise RuntimeError("%d channels (1..8 are restored)" % nch[i])
                if channel_weights is not None and multi and nch[i] != len(channel_weights):
                    raise RuntimeError("%d channels, but channel_weights has %d" % (nch[i], len(channel_weights)))
                if resample_on_device:
                    sr, n_nat, p_nat = audio_io.wav_info(paths[i])
                    n, promised = audio_io.converted_length(n_nat, sr, 44100), audio_io.converted_length(p_nat, sr, 44100)
                else:
                    n, promised = audio_io.wav_length(paths[i], 44100, with_promise=True)
                if promised != n:         # (a header that promises more than the file holds: planned at what is there)
                    with lock:
                        truncated.append((i, promised, n))
                if n < min_len:
                    if resample_on_device:
                        n_nat = audio_io.load_wav_native(paths[i])[0].shape[-1]
                        n = audio_io.converted_length(n_nat, sr, 44100)
                    else:
                        n = audio_io.load_wav(paths[i], 44100).shape[-1]
                if resample_on_device:
                    stage[i] = (sr, n_nat) if on_device(sr) else (44100, n)
                return n, None
            except Exception as e:    # noqa: BLE001 -- any unreadable file is this file's problem only
                return None, "%s: %s" % (type(e).__name__, e)

        def decode_into(i, row, n):
            """Worker: file i -> staging row (width n = the header's promise, at the row's rate).  Returns the number of
            samples really there (<= n: a longer decode is cut at the staging width), or raises -- the caller drops the row.
            (audio_io.load_wav's steps, with the host resampling timed on its own; with resample_on_device the row stays
            at the file's rate unless the device does not take its ratio.)"""
            t0 = time.perf_counter()
            if channels in (None, "mix"):
                x, sr = audio_io.load_wav_native(paths[i])
            else:               # (row is then (C, n): the file's channels, or its first one)
                x, sr = audio_io.load_wav_native(paths[i], mono=False)
                x = audio_io.select_channels(x, channels)
                x = x if multi else x[None]
                if x.shape[0] != row.shape[0]:
                    raise RuntimeError("the header promised %d channel(s), the decoder returned %d" % (row.shape[0], x.shape[0]))
            rs = 0.0
            if sr != 44100 and not (resample_on_device and stage[i][0] == sr):
                t1 = time.perf_counter()
                x = audio_io.resample_hq(x, sr, 44100)
                rs = time.perf_counter() - t1
            x = np.ascontiguousarray(x, dtype=np.float32)
            got = x.shape[-1]
            m = min(got, n)
            row[..., :m] = x[..., :m]
            row[..., m:] = 0.0
            with lock:
                cnt["decode_s"] += time.perf_counter() - t0
                cnt["resample_s"] += rs
                if got != n and not any(t[0] == i for t in truncated):
                    sr_row = row_rate(i)
                    truncated.append((i, audio_io.converted_length(n, sr_row, 44100), audio_io.converted_length(got, sr_row, 44100)))
            return m

        def row_rate(i):
            return stage[i][0] if resample_on_device else 44100

        def encode_from(row, i):
            t0 = time.perf_counter()
            final = os.path.join(outfolder, names[i])
            part = os.path.join(outfolder, ".part-%d-%s" % (os.getpid(), names[i]))   # (same extension: save_wave picks the container from it)
            try:
                if job.bit_depth is not None:      # (row is PCM already: straight into the container)
                    audio_io.save_pcm(row, part, rate_out, job.bit_depth, channels_first=True)
                elif multi:
                    audio_io.save_wave(row, part, rate_out, channels_first=True)
                else:
                    audio_io.save_wave(row, part, rate_out)
                os.replace(part, final)
            except BaseException:
                if os.path.exists(part):
                    os.remove(part)
                raise
            with lock:
                cnt["encode_s"] += time.perf_counter() - t0

        written, skipped, done = [], [], []
        loud_rows = {}         # index -> (LUFS before, gain in dB)
        tp_rows = {}           # index -> (dBTP before, dBTP after)
        lim_rows = {}          # index -> (largest gain reduction in dB, trim in dB, peak after in dB)
        word_rows = {}         # index -> (bits, clipped samples, peak after in dBFS)
        with ThreadPoolExecutor(max_workers=io_threads) as pool:
            scanned = list(pool.map(scan, range(len(files))))
            # every rank must deal from the SAME list: inside an initialised process group of this world size the scans are
            # all-gathered and a file any rank could not read is dropped by all (dist.agree_on_scan); without a group (explicit
            # rank / world) the ranks rely on seeing the same headers.  Each dropped file is REPORTED by one rank
            if world > 1 and vdist.dist.is_available() and vdist.dist.is_initialized() and vdist.dist.get_world_size() == world:
                scanned = vdist.agree_on_scan(scanned)
            usable = []
            for i, (n, why) in enumerate(scanned):
                if why is None and n < min_len:
                    why = "too short to restore: %d samples at 44.1 kHz (mode %d needs >= %d)" % (n, mode, min_len)
                if why is None and nch[i] > batch_size:
                    why = "%d channels do not fit a batch of %d rows (the channels of a file share one batch)" % (nch[i], batch_size)
                if why is not None:
                    if i % world == rank:
                        failed.append((i, why))
                else:
                    usable.append(i)
            lengths = {i: scanned[i][0] for i in usable}
            owner = vdist.deal_files([lengths[i] * nch[i] for i in usable], world)
            mine = sorted((i for i, o in zip(usable, owner) if o == rank), key=lambda i: (lengths[i], i))
            if skip_existing:
                # applied AFTER the deal and to this rank's own files only: the deal depends on nothing but the input headers,
                # so ranks that look at the output folder at different moments still agree on who owns what
                skipped = [names[i] for i in mine if os.path.exists(os.path.join(outfolder, names[i]))]
                mine = [i for i in mine if not os.path.exists(os.path.join(outfolder, names[i]))]
            plan = plan_batches([lengths[i] for i in mine], batch_size, ragged=your_vocoder_func is None,
                                rows=[nch[i] for i in mine] if multi else None)

            def rows_of(idx):
                """File r of a batch of files ``idx`` has the staging / result rows rows_of(idx)[r] .. rows_of(idx)[r + 1] (one per
                channel with channels="all", else one)."""
                return np.concatenate([[0], np.cumsum([nch[i] for i in idx])]).tolist()

            def item(idx, kind, host, real, rates):
                """The ``restore_batches`` item of the files ``idx``: lengths and rates once per ROW; the channel counts go along
                only with channels="all" (every other job yields the 4- or 5-field items it always did)."""
                per_row = lambda v: [v[r] for r, i in enumerate(idx) for _ in range(nch[i])]     # noqa: E731
                return _Batch(idx, kind, host, per_row(real), per_row(rates) if resample_on_device else None,
                              [nch[i] for i in idx] if multi else None).as_item()

            def submit_decode(b):
                kind, grp = plan[b]
                idx = [mine[g] for g in grp]
                lens = [stage[i][1] if resample_on_device else lengths[i] for i in idx]     # (staging: at each row's rate)
                row0 = rows_of(idx)
                try:
                    host = torch.empty((row0[-1], max(lens)), dtype=torch.float32, pin_memory=self._pin_memory())
                except Exception as e:    # noqa: BLE001 -- a staging block that cannot be had (host memory, pinning) costs THIS batch
                    for i in idx:
                        failed.append((i, "staging for a batch of %d x %d samples: %s: %s" % (len(idx), max(lens), type(e).__name__, e)))
                    return idx, kind, None, lens, []
                hv = host.numpy()
                return idx, kind, host, lens, [pool.submit(decode_into, i, hv[row0[r]:row0[r + 1]] if channels in ("first", "all")
                                                           else hv[r], lens[r]) for r, i in enumerate(idx)]

            def decoded():
                queue = [submit_decode(b) for b in range(min(ahead, len(plan)))]
                for b in range(len(plan)):
                    idx, kind, host, lens, futs = queue.pop(0)
                    if b + ahead < len(plan):
                        queue.append(submit_decode(b + ahead))
                    if host is None:          # (its staging block could not be allocated: the files are already in `failed`)
                        continue
                    t0 = time.perf_counter()
                    keep, real, real44 = [], [], []
                    for r, f in enumerate(futs):
                        try:
                            m = f.result()
                            m44 = audio_io.converted_length(m, row_rate(idx[r]), 44100)
                            if m44 < min_len:
                                raise RuntimeError("too short to restore: the header promised %d samples, the decoder "
                                                   "returned %d (mode %d needs >= %d)" % (lengths[idx[r]], m44, mode, min_len))
                            keep.append(r)
                            real.append(m)
                            real44.append(m44)
                            real_len[idx[r]] = m44
                        except Exception as e:    # noqa: BLE001 -- a decode error costs this file only
                            failed.append((idx[r], "%s: %s" % (type(e).__name__, e)))
                    cnt["stall_s"] += time.perf_counter() - t0
                    if not keep:
                        continue
                    if len(keep) < len(idx):          # (rare) drop the failed rows: the batch shrinks, the others go on
                        row0 = rows_of(idx)
                        host = host[[q for r in keep for q in range(row0[r], row0[r + 1])]].contiguous()
                        if self._pin_memory():
                            host = host.pin_memory()
                        idx = [idx[r] for r in keep]
                    rates = [row_rate(i) for i in idx]
                    row0 = rows_of(idx)
                    if kind == "samples" and min(real44) != max(real44):
                        # equal-length bucket (several 30 s segments, plugin vocoder) with a truncated member: one batch per file
                        for r in range(len(idx)):
                            yield item(idx[r:r + 1], kind, host[row0[r]:row0[r + 1], :real[r]], real[r:r + 1], rates[r:r + 1])
                        continue
                    yield item(idx, kind, host, real, rates)

            writes = deque()           # per batch: the futures of its rows (their views keep the batch's pinned result alive)
            dev_failed = []

            def drain(limit):
                while len(writes) > limit:
                    for i, w in writes.popleft():
                        try:
                            w.result()
                            written.append(names[i])
                            done.append(i)
                        except Exception as e:    # noqa: BLE001 -- a full disk / unwritable name costs this file
                            failed.append((i, "%s: %s" % (type(e).__name__, e)))

            source_error = None
            try:
                for idx, out_host, lens_out, *extra in self._restore_batches_isolated(decoded(), dev_failed, your_vocoder_func,
                                                                                       streams, mode, **job.kwargs()):
                    ov = out_host.numpy()
                    if job.bit_depth is not None:      # (the last field: {clipped, max |q|} per ROW)
                        from . import wordlength
                        qv, row0 = extra[-1].numpy(), rows_of(idx)
                        for r, i in enumerate(idx):
                            rows = qv[row0[r]:row0[r + 1]]
                            word_rows[i] = (job.bit_depth, int(rows[:, 0].sum()),
                                            wordlength.peak_db(int(rows[:, 1].max()), job.bit_depth))
                    if job.loudness is not None:
                        lv = extra[0].numpy()
                        for r, i in enumerate(idx):
                            if lv.shape[1] == 8:              # the limiter's record (loudness.py)
                                db = [20.0 * float(np.log10(v)) if v > 0 else -float("inf") for v in lv[r, [1, 3, 5, 6, 7]]]
                                loud_rows[i] = (float(lv[r, 0]), db[0] + db[3])
                                lim_rows[i] = (db[2], db[3], db[4])
                                if job.true_peak:
                                    tp_rows[i] = (db[1], db[4])
                                continue
                            loud_rows[i] = (float(lv[r, 0]), 20.0 * float(np.log10(lv[r, 1])))
                            if lv.shape[1] == 4:
                                before = 20.0 * float(np.log10(lv[r, 3])) if lv[r, 3] > 0 else -float("inf")
                                tp_rows[i] = (before, before + loud_rows[i][1])
                    row0 = rows_of(idx)
                    writes.append([(i, pool.submit(encode_from, ov[row0[r]:row0[r + 1], :lens_out[row0[r]]], i))
                                   for r, i in enumerate(idx)])
                    drain(ahead + 2)       # bounded backlog: pinned results do not pile up behind a slow disk
            except BatchSourceError as e:  # the source died: every batch it had handed over has been finished and is written below
                source_error = str(e)
            drain(0)
            failed.extend(dev_failed)
            # the books must balance: every file dealt to this rank is written, failed or skipped -- a file nobody accounted
            # for (the batch source died before it got there) is reported as failed, never dropped in silence
            seen = set(done) | {i for i, _ in failed}
            for i in mine:
                if i not in seen:
                    failed.append((i, "not processed: %s" % (source_error or "the device stage ended early")))
        if stats is not None:
            stats.update(rank=rank, world=world, files=len(written), folder_files=len(files), batches=len(plan),
                         audio_s=sum(real_len[i] * nch[i] for i in done) / 44100.0, wall_s=time.perf_counter() - t_start,
                         decode_worker_s=cnt["decode_s"], encode_worker_s=cnt["encode_s"], resample_worker_s=cnt["resample_s"],
                         resample_on_device=bool(resample_on_device), output_sample_rate=rate_out,
                         device_waited_for_decode_s=cnt["stall_s"], io_threads=io_threads,
                         failed=sorted((files[i], why) for i, why in failed), skipped=sorted(skipped),
                         truncated=sorted((files[i], n, m) for i, n, m in truncated if i in real_len or i in mine),
                         loudness=sorted((names[i],) + loud_rows[i] for i in done if i in loud_rows))
            if job.true_peak and job.loudness is not None:
                stats["true_peak"] = sorted((names[i],) + tp_rows[i] for i in done if i in tp_rows)
            if job.limiter:
                stats["limiter"] = sorted((names[i],) + lim_rows[i] for i in done if i in lim_rows)
            if job.bit_depth is not None:
                stats["word_length"] = sorted((names[i],) + word_rows[i] for i in done if i in word_rows)
        return sorted(written)

    @staticmethod
    def _pin_memory():
        return torch.cuda.is_available()

    def restore(self, input, output, cuda=False, mode=0, your_vocoder_func=None, seed=None, output_sample_rate=None,
                resample_on_device=False, loudness=None, peak_ceiling=-1.0, true_peak=False, channels=None,
                channel_weights=None, limiter=False, limiter_lookahead_ms=3.0, bit_depth=None, dither="tpdf", dither_seed=0):
        """File -> file (voicefixer/base.py:140-146).  ``resample_on_device`` (extension): the input is decoded at its own
        rate and converted on the device (``restore_inmem(sample_rate=...)``; ratios the device does not take are still
        resampled on the host); ``output_sample_rate``: the file is written at that rate (converted on the device);
        ``loudness`` / ``peak_ceiling`` / ``true_peak`` / ``limiter`` / ``limiter_lookahead_ms``: as ``restore_inmem``.
        ``channels`` (extension): None or "mix": a file
        of several channels is averaged to one (the reference's ``librosa.load``); "first": its first channel; "all": every
        channel is restored (``restore_inmem(channels="all")``) and the output has the input's channel count.
        ``bit_depth`` / ``dither`` / ``dither_seed``: as ``restore_inmem``; the file is written at that depth
        (``audio_io.save_pcm``).  None (default): 16 bits, truncated by ``audio_io.save_wave`` as the reference does."""
        job = _Output(output_sample_rate, loudness, peak_ceiling, true_peak, channel_weights, limiter=limiter,
                      limiter_lookahead_ms=limiter_lookahead_ms, bit_depth=bit_depth, dither=dither, dither_seed=dither_seed)
        channels = _check_channels(channels)

        per_channel = channels in ("first", "all")
        if per_channel or resample_on_device:       # decoded at the file's own rate, channel by channel or averaged by the decoder
            x, sr = audio_io.load_wav_native(input, mono=not per_channel)
            x = audio_io.select_channels(x, channels)
            if sr != 44100 and not (resample_on_device and max(audio_io.rate_ratio(sr, 44100)) <= audio_io.DEVICE_MAX_RATIO):
                x, sr = audio_io.resample_hq(x, sr, 44100), 44100
        else:
            x, sr = self._load_wav(input, sample_rate=44100), 44100
        kw = {"channels": "all", "channel_weights": channel_weights} if channels == "all" else {}
        if job.limiter:
            kw.update(limiter=True, limiter_lookahead_ms=job.limiter_lookahead_ms)
        if job.bit_depth is not None:
            kw.update(bit_depth=job.bit_depth, dither=job.dither, dither_seed=job.dither_seed)
        out_np_wav = self.restore_inmem(np.ascontiguousarray(x, dtype=np.float32), cuda=cuda, mode=mode,
                                        your_vocoder_func=your_vocoder_func, seed=seed, sample_rate=sr,
                                        output_sample_rate=output_sample_rate, loudness=loudness, peak_ceiling=peak_ceiling,
                                        true_peak=true_peak, **kw)
        # (channels_first: what came back is (C, N') whatever its sizes; for one channel this is what the default does)
        if job.bit_depth is not None:
            audio_io.save_pcm(out_np_wav, output, job.rate_out, job.bit_depth, channels_first=True)
            return
        audio_io.save_wave(out_np_wav, fname=output, sample_rate=job.rate_out, channels_first=True)
