#!/usr/bin/env python
"""The push-style session against the two-step route it replaces, host to host, in one process:

  session : VoiceFixer.open_stream(batch_size=1, output_sample_rate=RATE), the input pushed in blocks of BLOCK seconds
  two-step: VoiceFixer.restore_stream(batch_size=1) on the whole input, then a whole-row convert_rows to RATE

Median of --repeats runs each (alternating), the session's device-memory high-water mark above what the model holds, and
the time from the first push to the first non-empty result.  Prints one JSON line.

--limiter: the cost of the session's fixed-gain look-ahead limiter instead.  The signal gets one impulse per
second and the gain is set from the plain session's output so that every output chunk is bound; the plain session and the
session with gain_db and limiter=True (true peak) run alternating in one process, median of --repeats with the spread, and
one ops.limit_span call over one second of output is timed with HIP events.

--channels C: a session of C channels (channels="all").  Three legs alternate in one process -- the plain
C-channel session, C mono sessions back to back on the same channels (the route a stereo stream had to take before), and the
C-channel session with the linked leveller and limiter on -- median of --repeats with the spread; then one ops.limit_span_rows
and one ops.level_span_rows call over 1 s and over one chunk of C-channel output are timed with HIP events against C mono calls
and against a device copy of the same samples.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from voicefixer_amd import VoiceFixer, api, weights, _lib  # noqa: E402


def _spread(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts), "all": ts}


def limiter_leg(args, vf, wav, blk):
    from voicefixer_amd import loudness, ops
    cs, ov, rate = args.chunk_seconds, args.overlap_seconds, args.output_sample_rate
    n = len(wav)

    def session(**kw):
        outs = []
        with vf.open_stream(cs, ov, batch_size=1, output_sample_rate=rate, **kw) as s:
            for a in range(0, n, blk):
                outs.append(s.push(wav[a:a + blk]))
            outs.append(s.finish())
            stats = s.limiter_stats
        return np.concatenate(outs, axis=1), stats

    Z, _ = session()                      # warm-up, and the level the gain is set from
    step = int(cs * rate)
    peaks = [float(np.abs(Z[0, a:a + step]).max()) for a in range(0, Z.shape[1], step)]
    ceiling = -1.0
    gain_db = 20.0 * np.log10(10.0 ** (ceiling / 20.0) / min(peaks)) + 6.0     # the quietest chunk's peak 6 dB over the ceiling
    kw = dict(gain_db=float(gain_db), limiter=True, peak_ceiling=ceiling, true_peak=True)
    lim, stats = session(**kw)
    per_chunk = [float(np.abs(lim[0, a:a + step]).max()) for a in range(0, lim.shape[1], step)]
    t_plain, t_lim = [], []
    for _ in range(args.repeats):
        for ts, k in ((t_plain, {}), (t_lim, kw)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            session(**k)
            ts.append(time.perf_counter() - t0)
    # one ops.limit_span call over one second of output, HIP events
    H, Bk, Fw = loudness.limiter_reach(rate, 3.0, True)
    dev = vf._get_pipe().device
    row = torch.from_numpy(np.ascontiguousarray(Z[0, :3 * rate])).to(dev)
    out = torch.empty((rate,), dtype=torch.float32, device=dev)
    m0 = rate
    lo, hi = m0 - 2 * H - Bk, m0 + rate + 2 * H + Fw
    call = lambda: ops.limit_span(row[lo:hi], lo, None, rate, float(gain_db), m0, m0 + rate, out, ceiling, True, 3.0)
    for _ in range(3):
        call()
    ev = []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        ev.append(e0.elapsed_time(e1) * 1e-3)
    mp, ml = statistics.median(t_plain), statistics.median(t_lim)
    res = {"leg": "limiter", "minutes": args.minutes, "block_seconds": args.block_seconds, "chunk_seconds": cs, "overlap_seconds": ov,
           "output_sample_rate": rate, "repeats": args.repeats, "gain_db": float(gain_db), "peak_ceiling": ceiling,
           "every_chunk_bound": bool(min(peaks) * 10.0 ** (gain_db / 20.0) > 10.0 ** (ceiling / 20.0)),
           "chunk_peaks_out_db": [20.0 * np.log10(p) for p in per_chunk], "limiter_stats": stats,
           "plain_s": _spread(t_plain), "limiter_s": _spread(t_lim), "limiter_over_plain": ml / mp - 1.0,
           "limit_span_1s_call_s": _spread(ev), "device": torch.cuda.get_device_name(dev),
           "build_id": _lib.lib().vfx_build_id().decode()}
    print(json.dumps(res))


def _events(call, reps=20):
    for _ in range(3):
        call()
    ev = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        ev.append(e0.elapsed_time(e1) * 1e-3)
    return _spread(ev)


def channels_leg(args, vf, wav, blk):
    from voicefixer_amd import loudness, ops
    cs, ov, rate, C = args.chunk_seconds, args.overlap_seconds, args.output_sample_rate, args.channels
    n = wav.shape[1]

    def session(x, **kw):
        outs = []
        with vf.open_stream(cs, ov, batch_size=1, output_sample_rate=rate, **kw) as s:
            for a in range(0, n, blk):
                outs.append(s.push(x[..., a:a + blk]))
            outs.append(s.finish())
            stats = (s.leveller_stats, s.limiter_stats)
        return np.concatenate(outs, axis=1), stats

    linked = dict(channels="all", leveller=-20.0, limiter=True, true_peak=True)
    Z, _ = session(wav, channels="all")                          # warm-up of every leg
    monos = [session(wav[c])[0] for c in range(C)]
    _, stats = session(wav, **linked)
    rms = [float(np.sqrt(np.mean(np.square(Z[c].astype(np.float64) - monos[c][0])))) for c in range(C)]
    t_all, t_mono, t_link = [], [], []
    for _ in range(args.repeats):
        for ts, run in ((t_all, lambda: session(wav, channels="all")), (t_mono, lambda: [session(wav[c]) for c in range(C)]),
                        (t_link, lambda: session(wav, **linked))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            ts.append(time.perf_counter() - t0)
    # single calls of the linked span kernels over 1 s and over one chunk of output, HIP events
    dev = vf._get_pipe().device
    H, Bk, Fw = loudness.limiter_reach(rate, 3.0, True)
    hop = loudness.hop_length(rate)
    calls = {}
    for name, secs in (("1s", 1.0), ("chunk", cs)):
        m = int(secs * rate)
        m0 = 3 * rate
        need = m0 + m + 2 * rate
        reps_ = -(-need // Z.shape[1])
        prog = torch.from_numpy(np.ascontiguousarray(np.tile(Z, (1, reps_))[:, :need])).to(dev)
        out = torch.empty((C, m), dtype=torch.float32, device=dev)
        lo, hi = m0 - 2 * H - Bk, m0 + m + 2 * H + Fw
        win = prog[:, lo:hi].contiguous()
        calls["limit_rows_" + name] = _events(lambda: ops.limit_span_rows(win, lo, None, rate, 6.0, m0, m0 + m, out, -1.0, True, 3.0))
        calls["limit_mono_x%d_" % C + name] = _events(lambda: [ops.limit_span(win[c], lo, None, rate, 6.0, m0, m0 + m, out[c], -1.0,
                                                                               True, 3.0) for c in range(C)])
        # the leveller from the row's start (calls come in order): outputs [0, m) of a programme of m + 1.1 s
        head = prog[:, :m + 11 * hop].contiguous()
        state = ops.level_state(dev)
        calls["level_rows_" + name] = _events(lambda: ops.level_span_rows(head, 0, None, rate, -20.0, 0, m - m % hop, out, state))
        states = [ops.level_state(dev) for _ in range(C)]
        calls["level_mono_x%d_" % C + name] = _events(lambda: [ops.level_span(head[c], 0, None, rate, -20.0, 0, m - m % hop, out[c],
                                                                               states[c]) for c in range(C)])
        src = prog[:, m0:m0 + m].contiguous()
        calls["device_copy_" + name] = _events(lambda: out.copy_(src))
    ma, mm, ml = statistics.median(t_all), statistics.median(t_mono), statistics.median(t_link)
    res = {"leg": "channels", "channels": C, "minutes": args.minutes, "block_seconds": args.block_seconds, "chunk_seconds": cs,
           "overlap_seconds": ov, "output_sample_rate": rate, "repeats": args.repeats, "rms_vs_mono": rms,
           "leveller_stats": stats[0], "limiter_stats": stats[1], "all_s": _spread(t_all), "mono_sessions_s": _spread(t_mono),
           "linked_s": _spread(t_link), "all_over_monos": ma / mm - 1.0, "linked_over_all": ml / ma - 1.0, "span_calls_s": calls,
           "device": torch.cuda.get_device_name(dev), "build_id": _lib.lib().vfx_build_id().decode()}
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=5.0)
    ap.add_argument("--block-seconds", type=float, default=1.0)
    ap.add_argument("--chunk-seconds", type=float, default=30.0)
    ap.add_argument("--overlap-seconds", type=float, default=1.0)
    ap.add_argument("--output-sample-rate", type=int, default=48000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--limiter", action="store_true", help="measure the fixed-gain limiter of the session against the plain session")
    ap.add_argument("--channels", type=int, default=None, help="measure a session of this many channels (channels='all') against "
                    "as many mono sessions, and its linked leveller and limiter against the plain one")
    args = ap.parse_args()
    n = int(args.minutes * 60 * 44100)
    rng = np.random.default_rng(0)
    t = np.arange(n, dtype=np.float32) / 44100.0
    wav = (0.05 * rng.standard_normal(n).astype(np.float32) + 0.3 * np.sin(2 * np.pi * 200.0 * t)).astype(np.float32)
    blk = max(1, int(round(args.block_seconds * 44100)))
    vf = VoiceFixer.from_state(weights.seeded_vocoder_state(1234), weights.seeded_restorer_state(4321))
    dev = vf._get_pipe().device
    cs, ov, rate = args.chunk_seconds, args.overlap_seconds, args.output_sample_rate

    if args.limiter:
        wav[::44100] = 0.9
        return limiter_leg(args, vf, wav, blk)
    if args.channels is not None:
        if not 1 <= args.channels <= 8:
            ap.error("--channels takes 1..8")
        gains = [1.0, 0.5, 0.25, 0.7, 0.35, 0.9, 0.6, 0.45][:args.channels]
        prog = np.stack([(g * np.roll(wav, 4410 * c)).astype(np.float32) for c, g in enumerate(gains)])
        return channels_leg(args, vf, prog, blk)

    def two_step():
        y44 = vf.restore_stream(wav, cs, ov, batch_size=1)
        y, (m,) = api.convert_rows(torch.from_numpy(y44).to(dev), [y44.shape[1]], [44100], rate)
        return y[:, :m].cpu().numpy()

    def session():
        first = None
        outs = []
        t0 = time.perf_counter()
        with vf.open_stream(cs, ov, batch_size=1, output_sample_rate=rate) as s:
            for a in range(0, n, blk):
                y = s.push(wav[a:a + blk])
                if first is None and y.shape[1]:
                    first = time.perf_counter() - t0
                outs.append(y)
            outs.append(s.finish())
        return np.concatenate(outs, axis=1), first

    ref = two_step()                      # warm-up of both routes (tables, banks, allocator)
    got, _ = session()
    same = bool(got.shape == ref.shape and np.array_equal(got.view(np.uint32), ref.view(np.uint32)))
    t_two, t_ses, t_first, peak = [], [], [], []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        two_step()
        t_two.append(time.perf_counter() - t0)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        t0 = time.perf_counter()
        _, first = session()
        t_ses.append(time.perf_counter() - t0)
        t_first.append(first)
        peak.append(torch.cuda.max_memory_allocated(dev) - base)
    res = {"minutes": args.minutes, "block_seconds": args.block_seconds, "chunk_seconds": cs, "overlap_seconds": ov,
           "output_sample_rate": rate, "repeats": args.repeats, "bit_identical": same,
           "two_step_s_median": statistics.median(t_two), "session_s_median": statistics.median(t_ses),
           "two_step_s": t_two, "session_s": t_ses, "first_result_s_median": statistics.median(t_first),
           "session_peak_device_bytes": max(peak), "device": torch.cuda.get_device_name(dev),
           "build_id": _lib.lib().vfx_build_id().decode()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
