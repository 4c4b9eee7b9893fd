#!/usr/bin/env python
"""What the streaming loudness meter costs on the device, two legs, one JSON line each:

  span    : one ops.meter_span_rows call over --seconds (default 30) of signal at --rate plus one ops.meter_report, device-event
            time, next to a device-to-device copy of the same samples -- the yardstick of a bandwidth-bound kernel -- and to one
            ops.level_span call over the same row (the leveller runs the same quarter kernel), alternating in one process; median
            of --reps per pass, --passes passes (the spread of a leg's medians is the yardstick for the difference of two legs);
            the shader clock is sampled over the timed window (bench.ClockSampler).  A further leg feeds the same samples to a
            stream._SpanMeter in blocks of one second, as a session does.
  session : a --minutes (default 5) session (VoiceFixer.open_stream, seeded weights, blocks of --block-seconds) without and with
            ``meter=True``, alternating, host to host: median of --repeats with the spread.  ``--plain-only`` times the plain
            session alone: the leg a tree without the meter can run, for the comparison across commits.

    python tools/meter_bench.py [--leg span|session|both] [--rate 48000] [--plain-only]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _spread(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts), "all": [round(t, 5) for t in ts]}


def span_leg(args):
    import numpy as np
    import torch
    import bench
    from voicefixer_amd import loudness, ops, stream
    dev = torch.device("cuda", 0)
    fs = args.rate
    n = int(args.seconds * fs)
    hop = loudness.hop_length(fs)
    rng = np.random.default_rng(3)
    env = np.repeat(10.0 ** (rng.uniform(-40.0, -10.0, n // fs + 1) / 20.0), fs)[:n]       # the level moves every second
    x = torch.from_numpy((env * rng.standard_normal(n)).astype(np.float32)).to(dev)
    out, copy = torch.empty_like(x), torch.empty_like(x)
    state, qlog = ops.meter_state(dev), torch.zeros((n // hop + 1,), dtype=torch.float64, device=dev)
    lstate = ops.level_state(dev)
    rep = [None]

    def meter():
        ops.meter_span_rows(x, 0, n, fs, 0, n, state, qlog)
        rep[0] = ops.meter_report(state, qlog, fs)

    def blocks():
        mt = stream._SpanMeter(fs)
        for a in range(0, n, fs):
            mt.feed(x[a:a + fs])
        mt.finish()

    legs = {"copy_d2d": lambda: copy.copy_(x),
            "meter_span_and_report": meter,
            "level_span": lambda: ops.level_span(x, 0, n, fs, -20.0, 0, n, out, lstate),
            "span_meter_1s_blocks": blocks}
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    med = {k: [] for k in legs}
    sampler = bench.ClockSampler(torch.cuda.current_device(), period=0.02)
    with sampler:
        t0 = time.perf_counter()
        for _ in range(args.passes):
            ev = {k: [] for k in legs}
            for _ in range(args.reps):
                for k, fn in legs.items():                          # alternating: the legs see the same machine
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    ev[k].append((e0, e1))
            torch.cuda.synchronize()
            for k in legs:
                ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev[k])
                med[k].append(round(ms[len(ms) // 2], 4))
        t1 = time.perf_counter()
    clocks = sampler.summary(t0, t1)
    mid = {k: sorted(v)[len(v) // 2] for k, v in med.items()}
    print(json.dumps({"case": "meter_span", "rate": fs, "seconds": args.seconds, "samples": n, "quarters": n // hop,
                      "reps": args.reps, "medians_ms": med, "median_ms": mid,
                      "spread_ms": {k: round(max(v) - min(v), 4) for k, v in med.items()},
                      "times_the_copy": {k: round(mid[k] / mid["copy_d2d"], 3) for k in legs if k != "copy_d2d"},
                      "report": [float(v) for v in rep[0].cpu().numpy()],
                      "sclk_mhz": clocks.get("sclk_mhz"), "clock_source": clocks.get("source")}), flush=True)


def session_leg(args):
    import numpy as np
    import torch
    import bench
    from voicefixer_amd import VoiceFixer, _lib, weights
    n = int(args.minutes * 60 * 44100)
    rng = np.random.default_rng(0)
    t = np.arange(n, dtype=np.float32) / 44100.0
    wav = (0.05 * rng.standard_normal(n).astype(np.float32) + 0.3 * np.sin(2 * np.pi * 200.0 * t)).astype(np.float32)
    blk = max(1, int(round(args.block_seconds * 44100)))
    vf = VoiceFixer.from_state(weights.seeded_vocoder_state(1234), weights.seeded_restorer_state(4321))
    dev = vf._get_pipe().device

    def session(**kw):
        outs = []
        with vf.open_stream(args.chunk_seconds, 1.0, batch_size=1, output_sample_rate=args.rate, **kw) as s:
            for a in range(0, n, blk):
                outs.append(s.push(wav[a:a + blk]))
            outs.append(s.finish())
            report = s.loudness_report if kw else None
        return sum(o.shape[1] for o in outs), report

    kw = {} if args.plain_only else dict(meter=True)
    session()                                 # warm-up of both routes
    m, report = session(**kw)
    t_plain, t_meter = [], []
    sampler = bench.ClockSampler(torch.cuda.current_device(), period=0.05)
    with sampler:
        t0 = time.perf_counter()
        for _ in range(args.repeats):
            for ts, k in ((t_plain, {}), (t_meter, kw)):
                torch.cuda.synchronize()
                a = time.perf_counter()
                session(**k)
                ts.append(time.perf_counter() - a)
        t1 = time.perf_counter()
    clocks = sampler.summary(t0, t1)
    mp, mm = statistics.median(t_plain), statistics.median(t_meter)
    print(json.dumps({"case": "meter_session", "plain_only": bool(args.plain_only), "minutes": args.minutes,
                      "block_seconds": args.block_seconds, "chunk_seconds": args.chunk_seconds, "output_sample_rate": args.rate,
                      "samples_out": m, "repeats": args.repeats, "loudness_report": report, "plain_s": _spread(t_plain),
                      ("plain_again_s" if args.plain_only else "meter_s"): _spread(t_meter), "second_over_first": mm / mp - 1.0,
                      "sclk_mhz": clocks.get("sclk_mhz"), "clock_source": clocks.get("source"),
                      "device": torch.cuda.get_device_name(dev), "build_id": _lib.lib().vfx_build_id().decode()}), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--leg", choices=["span", "session", "both"], default="both")
    ap.add_argument("--rate", type=int, default=48000, help="the rate the meter runs at (the session's output rate)")
    ap.add_argument("--seconds", type=float, default=30.0, help="span leg: seconds of signal in one call")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--minutes", type=float, default=5.0, help="session leg: length of the input")
    ap.add_argument("--block-seconds", type=float, default=1.0)
    ap.add_argument("--chunk-seconds", type=float, default=30.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--plain-only", action="store_true", help="session leg: the plain session twice, no meter (any tree runs it)")
    args = ap.parse_args(argv)
    if args.leg in ("span", "both"):
        span_leg(args)
    if args.leg in ("session", "both"):
        session_leg(args)


if __name__ == "__main__":
    main()
