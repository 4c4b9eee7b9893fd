#!/usr/bin/env python
"""What the streaming loudness leveller costs on the device, two legs, one JSON line each:

  span    : one ops.level_span call over --seconds (default 30) of output at --rate, device-event time, next to a device-to-device
            copy of the same samples -- the yardstick of a bandwidth-bound kernel -- alternating in one process; median of --reps
            per pass, --passes passes (the spread of a leg's medians is the yardstick for the difference of two legs); the shader
            clock is sampled over the timed window (bench.ClockSampler).  A second pair of legs feeds the same samples to an
            api._SpanLeveller in blocks of one second, as a session does.
  session : a --minutes (default 5) session (VoiceFixer.open_stream, seeded weights, blocks of --block-seconds) without and with
            ``leveller=-20``, alternating, host to host: median of --repeats with the spread.

    python tools/leveller_bench.py [--leg span|session|both] [--rate 48000]
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
    from voicefixer_amd import api, loudness, ops
    dev = torch.device("cuda", 0)
    fs = args.rate
    n = int(args.seconds * fs)
    rng = np.random.default_rng(3)
    env = np.repeat(10.0 ** (rng.uniform(-40.0, -10.0, n // fs + 1) / 20.0), fs)[:n]       # the level moves every second
    x = torch.from_numpy((env * rng.standard_normal(n)).astype(np.float32)).to(dev)
    out, copy = torch.empty_like(x), torch.empty_like(x)
    state = ops.level_state(dev)

    def blocks():
        lv = api._SpanLeveller(fs, -20.0)
        for a in range(0, n, fs):
            lv.feed(x[a:a + fs])
        lv.finish(dev)

    legs = {"copy_d2d": lambda: copy.copy_(x),
            "level_span": lambda: ops.level_span(x, 0, n, fs, -20.0, 0, n, out, state),
            "span_leveller_1s_blocks": blocks}
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
    rec = state[:7].cpu().numpy()
    print(json.dumps({"case": "leveller_span", "rate": fs, "seconds": args.seconds, "samples": n, "quarters": n // loudness.hop_length(fs),
                      "reps": args.reps, "medians_ms": med, "median_ms": mid,
                      "spread_ms": {k: round(max(v) - min(v), 4) for k, v in med.items()},
                      "times_the_copy": {k: round(mid[k] / mid["copy_d2d"], 3) for k in legs if k != "copy_d2d"},
                      "record": {"min_gain_db": float(rec[0]), "max_gain_db": float(rec[1]), "anchors": int(rec[2]), "gated": int(rec[3])},
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
            stats = s.leveller_stats
        return sum(o.shape[1] for o in outs), stats

    kw = dict(leveller=-20.0)
    session()                                 # warm-up of both routes
    m, stats = session(**kw)
    t_plain, t_lev = [], []
    sampler = bench.ClockSampler(torch.cuda.current_device(), period=0.05)
    with sampler:
        t0 = time.perf_counter()
        for _ in range(args.repeats):
            for ts, k in ((t_plain, {}), (t_lev, kw)):
                torch.cuda.synchronize()
                a = time.perf_counter()
                session(**k)
                ts.append(time.perf_counter() - a)
        t1 = time.perf_counter()
    clocks = sampler.summary(t0, t1)
    mp, ml = statistics.median(t_plain), statistics.median(t_lev)
    print(json.dumps({"case": "leveller_session", "minutes": args.minutes, "block_seconds": args.block_seconds,
                      "chunk_seconds": args.chunk_seconds, "output_sample_rate": args.rate, "samples_out": m, "repeats": args.repeats,
                      "leveller_stats": stats, "plain_s": _spread(t_plain), "leveller_s": _spread(t_lev),
                      "leveller_over_plain": ml / mp - 1.0, "sclk_mhz": clocks.get("sclk_mhz"), "clock_source": clocks.get("source"),
                      "device": torch.cuda.get_device_name(dev), "build_id": _lib.lib().vfx_build_id().decode()}), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--leg", choices=["span", "session", "both"], default="both")
    ap.add_argument("--rate", type=int, default=48000, help="the output rate the leveller runs at")
    ap.add_argument("--seconds", type=float, default=30.0, help="span leg: seconds of output in one call")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--minutes", type=float, default=5.0, help="session leg: length of the input")
    ap.add_argument("--block-seconds", type=float, default=1.0)
    ap.add_argument("--chunk-seconds", type=float, default=30.0)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args(argv)
    if args.leg in ("span", "both"):
        span_leg(args)
    if args.leg in ("session", "both"):
        session_leg(args)


if __name__ == "__main__":
    main()
