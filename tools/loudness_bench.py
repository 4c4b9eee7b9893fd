#!/usr/bin/env python
"""What loudness normalisation costs on the device: device-event time of vfx_loudness_rows_f32 (measure +
apply, 4 launches) for one 32 x 10 s batch at 44.1 kHz and for one 30-minute row; one JSON line per case.
``--true-peak`` times, for the same two shapes and in one process, alternating: the sample-peak
measurement (3 launches), the true-peak measurement (the same + the fused oversample-and-reduce kernel), and what the
true peak cost before that kernel existed -- ops.resample_rows at up = R, down = 1 into an R-times-wider scratch, then
abs().amax per row.  Median of ``--reps`` per pass, ``--passes`` passes: the spread of a leg's medians is the yardstick
for the difference between two legs.  The shader clock is sampled over the timed window (bench.ClockSampler).
``--channels C`` times, for 32 rows of 10 s cut into programmes of C channels (32 // C of them and one of
the remainder: 16 stereo programmes at C = 2, 5 x 6 + 2 at C = 6), alternating in one process: ops.loudness_groups against
ops.loudness_rows(true_peak=True) on the same rows, measuring only and measuring + applying.
``--limiter`` times, for the same two shapes, alternating in one process: (a) the static true-peak
normalisation, (b) the limiter on rows the ceiling does not bind, (c) the limiter on rows bound by one click per second, (d)
the limiter on full-scale plateaus (a sine at fs / 4 under a ceiling of -6 dBTP: every tile does the full work).

    python tools/loudness_bench.py [--reps 20]
    python tools/loudness_bench.py --true-peak [--reps 10] [--passes 3]
    python tools/loudness_bench.py --channels 2 [--reps 10] [--passes 3]
    python tools/loudness_bench.py --limiter [--reps 10] [--passes 3]
    rocprofv3 --kernel-trace --stats -- python tools/loudness_bench.py     # per-kernel table
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(B, seconds, reps, fs=44100):
    import torch
    from voicefixer_amd import ops
    dev = torch.device("cuda", 0)
    n = int(seconds * fs)
    g = torch.Generator().manual_seed(3)
    x = (0.1 * torch.randn((B, n), generator=g)).to(dev)
    y = torch.empty_like(x)
    n_rows = torch.full((B,), n, dtype=torch.int32, device=dev)
    ops.loudness_rows(x, n_rows, fs, target=-16.0, out=y)           # warm-up (plan upload, code objects)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * reps)]
    for k in range(reps):
        ev[2 * k].record()
        ops.loudness_rows(x, n_rows, fs, target=-16.0, out=y)
        ev[2 * k + 1].record()
    torch.cuda.synchronize()
    ms = sorted(ev[2 * k].elapsed_time(ev[2 * k + 1]) for k in range(reps))
    print(json.dumps({"rows": B, "seconds": seconds, "rate": fs, "samples": B * n, "median_ms": round(ms[len(ms) // 2], 4),
                      "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}), flush=True)


def run_true_peak(B, seconds, reps, passes, fs=44100):
    import time
    import torch
    import bench
    from voicefixer_amd import loudness, ops
    dev = torch.device("cuda", 0)
    n = int(seconds * fs)
    R = loudness.oversampling(fs)
    g = torch.Generator().manual_seed(3)
    x = (0.1 * torch.randn((B, n), generator=g)).to(dev)
    n_rows = torch.full((B,), n, dtype=torch.int32, device=dev)
    wide = torch.empty((B, R * n), device=dev)                      # the composition's scratch: R times the input

    def composed():
        ops.resample_rows(x, n_rows, wide, R, 1)
        return wide.abs().amax(dim=1)

    legs = {"sample_peak_measure": lambda: ops.loudness_rows(x, n_rows, fs),
            "true_peak_measure": lambda: ops.loudness_rows(x, n_rows, fs, true_peak=True),
            "resample_rows_then_amax": composed}
    for fn in legs.values():                                        # warm-up: bank / plan uploads, code objects
        fn()
    a = ops.loudness_rows(x, n_rows, fs, true_peak=True)[:, 3].float()
    b = torch.maximum(composed(), x.abs().amax(dim=1))
    agree = float(((a - b).abs() / b).max())                        # the two ways measure the same peak
    torch.cuda.synchronize()
    med = {k: [] for k in legs}
    sampler = bench.ClockSampler(torch.cuda.current_device(), period=0.02)
    with sampler:
        t0 = time.perf_counter()
        for _ in range(passes):
            ev = {k: [] for k in legs}
            for _ in range(reps):
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
    macs = B * n * R * ops.true_peak_bank(dev, R)[1]
    fused = mid["true_peak_measure"] - mid["sample_peak_measure"]
    print(json.dumps({"case": "true_peak", "rows": B, "seconds": seconds, "rate": fs, "R": R, "samples": B * n, "reps": reps,
                      "medians_ms": med, "median_ms": mid,
                      "spread_ms": {k: round(max(v) - min(v), 4) for k, v in med.items()},
                      "fused_kernel_ms": round(fused, 4), "fused_kernel_tmacs": round(macs / fused / 1e9, 3) if fused > 0 else None,
                      "composition_tmacs": round(macs / mid["resample_rows_then_amax"] / 1e9, 3),
                      "scratch_bytes_composition": wide.numel() * 4,
                      "scratch_bytes_fused": int(_true_peak_bytes(B, n, R, dev)), "max_rel_disagreement": agree,
                      "sclk_mhz": clocks.get("sclk_mhz"), "clock_source": clocks.get("source")}), flush=True)


def run_channels(C, B, seconds, reps, passes, fs=44100):
    import time
    import torch
    import bench
    from voicefixer_amd import ops
    dev = torch.device("cuda", 0)
    n = int(seconds * fs)
    groups = [C] * (B // C) + ([B % C] if B % C else [])
    g = torch.Generator().manual_seed(3)
    x = (0.1 * torch.randn((B, n), generator=g)).to(dev)
    y = torch.empty_like(x)
    n_rows = torch.full((B,), n, dtype=torch.int32, device=dev)
    lens = [n] * B       # (the grouped legs take the lengths as a list: checked on the host, uploaded once with the group
    #                       starts and weights by the warm-up call and cached -- no copy and no read-back inside the timed
    #                       region, as in the per-row legs, so the difference between two legs is the kernels')
    legs = {"rows_measure": lambda: ops.loudness_rows(x, n_rows, fs, true_peak=True),
            "groups_measure": lambda: ops.loudness_groups(x, lens, groups, fs),
            "rows_apply": lambda: ops.loudness_rows(x, n_rows, fs, target=-23.0, out=y, true_peak=True),
            "groups_apply": lambda: ops.loudness_groups(x, lens, groups, fs, target=-23.0, out=y)}
    for fn in legs.values():                                        # warm-up: bank / plan / group uploads, code objects
        fn()
    torch.cuda.synchronize()
    med = {k: [] for k in legs}
    sampler = bench.ClockSampler(torch.cuda.current_device(), period=0.02)
    with sampler:
        t0 = time.perf_counter()
        for _ in range(passes):
            ev = {k: [] for k in legs}
            for _ in range(reps):
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
    print(json.dumps({"case": "channels", "channels": C, "groups": groups, "rows": B, "seconds": seconds, "rate": fs,
                      "reps": reps, "medians_ms": med, "median_ms": mid,
                      "spread_ms": {k: round(max(v) - min(v), 4) for k, v in med.items()},
                      "groups_minus_rows_measure_ms": round(mid["groups_measure"] - mid["rows_measure"], 4),
                      "groups_minus_rows_apply_ms": round(mid["groups_apply"] - mid["rows_apply"], 4),
                      "sclk_mhz": clocks.get("sclk_mhz"), "clock_source": clocks.get("source")}), flush=True)


def run_limiter(B, seconds, reps, passes, fs=44100, only=None):
    import math
    import time
    import torch
    import bench
    from voicefixer_amd import ops
    dev = torch.device("cuda", 0)
    n = int(seconds * fs)
    g = torch.Generator().manual_seed(3)
    quiet = (0.1 * torch.randn((B, n), generator=g)).to(dev)
    clicks = quiet.clone()
    clicks[:, fs // 2::fs] = 2.0                                    # one click per second
    k = torch.arange(n, dtype=torch.float64)
    plateau = torch.sin(2 * math.pi * k / 4 + math.pi / 4).float().to(dev).repeat(B, 1).contiguous()
    y = torch.empty_like(quiet)
    n_rows = torch.full((B,), n, dtype=torch.int32, device=dev)
    legs = {"a_static_true_peak": lambda: ops.loudness_rows(quiet, n_rows, fs, target=-23.0, out=y, true_peak=True),
            "b_limiter_not_bound": lambda: ops.loudness_limit(quiet, n_rows, fs, -23.0, -1.0, True, 3.0, out=y),
            "c_limiter_clicks": lambda: ops.loudness_limit(clicks, n_rows, fs, -23.0, -1.0, True, 3.0, out=y),
            "d_limiter_plateau": lambda: ops.loudness_limit(plateau, n_rows, fs, -1.0, -6.0, True, 3.0, out=y)}
    if only:                                                        # (a per-kernel table of one leg: rocprofv3 around this)
        legs = {name: fn for name, fn in legs.items() if name[0] in only}
    rec = {name: fn().cpu() for name, fn in legs.items()}               # warm-up: bank / plan uploads, code objects
    lim = [name for name in legs if name[0] != "a"]
    want = {"b_limiter_not_bound": 0, "c_limiter_clicks": B, "d_limiter_plateau": B}
    bound = {name: int(rec[name][:, 4].sum()) for name in lim}
    assert bound == {name: want[name] for name in lim}, bound
    torch.cuda.synchronize()
    med = {name: [] for name in legs}
    sampler = bench.ClockSampler(torch.cuda.current_device(), period=0.02)
    with sampler:
        t0 = time.perf_counter()
        for _ in range(passes):
            ev = {name: [] for name in legs}
            for _ in range(reps):
                for name, fn in legs.items():                       # alternating: the legs see the same machine
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    ev[name].append((e0, e1))
            torch.cuda.synchronize()
            for name in legs:
                ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev[name])
                med[name].append(round(ms[len(ms) // 2], 4))
        t1 = time.perf_counter()
    clocks = sampler.summary(t0, t1)
    mid = {name: sorted(v)[len(v) // 2] for name, v in med.items()}
    print(json.dumps({"case": "limiter", "rows": B, "seconds": seconds, "rate": fs, "samples": B * n, "reps": reps,
                      "medians_ms": med, "median_ms": mid,
                      "spread_ms": {name: round(max(v) - min(v), 4) for name, v in med.items()},
                      "min_g": {name: round(float(rec[name][:, 5].min()), 4) for name in lim},
                      "trim": {name: round(float(rec[name][:, 6].min()), 7) for name in lim},
                      "sclk_mhz": clocks.get("sclk_mhz"), "clock_source": clocks.get("source")}), flush=True)


def _true_peak_bytes(B, n, R, dev):
    from voicefixer_amd import _lib, ops
    return _lib.lib().vfx_true_peak_workspace_bytes(B, n, R, ops.true_peak_bank(dev, R)[1])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--true-peak", action="store_true", help="time the true-peak legs instead (DESIGN.md 3.11)")
    ap.add_argument("--passes", type=int, default=3, help="--true-peak / --channels / --limiter: passes of --reps alternating repetitions")
    ap.add_argument("--channels", type=int, default=0, metavar="C",
                    help="time programmes of C channels (1..8) against the per-row call instead (DESIGN.md 3.13)")
    ap.add_argument("--limiter", action="store_true", help="time the look-ahead limiter's legs instead (DESIGN.md 3.14)")
    ap.add_argument("--legs", default=None, metavar="LETTERS", help="--limiter: only these legs, e.g. c or ab (default: all four)")
    ap.add_argument("--shape", choices=["batch", "long", "both"], default="both",
                    help="--limiter: 32 x 10 s, one 30-minute row, or both (default)")
    args = ap.parse_args(argv)
    if args.limiter:
        if args.shape in ("batch", "both"):
            run_limiter(32, 10.0, args.reps, args.passes, only=args.legs)
        if args.shape in ("long", "both"):
            run_limiter(1, 1800.0, args.reps, args.passes, only=args.legs)
        return
    if args.channels:
        if not 1 <= args.channels <= 8:
            ap.error("--channels takes 1..8")
        run_channels(args.channels, 32, 10.0, args.reps, args.passes)
        return
    if args.true_peak:
        run_true_peak(32, 10.0, args.reps, args.passes)
        run_true_peak(1, 1800.0, args.reps, args.passes)
        return
    run(32, 10.0, args.reps)
    run(1, 1800.0, args.reps)


if __name__ == "__main__":
    main()
