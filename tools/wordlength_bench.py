#!/usr/bin/env python
"""What the word-length reduction costs on the device: device-event time of vfx_quantize_rows_f32 (one kernel
behind the clear of its result) for one 32 x 10 s batch at 44.1 kHz and for one 30-minute row, at 16 and 24 bits and for each
dither, next to a device-to-device copy of the same input bytes -- the yardstick of a bandwidth-bound kernel -- all legs
alternating in one process.  Median of ``--reps`` per pass, ``--passes`` passes: the spread of a leg's medians is the yardstick
for the difference between two legs.  The shader clock is sampled over the timed window (bench.ClockSampler).  ``--n0 K`` starts
every row at sample K of its file (K % 4 != 0: a thread's four samples straddle two Philox blocks).
``--folder N`` times a folder job instead: N files of ``--seconds`` (default 256 x 4 s) through ``restore_folder`` with seeded
weights, once on the default path (float32 rows cross, the encode workers truncate to 16 bits) and once with ``bit_depth=16,
dither="none"`` (PCM crosses, the workers only write), alternating ``--passes`` times: wall time and ``encode_worker_s`` of each.

    python tools/wordlength_bench.py [--reps 10] [--passes 3] [--n0 0]
    python tools/wordlength_bench.py --folder 256 [--seconds 4] [--passes 2]
    rocprofv3 --kernel-trace --stats -- python tools/wordlength_bench.py     # per-kernel table
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(B, seconds, reps, passes, start=0, fs=44100):
    import time
    import torch
    import bench
    from voicefixer_amd import ops, wordlength
    dev = torch.device("cuda", 0)
    n = int(seconds * fs)
    g = torch.Generator().manual_seed(3)
    x = (0.1 * torch.randn((B, n), generator=g)).to(dev)
    copy = torch.empty_like(x)
    n_rows = torch.full((B,), n, dtype=torch.int32, device=dev)
    n0 = torch.full((B,), int(start), dtype=torch.int64, device=dev) if start else None
    outs = {16: torch.empty((B, n), dtype=torch.int16, device=dev), 24: torch.empty((B, n), dtype=torch.int32, device=dev)}
    legs = {"copy_d2d": lambda: copy.copy_(x)}
    for bits in wordlength.DEPTHS:
        for kind in wordlength.DITHERS:
            legs["q%d_%s" % (bits, kind)] = (lambda b=bits, k=kind: ops.quantize_rows(x, n_rows, b, k, 1, n0=n0, out=outs[b]))
    for fn in legs.values():                                        # warm-up: code objects
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
    moved = {"copy_d2d": 8}
    moved.update({k: 4 + (2 if k.startswith("q16") else 4) for k in legs if k != "copy_d2d"})       # bytes per sample
    print(json.dumps({"case": "wordlength", "rows": B, "seconds": seconds, "rate": fs, "samples": B * n, "n0": int(start),
                      "reps": reps, "medians_ms": med, "median_ms": mid,
                      "spread_ms": {k: round(max(v) - min(v), 4) for k, v in med.items()},
                      "times_the_copy": {k: round(mid[k] / mid["copy_d2d"], 3) for k in legs if k != "copy_d2d"},
                      "gb_per_s": {k: round(B * n * moved[k] / mid[k] / 1e6, 1) for k in legs},
                      "sclk_mhz": clocks.get("sclk_mhz"), "clock_source": clocks.get("source")}), flush=True)


def run_folder(files, seconds, passes, batch_size=32, fs=44100):
    import shutil
    import tempfile
    import numpy as np
    import voicefixer_amd
    from voicefixer_amd import audio_io, weights
    vf = voicefixer_amd.VoiceFixer.from_state(weights.seeded_vocoder_state(1234), weights.seeded_restorer_state(4321))
    root = tempfile.mkdtemp(prefix="wordlength_bench_")
    try:
        ind = os.path.join(root, "in")
        os.makedirs(ind)
        rng = np.random.default_rng(5)
        n = int(seconds * fs)
        for k in range(files):
            audio_io.save_wave((0.1 * rng.standard_normal(n)).astype(np.float32)[None], os.path.join(ind, "f%04d.wav" % k))
        legs = {"default_float_rows": {}, "bit_depth_16_none": {"bit_depth": 16, "dither": "none"}}
        vf.restore_folder(ind, os.path.join(root, "warm"), batch_size=batch_size)            # warm-up: code objects, pools
        rec = {k: [] for k in legs}
        for p in range(passes):
            for name, kw in legs.items():                           # alternating
                st = {}
                vf.restore_folder(ind, os.path.join(root, "%s_%d" % (name, p)), batch_size=batch_size, stats=st, **kw)
                assert st["files"] == files and not st["failed"], st["failed"]
                rec[name].append({"wall_s": round(st["wall_s"], 4), "encode_worker_s": round(st["encode_worker_s"], 4),
                                  "decode_worker_s": round(st["decode_worker_s"], 4)})
        print(json.dumps({"case": "wordlength_folder", "files": files, "seconds": seconds, "batch_size": batch_size,
                          "io_threads": st["io_threads"], "passes": rec,
                          "median": {name: {f: sorted(r[f] for r in v)[len(v) // 2] for f in v[0]} for name, v in rec.items()}}),
              flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--passes", type=int, default=3, help="passes of --reps alternating repetitions (--folder: alternating jobs)")
    ap.add_argument("--n0", type=int, default=0, metavar="K", help="absolute index of every row's first sample (default 0)")
    ap.add_argument("--shape", choices=["batch", "long", "both"], default="both", help="32 x 10 s, one 30-minute row, or both (default)")
    ap.add_argument("--folder", type=int, default=0, metavar="N", help="time a restore_folder job of N files instead")
    ap.add_argument("--seconds", type=float, default=4.0, help="--folder: length of every file (default 4 s)")
    args = ap.parse_args(argv)
    if args.folder:
        run_folder(args.folder, args.seconds, args.passes)
        return
    if args.shape in ("batch", "both"):
        run(32, 10.0, args.reps, args.passes, args.n0)
    if args.shape in ("long", "both"):
        run(1, 1800.0, args.reps, args.passes, args.n0)


if __name__ == "__main__":
    main()
