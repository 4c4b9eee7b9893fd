#!/usr/bin/env python
"""What loudness normalisation costs on the device: device-event time of vfx_loudness_rows_f32 (measure +
apply, 4 launches) for one 32 x 10 s batch at 44.1 kHz and for one 30-minute row; one JSON line per case.

    python tools/loudness_bench.py [--reps 20]
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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args(argv)
    run(32, 10.0, args.reps)
    run(1, 1800.0, args.reps)


if __name__ == "__main__":
    main()
