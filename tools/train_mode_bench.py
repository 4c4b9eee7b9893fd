#!/usr/bin/env python
"""Cost of mode 2 (train-mode BatchNorm + seeded dropout) against mode 0 on one MI355X: ``VoiceFixer.restore_batches`` on
batches of 32 x 10 s (bench.py's synthetic speech-like input, seeded weights), alternating the two modes, plus the
achieved bandwidth of ``vfx_bn_stats_f32`` on a level-0 UNet map of that batch (32 channels x 1024 rows x 127 columns).
Prints one JSON line and, with --out, writes it there (profiles/).  Shader clock / socket power are sampled during
every timed region as ``bench.py --full`` samples them.

    python tools/train_mode_bench.py --steps 3 --warmup 1 --out profiles/train_mode_b32.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402  (ClockSampler, synth_batch)
from voicefixer_amd import VoiceFixer, _lib, ops, weights  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    vf = VoiceFixer.from_state(weights.seeded_vocoder_state(1234), weights.seeded_restorer_state(4321))
    n = int(args.seconds * 44100)
    host = bench.synth_batch(args.batch, n, 0, "cpu").float().contiguous().pin_memory()
    item = (list(range(args.batch)), "ragged", host, [n] * args.batch)

    def step(mode):
        for _ in vf.restore_batches(iter([item]), mode=mode, seed=args.seed if mode == 2 else None):
            pass

    for mode in (0, 2):
        for _ in range(args.warmup):
            step(mode)
    torch.cuda.synchronize()
    ms = {0: [], 2: []}
    clocks = {}
    sampler = bench.ClockSampler(0)
    with sampler:
        for _ in range(args.steps):
            for mode in (0, 2):
                t0 = time.perf_counter()
                step(mode)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                ms[mode].append(1e3 * (t1 - t0))
                clocks.setdefault("mode%d" % mode, []).append((t0, t1))
    clocks = {k: sampler.summary(v[-1][0], v[-1][1]) for k, v in clocks.items()}

    # vfx_bn_stats_f32 on a level-0 map of the batch (Tp = 1024 rows for 10 s): bytes of the valid region read once
    T = 1 + n // 441
    Tp = (T + 63) // 64 * 64
    x = ops.guarded(args.batch, 32, Tp * 128, 128 + 8, "cuda")
    x.normal_()
    g, b = torch.ones(32, device="cuda"), torch.zeros(32, device="cuda")
    sc, sh = torch.empty(args.batch * 32, device="cuda"), torch.empty(args.batch * 32, device="cuda")
    for _ in range(3):
        ops.bn_stats(x, Tp * 128, 7, g, b, sc, sh)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 20
    e0.record()
    for _ in range(reps):
        ops.bn_stats(x, Tp * 128, 7, g, b, sc, sh)
    e1.record()
    torch.cuda.synchronize()
    stats_ms = e0.elapsed_time(e1) / reps
    nbytes = args.batch * 32 * Tp * 128 * 4

    best = {m: min(v) for m, v in ms.items()}
    line = {"what": "restore_batches, batch %d x %.0f s, mode 2 (seed %d) vs mode 0, alternating" % (args.batch, args.seconds, args.seed),
            "build_id": _lib.lib().vfx_build_id().decode(), "device": torch.cuda.get_device_name(0),
            "ms_per_batch": {"mode0": [round(v, 1) for v in ms[0]], "mode2": [round(v, 1) for v in ms[2]]},
            "best_ms": {"mode0": round(best[0], 1), "mode2": round(best[2], 1)},
            "mode2_over_mode0": round(best[2] / best[0], 3),
            "bn_stats_level0": {"shape": [args.batch, 32, Tp, 127], "ms": round(stats_ms, 4),
                                "gb_per_s": round(nbytes / (stats_ms * 1e-3) / 1e9, 1)},
            "clocks": clocks}
    print(json.dumps(line))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(line, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
