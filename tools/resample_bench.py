#!/usr/bin/env python
"""What rate conversion costs on the device and what it saves on the host.

    python tools/resample_bench.py kernels [--reps 5]      # vfx_resample_rows_f32 on 32 x 10 s rows for every rate pair
                                                           # (run it under `rocprofv3 --kernel-trace --stats -- ...` for
                                                           # the per-kernel table; HIP-event times are printed as well)
    python tools/resample_bench.py folder [--files 256]    # restore_folder on a synthetic folder of 10 s PCM16 files at
                                                           # 16 kHz (tmpfs): host vs device resampling, default io_threads
                                                           # and io_threads = 2; one JSON line per run

Both use the seeded weights (weights.seeded_*): the device stage costs what it costs with real checkpoints.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAIRS = [(8000, 44100), (16000, 44100), (32000, 44100), (22050, 44100), (24000, 44100), (48000, 44100), (96000, 44100),
         (44100, 48000), (44100, 16000)]


def kernels(args):
    import torch
    from voicefixer_amd import audio_io, ops
    dev = torch.device("cuda", 0)
    B = args.batch
    g = torch.Generator().manual_seed(1)
    for sr_in, sr_out in PAIRS:
        up, down = audio_io.rate_ratio(sr_in, sr_out)
        n = int(args.seconds * sr_in)
        ny = audio_io.converted_length(n, sr_in, sr_out)
        x = (torch.rand((B, n), generator=g) * 2 - 1).to(dev)
        y = torch.empty((B, ny), device=dev)
        n_rows = torch.full((B,), n, dtype=torch.int32, device=dev)
        ops.resample_rows(x, n_rows, y, up, down)            # warm-up (bank upload)
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * args.reps)]
        for k in range(args.reps):
            ev[2 * k].record()
            ops.resample_rows(x, n_rows, y, up, down)
            ev[2 * k + 1].record()
        torch.cuda.synchronize()
        ms = sorted(ev[2 * k].elapsed_time(ev[2 * k + 1]) for k in range(args.reps))
        _, J, _ = ops.resample_bank(dev, up, down)
        print(json.dumps({"pair": [sr_in, sr_out], "up": up, "down": down, "J": J, "rows": B, "seconds": args.seconds,
                          "outputs": B * ny, "median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4),
                          "gmac_per_s": round(B * ny * J / (ms[len(ms) // 2] * 1e-3) / 1e9, 1)}), flush=True)


def folder(args):
    import torch
    from scipy.io import wavfile
    import voicefixer_amd
    from voicefixer_amd import weights, dist as vdist
    base = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        ind = os.path.join(base, "in")
        os.makedirs(ind)
        rng = np.random.default_rng(0)
        n = int(16000 * args.seconds)
        t = np.arange(n) / 16000.0
        for i in range(args.files):
            x = 0.3 * np.sin(2 * np.pi * (120 + i) * t) * (0.6 + 0.4 * np.sin(2 * np.pi * 3 * t)) + 0.02 * rng.standard_normal(n)
            wavfile.write(os.path.join(ind, "f%04d.wav" % i), 16000, np.round(x * 32767).astype(np.int16))
        vf = voicefixer_amd.VoiceFixer.from_state(weights.seeded_vocoder_state(1234), weights.seeded_restorer_state(4321))
        warm = os.path.join(base, "warm")
        os.makedirs(warm)
        for f in sorted(os.listdir(ind))[:32]:
            shutil.copy(os.path.join(ind, f), warm)
        for dev_rs in (False, True):          # warm-up: both paths (kernels, banks, pinned pools)
            vf.restore_folder(warm, os.path.join(base, "wout"), resample_on_device=dev_rs)
        default_threads = vdist.default_io_threads(1)
        for threads in (default_threads, 2):
            for dev_rs in (False, True):
                out = os.path.join(base, "out")
                shutil.rmtree(out, ignore_errors=True)
                st = {}
                torch.cuda.synchronize()
                vf.restore_folder(ind, out, io_threads=threads, stats=st, resample_on_device=dev_rs)
                print(json.dumps({"resample_on_device": dev_rs, "io_threads": threads, "files": st["files"],
                                  "audio_s": round(st["audio_s"], 1), "wall_s": round(st["wall_s"], 3),
                                  "x_real_time": round(st["audio_s"] / st["wall_s"], 1),
                                  "decode_worker_s": round(st["decode_worker_s"], 3),
                                  "resample_worker_s": round(st["resample_worker_s"], 3),
                                  "encode_worker_s": round(st["encode_worker_s"], 3),
                                  "device_waited_for_decode_s": round(st["device_waited_for_decode_s"], 3),
                                  "host_cores": len(os.sched_getaffinity(0)), "failed": len(st["failed"])}), flush=True)
    finally:
        shutil.rmtree(base, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    k = sub.add_parser("kernels")
    k.add_argument("--batch", type=int, default=32)
    k.add_argument("--seconds", type=float, default=10.0)
    k.add_argument("--reps", type=int, default=5)
    f = sub.add_parser("folder")
    f.add_argument("--files", type=int, default=256)
    f.add_argument("--seconds", type=float, default=10.0)
    args = ap.parse_args()
    kernels(args) if args.cmd == "kernels" else folder(args)


if __name__ == "__main__":
    main()
