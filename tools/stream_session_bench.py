#!/usr/bin/env python
"""The push-style session against the two-step route it replaces, host to host, in one process:

  session : VoiceFixer.open_stream(batch_size=1, output_sample_rate=RATE), the input pushed in blocks of BLOCK seconds
  two-step: VoiceFixer.restore_stream(batch_size=1) on the whole input, then a whole-row convert_rows to RATE

Median of --repeats runs each (alternating), the session's device-memory high-water mark above what the model holds, and
the time from the first push to the first non-empty result.  Prints one JSON line.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=5.0)
    ap.add_argument("--block-seconds", type=float, default=1.0)
    ap.add_argument("--chunk-seconds", type=float, default=30.0)
    ap.add_argument("--overlap-seconds", type=float, default=1.0)
    ap.add_argument("--output-sample-rate", type=int, default=48000)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    n = int(args.minutes * 60 * 44100)
    rng = np.random.default_rng(0)
    t = np.arange(n, dtype=np.float32) / 44100.0
    wav = (0.05 * rng.standard_normal(n).astype(np.float32) + 0.3 * np.sin(2 * np.pi * 200.0 * t)).astype(np.float32)
    blk = max(1, int(round(args.block_seconds * 44100)))
    vf = VoiceFixer.from_state(weights.seeded_vocoder_state(1234), weights.seeded_restorer_state(4321))
    dev = vf._get_pipe().device
    cs, ov, rate = args.chunk_seconds, args.overlap_seconds, args.output_sample_rate

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
