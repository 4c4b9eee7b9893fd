#!/usr/bin/env python
"""Every conv-family launch of one batch through the path: operator, shape, the kernel family that ran it, tile, whether
split-K ran, milliseconds
(development; GPU).   python tools/launch_table.py [--batch 32] [--seconds 10] [--taps-only]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from voicefixer_amd import engine, launch_record, ops, weights  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--taps-only", action="store_true", help="only the launches that ran on the first-generation conv_taps_kernel")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = int(round(args.seconds * 44100))
    pipe = engine.Pipeline(weights.seeded_vocoder_state(1234), weights.seeded_restorer_state(4321), dev)
    wav = bench.synth_batch(args.batch, n, 1000, dev)
    pipe.restore(wav, n)
    torch.cuda.synchronize()
    ops.PROFILE = []
    with launch_record.LaunchRecorder() as rec:
        pipe.restore(wav, n)
        torch.cuda.synchronize()
    prof, ops.PROFILE = ops.PROFILE, None
    assert sum(len(r["prof"]) for r in rec.records) == len([p for p in prof if p[0] != -1])
    tot = 0.0
    for r in rec.records:
        fam = launch_record.family(r["code"])
        if args.taps_only and not fam.startswith("conv_taps"):
            continue
        for (tile, macs, e0, e1) in r["prof"]:
            ms = e0.elapsed_time(e1)
            tot += ms
            print("%-15s %-44s %-18s tile %3dx%-3d split-K %-3s %7.3f ms %7.1f TFLOP/s"
                  % (r["op"], launch_record.shape_text(r), fam, r["BM"], r["BL"],
                     "yes" if fam.startswith("conv_taps") and launch_record.split_k(r) else "no", ms, 2e-9 * macs / ms))
    print("total %.3f ms" % tot)


if __name__ == "__main__":
    main()
