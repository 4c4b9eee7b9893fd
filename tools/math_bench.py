#!/usr/bin/env python
"""f32 vs bf16x3 vs f16 contraction arithmetic on ONE device, in ONE process: the workload of bench.py's default (batch 32 x
10 s synthetic utterances, seeded random weights, mode 0), host to host (H2D of the batch, Pipeline.restore, D2H of the result).

    python tools/math_bench.py [--batch 32] [--seconds 10] [--steps 5] [--warmup 2] [--rounds 2] [--out FILE]

The arithmetics alternate round by round (f32, bf16x3, f16, f32, ...) so that clock drift is shared.  Per arithmetic:
  step_ms       host-to-host milliseconds per batch (median over rounds of the mean over --steps steps);
  resstack_ms   the 48 launches of the ResStacks with C >= 128 (two per layer, 24 layers), per step, from HIP events on a
                separate profiled pass (ops.PROFILE): their sum and the per-launch list in launch order;
  clocks        shader clock and board power while the timed steps ran (bench.ClockSampler).
bench.py itself is not changed: its --math choices stay f32 / bf16x3."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from bench import ClockSampler, synth_batch, SR  # noqa: E402
from voicefixer_amd import engine, ops, weights  # noqa: E402
from voicefixer_amd.api import VoiceFixer  # noqa: E402

MATHS = ("f32", "bf16x3", "f16")
STAGE_LAUNCHES = 17          # per UpsampleNet stage: one transposed convolution, then 16 ResStack convolutions (unfused form)
WIDE_STAGES = 3              # C = 512, 256, 128


def resstack_launches(pipe, host, n):
    """One profiled restore: per-launch ms of the 48 wide ResStack convolutions, in launch order."""
    marks = []
    real = engine.VocoderEngine.forward_cond

    def marked(self, *a, **kw):
        marks.append(len(ops.PROFILE))
        return real(self, *a, **kw)

    engine.VocoderEngine.forward_cond = marked
    ops.PROFILE = []
    try:
        pipe.restore(host.to(pipe.device), n).cpu()
        torch.cuda.synchronize()
        prof = ops.PROFILE
    finally:
        ops.PROFILE = None
        engine.VocoderEngine.forward_cond = real
    start = marks[0] + 6       # condnet (5 launches) and the pre convolution
    out = []
    for j in range(WIDE_STAGES):
        s0 = start + j * STAGE_LAUNCHES + 1
        for tile, macs, e0, e1 in prof[s0:s0 + 16]:
            out.append((tile, e0.elapsed_time(e1)))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    n = int(round(args.seconds * SR))
    vf = VoiceFixer.from_state(weights.seeded_vocoder_state(1234), weights.seeded_restorer_state(4321))
    pipe = vf._get_pipe()
    host = synth_batch(args.batch, n, 1000, "cpu").pin_memory()

    def step():
        return pipe.restore(host.to(dev, non_blocking=True), n).cpu()

    res = {m: {"step_ms": [], "clocks": []} for m in MATHS}
    outs = {}
    for m in MATHS:                     # first use packs the weight planes: outside every timed region
        pipe.set_math(m)
        for _ in range(args.warmup):
            outs[m] = step()
    torch.cuda.synchronize()
    for r in range(args.rounds):
        for m in MATHS:
            pipe.set_math(m)
            step()
            torch.cuda.synchronize()
            sampler = ClockSampler(dev.index)
            with sampler:
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    step()
                dt = time.perf_counter() - t0
            res[m]["step_ms"].append(dt / args.steps * 1e3)
            res[m]["clocks"].append(sampler.summary())
    rows = {}
    for m in MATHS:
        pipe.set_math(m)
        launches = resstack_launches(pipe, host, n)
        rows[m] = {"step_ms": round(statistics.median(res[m]["step_ms"]), 2),
                   "step_ms_rounds": [round(v, 2) for v in res[m]["step_ms"]],
                   "x_realtime": round(args.batch * args.seconds / (statistics.median(res[m]["step_ms"]) / 1e3), 1),
                   "resstack_launches": len(launches),
                   "resstack_ms": round(sum(v for _, v in launches), 3),
                   "resstack_tiles": sorted({t for t, _ in launches}),
                   "resstack_per_launch_ms": [round(v, 4) for _, v in launches],
                   "clocks": res[m]["clocks"]}
    pipe.set_math("f32")
    ref = outs["f32"].double()
    for m in MATHS:
        d = outs[m].double() - ref
        rows[m]["wav_rms_vs_f32"] = float(torch.sqrt(torch.mean(d * d)))
    rows["f16_fallbacks"] = pipe.f16_fallbacks
    doc = {"workload": "batch %d x %.0f s synthetic, seeded weights, host to host, one process" % (args.batch, args.seconds),
           "device": torch.cuda.get_device_name(dev), "steps": args.steps, "rounds": args.rounds, "results": rows}
    for m in MATHS:
        r = rows[m]
        print("%-7s step %8.2f ms  (%6.1fx real-time)   48 wide ResStack launches %8.3f ms   tiles %s   wav rms vs f32 %.2e"
              % (m, r["step_ms"], r["x_realtime"], r["resstack_ms"], r["resstack_tiles"], r["wav_rms_vs_f32"]))
    f = rows["f16"]["resstack_ms"]
    print("f16 / f32: family %.3f, step %.3f;  f16 / bf16x3: family %.3f, step %.3f"
          % (f / rows["f32"]["resstack_ms"], rows["f16"]["step_ms"] / rows["f32"]["step_ms"],
             f / rows["bf16x3"]["resstack_ms"], rows["f16"]["step_ms"] / rows["bf16x3"]["step_ms"]))
    line = json.dumps(doc)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
