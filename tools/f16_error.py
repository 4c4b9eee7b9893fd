#!/usr/bin/env python
"""CPU emulation of narrow-operand convolution arithmetic on the fp32 oracle: before a convolution, both operands are rounded to
fp16 or bf16 (round to nearest even), the convolution itself is computed in fp32.  Backs DESIGN.md 3.7.

    python tools/f16_error.py [golden .npz, default tests/golden/restore_speech_T51.npz]

Seeded weights (vocoder 1234, restorer 4321).  Scopes:
  resstack   the k = 3 convolutions of the ResStacks with 512 / 256 / 128 channels (what set_math("f16") runs in f16)
  conv1d     every Conv1d of the vocoder
  every      every convolution of the path (Conv1d, ConvTranspose1d, Conv2d, ConvTranspose2d)
Per scope and type: the end-to-end waveform difference against the fp32 oracle (RMS, MAE, max), and -- for the vocoder --
the per-stage difference relative to the stage's own peak (condnet, up1..up4 and res1..res4: the outputs of the four
UpsampleNet transposed convolutions and of the four ResStacks, and the waveform), and how far the emulated f16 waveform itself
moves when the weights are perturbed at fp32-rounding level (2e-7 relative): the noise floor of any end-to-end comparison of
f16 results (tests/test_f16_gpu.py: E2E_FLOOR)."""
import contextlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from oracle import oracle  # noqa: E402
from voicefixer_amd import weights  # noqa: E402

NARROW = {"fp16": torch.float16, "bf16": torch.bfloat16}
K3_PER_VOCODER = 5 + 16 * 4       # condnet, then 16 per ResStack stage
RESSTACK_F16 = range(5, 5 + 16 * 3)


@contextlib.contextmanager
def emulated(dtype, scope):
    rnd = lambda t: t.to(dtype).float()
    names = ("conv1d",) if scope in ("resstack", "conv1d") else ("conv1d", "conv_transpose1d", "conv2d", "conv_transpose2d")
    real = {n: getattr(F, n) for n in names}
    count = [0]

    def make(n):
        def f(x, w, *a, **kw):
            if scope == "resstack":
                if w.dim() != 3 or w.shape[-1] != 3:
                    return real[n](x, w, *a, **kw)
                k = count[0] % K3_PER_VOCODER
                count[0] += 1
                if k not in RESSTACK_F16:
                    return real[n](x, w, *a, **kw)
            return real[n](rnd(x), rnd(w), *a, **kw)
        return f

    for n in names:
        setattr(F, n, make(n))
    try:
        yield
    finally:
        for n, f in real.items():
            setattr(F, n, f)


def vocoder_stages(cond, vsd):
    st = {}
    wav = oracle.vocoder_generator(cond, vsd, stages=st)
    st["wav"] = wav
    return {k: v for k, v in st.items() if k != "pre"}


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "restore_speech_T51.npz")
    g = np.load(path)
    vsd, rsd = weights.seeded_vocoder_state(1234), weights.seeded_restorer_state(4321)
    torch.set_grad_enabled(False)
    ref = oracle.restore_inmem(g["wav"], vsd, rsd).astype(np.float64)
    print("input %s: %d samples; fp32 oracle output RMS %.4f" % (os.path.basename(path), g["wav"].shape[0],
                                                                float(np.sqrt(np.mean(ref ** 2)))))
    print("\nend to end (waveform vs the fp32 oracle)")
    print("%-6s %-9s %10s %10s %10s" % ("type", "scope", "RMS", "MAE", "max"))
    for tname, dt in NARROW.items():
        for scope in ("resstack", "conv1d", "every"):
            with emulated(dt, scope):
                out = oracle.restore_inmem(g["wav"], vsd, rsd).astype(np.float64)
            d = out - ref
            print("%-6s %-9s %10.3e %10.3e %10.3e" % (tname, scope, np.sqrt(np.mean(d ** 2)), np.abs(d).mean(), np.abs(d).max()))
    # per stage of the vocoder on the restorer's fp32 output
    seg = torch.as_tensor(g["wav"])[None]
    den = oracle.from_log(oracle.restorer_forward(oracle.wav_to_mel(seg), rsd))
    cond = oracle.mel_to_cond(den)
    base = vocoder_stages(cond, vsd)
    print("\nvocoder per stage (max |diff| / stage peak), scope resstack")
    keys = list(base)
    print("%-6s %s" % ("type", " ".join("%9s" % k for k in keys)))
    for tname, dt in NARROW.items():
        with emulated(dt, "resstack"):
            st = vocoder_stages(cond, vsd)
        cells = []
        for k in keys:
            a, b = st[k].double(), base[k].double()
            cells.append("%9.2e" % (float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)))
        print("%-6s %s" % (tname, " ".join(cells)))
    gen = torch.Generator().manual_seed(0)
    vsd2 = {k: (v * (1 + 2e-7 * torch.randn(v.shape, generator=gen)) if v.is_floating_point() else v) for k, v in vsd.items()}
    rms = lambda a, b: float(torch.sqrt(torch.mean((a.double() - b.double()) ** 2)))
    f32a, f32b = oracle.vocoder_generator(cond, vsd), oracle.vocoder_generator(cond, vsd2)
    with emulated(torch.float16, "resstack"):
        e1, e2 = oracle.vocoder_generator(cond, vsd), oracle.vocoder_generator(cond, vsd2)
    print("\nweights perturbed by 2e-7 relative (vocoder waveform RMS change): fp32 %.3e, fp16-emulated %.3e (fp16 vs fp32: %.3e)"
          % (rms(f32a, f32b), rms(e1, e2), rms(e1, f32a)))


if __name__ == "__main__":
    main()
