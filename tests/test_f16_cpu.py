"""The opt-in f16 arithmetic without a GPU: weight packing, the C ABI declaration / export / binding, the public switch
and the command-line flag."""
import os
import re

import pytest
import torch

from voicefixer_amd import _lib, engine, packing
from conftest import ROOT


def test_pack_f16_round_trips_the_rne_rounded_weights():
    g = torch.Generator().manual_seed(4)
    for C in (128, 256, 512):
        w = torch.randn(C, C, 3, generator=g)        # torch Conv1d layout (Cout, Cin, k)
        p = packing.pack_f16(packing.pack_conv1d(w))
        assert p.dtype == torch.float16 and tuple(p.shape) == (3, C // 8, C, 8)
        # element [t][c8][n][e] = w[n][8 c8 + e][t]
        back = p.permute(0, 1, 3, 2).reshape(3, C, C).permute(2, 1, 0)    # -> (Cout, Cin, k)
        assert torch.equal(back, w.to(torch.float16))


def test_pack_f16_declines_what_the_kernel_does_not_take():
    assert packing.pack_f16(packing.pack_conv1d(torch.zeros(64, 64, 3))) is None       # C = 64 stays fp32
    assert packing.pack_f16(packing.pack_conv1d(torch.zeros(128, 64, 3))) is None      # Cin != Cout
    assert packing.pack_f16(packing.pack_conv1d(torch.zeros(128, 128, 7))) is None     # k != 3
    w = torch.zeros(128, 128, 3)
    w[3, 4, 1] = 7e4                                                                    # outside the fp16 range
    assert packing.pack_f16(packing.pack_conv1d(w)) is None


def test_conv1d_f16_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "vfx_hip.h")).read()
    assert re.search(r"int vfx_conv1d_f16\(const vfx_tensor\* x, const void\* w_f16, const float\* bias", hdr)
    assert re.search(r"#define VFX_ENOTSUP \(-4\)", hdr)
    assert re.search(r"code 32\s+convh_kernel", hdr)
    vmap = open(os.path.join(ROOT, "voicefixer_amd", "csrc", "vfx.map")).read()
    assert "vfx_*;" in vmap
    assert "vfx_conv1d_f16" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["vfx_conv1d_f16"]
    assert len(args) == 12 and _lib.ENOTSUP == -4
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "vfx_conv1d_f16" in {ln.split()[-1] for ln in out.splitlines() if ln.split()}


def test_public_classes_do_not_offer_f16_yet(seeded_states):
    """f16 is an engine-level arithmetic until it beats f32 and bf16x3: the public classes refuse it."""
    import voicefixer_amd
    vf = voicefixer_amd.VoiceFixer.from_state(*seeded_states)
    voc = voicefixer_amd.Vocoder.from_state(seeded_states[0])
    for obj in (vf, voc):
        for bad in ("f16", "fp8", "bf16"):
            with pytest.raises(ValueError):
                obj.set_math(bad)
        obj.set_math("bf16x3")
        obj.set_math("f32")
    assert engine.MATHS == ("f32", "bf16x3", "f16")
