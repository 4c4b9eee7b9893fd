"""Mode 2 (train-mode BatchNorm + seeded dropout) without a GPU: the Philox specification, the float64 restatement of the
train-mode restorer against the reference's own modules, and the API / CLI / C ABI contract."""
import copy
import os
import re

import numpy as np
import pytest
import torch

import voicefixer_amd
from voicefixer_amd import __main__ as cli, _lib, dropout
from oracle import ref_shim

import train_reference as tref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, want):
    """The Random123 known-answer vectors of Philox4x32-10."""
    assert tuple(int(w) for w in dropout.philox4x32_10(ctr, key)) == want


def test_mask_layout():
    """Word i % 4 of counter (i // 4, segment, layer, 0), i = t * 512 + c; a mask is a prefix of a longer one (it does not
    depend on T), halves are dropped, and segment / layer / seed change it."""
    key = dropout.key_of(0x1234_5678_9abc_def0)
    assert key == (0x9abcdef0, 0x12345678)
    m = dropout.mask(0x1234_5678_9abc_def0, 3, 1, 7)
    t, c = 5, 301
    i = t * 512 + c
    w = dropout.philox4x32_10((i // 4, 3, 1, 0), key)[i % 4]
    assert m[t, c] == (0.0 if w < 2 ** 31 else 2.0)
    assert np.array_equal(dropout.mask(9, 0, 0, 40)[:7], dropout.mask(9, 0, 0, 7))
    assert set(np.unique(m)) <= {0.0, 2.0}
    big = dropout.mask(9, 0, 0, 400)
    assert abs(float((big == 0).mean()) - 0.5) < 0.01
    for other in (dropout.mask(10, 0, 0, 400), dropout.mask(9, 1, 0, 400), dropout.mask(9, 0, 1, 400)):
        assert not np.array_equal(big, other)
    with pytest.raises(ValueError):
        dropout.check_seed(2 ** 64)
    with pytest.raises(TypeError):
        dropout.check_seed(1.5)


def test_restatement_raises_like_torch_at_64_frames(seeded_states):
    """A segment of T <= 64 frames leaves the centre block one value per channel: the reference's ValueError."""
    rsd = {k: v.double() for k, v in seeded_states[1].items()}
    mel = torch.rand(1, 1, 64, 128, dtype=torch.float64)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        tref.restorer_forward(mel, rsd, tref.masks_for(1, 0, 64))


class _Mask(torch.nn.Module):
    def __init__(self, m):
        super().__init__()
        self.m = m

    def forward(self, x):
        return x * self.m


@pytest.mark.skipif(not ref_shim.reference_available(), reason="needs the reference's sources")
@pytest.mark.parametrize("T", [65, 230])
def test_restatement_matches_reference_modules(seeded_states, tmp_path, T):
    """The reference's own Generator in .train() (on a deep copy: its running statistics move), its two nn.Dropout
    replaced by the specification's masks, against the float64 restatement: mask, unet_out and restored log-mel."""
    vsd, rsd = seeded_states
    vf = ref_shim.build_reference_models(str(tmp_path), vsd, {"generator." + k: v for k, v in rsd.items()})
    gen = copy.deepcopy(vf._model.generator)
    assert all(torch.equal(v, rsd[k]) for k, v in gen.state_dict().items() if k in rsd)
    m0, m1 = tref.masks_for(11, 2, T, torch.float32)
    gen.denoiser[5] = _Mask(m0)
    gen.denoiser[12] = _Mask(m1)
    gen.train()
    g = torch.Generator().manual_seed(T)
    mel = torch.rand(1, 1, T, 128, generator=g) ** 2
    with torch.no_grad():
        ref = gen(None, mel)
        mine = tref.restorer_forward(mel.double(), {k: v.double() for k, v in rsd.items()},
                                     tref.masks_for(11, 2, T))
    mask_ref = (ref["clean"] / mel).double()        # clean = mask * noisy (restorer/model.py:106)
    assert torch.allclose(mask_ref, mine["mask"], atol=1e-4)
    for k in ("unet_out", "mel"):
        a, b = ref[k].double(), mine[k]
        assert float((a - b).abs().max() / b.abs().max()) < 1e-4, k


def test_api_mode2_contract(seeded_states):
    vf = voicefixer_amd.VoiceFixer.from_state(*seeded_states)
    with pytest.raises(NotImplementedError, match="seed="):
        vf.restore_inmem(np.zeros(44100, np.float32), mode=2)
    with pytest.raises(ValueError):
        vf.restore_inmem(np.zeros(44100, np.float32), mode=2, seed=-1)
    # with a seed, mode 2 gets as far as the device
    with pytest.raises(RuntimeError, match="no HIP device"):
        vf.restore_inmem(np.zeros(44100, np.float32), mode=2, seed=5)
    with pytest.raises(NotImplementedError):
        vf.restore_stream(np.zeros(44100, np.float32), mode=2)


def test_cli_seed(tmp_path, monkeypatch):
    a = cli.build_parser().parse_args(["--mode", "2", "--seed", "123"])
    assert a.seed == 123 and a.mode == "2"
    assert cli.build_parser().parse_args([]).seed is None
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["--seed", str(2 ** 64)])
    w = tmp_path / "a.wav"
    w.write_bytes(b"x")
    monkeypatch.setenv("HOME", str(tmp_path))
    # past the mode check: the next thing that fails is the missing checkpoint ("Error 0")
    with pytest.raises(RuntimeError, match="Error 0"):
        cli.main(["-i", str(w), "-o", str(tmp_path / "o.wav"), "--mode", "2", "--seed", "7", "--silent"])


def test_train_mode_symbols_declared_and_bound():
    names = ("vfx_bn_stats_workspace_bytes", "vfx_bn_stats_f32", "vfx_bn_apply_f32", "vfx_dropout_f32")
    with open(os.path.join(ROOT, "include", "vfx_hip.h")) as f:
        header = f.read()
    for n in names:
        assert re.search(r"\b%s\(" % n, header), n
        assert n in _lib.SIGNATURES, n
    with open(os.path.join(ROOT, "voicefixer_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert "vfx_train.hip" in mk and re.search(r"check_no_pk_fma:.*vfx_train\.o", mk)
