"""The oracle (and the seeded-checkpoint manifests) against the reference's own modules, through
tests/golden/reference_parity.npz: what the reference computed on these inputs, recorded by
``python oracle/make_golden.py --parity``.  Runs without the reference and without a GPU."""
import hashlib
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle import oracle


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(GOLDEN, "reference_parity.npz"))


def _sha256(t):
    """oracle/make_golden.py: tensor_sha256 -- dtype, shape and bytes."""
    t = t.detach().cpu().contiguous()
    h = hashlib.sha256(("%s%s" % (t.dtype, tuple(t.shape))).encode())
    h.update(t.numpy().tobytes())
    return h.hexdigest()


def test_manifests_match_reference(ref, seeded_states):
    """The reference took the seeded state dicts verbatim: same keys in the same order, every tensor bit-identical."""
    vsd, rsd = seeded_states
    for tag, sd in (("restorer", rsd), ("vocoder", vsd)):
        assert list(sd.keys()) == [str(k) for k in ref[tag + "_keys"]]
        for k, h in zip(sd, ref[tag + "_sha256"]):
            assert _sha256(sd[k]) == str(h), k


@pytest.mark.parametrize("n", [4410 + 17, 44100 // 2 + 123])
def test_restore_inmem_matches_reference(ref, seeded_states, n):
    vsd, rsd = seeded_states
    g = torch.Generator().manual_seed(n)
    wav = (0.15 * torch.randn(n, generator=g)).numpy().astype(np.float32)
    assert np.array_equal(wav, ref["restore_%d_wav" % n])
    with torch.no_grad():
        out = oracle.restore_inmem(wav, vsd, rsd)
    want = ref["restore_%d_out" % n]
    assert want.shape == out.shape == (1, n)
    assert np.sqrt(np.mean((want - out) ** 2)) < 1e-5


def test_stft_fft_vs_conv_dft(ref):
    """oracle uses an FFT, the reference (torchlibrosa) a conv-DFT: same magnitudes."""
    g = torch.Generator().manual_seed(3)
    wav = torch.randn(2, 9000, generator=g) * 0.3
    assert np.array_equal(wav.numpy(), ref["stft_wav"])
    sp = torch.from_numpy(ref["stft_mag"])
    with torch.no_grad():
        mine = oracle.stft_mag(wav)
    assert sp.shape == (2, 1, 21, 1025)
    rel = (sp[:, 0] - mine).norm() / mine.norm()
    assert rel < 5e-6


def test_vocoder_forward_legacy_ckpt(ref):
    """The reference loads legacy weight_g/weight_v checkpoints through torch's compat
    hook; both key styles must give the same generator."""
    from voicefixer_amd import weights
    legacy = weights.seeded_vocoder_state(1234, legacy=True)
    g = torch.Generator().manual_seed(5)
    mel = 10 ** (torch.rand((1, 1, 12, 128), generator=g) * 4 - 2)
    assert np.array_equal(mel.numpy(), ref["legacy_mel"])
    with torch.no_grad():
        out = oracle.vocoder_forward(mel, legacy)
    assert (torch.from_numpy(ref["legacy_out"]) - out).abs().max() < 2e-5
