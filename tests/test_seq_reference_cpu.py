"""The float64 references of tests/test_seq_kernels_gpu.py (oracle/f64_reference.py) against the project's own oracle, on
the CPU: torch.nn.GRU with packed sequences against oracle._gru_dir row by row, torch.stft against oracle.stft_mag, and
the cond / UNet-input / post statements against oracle.mel_to_cond, oracle.to_log and oracle.trim_center.  Keeps the
references honest without a GPU."""
import math

import torch

from oracle import oracle, f64_reference as ref64
from voicefixer_amd import weights


def _gru_dir64(x, p, suf, reverse):
    return oracle._gru_dir(x, p["weight_ih_l0" + suf], p["weight_hh_l0" + suf], p["bias_ih_l0" + suf],
                           p["bias_hh_l0" + suf], reverse)


def test_packed_gru_equals_the_oracle_recurrence_row_by_row():
    p = ref64.gru_params(weights.seeded_restorer_state(4321), "denoiser.7.gru", 0, whh_scale=4.0)
    T, lengths = 70, [70, 69, 3, 33, 2]
    x = torch.randn((len(lengths), T, 512), generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    got = ref64.gru_bidir(x, p, lengths)
    for b, t in enumerate(lengths):
        xb = x[b:b + 1, :t]
        want = torch.cat([_gru_dir64(xb, p, "", False), _gru_dir64(xb, p, "_reverse", True)], -1)[0]
        assert (got[b, :t] - want).abs().max() < 1e-12, b
        assert (got[b, t:] == 0).all()
    # the plain (unpacked) form, and the input projection the kernels are fed
    full = ref64.gru_bidir(x[:2], p)
    assert (full[0] - got[0]).abs().max() < 1e-12
    gi = ref64.gru_input_projection(x[:1], p)
    assert gi.shape == (1, T, 1536)
    assert (gi[0, :, :768] - (x[0] @ p["weight_ih_l0"].t() + p["bias_ih_l0"])).abs().max() < 1e-12


def test_torch_stft_mel_equals_the_oracle_front_end():
    g = torch.Generator().manual_seed(2)
    lengths = [1025, 1465, 441 * 7 + 440]
    wav = 0.3 * torch.randn((len(lengths), max(lengths)), generator=g)
    got = ref64.stft_mel(wav, lengths)
    fb = oracle.mel_filterbank().double()
    for b, n in enumerate(lengths):
        want = oracle.stft_mag(wav[b:b + 1, :n], torch.float64)[0] @ fb
        assert got[b].shape == (1 + n // 441, 128)
        assert ((got[b] - want).abs() / want.abs().clamp(min=1e-12)).max() < 1e-9
    # a pure sine reaches the 1e-8 power clamp in float64 as well
    t = torch.arange(441 * 20, dtype=torch.float64)
    s = (0.5 * torch.sin(2 * math.pi * 1234.5 * t / 44100)).float()[None]
    sp = oracle.stft_mag(s, torch.float64)
    assert (sp == 1e-4).any()
    assert ((ref64.stft_mel(s, [s.shape[1]])[0] - sp[0] @ fb).abs() / (sp[0] @ fb)).max() < 1e-9


def test_oracle_mel_statement_uses_peak_normalisation_and_zero_padding():
    g = torch.Generator().manual_seed(3)
    n = 441 * 5 + 17
    wav = torch.randn((2, n + 4), generator=g)
    wav[1] *= 7.0
    wav[:, n:] = 100.0                       # past N: neither the peak nor the frames see it
    got = ref64.oracle_mel(wav, n)
    x = wav[:, :n].double()
    x = x / x.abs().amax(1, keepdim=True)
    xp = torch.nn.functional.pad(x, (1024, 1024))   # zero ("constant") padding
    frames = xp.unfold(-1, 2048, 441)
    mag = torch.fft.rfft(frames * torch.hann_window(2048, periodic=True, dtype=torch.float64), dim=-1).abs()
    assert (got - mag @ ref64.slaney_filterbank()).abs().max() < 1e-9 * got.abs().max()


def test_cond_statement_equals_the_oracle_mel_to_cond():
    g = torch.Generator().manual_seed(4)
    T, lengths = 41, [41, 40, 3, 2]
    mel = 10 ** (torch.rand((len(lengths), T, 128), generator=g, dtype=torch.float64) * 11 - 7)
    mel[:, ::3, ::4] = 0.0
    got = ref64.mel_to_cond(mel, lengths)
    for b, t in enumerate(lengths):
        want = oracle.mel_to_cond(mel[b:b + 1, None, :t])[0]
        assert got[b].shape == want.shape == (128, t + t % 2 + 4)
        assert (got[b] - want).abs().max() < 1e-12
    assert (ref64.mel_weight() == oracle.mel_weight().double()).all()


def test_unet_input_statement_equals_the_oracle_to_log():
    g = torch.Generator().manual_seed(5)
    mel = 10 ** (torch.rand((2, 9, 128), generator=g, dtype=torch.float64) * 12 - 10)
    mask = torch.rand((2, 9, 128), generator=g, dtype=torch.float64)
    got = ref64.unet_input(mel, mask, [9, 4])
    for b, t in enumerate([9, 4]):
        assert torch.equal(got[b][0], oracle.to_log(mel[b, :t, :127]))
        assert torch.equal(got[b][1], oracle.to_log(mask[b, :t, :127] * mel[b, :t, :127]))


def test_post_statement_equals_the_oracle_peak_rule_and_trim():
    g = torch.Generator().manual_seed(6)
    ly_rows, n_rows = [1000, 999, 800, 801], [900, 900, 799, 800]
    y = 0.3 * torch.randn((4, 1010), generator=g)
    y[1, 10] = -2.0
    y[2, 5] = 1.0
    y[3, 700] = 3.0
    y[3, 801] = 9.0                          # past the row: does not count
    got = ref64.post_rows(y, ly_rows, n_rows)
    for b, (ly, n) in enumerate(zip(ly_rows, n_rows)):
        e = y[b:b + 1, :ly].double()
        pk = e.abs().max()
        if pk > 1.0:
            e = e / pk
        want = oracle.trim_center(e, n)[0]
        assert torch.equal(got[b], want), b
    # the quotient of two float32 values, computed in float64 and rounded once, is the correctly rounded float32 one
    a = torch.randn(4096, generator=g)
    d = torch.rand(4096, generator=g) * 8 + 1
    assert torch.equal((a.double() / d.double()).float(), a / d)
