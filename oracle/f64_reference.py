"""FLOAT64 REFERENCES OF THE SEQUENCE, FRONT-END AND PER-ROW KERNELS -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Plain double-precision statements of what the recurrence (vfx_gru_bidir_f32 / vfx_gru_bidir2_f32), the analysis front-end
(vfx_stft_mel_f32 / _rows_f32 / _oracle_f32) and the per-row bookkeeping kernels (vfx_mel_to_cond_rows_f32,
vfx_unet_input_f32, vfx_post_rows_f32) compute, written from torch primitives (``torch.nn.GRU`` with
packed sequences, ``torch.stft``) rather than through ``oracle.py``, so the two can check each other:
tests/test_seq_reference_cpu.py pins these statements against the oracle on the CPU, tests/test_seq_kernels_gpu.py holds the
kernels to them.  Ragged batches are given as a list of per-row lengths; every function returns float64 CPU tensors.
"""
import torch

N_FFT = 2048
HOP = 441
N_MELS = 128
H = 256


# --------------------------------------------------------------------------------------
# recurrence
# --------------------------------------------------------------------------------------
def gru_params(sd, prefix, layer=0, whh_scale=1.0):
    """The eight tensors of one bidirectional GRU layer of a state dict, as float64, keyed like torch.nn.GRU's own
    parameters (``weight_hh_l0_reverse`` ...).  ``whh_scale`` multiplies both W_hh (saturating the gates)."""
    p = {}
    for suf in ("", "_reverse"):
        for name in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
            key = "%s_l%d%s" % (name, layer, suf)
            v = sd["%s.%s" % (prefix, key)].to(torch.float64)
            p["%s_l0%s" % (name, suf)] = v * whh_scale if name == "weight_hh" else v
    return p


def gru_input_projection(x, p):
    """gi = [W_ih x + b_ih (forward) | W_ih' x + b_ih' (reverse)]: x (B, T, 512) -> (B, T, 1536), float64."""
    x = x.to(torch.float64)
    return torch.cat([x @ p["weight_ih_l0"].t() + p["bias_ih_l0"],
                      x @ p["weight_ih_l0_reverse"].t() + p["bias_ih_l0_reverse"]], dim=-1)


def gru_bidir(x, p, lengths=None):
    """torch.nn.GRU(512, 256, bidirectional=True, batch_first=True) in float64, h0 = 0: x (B, T, 512) -> (B, T, 512)
    = [forward | reverse].  ``lengths``: per-row frame counts; the batch then goes through pack_padded_sequence, so
    the reverse direction of row b starts at its own frame lengths[b] - 1, and frames >= lengths[b] come back as 0."""
    B, T, n_in = x.shape
    gru = torch.nn.GRU(n_in, H, num_layers=1, bidirectional=True, batch_first=True).to(torch.float64)
    with torch.no_grad():
        for k, v in p.items():
            getattr(gru, k).copy_(v)
        x = x.to(torch.float64)
        if lengths is None:
            return gru(x)[0]
        packed = torch.nn.utils.rnn.pack_padded_sequence(x, torch.as_tensor(list(lengths)), batch_first=True,
                                                         enforce_sorted=False)
        out, _ = torch.nn.utils.rnn.pad_packed_sequence(gru(packed)[0], batch_first=True, total_length=T)
        return out


# --------------------------------------------------------------------------------------
# analysis front-end
# --------------------------------------------------------------------------------------
def htk_filterbank():
    """The HTK filterbank of the restorer front-end, (1025, 128) float64: the reference's float32 matrix
    (voicefixer/tools/mel_scale.py) is the constant both the oracle and the device tables hold."""
    from oracle import oracle
    return oracle.mel_filterbank().to(torch.float64)


def slaney_filterbank():
    """The slaney-normalised filterbank of Vocoder.oracle (librosa.filters.mel), (1025, 128) float64."""
    from voicefixer_amd import frontend_tables
    return torch.from_numpy(frontend_tables.slaney_mel_basis()).to(torch.float64).t().contiguous()


def _stft_mag(x, pad_mode):
    win = torch.hann_window(N_FFT, periodic=True, dtype=torch.float64)
    X = torch.stft(x, N_FFT, hop_length=HOP, win_length=N_FFT, window=win, center=True, pad_mode=pad_mode,
                   return_complex=True)          # (B, 1025, T)
    return X.transpose(1, 2)                   # (B, T, 1025)


def stft_mel(wav, lengths):
    """vfx_stft_mel_f32 / vfx_stft_mel_rows_f32: row b = wav[b, :lengths[b]] -> (1 + n_b // 441, 128) linear mel of the
    centred, reflect-padded STFT (periodic hann, n_fft 2048, hop 441), magnitude sqrt(max(|X|^2, 1e-8)).  Returns a
    list of per-row float64 tensors."""
    fb = htk_filterbank()
    out = []
    for b, n in enumerate(lengths):
        X = _stft_mag(wav[b:b + 1, :n].to(torch.float64), "reflect")[0]
        mag = torch.clamp(X.real ** 2 + X.imag ** 2, min=1e-8).sqrt()
        out.append(mag @ fb)
    return out


def oracle_mel(wav, n):
    """vfx_peak_f32 + vfx_stft_mel_oracle_f32: x = wav[b, :n] / max|wav[b, :n]| -> |STFT| with zero padding (librosa
    >= 0.10 "constant"), no clamp -> slaney mel.  (B, 1 + n // 441, 128) float64."""
    x = wav[:, :n].to(torch.float64)
    x = x / x.abs().amax(dim=1, keepdim=True)
    return _stft_mag(x, "constant").abs() @ slaney_filterbank()


# --------------------------------------------------------------------------------------
# per-row bookkeeping
# --------------------------------------------------------------------------------------
def mel_weight():
    """a * exp(b * k), k = 1 .. 128, evaluated in float32 as voicefixer/vocoder/config.py does -> float64."""
    k = torch.arange(1, N_MELS + 1, dtype=torch.float32)
    return (18.8927416350036 * torch.exp(0.0269863588184314 * k)).to(torch.float64)


def mel_to_cond(mel, lengths):
    """vfx_mel_to_cond_rows_f32: mel (B, T, 128) linear -> list of per-row conds (128, T_b + T_b % 2 + 4):
    S = 20 log10(max(1e-5, |mel / w|)) - 20, c = clip(8 (S + 115) / 115 - 4, -4, 4), then T_b % 2 + 4 frames of -4."""
    w = mel_weight()
    out = []
    for b, t in enumerate(lengths):
        m = (mel[b, :t].to(torch.float64) / w).abs()
        S = 20.0 * torch.log10(torch.clamp(m, min=1e-5)) - 20.0
        c = torch.clamp(8.0 * (S + 115.0) / 115.0 - 4.0, -4.0, 4.0).t()
        out.append(torch.cat([c, torch.full((N_MELS, t % 2 + 4), -4.0, dtype=torch.float64)], dim=1))
    return out


def unet_input(mel, mask_tm, lengths):
    """vfx_unet_input_f32 channels 0 and 1 of row b: log10(max(mel, 1e-8)) and log10(max(mask * mel, 1e-8)) of its
    first lengths[b] frames (bins 0 .. 126; bin 127 and the frames past the row are zero).  mel, mask_tm: (B, T, 128)
    frame-major.  Returns a list of (2, T_b, 127) float64 tensors."""
    out = []
    for b, t in enumerate(lengths):
        m = mel[b, :t, :127].to(torch.float64)
        k = mask_tm[b, :t, :127].to(torch.float64)
        out.append(torch.stack([torch.log10(torch.clamp(m, min=1e-8)), torch.log10(torch.clamp(k * m, min=1e-8))]))
    return out


def post_rows(y, ly_rows, n_rows):
    """vfx_post_rows_f32: row b keeps n_b samples of its own ly_b: peak = max |y[b, :ly_b]|, the window starts at
    (ly_b - n_b) // 2, and is divided by the peak when the peak exceeds 1.  Returns a list of float64 rows; the
    division of two float32 values in float64, rounded once to float32, is the correctly rounded float32 quotient."""
    out = []
    for b, (ly, n) in enumerate(zip(ly_rows, n_rows)):
        row = y[b, :ly].to(torch.float64)
        pk = row.abs().max()
        s = (ly - n) // 2
        seg = row[s:s + n]
        out.append(seg / pk if pk > 1.0 else seg)
    return out

