"""FLOAT64 REFERENCES OF THE SEQUENCE, FRONT-END, PER-ROW AND CONVOLUTION KERNELS -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Plain double-precision statements of what the recurrence (vfx_gru_bidir_f32 / vfx_gru_bidir2_f32), the analysis front-end
(vfx_stft_mel_f32 / _rows_f32 / _oracle_f32), the per-row bookkeeping kernels (vfx_mel_to_cond_rows_f32,
vfx_unet_input_f32, vfx_post_rows_f32) and the four convolution entry points that conv_taps_kernel serves (vfx_conv1d_f32,
vfx_convtr1d_f32, vfx_conv2d_f32, vfx_convtr2d_3x3s2_f32, with their fused activations, bias, residual and per-row lengths)
compute, written from torch primitives (``torch.nn.GRU`` with packed sequences, ``torch.stft``, ``torch.matmul``) rather than
through ``oracle.py``, so the two can check each other: tests/test_seq_reference_cpu.py and tests/test_conv_reference_cpu.py
pin these statements against the oracle and the torch operators on the CPU, tests/test_seq_kernels_gpu.py and
tests/test_conv_taps_gpu.py hold the kernels to them.  Ragged batches are given as a list of per-row lengths; every function
returns float64 CPU tensors.  The last sections are the yardsticks of tests/test_convwg4s_gpu.py and tests/test_convtw_gpu.py:
the 3x3 convolution as a plain fp32 Winograd F(4,3) (conv2d_f43_f32) with the per-quad error figure, and the transposed 1-D
convolution as a plain fp32 Winograd F(3,2) (convtr1d_f32_f32) -- functions that return float32.  tests/test_resblk4_gpu.py
holds the fused C = 64 ResStack layer to ``resblock`` and measures its bound on ``resblock_f43_f32`` (two
``conv1d_f43_f32``: the dilated 1-D convolution as a plain fp32 F(4,3)).
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



# --------------------------------------------------------------------------------------
# first-generation convolution family (vfx_conv1d_f32, vfx_convtr1d_f32, vfx_conv2d_f32, vfx_convtr2d_3x3s2_f32)
# --------------------------------------------------------------------------------------
# Written from include/vfx_hip.h and the torch operators the entry points replace: every convolution is a sum over its
# taps of one matrix product with a shifted slice of the (padded) input, so there is no algorithm to trust but the
# index arithmetic on this page -- tests/test_conv_reference_cpu.py pins it against torch.nn.functional and the oracle's
# modules.  Layouts are torch's own ((B, C, L) and dense (B, C, H, W) maps, torch weight layouts); to_pitch / from_pitch
# move maps to and from the device's pitch layout.  Every function takes `lengths`: per-row valid extents (samples, or
# map rows), each row then being computed as if it were alone in the batch; outputs past a row's own end are NaN.
# `magnitude=True` returns sum |pre(x)| |w| + |bias| + |res| per output instead of the value: the scale that the
# rounding error of the sum grows with.
PRE_NONE, PRE_LRELU, PRE_AFFINE_LRELU = 0, 1, 2
POST_NONE, POST_LRELU, POST_ELU, POST_TANH, POST_SIGMOID, POST_LRELU_SNAKE = 0, 1, 2, 3, 4, 5


def to_pitch(x, pitch_log2, fill=0.0):
    """Dense (B, C, H, W = P - 1) -> pitch map (B, C, H * P) with `fill` in the pad column."""
    B, Cn, Hh, W = x.shape
    P = 1 << pitch_log2
    assert W == P - 1
    out = torch.full((B, Cn, Hh, P), fill, dtype=x.dtype)
    out[..., :W] = x
    return out.reshape(B, Cn, Hh * P)


def from_pitch(y, H, pitch_log2):
    """Pitch map (B, C, >= H * P) -> (B, C, H, P), pad column included."""
    P = 1 << pitch_log2
    return y[:, :, :H * P].reshape(y.shape[0], y.shape[1], H, P)


def conv_pre(x, pre=PRE_NONE, slope=0.0, scale=None, shift=None):
    """The fused pre-activation of the input (VFX_PRE_*), float64; scale / shift are per input channel."""
    x = x.to(torch.float64)
    if pre == PRE_AFFINE_LRELU:
        shp = [1, -1] + [1] * (x.dim() - 2)
        x = x * scale.to(torch.float64).reshape(shp) + shift.to(torch.float64).reshape(shp)
    if pre in (PRE_LRELU, PRE_AFFINE_LRELU):
        x = torch.where(x > 0, x, x * float(slope))
    return x


def conv_post(v, post=POST_NONE, slope=0.0):
    """The fused post-activation (VFX_POST_*), float64."""
    if post in (POST_LRELU, POST_LRELU_SNAKE):
        v = torch.where(v > 0, v, v * float(slope))
        return v + torch.sin(v) if post == POST_LRELU_SNAKE else v
    if post == POST_ELU:
        return torch.where(v > 0, v, torch.expm1(v))
    if post == POST_TANH:
        return torch.tanh(v)
    if post == POST_SIGMOID:
        return 1.0 / (1.0 + torch.exp(-v))
    assert post == POST_NONE
    return v


def post_lipschitz(post):
    """Lipschitz constant of the post-activation (v + sin v has slope up to 2)."""
    return 2.0 if post == POST_LRELU_SNAKE else 1.0


def conv_pre32(x, pre=PRE_NONE, slope=0.0, scale=None, shift=None):
    """The pre-activated input x~ in float32 as conv_x3_kernel's staging code forms it: the affine part one fused
    multiply-add (fmaf(x, scale, shift): the exact product plus the shift in float64, rounded to float32 -- a double rounding
    that differs from the fused operation only on a tie of the float64 sum), then v > 0 ? v : v * slope with the slope as
    float32."""
    x = x.to(torch.float32)
    if pre == PRE_AFFINE_LRELU:
        shp = [1, -1] + [1] * (x.dim() - 2)
        x = (x.double() * scale.to(torch.float32).double().reshape(shp) + shift.to(torch.float32).double().reshape(shp)).float()
    if pre in (PRE_LRELU, PRE_AFFINE_LRELU):
        x = torch.where(x > 0, x, x * torch.tensor(float(slope), dtype=torch.float32))
    return x


def split_bf16(v):
    """v (float32) -> (hi, lo) float32 with hi = bf16(v), lo = bf16(v - hi), both round-to-nearest-even: the two planes of
    VFX_MATH_BF16X3 (packing.pack_x3 writes the same planes of the weights; v - hi is exact in float32)."""
    v = v.to(torch.float32)
    hi = v.to(torch.bfloat16).to(torch.float32)
    lo = (v - hi).to(torch.bfloat16).to(torch.float32)
    return hi, lo


def _terms(x, w, pre, pre_slope, scale, shift, magnitude, split):
    """The (input, weight) float64 pairs whose convolutions add up to the bare sum.  split=None: one pair, pre(x) and w.
    split="bf16x3" (the stated arithmetic of conv_x3_kernel, include/vfx_hip.h VFX_MATH_BF16X3): x~ = conv_pre32(x) and w
    are split into bf16 planes and the sum is  xh wh + xh wl + xl wh  =  conv(xh, wh + wl) + conv(xl, wh),  every product and
    the sum exact to float64.  The reference, not a model of the kernel: no tile, chunk or staging order appears.
    magnitude: one pair (|x~|, |w|) either way."""
    assert split in (None, "bf16x3")
    if split is None:
        xa, w64 = conv_pre(x, pre, pre_slope, scale, shift), w.to(torch.float64)
        return [(xa.abs(), w64.abs())] if magnitude else [(xa, w64)]
    xt = conv_pre32(x, pre, pre_slope, scale, shift)
    if magnitude:
        return [(xt.double().abs(), w.to(torch.float32).double().abs())]
    (xh, xl), (wh, wl) = split_bf16(xt), split_bf16(w)
    return [(xh.double(), wh.double() + wl.double()), (xl.double(), wh.double())]


def bf16x3_tripled(x, w, pre=PRE_NONE, pre_slope=0.0, scale=None, shift=None, cin_dim=1):
    """The yardstick problem of the bf16x3 device bound: (cat[xh, xh, xl], cat[wh, wl, wh]) along the input channels, float32
    (x~ already activated: run the operator without pre-activation).  Every product of two bf16 values is exact in fp32, so
    torch's fp32 CPU operator on this pair scores fp32 accumulation of the same 3 K-term sum the statement adds exactly.
    cin_dim: the weight's input-channel dimension (1 for Conv weights, 0 for ConvTranspose weights)."""
    (xh, xl), (wh, wl) = split_bf16(conv_pre32(x, pre, pre_slope, scale, shift)), split_bf16(w)
    return torch.cat([xh, xh, xl], dim=1), torch.cat([wh, wl, wh], dim=cin_dim)


def _finish(acc, bias, res, post, post_slope, magnitude):
    """acc (B, Cout, ...) + bias + res -> post(...); or the magnitude |acc| + |bias| + |res| (acc then already is
    sum |x~| |w|)."""
    shp = [1, -1] + [1] * (acc.dim() - 2)
    if magnitude:
        if bias is not None:
            acc = acc + bias.to(torch.float64).abs().reshape(shp)
        return acc + res.to(torch.float64).abs() if res is not None else acc
    if bias is not None:
        acc = acc + bias.to(torch.float64).reshape(shp)
    if res is not None:
        acc = acc + res.to(torch.float64)
    return conv_post(acc, post, post_slope)


def _by_rows(fn, x, res, lengths, out_len):
    """Ragged batches: run `fn(x_row, res_row)` on every row cut to its own extent (along dim 2) and paste the results
    into a NaN-filled (B, Cout, out_len(max extent), ...) batch."""
    outs = []
    for b, n in enumerate(lengths):
        xb = x[b:b + 1, :, :n]
        outs.append(fn(xb, None if res is None else res[b:b + 1, :, :out_len(n)]))
    full = torch.full((len(outs), outs[0].shape[1], out_len(x.shape[2])) + tuple(outs[0].shape[3:]), float("nan"),
                      dtype=torch.float64)
    for b, o in enumerate(outs):
        full[b:b + 1, :, :o.shape[2]] = o
    return full


def conv1d(x, w, bias=None, res=None, dilation=1, reflect=False, pre=PRE_NONE, pre_slope=0.0, scale=None, shift=None,
           post=POST_NONE, post_slope=0.0, lengths=None, magnitude=False, split=None):
    """vfx_conv1d_f32: y[b,n,l] = post(bias[n] + res[b,n,l] + sum_{c,t} w[n,c,t] pre(x)[b,c,l + (t - (k-1)/2) dilation]),
    the pre-activated input padded with zeros, or mirrored about its first and last sample (ReflectionPad1d).
    x (B, Cin, L), w (Cout, Cin, k) with k odd -> (B, Cout, L) float64.  `split`: see _terms."""
    if lengths is not None:
        return _by_rows(lambda xb, rb: conv1d(xb, w, bias, rb, dilation, reflect, pre, pre_slope, scale, shift, post,
                                              post_slope, None, magnitude, split), x, res, lengths, lambda n: n)
    k = w.shape[2]
    assert k % 2 == 1
    L, p = x.shape[2], (k - 1) // 2 * dilation
    acc = torch.zeros((x.shape[0], w.shape[0], L), dtype=torch.float64)
    for xa, w64 in _terms(x, w, pre, pre_slope, scale, shift, magnitude, split):
        if reflect:
            assert p < L
            idx = torch.arange(-p, L + p).abs()
            idx = torch.where(idx > L - 1, 2 * (L - 1) - idx, idx)
            xp = xa[:, :, idx]
        else:
            xp = torch.zeros((x.shape[0], x.shape[1], L + 2 * p), dtype=torch.float64)
            xp[:, :, p:p + L] = xa
        for t in range(k):
            acc += torch.matmul(w64[:, :, t], xp[:, :, t * dilation:t * dilation + L])
    return _finish(acc, bias, res, post, post_slope, magnitude)


def convtr1d(x, w, bias=None, stride=2, pre=PRE_NONE, pre_slope=0.0, scale=None, shift=None, post=POST_NONE,
             post_slope=0.0, lengths=None, magnitude=False, split=None):
    """vfx_convtr1d_f32 = ConvTranspose1d(Cin, Cout, kernel 2s, stride s, padding s // 2 + s % 2, output_padding s % 2):
    input sample i adds w[c,n,t] x[b,c,i] to position i s + t - padding; positions outside [0, s Lin) are dropped.
    x (B, Cin, Lin), w (Cin, Cout, 2s) -> (B, Cout, s Lin) float64."""
    if lengths is not None:
        return _by_rows(lambda xb, rb: convtr1d(xb, w, bias, stride, pre, pre_slope, scale, shift, post, post_slope,
                                                None, magnitude, split), x, None, lengths, lambda n: n * stride)
    s = stride
    assert w.shape[2] == 2 * s
    Lin, pad = x.shape[2], s // 2 + s % 2
    full = torch.zeros((x.shape[0], w.shape[1], (Lin + 1) * s), dtype=torch.float64)   # positions i s + t, t < 2s
    for xa, w64 in _terms(x, w, pre, pre_slope, scale, shift, magnitude, split):
        for t in range(2 * s):
            full[:, :, t:t + Lin * s:s] += torch.matmul(w64[:, :, t].t(), xa)
    return _finish(full[:, :, pad:pad + s * Lin].clone(), bias, None, post, post_slope, magnitude)


def conv2d(x, w, bias=None, res=None, pre=PRE_NONE, pre_slope=0.0, scale=None, shift=None, post=POST_NONE,
           post_slope=0.0, lengths=None, magnitude=False, split=None):
    """vfx_conv2d_f32 on dense maps: Conv2d(k x k, k = 1 or 3, stride 1, padding k // 2) of the pre-activated input,
    zero padding on all four sides (on the device the pad column of the pitch map IS the left / right padding, and
    the output's pad column is written as zero: see to_pitch).  x (B, Cin, H, W), w (Cout, Cin, k, k) -> (B, Cout, H, W)
    float64.  `lengths`: map rows per batch item."""
    if lengths is not None:
        return _by_rows(lambda xb, rb: conv2d(xb, w, bias, rb, pre, pre_slope, scale, shift, post, post_slope, None,
                                              magnitude, split), x, res, lengths, lambda n: n)
    k = w.shape[2]
    assert k in (1, 3) and w.shape[3] == k
    B, _, Hh, W = x.shape
    p = k // 2
    acc = torch.zeros((B, w.shape[0], Hh, W), dtype=torch.float64)
    for xa, w64 in _terms(x, w, pre, pre_slope, scale, shift, magnitude, split):
        xp = torch.zeros((B, x.shape[1], Hh + 2 * p, W + 2 * p), dtype=torch.float64)
        xp[:, :, p:p + Hh, p:p + W] = xa
        for ky in range(k):
            for kx in range(k):
                acc += torch.einsum("nc,bchw->bnhw", w64[:, :, ky, kx], xp[:, :, ky:ky + Hh, kx:kx + W])
    return _finish(acc, bias, res, post, post_slope, magnitude)


def convtr2d_3x3s2(x, w, pre=PRE_NONE, pre_slope=0.0, scale=None, shift=None, post=POST_NONE, post_slope=0.0,
                   lengths=None, magnitude=False):
    """vfx_convtr2d_3x3s2_f32 = ConvTranspose2d(3 x 3, stride 2, padding 0) followed by DecoderBlockRes' cut of the last
    output row: input (i, j) adds w[c,n,ky,kx] x[b,c,i,j] to (2 i + ky, 2 j + kx); (h, w) -> (2 h, 2 w + 1).
    x (B, Cin, h, w), w (Cin, Cout, 3, 3) -> (B, Cout, 2 h, 2 w + 1) float64.  `lengths`: input map rows per item."""
    if lengths is not None:
        return _by_rows(lambda xb, rb: convtr2d_3x3s2(xb, w, pre, pre_slope, scale, shift, post, post_slope, None,
                                                      magnitude), x, None, lengths, lambda n: 2 * n)
    B, _, h, wd = x.shape
    xa = conv_pre(x, pre, pre_slope, scale, shift)
    w64 = w.to(torch.float64)
    if magnitude:
        xa, w64 = xa.abs(), w64.abs()
    full = torch.zeros((B, w.shape[1], 2 * h + 1, 2 * wd + 1), dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            full[:, :, ky:ky + 2 * h:2, kx:kx + 2 * wd:2] += torch.einsum("cn,bchw->bnhw", w64[:, :, ky, kx], xa)
    return _finish(full[:, :, :2 * h].clone(), None, None, post, post_slope, magnitude)


def conv_error(got, ref, mag, lipschitz=1.0):
    """The figure the convolution tests bound: |got - ref| / (lipschitz * magnitude + |ref|) per output, over the
    outputs where ref is not NaN (rows of a ragged batch end early).  Returns (max, sum of squares, count)."""
    ok = ~torch.isnan(ref)
    e = (got.to(torch.float64) - ref).abs() / (lipschitz * mag + ref.abs()).clamp(min=1e-300)
    e = torch.where(ok, e, torch.zeros_like(e))      # a NaN in `got` at a valid output stays NaN and fails the bound
    bad = torch.isnan(got.to(torch.float64)) & ok
    mx = float("inf") if bool(bad.any()) else float(e.max())
    return mx, float((e * e).sum()), int(ok.sum())


# --------------------------------------------------------------------------------------
# the 3x3 convolution as Winograd F(4,3) along the map rows, in fp32 (the error yardstick of convwg4s_kernel)
# --------------------------------------------------------------------------------------
# An F(4,3) kernel cannot be held to a multiple of the DIRECT fp32 operator's error: a plain fp32 F(4,3) is 4.3 x (maximum)
# and 2.2 x (RMS) the direct operator against float64 at 64 -> 64 channels (transform constants up to 8).  So the bound of
# tests/test_convwg4s_gpu.py is measured on this fp32 statement of the same algorithm: standard matrices (the header of
# voicefixer_amd/csrc/vfx_convwg.inc writes them out), every operation separately rounded, bias and residual added after
# the output transform.  It is the reference, not a model of the kernel.
def _f43_weights(w):
    """U = G w along the kernel's row axis, formed in float64 and rounded once (as packing.pack_wino4_2d does):
    w (Cout, Cin, 3, 3) -> (6 planes, Cout, Cin, 3 kernel columns) float32."""
    g0, g1, g2 = (w[:, :, ky].to(torch.float64) for ky in range(3))
    return torch.stack([g0 / 4, -(g0 + g1 + g2) / 6, -(g0 - g1 + g2) / 6, g0 / 24 + g1 / 12 + g2 / 6,
                        g0 / 24 - g1 / 12 + g2 / 6, g2]).to(torch.float32)


def conv2d_f43_f32(x, w, bias=None, res=None, pre=PRE_NONE, pre_slope=0.0, scale=None, shift=None, post=POST_NONE,
                   post_slope=0.0, lengths=None):
    """conv2d (k = 3) computed in float32 as F(4,3) along the map rows and direct along the columns: V = B^T d of the
    pre-activated, zero-padded input rows 4k - 1 .. 4k + 4, six planes m_p = sum_{c,kx} U_p V_p, y = A^T m, then bias,
    residual and the post-activation.  x (B, Cin, H, W), w (Cout, Cin, 3, 3) -> (B, Cout, H, W) float32 (NaN past a
    row's own height when `lengths` is given)."""
    if lengths is not None:
        return _by_rows(lambda xb, rb: conv2d_f43_f32(xb, w, bias, rb, pre, pre_slope, scale, shift, post, post_slope).double(),
                        x, res, lengths, lambda n: n).float()
    assert tuple(w.shape[2:]) == (3, 3)
    B, Cin, Hh, W = x.shape
    f32 = torch.float32
    xa = x.to(f32)
    if pre == PRE_AFFINE_LRELU:
        xa = xa * scale.to(f32).reshape(1, -1, 1, 1) + shift.to(f32).reshape(1, -1, 1, 1)
    if pre in (PRE_LRELU, PRE_AFFINE_LRELU):
        xa = torch.where(xa > 0, xa, xa * torch.tensor(float(pre_slope), dtype=f32))
    nblk = (Hh + 3) // 4
    xp = torch.zeros((B, Cin, 4 * nblk + 2, W + 2), dtype=f32)
    xp[:, :, 1:1 + Hh, 1:1 + W] = xa
    d = xp.unfold(2, 6, 4)                              # (B, Cin, nblk, W + 2, 6): rows 4k - 1 .. 4k + 4 of quad-row k
    d0, d1, d2, d3, d4, d5 = (d[..., j] for j in range(6))
    V = [4 * d0 - 5 * d2 + d4, -4 * d1 - 4 * d2 + d3 + d4, 4 * d1 - 4 * d2 - d3 + d4,
         -2 * d1 - d2 + 2 * d3 + d4, 2 * d1 - d2 - 2 * d3 + d4, 4 * d1 - 5 * d3 + d5]
    U = _f43_weights(w)
    m = []
    for p in range(6):
        acc = torch.zeros((B, w.shape[0], nblk, W), dtype=f32)
        for kx in range(3):
            acc = acc + torch.einsum("nc,bckw->bnkw", U[p, :, :, kx], V[p][..., kx:kx + W])
        m.append(acc)
    y = torch.stack([m[0] + m[1] + m[2] + m[3] + m[4], m[1] - m[2] + 2 * (m[3] - m[4]), m[1] + m[2] + 4 * (m[3] + m[4]),
                     m[1] - m[2] + 8 * (m[3] - m[4]) + m[5]], dim=3)          # (B, Cout, nblk, 4, W)
    y = y.reshape(B, w.shape[0], 4 * nblk, W)[:, :, :Hh]
    if bias is not None:
        y = y + bias.to(f32).reshape(1, -1, 1, 1)
    if res is not None:
        y = y + res.to(f32)
    return conv_post(y, post, post_slope)


# --------------------------------------------------------------------------------------
# the transposed 1-D convolution as Winograd F(3,2) along the input axis, in fp32 (the error yardstick of convtw_kernel)
# --------------------------------------------------------------------------------------
# Same spirit as conv2d_f43_f32: a plain fp32 statement of the algorithm the header of voicefixer_amd/csrc/vfx_convtw.inc
# writes out, every operation separately rounded, the bias added after the output transform.  The reference, not a model
# of the kernel: tests/test_convtw_gpu.py allows the device MARGIN times this statement's own figure.
def _f32_tr_weights(w, stride):
    """U = G g for every output phase r, g0 = w[r + s], g1 = w[r], formed in float64 and rounded once (as
    packing.pack_wino32_tr does): w (Cin, Cout, 2 s) -> (4 planes, Cin, Cout, s phases) float32."""
    s = stride
    g0, g1 = w[:, :, s:].to(torch.float64), w[:, :, :s].to(torch.float64)
    return torch.stack([g0, (g0 + g1) * 0.5, (g0 - g1) * 0.5, g1]).to(torch.float32)


def convtr1d_f32_f32(x, w, bias=None, stride=2, lengths=None):
    """convtr1d (no activations) computed in float32 as F(3,2) along the input axis: every output phase r is the two-tap
    correlation out[q s + r - pad] = w[r + s] x[q - 1] + w[r] x[q], q = 0 .. Lin; three consecutive q share d_j =
    x[3T - 1 + j]: V = B^T d, four planes m_k = sum_ci U_k V_k, y(3T) = m0 + m1 + m2, y(3T + 1) = m1 - m2, y(3T + 2) =
    m1 + m2 + m3, then the bias.  x (B, Cin, Lin), w (Cin, Cout, 2 s) -> (B, Cout, s Lin) float32 (NaN past a row's own
    end when `lengths` is given)."""
    if lengths is not None:
        return _by_rows(lambda xb, rb: convtr1d_f32_f32(xb, w, bias, stride).double(), x, None, lengths,
                        lambda n: n * stride).float()
    s = stride
    assert w.shape[2] == 2 * s
    f32 = torch.float32
    B, Cin, Lin = x.shape
    pad = s // 2 + s % 2
    nT = (Lin + 1 + 2) // 3                             # triples of q = 0 .. Lin
    xp = torch.zeros((B, Cin, 3 * nT + 2), dtype=f32)
    xp[:, :, 1:1 + Lin] = x.to(f32)
    d = xp.unfold(2, 4, 3)                              # (B, Cin, nT, 4): x[3T - 1 .. 3T + 2]
    d0, d1, d2, d3 = (d[..., j] for j in range(4))
    V = [d0 - d2, d1 + d2, d2 - d1, d3 - d1]
    U = _f32_tr_weights(w, s)
    m = [torch.einsum("cnr,bct->bnrt", U[k], V[k]) for k in range(4)]       # (B, Cout, s, nT)
    y = torch.stack([m[0] + m[1] + m[2], m[1] - m[2], m[1] + m[2] + m[3]], dim=4)      # (B, Cout, s, nT, 3): q = 3T + i
    y = y.permute(0, 1, 3, 4, 2).reshape(B, w.shape[1], 3 * nT * s)[:, :, pad:pad + s * Lin]    # position q s + r - pad
    if bias is not None:
        y = y + bias.to(f32).reshape(1, -1, 1)
    return y.contiguous()


# --------------------------------------------------------------------------------------
# one ResStack layer, and the dilated 1-D convolution as Winograd F(4,3) in fp32 (the yardstick of resblk4_kernel / resblk4s_kernel)
# --------------------------------------------------------------------------------------
def resblock(x, w1, b1, w2, b2, dilation, slope=0.01, post=POST_NONE, post_slope=0.0, lengths=None, magnitude=False):
    """vfx_resblock_f32 / vfx_resblock_wino4_f32: post(x + b2 + conv_k3_d1(lrelu(b1 + conv_k3_dil(lrelu(x))))), both
    convolutions zero-padded at the row's own ends, as two conv1d.  x (B, C, L), w1 / w2 (C, C, 3) -> (B, C, L) float64.
    `magnitude=True`: M = |x| + |b2| + sum |w2| mag1 with mag1 = sum |w1| |lrelu(x)| + |b1| the first convolution's own
    magnitude (zero outside the row): the first-order size of what one relative rounding error per partial sum of
    either convolution can do to an output (|lrelu(v)| <= |v|, and the leaky ReLU's slope is at most 1)."""
    if lengths is not None:
        return _by_rows(lambda xb, rb: resblock(xb, w1, b1, w2, b2, dilation, slope, post, post_slope, None, magnitude),
                        x, None, lengths, lambda n: n)
    mid = conv1d(x, w1, b1, None, dilation, pre=PRE_LRELU, pre_slope=slope, magnitude=magnitude)
    if magnitude:
        return conv1d(mid, w2, b2, x, 1, magnitude=True)
    return conv1d(mid, w2, b2, x, 1, pre=PRE_LRELU, pre_slope=slope, post=post, post_slope=post_slope)


def _f43_weights_1d(w, dtype):
    """U = G w along the taps, formed in float64 and rounded once to `dtype` (as packing.pack_wino4 does):
    w (Cout, Cin, 3) -> (6 planes, Cout, Cin)."""
    g0, g1, g2 = (w[:, :, t].to(torch.float64) for t in range(3))
    return torch.stack([g0 / 4, -(g0 + g1 + g2) / 6, -(g0 - g1 + g2) / 6, g0 / 24 + g1 / 12 + g2 / 6,
                        g0 / 24 - g1 / 12 + g2 / 6, g2]).to(dtype)


def conv1d_f43_f32(x, w, bias=None, res=None, dilation=1, pre=PRE_NONE, pre_slope=0.0, post=POST_NONE, post_slope=0.0,
                   lengths=None, dtype=torch.float32):
    """conv1d (k = 3, zero padding) computed in `dtype` as dilated Winograd F(4,3) with the standard matrices (the header of
    voicefixer_amd/csrc/vfx_convwg.inc writes them out): a quad is four outputs a dilation apart, positions
    4d blk + i d + r (i = 0 .. 3); its six inputs are d_j = pre(x)[4d blk + r + (j - 1) d]; V = B^T d, six planes
    m_p = sum_c U_p V_p (one chain over the channels), y = A^T m, then bias, residual and the post-activation.  Every
    operation is separately rounded.  The reference yardstick, not a model of a kernel.  x (B, Cin, L), w (Cout, Cin, 3)
    -> (B, Cout, L) of `dtype` (NaN past a row's own end when `lengths` is given)."""
    if lengths is not None:
        return _by_rows(lambda xb, rb: conv1d_f43_f32(xb, w, bias, rb, dilation, pre, pre_slope, post, post_slope, None,
                                                      dtype).double(), x, res, lengths, lambda n: n).to(dtype)
    assert w.shape[2] == 3 and pre in (PRE_NONE, PRE_LRELU)
    B, Cin, L = x.shape
    dl = dilation
    xa = x.to(dtype)
    if pre == PRE_LRELU:
        xa = torch.where(xa > 0, xa, xa * torch.tensor(float(pre_slope), dtype=dtype))
    nblk = (L + 4 * dl - 1) // (4 * dl)
    xp = torch.zeros((B, Cin, (4 * nblk + 2) * dl), dtype=dtype)
    xp[:, :, dl:dl + L] = xa
    d = xp.reshape(B, Cin, 4 * nblk + 2, dl).unfold(2, 6, 4)        # (B, Cin, nblk, d, 6): positions 4d blk + r + (j - 1) d
    d0, d1, d2, d3, d4, d5 = (d[..., j] for j in range(6))
    V = [4 * d0 - 5 * d2 + d4, -4 * d1 - 4 * d2 + d3 + d4, 4 * d1 - 4 * d2 - d3 + d4,
         -2 * d1 - d2 + 2 * d3 + d4, 2 * d1 - d2 - 2 * d3 + d4, 4 * d1 - 5 * d3 + d5]
    U = _f43_weights_1d(w, dtype)
    m = [torch.einsum("nc,bckr->bnkr", U[p], V[p]) for p in range(6)]
    y = torch.stack([m[0] + m[1] + m[2] + m[3] + m[4], m[1] - m[2] + 2 * (m[3] - m[4]), m[1] + m[2] + 4 * (m[3] + m[4]),
                     m[1] - m[2] + 8 * (m[3] - m[4]) + m[5]], dim=3)           # (B, Cout, nblk, 4, d)
    y = y.reshape(B, w.shape[0], 4 * nblk * dl)[:, :, :L]
    if bias is not None:
        y = y + bias.to(dtype).reshape(1, -1, 1)
    if res is not None:
        y = y + res.to(dtype)
    return conv_post(y, post, post_slope).contiguous()


def resblock_f43_f32(x, w1, b1, w2, b2, dilation, slope=0.01, post=POST_NONE, post_slope=0.0, lengths=None,
                     dtype=torch.float32):
    """resblock as two conv1d_f43_f32: the dilated half, its result rounded to `dtype` (and, every row being taken alone,
    absent outside the row: the second half's zero padding), then the dilation-1 half with x as the residual."""
    if lengths is not None:
        return _by_rows(lambda xb, rb: resblock_f43_f32(xb, w1, b1, w2, b2, dilation, slope, post, post_slope, None,
                                                        dtype).double(), x, None, lengths, lambda n: n).to(dtype)
    mid = conv1d_f43_f32(x, w1, b1, None, dilation, PRE_LRELU, slope, dtype=dtype)
    return conv1d_f43_f32(mid, w2, b2, x, 1, PRE_LRELU, slope, post, post_slope, dtype=dtype)


def quad_figure(got, ref, mag, lipschitz=1.0):
    """The figure natural to F(4,3), whose four vertically adjacent outputs share six products and six input rows:
    |got - ref| / M with M the maximum of lipschitz * magnitude + |ref| over the outputs of the same quad -- map rows
    4k .. 4k + 3 of one batch row (cut at that row's own height: where ref is NaN), same channel and column.  Dense maps
    (B, C, H, W).  Returns (max, sum of squares, count), like conv_error, and is never larger than it."""
    ok = ~torch.isnan(ref)
    den = torch.where(ok, lipschitz * mag + ref.abs(), torch.zeros_like(ref))
    B, Cn, Hh, W = ref.shape
    Hp = (Hh + 3) // 4 * 4
    dp = torch.zeros((B, Cn, Hp, W), dtype=den.dtype)
    dp[:, :, :Hh] = den
    M = dp.reshape(B, Cn, Hp // 4, 4, W).amax(dim=3, keepdim=True).expand(B, Cn, Hp // 4, 4, W).reshape(B, Cn, Hp, W)[:, :, :Hh]
    e = (got.to(torch.float64) - ref).abs() / M.clamp(min=1e-300)
    e = torch.where(ok, e, torch.zeros_like(e))
    bad = torch.isnan(got.to(torch.float64)) & ok
    mx = float("inf") if bool(bad.any()) else float(e.max())
    return mx, float((e * e).sum()), int(ok.sum())
