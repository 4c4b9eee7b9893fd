"""The kernels around the convolutions -- the GRU recurrence, the STFT / mel front-end and the per-row (ragged-batch)
bookkeeping kernels -- each compared on its own with the float64 statement of the same operator in
oracle/f64_reference.py, at production lengths and at the ends of ragged rows, with NaN canaries on every buffer a kernel
must not read or write past.  Every test prints one ``SEQERR`` line with the measured error and its bound.  Needs an MI355X."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from voicefixer_amd import ops, packing, weights  # noqa: E402
from oracle import oracle, f64_reference as ref64  # noqa: E402  (checkers only)

DEV = "cuda"
NAN = float("nan")


def _report(name, **vals):
    print("SEQERR %s %s" % (name, " ".join("%s=%.3g" % kv for kv in vals.items())))


def _rows_dev(lengths):
    return torch.tensor(lengths, dtype=torch.int32, device=DEV)


# --------------------------------------------------------------------------------------
# 1. recurrence: vfx_gru_bidir_f32 (one workgroup per sequence) and vfx_gru_bidir2_f32 (two CUs per sequence)
# --------------------------------------------------------------------------------------
# Bound: the kernel's max |error| and its RMS error against the float64 nn.GRU <= GRU_MARGIN x those of the fp32
# restatement of the same recurrence (oracle._gru_dir in float32, fed the same fp32 gi), measured in the test on the same
# case, with the floors below.  The restatement's max error is 1.2e-7 .. 7e-7 (W_hh x 4: up to 1.6e-6 at B 60) and does
# not grow with T (the recurrence is contracting: rounding does not accumulate); the kernels measured 1.2e-7 .. 1.0e-6 on
# the MI355X, 0.4x .. 1.5x the restatement.  An error that grows with T, or one confined to a row's last frames, exceeds
# the bound; the floors (about 8 ulp of a hidden value near 1 for the max, 4 ulp for the RMS) only matter when the
# restatement happens to be exceptionally accurate.
GRU_MARGIN = 4.0
GRU_FLOOR = 5e-7
GRU_RMS_FLOOR = 2.5e-7

_STATE = {}


def _restorer_state():
    if "rsd" not in _STATE:
        _STATE["rsd"] = weights.seeded_restorer_state(4321)
    return _STATE["rsd"]


def _gru_case(B, T, whh_scale, seed):
    """x, the float64 layer (seeded restorer state, denoiser.7.gru layer 0, |w| <= 1/16, b_hh != 0), gi in float64."""
    p = ref64.gru_params(_restorer_state(), "denoiser.7.gru", 0, whh_scale)
    assert (p["bias_hh_l0"] != 0).all() and (p["bias_hh_l0_reverse"] != 0).all()   # b_hn inside r * (.) is visible
    x = torch.randn((B, T, 512), generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    return x, p, ref64.gru_input_projection(x, p)


def _gru_fp32_restatement(gi32, p, lengths):
    """oracle._gru_dir in float32 on the kernels' own fp32 gi (W_ih = identity, b_ih = 0: x @ I is exact), every row
    alone: the recurrence only.  (B, T, 512) with zeros past a row."""
    B, T, _ = gi32.shape
    eye, zero = torch.eye(768), torch.zeros(768)
    out = torch.zeros((B, T, 512), dtype=torch.float64)
    for b, t in enumerate(lengths):
        g = gi32[b:b + 1, :t]
        fwd = oracle._gru_dir(g[..., :768], eye, p["weight_hh_l0"].float(), zero, p["bias_hh_l0"].float(), False)
        bwd = oracle._gru_dir(g[..., 768:], eye, p["weight_hh_l0_reverse"].float(), zero, p["bias_hh_l0_reverse"].float(),
                              True)
        out[b, :t] = torch.cat([fwd, bwd], -1)[0].double()
    return out


def _run_gru(kernel, gi32, p, T, lengths, pad):
    """Launch one kernel on gi32 (B, T, 1536) into a NaN-prefilled (B, 512, T + pad) output; returns it on the host."""
    B = gi32.shape[0]
    bhh = torch.stack([p["bias_hh_l0"], p["bias_hh_l0_reverse"]]).float().to(DEV)
    w, wr = p["weight_hh_l0"].float(), p["weight_hh_l0_reverse"].float()
    out = torch.full((B, 512, T + pad), NAN, device=DEV)
    ov = out[:, :, :T]
    if lengths is not None:
        ops.with_rows(ov, _rows_dev(lengths))
    gi = gi32.contiguous().to(DEV)
    if kernel == "one_wg":
        ops.gru_bidir(gi, packing.pack_gru_whh(w, wr, *ops.gru_layout()).to(DEV), bhh, ov, T)
        torch.cuda.synchronize()
    else:
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        keep = ops.gru_bidir2(gi, torch.stack([w.t().contiguous(), wr.t().contiguous()]).to(DEV), bhh, ov, T, err)
        torch.cuda.synchronize()
        assert int(err.item()) == 0, "two-CU GRU: a partner workgroup never answered"
        del keep
    return out.cpu()


def _check_gru(name, got, want, r32, lengths, T):
    """got (B, 512, T + pad) channel-major; want / r32 (B, T, 512).  Frames < T_b within the bound, the rest still NaN."""
    err, err_ref = [], []
    for b, t in enumerate(lengths):
        g = got[b, :, :t].t().double()
        assert torch.isfinite(g).all(), "row %d: non-finite output inside the row" % b
        assert torch.isnan(got[b, :, t:]).all(), "row %d: frames >= %d were written" % (b, t)
        err.append((g - want[b, :t]).flatten())
        err_ref.append((r32[b, :t] - want[b, :t]).flatten())
    err, err_ref = torch.cat(err), torch.cat(err_ref)
    worst, worst_ref = err.abs().max().item(), err_ref.abs().max().item()
    rms, rms_ref = err.pow(2).mean().sqrt().item(), err_ref.pow(2).mean().sqrt().item()
    bound, rms_bound = max(GRU_MARGIN * worst_ref, GRU_FLOOR), max(GRU_MARGIN * rms_ref, GRU_RMS_FLOOR)
    _report(name, kernel_max=worst, fp32_restatement_max=worst_ref, bound=bound, kernel_rms=rms,
            fp32_restatement_rms=rms_ref, rms_bound=rms_bound)
    assert worst <= bound, "%s: max |err| %.3g > %.3g (fp32 restatement %.3g)" % (name, worst, bound, worst_ref)
    assert rms <= rms_bound, "%s: RMS err %.3g > %.3g (fp32 restatement %.3g)" % (name, rms, rms_bound, rms_ref)


def _gru_expected(B, T, whh_scale, seed, lengths):
    key = (B, T, whh_scale, seed, tuple(lengths) if lengths else None)
    if key not in _STATE:
        x, p, gi = _gru_case(B, T, whh_scale, seed)
        rl = lengths or [T] * B
        want = ref64.gru_bidir(x, p, lengths)
        gi32 = gi.float()
        if lengths is not None:
            for b, t in enumerate(lengths):
                gi32[b, t:] = NAN          # the kernel must not read past a row
        _STATE[key] = (p, gi32, want, _gru_fp32_restatement(gi32, p, rl))
    return _STATE[key]


GRU_KERNELS = ["one_wg", "two_cu"]


@pytest.mark.parametrize("kernel", GRU_KERNELS)
@pytest.mark.parametrize("whh_scale", [1.0, 4.0])
@pytest.mark.parametrize("B,T", [(2, 3), (2, 37), (2, 1001), (1, 3001)])
def test_gru_production_lengths_against_float64(kernel, whh_scale, B, T):
    """T 3 (the shortest legal segment), 37, 1001 (10 s) and 3001 (a 30 s segment); W_hh x 4 saturates the gates."""
    p, gi32, want, r32 = _gru_expected(B, T, whh_scale, 100 + T, None)
    got = _run_gru(kernel, gi32, p, T, None, 5)
    _check_gru("gru_%s_B%d_T%d_whh%g" % (kernel, B, T, whh_scale), got, want, r32, [T] * B, T)


@pytest.mark.parametrize("kernel", GRU_KERNELS)
def test_gru_full_launch_against_float64(kernel):
    """B = ops.GRU2_MAX_B: one full two-CU launch (240 workgroups)."""
    B, T = ops.GRU2_MAX_B, 101
    p, gi32, want, r32 = _gru_expected(B, T, 1.0, 7, None)
    got = _run_gru(kernel, gi32, p, T, None, 3)
    _check_gru("gru_%s_B%d_T%d" % (kernel, B, T), got, want, r32, [T] * B, T)


GRU_RAGGED_T = 1001
GRU_RAGGED_ROWS = [GRU_RAGGED_T, GRU_RAGGED_T - 1, 3, 64, 65, GRU_RAGGED_T // 2 + 1, 2]


@pytest.mark.parametrize("whh_scale", [1.0, 4.0])
@pytest.mark.parametrize("kernel", GRU_KERNELS)
def test_gru_ragged_rows_against_packed_float64(kernel, whh_scale):
    """out->rows: the reverse direction of every row starts at the row's own last frame (the float64 reference runs the
    batch through pack_padded_sequence), gi frames >= T_b are NaN and must not be read, out frames >= T_b stay NaN."""
    T = GRU_RAGGED_T
    p, gi32, want, r32 = _gru_expected(len(GRU_RAGGED_ROWS), T, whh_scale, 11, GRU_RAGGED_ROWS)
    got = _run_gru(kernel, gi32, p, T, GRU_RAGGED_ROWS, 4)
    _check_gru("gru_%s_ragged_whh%g" % (kernel, whh_scale), got, want, r32, GRU_RAGGED_ROWS, T)


def test_denoiser_gru_group_walk_against_float64_oracle():
    """RestorerEngine.denoiser with t_rows and gru_group = 3 for B = 7: the gi[b0:b1] / t_rows[b0:b1] slicing of the group
    walk.  Every row of the mask against oracle.denoiser in float64 on that row alone; bound = GRU_MARGIN x the fp32
    oracle's own error on the same rows (7.8e-8; the engine measured 9.0e-8), floor GRU_FLOOR."""
    from voicefixer_amd import engine
    rsd = _restorer_state()
    eng = engine.RestorerEngine(rsd, DEV)
    eng.gru_group = 3
    T = 301
    rows = [T, T - 1, 3, 64, 65, T // 2 + 1, 2]
    g = torch.Generator().manual_seed(21)
    mel = 10 ** (torch.rand((len(rows), T, 128), generator=g) * 4 - 3)
    for b, t in enumerate(rows):
        mel[b, t:] = 0.0
    mask = eng.denoiser(mel.to(DEV), T, _rows_dev(rows))
    torch.cuda.synchronize()
    got = mask.cpu()
    assert int(eng.gru_err.item()) == 0
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in rsd.items()}
    worst, worst_ref = 0.0, 0.0
    with torch.no_grad():
        for b, t in enumerate(rows):
            m = mel[b:b + 1, None, :t]
            want = oracle.denoiser(m.double(), sd64)[0, 0]
            r32 = oracle.denoiser(m, rsd)[0, 0].double()
            gb = got[b, :, :t].t().double()
            assert torch.isfinite(gb).all()
            worst = max(worst, (gb - want).abs().max().item())
            worst_ref = max(worst_ref, (r32 - want).abs().max().item())
    bound = max(GRU_MARGIN * worst_ref, GRU_FLOOR)
    _report("denoiser_group3_ragged", kernel_max=worst, fp32_restatement_max=worst_ref, bound=bound)
    assert worst <= bound


# --------------------------------------------------------------------------------------
# 2. front end
# --------------------------------------------------------------------------------------
def _signal(kind, n, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64)
    if kind == "noise_sine_quiet":       # noise + sine with a stretch 60 dB down
        x = 0.1 * torch.randn(n, generator=g, dtype=torch.float64) + 0.3 * torch.sin(2 * math.pi * 440.0 * t / 44100)
        x[n // 3: n // 3 + max(n // 4, 3000)] *= 1e-3
    elif kind == "dc":                   # a DC offset under weak noise
        x = 0.25 + 0.05 * torch.randn(n, generator=g, dtype=torch.float64)
    elif kind == "sine":                 # pure sine: the far side lobes reach the 1e-8 power clamp
        x = 0.5 * torch.sin(2 * math.pi * 1234.5 * t / 44100)
    elif kind == "full_scale":           # content at full scale
        x = torch.clamp(1.5 * torch.randn(n, generator=g, dtype=torch.float64), -0.999, 0.999)
    else:
        raise ValueError(kind)
    return x.float()


# Bounds in the domains the model consumes (log10 mel for the UNet input, 20 log10 for the vocoder cond), per bin, in
# two bands of the bin's float64 value relative to the largest bin of its frame:
#   STRONG: >= 1e-3 of the frame maximum: the FFT's fp32 rounding is far below the bin;
#   WEAK:   1e-6 .. 1e-3 of it: the bin is within reach of the fp32 transform's noise floor (about 1e-7 of the frame's
#           energy), e.g. the far side lobes of a pure sine, which sit at the 1e-8 power clamp in float64 and at
#           fp32 noise in any fp32 transform.
# Plus the relative norm of every row.  Set from the first measurement on the MI355X (radix-2 Stockham FFT in fp32, twiddle
# table), every signal and length of the tests below:
#   STRONG: device max 1.5e-5 (pure sine, N 1465; 3.8e-6 for the other signals), CPU fp32 restatement 1.1e-5.  A bin at
#           1e-3 of its frame maximum carrying fp32 noise of 1e-7 of the maximum is off by 1e-4 relative = 4.3e-5 in
#           log10: the bound is that rounding model, 2.7x the largest measured value.
#   WEAK:   device max 3.3e-3 (the pure sine's side lobes at the power clamp; 6.6e-6 for every other signal), CPU fp32
#           restatement 4.5e-3: 3x the largest measured value.
#   REL_NORM: device max 1.3e-7, CPU fp32 restatement 1.2e-7; 7.5x (the suite's older test_stft_mel allows 1e-5).
STFT_LOG10_STRONG = 4e-5
STFT_LOG10_WEAK = 1e-2
STFT_REL_NORM = 1e-6


def _mel_errors(got, want):
    """(max |dlog10| over bins >= 1e-3 x frame max, the same over 1e-6 .. 1e-3, relative norm)."""
    got, want = got.double(), want.double()
    fmax = want.amax(dim=-1, keepdim=True)
    d = (torch.log10(torch.clamp(got, min=1e-30)) - torch.log10(want)).abs()
    strong = want >= 1e-3 * fmax
    weak = (want >= 1e-6 * fmax) & ~strong
    ds = d[strong].max().item() if strong.any() else 0.0
    dw = d[weak].max().item() if weak.any() else 0.0
    return ds, dw, ((got - want).norm() / want.norm()).item()


def _check_mel(name, got, want, r32):
    assert torch.isfinite(got).all() and (got >= 0).all()
    ds, dw, rel = _mel_errors(got, want)
    rs, rw, rrel = _mel_errors(r32, want)
    _report(name, dlog10_strong=ds, dlog10_weak=dw, rel=rel, fp32_dlog10_strong=rs, fp32_dlog10_weak=rw, fp32_rel=rrel)
    assert rel <= STFT_REL_NORM, "%s: relative norm %.3g" % (name, rel)
    assert ds <= STFT_LOG10_STRONG, "%s: |dlog10| %.3g on a bin >= 1e-3 of its frame max" % (name, ds)
    assert dw <= STFT_LOG10_WEAK, "%s: |dlog10| %.3g on a bin 1e-6 .. 1e-3 of its frame max" % (name, dw)


STFT_LENGTHS = [1025, 1025 + 440, 441 * 40, 441 * 40 + 440, 441000, 1323000]
SIGNAL_PAIRS = [("noise_sine_quiet", "dc"), ("sine", "full_scale")]


@pytest.mark.parametrize("kinds", SIGNAL_PAIRS, ids=["-".join(k) for k in SIGNAL_PAIRS])
@pytest.mark.parametrize("n", STFT_LENGTHS)
def test_stft_mel_against_float64(n, kinds):
    """vfx_stft_mel_f32 against torch.stft in float64 (centre, reflect, periodic hann) + the HTK filterbank."""
    wav = torch.stack([_signal(k, n, 40 + i) for i, k in enumerate(kinds)])
    T = 1 + n // 441
    wd = torch.full((2, n + 7), NAN, device=DEV)      # NaN past N: the reflect must turn at N - 1
    wd[:, :n] = wav.to(DEV)
    flat = torch.full(((2 * T + 1) * 128,), NAN, device=DEV)   # one frame of NaN after the last row
    ops.stft_mel(wd, flat[:2 * T * 128].view(2, T, 128), n)
    torch.cuda.synchronize()
    assert torch.isnan(flat[2 * T * 128:]).all()
    got = flat[:2 * T * 128].view(2, T, 128).cpu()
    want = ref64.stft_mel(wav, [n, n])
    r32 = oracle.wav_to_mel(wav)[:, 0]
    for b in range(2):
        _check_mel("stft_mel_N%d_%s" % (n, kinds[b]), got[b], want[b], r32[b])


STFT_ROW_KINDS = ["noise_sine_quiet", "dc", "sine", "full_scale", "noise_sine_quiet", "sine"]


def test_stft_mel_rows_equal_the_plain_kernel_row_by_row():
    """vfx_stft_mel_rows_f32 on one batch whose rows have the lengths above: samples past each row's end are NaN (the
    reflect must turn at the row's own end), mel frames >= T_b stay NaN, every row equals vfx_stft_mel_f32 on that row alone
    bit for bit, and the float64 check holds row by row."""
    lengths = STFT_LENGTHS
    B, nmax = len(lengths), max(lengths)
    wav = torch.full((B, nmax + 9), NAN)
    for b, (n, k) in enumerate(zip(lengths, STFT_ROW_KINDS)):
        wav[b, :n] = _signal(k, n, 70 + b)
    wd = wav.to(DEV)
    T = 1 + nmax // 441
    mel = torch.full((B, T, 128), NAN, device=DEV)
    ops.stft_mel_rows(wd, mel, _rows_dev(lengths), T)
    alone = []
    for b, n in enumerate(lengths):
        m = torch.full((1, 1 + n // 441, 128), NAN, device=DEV)
        ops.stft_mel(wd[b:b + 1], m, n)
        alone.append(m)
    torch.cuda.synchronize()
    got = mel.cpu()
    for b, n in enumerate(lengths):
        tb = 1 + n // 441
        assert torch.equal(got[b, :tb], alone[b][0].cpu()), "row %d (n %d) differs from the plain kernel" % (b, n)
        assert torch.isnan(got[b, tb:]).all(), "row %d: frames >= %d were written" % (b, tb)
        x = wav[b:b + 1, :n]
        _check_mel("stft_mel_rows_n%d_%s" % (n, STFT_ROW_KINDS[b]), got[b, :tb], ref64.stft_mel(x, [n])[0],
                   oracle.wav_to_mel(x)[0, 0])


def test_oracle_front_end_against_float64():
    """ops.oracle_mel (vfx_peak_f32 + vfx_stft_mel_oracle_f32: zero padding, wav / peak, slaney mel) on two rows of
    different peaks.  A sample larger than either peak sits right after N: the peak and the frames must not see it."""
    n = 441 * 30 + 200
    wav = torch.stack([_signal("noise_sine_quiet", n, 80), 3.0 * _signal("full_scale", n, 81)])
    wd = torch.zeros((2, n + 16), device=DEV)
    wd[:, :n] = wav.to(DEV)
    wd[:, n] = 50.0
    got, T = ops.oracle_mel(wd, n)
    torch.cuda.synchronize()
    got = got.cpu()
    assert T == 1 + n // 441 and got.shape == (2, T, 128)
    want = ref64.oracle_mel(wav, n)
    x = wav / wav.abs().amax(dim=1, keepdim=True)
    fb32 = ref64.slaney_filterbank().float()
    win = torch.hann_window(2048, periodic=True)
    r32 = torch.stft(x, 2048, 441, window=win, center=True, pad_mode="constant", return_complex=True).abs()
    r32 = r32.transpose(1, 2) @ fb32
    for b in range(2):
        _check_mel("oracle_mel_row%d" % b, got[b], want[b], r32[b])


# --------------------------------------------------------------------------------------
# 3. per-row bookkeeping kernels
# --------------------------------------------------------------------------------------
def _cond_input(B, T, lengths, seed):
    """mel (B, T, 128): 1e-7 .. 1e4 with exact zeros, negatives, values on the 1e-5 floor and on both clip bounds
    (after the mel-weight division); frames >= T_b are NaN (must not be read)."""
    g = torch.Generator().manual_seed(seed)
    w = ref64.mel_weight().float()
    mel = 10 ** (torch.rand((B, T, 128), generator=g) * 11 - 7)
    mel[:, 0::7, 0::5] = 0.0
    mel[:, 1::7, 3::11] *= -1.0
    mel[:, 2::7, :] = (1e-5 * w.double()).float()                  # on the 1e-5 floor
    mel[:, 3::7, :] = (10 ** (-115 / 20 + 1) * w.double()).float()  # S = -115: c = -4
    mel[:, 4::7, :] = (10.0 * w.double()).float()                  # S = 0: c = +4
    for b, t in enumerate(lengths):
        mel[b, t:] = NAN
    return mel


def test_mel_to_cond_rows_against_float64():
    """vfx_mel_to_cond_rows_f32 (ops.mel_to_cond with t_rows): rows of both parities; frames T_b .. T_b + T_b % 2 + 3 are
    exactly -4, nothing is written past them.  Bound: MEL_COND_MARGIN x the fp32 oracle.mel_to_cond's own error on
    the same rows (3e-6 on a 10 s mel), floor 2e-6."""
    T = 1001
    lengths = [T, T - 1, 64, 65, 3, 2, 500]
    B = len(lengths)
    mel = _cond_input(B, T, lengths, 90)
    Tc = T + T % 2 + 4
    pad = 8
    cond = torch.full((B, 128, Tc + pad), NAN, device=DEV)
    ops.mel_to_cond(mel.to(DEV), cond, T, _rows_dev(lengths))
    torch.cuda.synchronize()
    got = cond.cpu()
    want = ref64.mel_to_cond(mel, lengths)
    worst, worst_ref = 0.0, 0.0
    for b, t in enumerate(lengths):
        tc = t + t % 2 + 4
        assert torch.equal(got[b, :, t:tc], torch.full((128, tc - t), -4.0)), "row %d: tail frames are not -4" % b
        assert torch.isnan(got[b, :, tc:]).all(), "row %d: frames >= %d were written" % (b, tc)
        gb = got[b, :, :t].double()
        assert torch.isfinite(gb).all()
        worst = max(worst, (gb - want[b][:, :t]).abs().max().item())
        r32 = oracle.mel_to_cond(mel[b:b + 1, None, :t])[0, :, :t].double()
        worst_ref = max(worst_ref, (r32 - want[b][:, :t]).abs().max().item())
    bound = max(4.0 * worst_ref, 2e-6)
    _report("mel_to_cond_rows", kernel_max=worst, fp32_restatement_max=worst_ref, bound=bound)
    assert worst <= bound


# log10f of one fp32 product: a few ulp of max(1, |log10|)
UNET_IN_TOL = 1e-6


def test_unet_input_rows_against_float64():
    """vfx_unet_input_f32 with mask->rows: frames >= T_b are exactly 0 (all channels), bin 127 is exactly 0, frames < T_b
    match log10(max(., 1e-8)) in float64; mel and mask frames >= T_b are NaN and must not be read."""
    T, Tp, nch = 200, 256, 4
    lengths = [T, T - 1, 64, 65, 3, 2, 129]
    B = len(lengths)
    g = torch.Generator().manual_seed(95)
    mel = 10 ** (torch.rand((B, T, 128), generator=g) * 12 - 10)      # 1e-10 .. 1e2: the 1e-8 floor is crossed
    mel[:, ::5, ::3] = 0.0
    mask = torch.rand((B, T, 128), generator=g)
    mask[:, ::7, ::2] = 0.0
    for b, t in enumerate(lengths):
        mel[b, t:] = NAN
        mask[b, t:] = NAN
    mask_cm = torch.full((B, 128, T + 4), NAN, device=DEV)
    mask_cm[:, :, :T] = mask.transpose(1, 2).to(DEV)
    mv = ops.with_rows(mask_cm[:, :, :T], _rows_dev(lengths))
    u = torch.full((B, nch, Tp * 128), NAN, device=DEV)
    ops.unet_input(mel.to(DEV), mv, u, T, Tp)
    torch.cuda.synchronize()
    got = u.cpu().reshape(B, nch, Tp, 128)
    want = ref64.unet_input(mel, mask, lengths)
    assert (got[:, :, :, 127] == 0).all() and (got[:, 2:] == 0).all()
    worst = 0.0
    for b, t in enumerate(lengths):
        assert (got[b, :, t:] == 0).all(), "row %d: frames >= %d are not zero" % (b, t)
        gb = got[b, :2, :t, :127].double()
        assert torch.isfinite(gb).all()
        worst = max(worst, ((gb - want[b]).abs() / want[b].abs().clamp(min=1.0)).max().item())
    _report("unet_input_rows", kernel_max_rel=worst, bound=UNET_IN_TOL)
    assert worst <= UNET_IN_TOL


def test_post_rows_bit_exact():
    """vfx_post_rows_f32 with ly_rows: the peak rule (> 1) over the row's own ly_b samples, the centre trim from
    floor((ly_b - n_b) / 2), columns >= n_b untouched.  Bit-exact: fp32 division is correctly rounded, and the float64
    quotient of the same operands rounded once to fp32 is the same number."""
    g = torch.Generator().manual_seed(97)
    ly_rows = [44100, 44100 - 441, 30870, 22050, 20001, 20000]
    n_rows = [44000, 43000, 30000, 21000, 19998, 19999]   # d = 100, 659 (odd), 870, 1050, 3, 1 (odd)
    B, Ly = len(ly_rows), max(ly_rows) + 64
    n_max = max(n_rows)
    y = 0.2 * torch.randn((B, Ly), generator=g)
    y[0, 123] = 0.75                      # row 0: peak below 1 -> unchanged
    y[1] = torch.clamp(y[1], -0.99, 0.99)
    y[1, 40000] = 1.0                     # row 1: peak exactly 1.0 -> unchanged (the rule is > 1)
    y[2, 5000] = -3.7                     # row 2: negative peak above 1 in magnitude
    y[3, 100] = 2.5                       # row 3: peak 2.5 ...
    y[3, ly_rows[3]] = 40.0               # ... and a larger spike right after the row's end, which must not count
    y[4, 777] = 1.5
    y[5] *= 6.0                           # row 5: many samples above 1
    for b, ly in enumerate(ly_rows):
        y[b, ly + 1:] = 1e3 * (b + 1)     # everything past a row's end is larger than its peak
    out = torch.full((B, n_max + 16), NAN, device=DEV)
    ws = torch.empty((B,), dtype=torch.int32, device=DEV)
    ops.post_rows(y.to(DEV), Ly, out, _rows_dev(n_rows), n_max, ws, ly_rows=_rows_dev(ly_rows))
    torch.cuda.synchronize()
    got = out.cpu()
    want = ref64.post_rows(y, ly_rows, n_rows)
    for b, n in enumerate(n_rows):
        assert torch.equal(got[b, :n], want[b].float()), "row %d: not bit-exact (max diff %g)" % (
            b, (got[b, :n].double() - want[b]).abs().max().item())
        assert torch.isnan(got[b, n:]).all(), "row %d: columns >= %d were written" % (b, n)
    _report("post_rows", mismatches=0)


@pytest.mark.parametrize("T,Cn", [(37, 128), (1001, 128), (33, 77), (70, 50)])
def test_tm_to_cm_bit_exact(T, Cn):
    """vfx_tm_to_cm_f32: (B, T, C) -> a channel-major destination with a guard band on both sides of every row and a
    channel stride != T; the transpose is bit-exact and nothing outside [0, T) of any row is written."""
    B, G = 3, 12
    src = torch.randn((B, T, Cn), generator=torch.Generator().manual_seed(T + Cn))
    buf = torch.full((B, Cn, G + T + 5 + G), NAN, device=DEV)
    dst = buf[:, :, G:G + T]
    assert dst.stride(1) != T
    ops.tm_to_cm(src.to(DEV), dst, T, Cn)
    torch.cuda.synchronize()
    got = buf.cpu()
    assert torch.equal(got[:, :, G:G + T], src.transpose(1, 2))
    assert torch.isnan(got[:, :, :G]).all() and torch.isnan(got[:, :, G + T:]).all()
    _report("tm_to_cm_T%d_C%d" % (T, Cn), mismatches=0)
