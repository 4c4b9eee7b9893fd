"""The float64 statements of the four convolution entry points (oracle/f64_reference.py: conv1d, convtr1d, conv2d,
convtr2d_3x3s2, with their fused activations, bias, residual, per-row lengths and magnitudes) against the fp32 torch
operators on random inputs, and against the oracle's own modules (conv_block_res, decoder_block's transposed convolution,
the vocoder's UpsampleNet layer) with the seeded weights.  Keeps the references of tests/test_conv_taps_gpu.py honest
without a GPU."""
import pytest
import torch
import torch.nn.functional as F

from oracle import oracle, f64_reference as ref64
from voicefixer_amd import weights

TOL = 2e-5      # fp32 torch operator against the float64 statement, relative to the output peak


def _rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _close(got64, want32, tol=TOL):
    assert got64.dtype == torch.float64 and tuple(got64.shape) == tuple(want32.shape)
    err = (got64 - want32.double()).abs().max().item()
    assert err <= tol * max(1.0, want32.abs().max().item()), err


def _pre32(x, pre, slope, scale, shift):
    if pre == ref64.PRE_AFFINE_LRELU:
        shp = [1, -1] + [1] * (x.dim() - 2)
        x = x * scale.reshape(shp) + shift.reshape(shp)
    return F.leaky_relu(x, slope) if pre != ref64.PRE_NONE else x


def _post32(y, post, slope):
    if post == ref64.POST_LRELU:
        return F.leaky_relu(y, slope)
    if post == ref64.POST_ELU:
        return F.elu(y)
    if post == ref64.POST_TANH:
        return torch.tanh(y)
    if post == ref64.POST_SIGMOID:
        return torch.sigmoid(y)
    if post == ref64.POST_LRELU_SNAKE:
        u = F.leaky_relu(y, slope)
        return u + torch.sin(u)
    return y


@pytest.mark.parametrize("k,dil,reflect,pre,post", [
    (1, 1, False, ref64.PRE_NONE, ref64.POST_SIGMOID), (3, 1, False, ref64.PRE_LRELU, ref64.POST_ELU),
    (3, 9, False, ref64.PRE_AFFINE_LRELU, ref64.POST_LRELU), (7, 1, True, ref64.PRE_NONE, ref64.POST_LRELU_SNAKE),
    (5, 2, True, ref64.PRE_LRELU, ref64.POST_TANH), (3, 40, False, ref64.PRE_NONE, ref64.POST_NONE)])
def test_conv1d_statement_equals_torch(k, dil, reflect, pre, post):
    B, Cin, Cout, L = 3, 10, 6, 37                       # dilation 40 > L: the outer taps see padding only
    x, w = _rand((B, Cin, L), 1), _rand((Cout, Cin, k), 2, (Cin * k) ** -0.5)
    bias, res = _rand((Cout,), 3, 0.3), _rand((B, Cout, L), 4)
    scale, shift = 0.8 + 0.4 * torch.rand(Cin, generator=torch.Generator().manual_seed(5)), _rand((Cin,), 6, 0.3)
    p = (k - 1) // 2 * dil
    xa = _pre32(x, pre, 0.1, scale, shift)
    xp = F.pad(xa, (p, p), mode="reflect") if reflect else F.pad(xa, (p, p))
    want = _post32(F.conv1d(xp, w, bias, dilation=dil) + res, post, 0.2)
    kw = dict(dilation=dil, reflect=reflect, pre=pre, pre_slope=0.1, scale=scale, shift=shift, post=post, post_slope=0.2)
    _close(ref64.conv1d(x, w, bias, res, **kw), want)
    # magnitude: the same sum over absolute values, no post-activation
    mag = ref64.conv1d(x, w, bias, res, magnitude=True, **kw)
    xpa = xp.abs()
    _close(mag, F.conv1d(xpa, w.abs(), bias.abs(), dilation=dil) + res.abs())
    lin = ref64.conv1d(x, w, bias, res, **dict(kw, post=ref64.POST_NONE))
    assert (mag >= lin.abs() - 1e-12).all()
    # ragged rows: every row equals the row alone at its own length, reflect padding mirrors at the row's own end
    lengths = [37, 9, 20]
    if p < min(lengths) or not reflect:
        rag = ref64.conv1d(x, w, bias, res, lengths=lengths, **kw)
        for b, n in enumerate(lengths):
            alone = ref64.conv1d(x[b:b + 1, :, :n], w, bias, res[b:b + 1, :, :n], **kw)
            assert torch.equal(rag[b:b + 1, :, :n], alone) and torch.isnan(rag[b, :, n:]).all()


@pytest.mark.parametrize("s", [2, 3, 7])
def test_convtr1d_statement_equals_torch(s):
    B, Cin, Cout, Lin = 2, 12, 5, 23
    x, w, bias = _rand((B, Cin, Lin), 7), _rand((Cin, Cout, 2 * s), 8, (2 * Cin) ** -0.5), _rand((Cout,), 9, 0.3)
    want = F.conv_transpose1d(x + torch.sin(x), w, bias, stride=s, padding=s // 2 + s % 2, output_padding=s % 2)
    assert want.shape[2] == s * Lin
    _close(ref64.convtr1d(x + torch.sin(x), w, bias, s), want)
    want = F.leaky_relu(F.conv_transpose1d(F.leaky_relu(x, 0.2), w, bias, stride=s, padding=s // 2 + s % 2,
                                           output_padding=s % 2), 0.3)
    kw = dict(pre=ref64.PRE_LRELU, pre_slope=0.2, post=ref64.POST_LRELU, post_slope=0.3)
    _close(ref64.convtr1d(x, w, bias, s, **kw), want)
    _close(ref64.convtr1d(x, w, bias, s, magnitude=True, **kw),
           F.conv_transpose1d(F.leaky_relu(x, 0.2).abs(), w.abs(), bias.abs(), stride=s, padding=s // 2 + s % 2,
                              output_padding=s % 2))
    rag = ref64.convtr1d(x, w, bias, s, lengths=[23, 4], **kw)
    assert torch.equal(rag[1:, :, :4 * s], ref64.convtr1d(x[1:, :, :4], w, bias, s, **kw))
    assert torch.isnan(rag[1, :, 4 * s:]).all() and not torch.isnan(rag[0]).any()


@pytest.mark.parametrize("k,lp,pre,post", [(1, 3, ref64.PRE_NONE, ref64.POST_NONE), (3, 3, ref64.PRE_AFFINE_LRELU, ref64.POST_LRELU),
                                           (3, 1, ref64.PRE_AFFINE_LRELU, ref64.POST_NONE), (3, 5, ref64.PRE_NONE, ref64.POST_NONE)])
def test_conv2d_statement_equals_torch(k, lp, pre, post):
    B, Cin, Cout, H, W = 2, 9, 4, 6, (1 << lp) - 1
    x, w = _rand((B, Cin, H, W), 10), _rand((Cout, Cin, k, k), 11, (Cin * k * k) ** -0.5)
    bias, res = _rand((Cout,), 12, 0.3), _rand((B, Cout, H, W), 13)
    scale, shift = 0.8 + 0.4 * torch.rand(Cin, generator=torch.Generator().manual_seed(14)), _rand((Cin,), 15, 0.3)
    xa = _pre32(x, pre, 0.01, scale, shift)
    want = _post32(F.conv2d(xa, w, bias, padding=k // 2) + res, post, 0.01)
    kw = dict(pre=pre, pre_slope=0.01, scale=scale, shift=shift, post=post, post_slope=0.01)
    _close(ref64.conv2d(x, w, bias, res, **kw), want)
    _close(ref64.conv2d(x, w, bias, res, magnitude=True, **kw), F.conv2d(xa.abs(), w.abs(), bias.abs(), padding=k // 2) + res.abs())
    rag = ref64.conv2d(x, w, bias, res, lengths=[6, 2], **kw)
    assert torch.equal(rag[1:, :, :2], ref64.conv2d(x[1:, :, :2], w, bias, res[1:, :, :2], **kw))
    assert torch.isnan(rag[1, :, 2:]).all()
    # the pitch layout: pad column carried as `fill`, rows P apart
    pm = ref64.to_pitch(x, lp, fill=float("nan"))
    assert pm.shape == (B, Cin, H << lp)
    back = ref64.from_pitch(pm, H, lp)
    assert torch.equal(back[..., :W], x) and torch.isnan(back[..., W]).all()


@pytest.mark.parametrize("h,lp", [(1, 1), (2, 2), (5, 3)])
def test_convtr2d_statement_equals_torch(h, lp):
    B, Cin, Cout, W = 2, 7, 3, (1 << lp) - 1
    x, w = _rand((B, Cin, h, W), 16), _rand((Cin, Cout, 3, 3), 17, (2.25 * Cin) ** -0.5)
    scale, shift = 0.8 + 0.4 * torch.rand(Cin, generator=torch.Generator().manual_seed(18)), _rand((Cin,), 19, 0.3)
    xa = _pre32(x, ref64.PRE_AFFINE_LRELU, 0.0, scale, shift)
    want = F.conv_transpose2d(xa, w, stride=2)[:, :, :-1]
    assert want.shape[2:] == (2 * h, 2 * W + 1)
    kw = dict(pre=ref64.PRE_AFFINE_LRELU, pre_slope=0.0, scale=scale, shift=shift)
    _close(ref64.convtr2d_3x3s2(x, w, **kw), want)
    _close(ref64.convtr2d_3x3s2(x, w, magnitude=True, **kw), F.conv_transpose2d(xa.abs(), w.abs(), stride=2)[:, :, :-1])
    if h > 1:
        rag = ref64.convtr2d_3x3s2(x, w, lengths=[h, 1], **kw)
        assert torch.equal(rag[1:, :, :2], ref64.convtr2d_3x3s2(x[1:, :, :1], w, **kw))
        assert torch.isnan(rag[1, :, 2:]).all()


def test_post_activations_and_error_figure():
    v = torch.linspace(-6, 6, 241, dtype=torch.float64)
    for post in (ref64.POST_NONE, ref64.POST_LRELU, ref64.POST_ELU, ref64.POST_TANH, ref64.POST_SIGMOID, ref64.POST_LRELU_SNAKE):
        got = ref64.conv_post(v, post, 0.2)
        assert (got - _post32(v, post, 0.2)).abs().max() < 1e-14
        slope = ((got[1:] - got[:-1]) / (v[1:] - v[:-1])).abs().max().item()
        assert slope <= ref64.post_lipschitz(post) + 1e-9, post
    ref = torch.tensor([1.0, float("nan"), -2.0], dtype=torch.float64)
    mag = torch.tensor([3.0, 1.0, 2.0], dtype=torch.float64)
    mx, ss, n = ref64.conv_error(torch.tensor([1.0 + 4e-6, 7.0, -2.0], dtype=torch.float64), ref, mag)
    assert n == 2 and abs(mx - 1e-6) < 1e-11 and abs(ss - mx * mx) < 1e-16      # 4e-6 / (3 + 1); the NaN row end is not scored
    assert ref64.conv_error(torch.tensor([float("nan"), 0.0, -2.0]), ref, mag)[0] == float("inf")


def test_conv_statements_equal_the_oracle_modules(seeded_states):
    vsd, rsd = seeded_states
    # ConvBlockRes with a shortcut (decoder level 6 -> 5: 768 -> 384 would be large; encoder block 2, 32 -> 64, is the same code)
    p = "unet.encoder_block2.conv_block1"
    x = _rand((2, 32, 8, 63), 20)
    want = oracle.conv_block_res(x, rsd, p)
    s1, sh1 = weights.bn_affine(rsd, p + ".bn1")
    s2, sh2 = weights.bn_affine(rsd, p + ".bn2")
    sc = ref64.conv2d(x, rsd[p + ".shortcut.weight"], rsd[p + ".shortcut.bias"])
    y1 = ref64.conv2d(x, rsd[p + ".conv1.weight"], pre=ref64.PRE_AFFINE_LRELU, pre_slope=0.01, scale=s1, shift=sh1)
    got = ref64.conv2d(y1, rsd[p + ".conv2.weight"], res=sc, pre=ref64.PRE_AFFINE_LRELU, pre_slope=0.01, scale=s2, shift=sh2)
    _close(got, want)
    # the decoder's transposed convolution (BatchNorm + ReLU in front, last output row cut)
    p = "unet.decoder_block6"
    x = _rand((1, 64, 4, 63), 21)
    skip = torch.zeros((1, 32, 8, 127))
    s, sh = weights.bn_affine(rsd, p + ".bn1")
    got = ref64.convtr2d_3x3s2(x, rsd[p + ".conv1.weight"], pre=ref64.PRE_AFFINE_LRELU, pre_slope=0.0, scale=s, shift=sh)
    want = F.conv_transpose2d(F.relu(oracle._bn2d(x, rsd, p + ".bn1")), rsd[p + ".conv1.weight"], stride=2)[:, :, :-1]
    _close(got, want)
    assert oracle.decoder_block(x, skip, rsd, p).shape == (1, 32, 8, 127)      # the module the statement is cut from
    # UpsampleNet: snake (fused upstream) + weight-normed ConvTranspose1d, stride 7 and 3, then the k = 7 reflect-padded
    # pre-convolution with its leaky ReLU
    sd = oracle._canon(vsd)
    for up, s in (("generator.3", 7), ("generator.9", 3)):
        w = oracle._wn(sd, up + ".layer")
        x = _rand((2, w.shape[0], 11), 22)
        want = F.conv_transpose1d(x, w, sd[up + ".layer.bias"], stride=s, padding=s // 2 + s % 2, output_padding=s % 2)
        _close(ref64.convtr1d(x, w, sd[up + ".layer.bias"], s), want)
    w = oracle._wn(sd, "generator.1")
    x = _rand((2, w.shape[1], 19), 23)
    want = F.leaky_relu(F.conv1d(F.pad(x, (3, 3), mode="reflect"), w, sd["generator.1.bias"]), 0.2)
    _close(ref64.conv1d(x, w, sd["generator.1.bias"], reflect=True, post=ref64.POST_LRELU, post_slope=0.2), want)


# --------------------------------------------------------------------------------------
# the fp32 F(4,3) statement and the per-quad figure (the yardstick of tests/test_convwg4s_gpu.py)
# --------------------------------------------------------------------------------------
ULP = 2.0 ** -23


def _f43_operands(B, Cin, Cout, H, lp, pre, bias, res, seed):
    W = (1 << lp) - 1
    x, w = _rand((B, Cin, H, W), seed), _rand((Cout, Cin, 3, 3), seed + 1, (Cin * 9) ** -0.5)
    affine = pre == ref64.PRE_AFFINE_LRELU
    scale = 0.8 + 0.4 * torch.rand(Cin, generator=torch.Generator().manual_seed(seed + 2)) if affine else None
    shift = _rand((Cin,), seed + 3, 0.3) if affine else None
    return x, w, (_rand((Cout,), seed + 4, 0.3) if bias else None), (_rand((B, Cout, H, W), seed + 5) if res else None), scale, shift


# pre, post, bias, residual: what tests/test_convwg4s_gpu.py launches (the product's two convolutions of a ConvBlockRes, the
# train-mode first convolution, and the edge rows' bias + residual + post-activation / ELU / slope 0 and 1 combinations)
F43_COMBOS = [(ref64.PRE_AFFINE_LRELU, 0.01, ref64.POST_LRELU, 0.01, True, False), (ref64.PRE_NONE, 0.0, ref64.POST_NONE, 0.0, False, True),
              (ref64.PRE_NONE, 0.0, ref64.POST_NONE, 0.0, False, False), (ref64.PRE_AFFINE_LRELU, 0.01, ref64.POST_LRELU, 0.01, True, True),
              (ref64.PRE_NONE, 0.0, ref64.POST_LRELU, 0.01, True, True), (ref64.PRE_AFFINE_LRELU, 0.0, ref64.POST_ELU, 0.0, True, True),
              (ref64.PRE_AFFINE_LRELU, 1.0, ref64.POST_LRELU, 0.0, True, False), (ref64.PRE_NONE, 0.0, ref64.POST_NONE, 0.0, True, True)]


@pytest.mark.parametrize("combo", range(len(F43_COMBOS)))
@pytest.mark.parametrize("H,lp", [(8, 1), (9, 4), (6, 4), (7, 1), (4, 4), (1, 1)])
def test_f43_f32_statement_equals_the_float64_convolution(combo, H, lp):
    """conv2d_f43_f32 is the same operator as conv2d: its conv_error figure against the float64 statement is at most
    16 x 2^-23 (a plain fp32 F(4,3) measures 3 - 4 x 2^-23 at these channel counts: the bound leaves room for the draw,
    not for a wrong row, column, plane or coefficient, which is off by the order of the output).  Map heights with
    H % 4 in {0, 1, 2, 3}, P in {2, 16}, per-row heights."""
    pre, pre_slope, post, post_slope, bias, res = F43_COMBOS[combo]
    x, w, b, r, scale, shift = _f43_operands(3, 16, 8, H, lp, pre, bias, res, 100 + 7 * combo + H)
    kw = dict(pre=pre, pre_slope=pre_slope, scale=scale, shift=shift, post=post, post_slope=post_slope)
    for lengths in (None, [H, 1, max(1, H - 3)]):
        got = ref64.conv2d_f43_f32(x, w, b, r, lengths=lengths, **kw)
        assert got.dtype == torch.float32
        ref = ref64.conv2d(x, w, b, r, lengths=lengths, **kw)
        mag = ref64.conv2d(x, w, b, r, lengths=lengths, magnitude=True, **kw)
        assert torch.equal(torch.isnan(got), torch.isnan(ref))
        mx, ss, n = ref64.conv_error(got, ref, mag)
        assert n == int((~torch.isnan(ref)).sum()) and mx <= 16 * ULP, mx
        assert ref64.quad_figure(got, ref, mag)[0] <= mx


def test_f43_weights_are_the_packed_ones():
    """U = G w of the statement holds bit for bit the values packing.pack_wino4_2d hands the kernel in slab kx * 6 + plane
    (compared as sorted values: the order within a slab is pack_direct's MFMA operand layout)."""
    from voicefixer_amd import packing
    w = _rand((32, 16, 3, 3), 300, 0.1)
    U = ref64._f43_weights(w)                                              # (6, Cout, Cin, 3)
    packed = packing.pack_wino4_2d(packing.pack_conv2d(w))                 # [18][Cin / 8][Cout][8]
    assert packed.shape == (18, 2, 32, 8)
    for kx in range(3):
        for p in range(6):
            assert torch.equal(packed[kx * 6 + p].flatten().sort().values, U[p, :, :, kx].flatten().sort().values)


def test_quad_figure_reduces_to_conv_error_and_is_never_larger():
    g = torch.Generator().manual_seed(41)
    B, Cn, H, W = 2, 3, 11, 5
    ref = torch.randn((B, Cn, H, W), generator=g, dtype=torch.float64)
    ref[1, :, 6:] = float("nan")                                           # row 1 is 6 map rows high
    got = ref + 1e-6 * torch.randn((B, Cn, H, W), generator=g, dtype=torch.float64)
    got[1, :, 6:] = 123.0                                                  # whatever lies past a row's end is not scored
    # equal denominators within every quad: |ref| and the magnitude constant over the four rows
    blk = torch.arange(H) // 4
    ref_eq = torch.where(torch.isnan(ref), ref, ref[:, :, blk * 4])
    mag_eq = torch.rand((B, Cn, 3, W), generator=g, dtype=torch.float64)[:, :, blk]
    got_eq = ref_eq + (got - ref)
    a, b = ref64.quad_figure(got_eq, ref_eq, mag_eq, 2.0), ref64.conv_error(got_eq, ref_eq, mag_eq, 2.0)
    assert a[2] == b[2] == B * Cn * H * W - Cn * 5 * W and abs(a[0] - b[0]) <= 1e-15 * b[0] and abs(a[1] - b[1]) <= 1e-12 * b[1]
    # unequal ones: never larger, and one large neighbour lowers the figure of the small output next to it
    mag = torch.rand((B, Cn, H, W), generator=g, dtype=torch.float64)
    a, b = ref64.quad_figure(got, ref, mag), ref64.conv_error(got, ref, mag)
    assert a[2] == b[2] and a[0] <= b[0] and a[1] < b[1]
    ref1 = torch.tensor([1.0, 100.0, 1.0, 1.0, 1.0], dtype=torch.float64).reshape(1, 1, 5, 1)
    got1 = ref1 + torch.tensor([1e-3, 0.0, 0.0, 0.0, 1e-3], dtype=torch.float64).reshape(1, 1, 5, 1)
    mx, ss, n = ref64.quad_figure(got1, ref1, torch.zeros_like(ref1))
    assert n == 5 and abs(mx - 1e-3) < 1e-15 and abs(ss - (1e-6 + 1e-10)) < 1e-15     # row 4 is a quad of its own: 1e-3 / 1
    assert ref64.quad_figure(torch.full_like(ref1, float("nan")), ref1, torch.zeros_like(ref1))[0] == float("inf")
    # a quad is cut at the row's own height: the NaN rows of a ragged batch do not enter its maximum
    ref2 = ref1.clone()
    ref2[0, 0, 1] = float("nan")
    assert abs(ref64.quad_figure(got1, ref2, torch.zeros_like(ref1))[0] - 1e-3) < 1e-15


def _start_values_f32(t, scheme):
    """fp32 emulation of carrying a residual quad t = (t0 .. t3) through the accumulators of an F(4,3) kernel whose
    products are all zero: start values m with A^T m = t, then the output transform as convwg4s_kernel writes it.
    'planes0135': m2 = m4 = 0, m3 = (t2 - t1) / 2, m1 = 2 t1 - t2, m0 = t0 - m1 - m3, m5 = t3 - m1 - 8 m3;
    'planes0125': m3 = m4 = 0, m1 = (t1 + t2) / 2, m2 = (t2 - t1) / 2, m0 = t0 - t2, m5 = t3 - t1."""
    import numpy as np
    f32 = np.float32
    t0, t1, t2, t3 = t
    z = np.zeros_like(t0)
    if scheme == "planes0135":
        m3 = f32(0.5) * (t2 - t1)
        m1 = f32(2) * t1 - t2
        m = [t0 - m1 - m3, m1, z, m3, z, t3 - m1 - f32(8) * m3]
    else:
        m = [t0 - t2, f32(0.5) * (t1 + t2), f32(0.5) * (t2 - t1), z, z, t3 - t1]
    p12, m12, p34, m34 = m[1] + m[2], m[1] - m[2], m[3] + m[4], m[3] - m[4]
    out = np.stack([(m[0] + p12) + p34, f32(2) * m34 + m12, f32(4) * p34 + p12, (f32(8) * m34 + m12) + m[5]])
    assert out.dtype == f32
    return out


@pytest.mark.parametrize("scheme", ["planes0135", "planes0125"])
@pytest.mark.parametrize("dist", ["gauss", "lognormal"])
def test_start_values_carry_a_residual_within_the_floor(scheme, dist):
    """The floor of test_residual_pass_through (tests/test_convwg4s_gpu.py) is within reach of an fp32 kernel that carries
    the residual in its accumulators' start values: it returns it within 4 x 2^-23 in quad_figure (measured: 2.9 x 2^-23
    with planes 0, 1, 3, 5 and 0.98 x 2^-23 with planes 0, 1, 2, 5), on unit Gaussian residuals and on ones scaled by a
    log-normal factor (sigma 1.5) per output.  Zero weights: the magnitude is |residual|, the reference the residual.
    (convwg4s_kernel now adds the residual after the output transform and is exact here; the 1-D kernels still use
    planes 0, 1, 3, 5.)"""
    import numpy as np
    rng = np.random.default_rng(1)
    n = 500000
    t = rng.standard_normal((4, n))
    if dist == "lognormal":
        t = t * np.exp(1.5 * rng.standard_normal((4, n)))
    t = t.astype(np.float32)
    got = torch.from_numpy(_start_values_f32(t, scheme)).reshape(1, 1, 4, n)
    ref = torch.from_numpy(t).to(torch.float64).reshape(1, 1, 4, n)
    mx, ss, cnt = ref64.quad_figure(got, ref, ref.abs())
    print("start values %s %s: quad figure max %.2f x 2^-23, rms %.3f x 2^-23" % (scheme, dist, mx / ULP, (ss / cnt) ** 0.5 / ULP))
    assert cnt == 4 * n and mx <= 4 * ULP


# --------------------------------------------------------------------------------------
# the fp32 F(3,2) statement of the transposed 1-D convolution (the yardstick of tests/test_convtw_gpu.py)
# --------------------------------------------------------------------------------------
MARGIN = 4.0
RMS_FLOOR = 2.0 ** -24 / 3.0 ** 0.5 / 2.0      # the floors of tests/test_conv_taps_gpu.py
F32_TR_LENGTHS = [1, 2, 3, 95, 96, 97, "ragged"]


def _rms(fig):
    return (fig[1] / max(fig[2], 1)) ** 0.5


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("Lin", F32_TR_LENGTHS)
@pytest.mark.parametrize("s", [1, 2, 3, 7, 8])
def test_convtr1d_f32_f32_statement_equals_the_float64_convolution(s, Lin, with_bias):
    """convtr1d_f32_f32 is the same operator as convtr1d.  Its conv_error figure against the float64 statement is held to
    the level torch's own direct fp32 conv_transpose1d reaches on the same inputs: at most MARGIN = 4 times that
    operator's figure, maximum and RMS, with the floors of the GPU tests (2^-23; 2^-24 / sqrt(3) / 2) where the operator
    is (nearly) exact -- the relation tests/test_convtw_gpu.py then asks of the device against this statement.  A wrong
    tap, phase, triple or coefficient is off by the order of the output.  Lengths of one and two triples and one to
    either side, and per-row lengths."""
    B, Cin, Cout = 6, 64, 5
    lengths = [97, 1, 2, 3, 95, 96] if Lin == "ragged" else None
    L = 97 if Lin == "ragged" else Lin
    seed = 4000 + 10 * s + F32_TR_LENGTHS.index(Lin)
    x, w = _rand((B, Cin, L), seed), _rand((Cin, Cout, 2 * s), seed + 1, (2 * Cin) ** -0.5)
    bias = _rand((Cout,), seed + 2, 0.3) if with_bias else None
    got = ref64.convtr1d_f32_f32(x, w, bias, s, lengths=lengths)
    assert got.dtype == torch.float32
    ref = ref64.convtr1d(x, w, bias, s, lengths=lengths)
    mag = ref64.convtr1d(x, w, bias, s, lengths=lengths, magnitude=True)
    assert got.shape == ref.shape == (B, Cout, s * L) and torch.equal(torch.isnan(got), torch.isnan(ref))
    direct = torch.full(ref.shape, float("nan"))
    for b, n in enumerate(lengths or [L] * B):
        # (the full transposed convolution, cut: torch takes no output_padding of 1 at stride 1)
        pad = s // 2 + s % 2
        direct[b:b + 1, :, :n * s] = F.conv_transpose1d(x[b:b + 1, :, :n], w, bias, stride=s)[:, :, pad:pad + n * s]
    fs, fd = ref64.conv_error(got, ref, mag), ref64.conv_error(direct, ref, mag)
    print("F32TR s%d Lin %s %s: statement max %.3e rms %.3e, torch direct max %.3e rms %.3e" % (
        s, Lin, "bias" if with_bias else "nobias", fs[0], _rms(fs), fd[0], _rms(fd)))
    assert fs[2] == fd[2] == int((~torch.isnan(ref)).sum()) > 0
    assert fs[0] <= MARGIN * max(fd[0], ULP), (fs[0], fd[0])
    assert _rms(fs) <= MARGIN * max(_rms(fd), RMS_FLOOR), (_rms(fs), _rms(fd))


@pytest.mark.parametrize("s", [1, 3, 7])
def test_f32_tr_weights_are_the_packed_ones(s):
    """U = G g of the statement holds bit for bit the values packing.pack_wino32_tr hands the kernel, once its blob
    [4 planes][Cin / 8][s Cout][8] is un-permuted: row c s + r is (channel c, phase r), and position e of a group of 8
    input channels is channel (0, 2, 4, 6, 1, 3, 5, 7)[e] (packing.pack_direct)."""
    from voicefixer_amd import packing
    Cin, Cout = 24, 10
    w = _rand((Cin, Cout, 2 * s), 310 + s, 0.1)
    U = ref64._f32_tr_weights(w, s)                                        # (4, Cin, Cout, s)
    blob = packing.pack_wino32_tr(packing.pack_convtr1d(w), s)             # [4][Cin / 8][s Cout][8]
    assert blob.shape == (4, Cin // 8, s * Cout, 8) and U.shape == (4, Cin, Cout, s)
    lane_ci = torch.tensor([0, 2, 4, 6, 1, 3, 5, 7])
    un = torch.empty_like(U)
    b5 = blob.reshape(4, Cin // 8, Cout, s, 8)
    for grp in range(Cin // 8):
        un[:, grp * 8 + lane_ci] = b5[:, grp].permute(0, 3, 1, 2)          # (4, 8, Cout, s)
    assert torch.equal(un, U)


@pytest.mark.parametrize("s", [1, 2, 7])
def test_convtr1d_f32_f32_zero_weights_return_the_bias(s):
    B, Cin, Cout, Lin = 3, 16, 4, 11
    x, bias = _rand((B, Cin, Lin), 320 + s), _rand((Cout,), 330 + s)
    for lengths in (None, [11, 1, 5]):
        got = ref64.convtr1d_f32_f32(x, torch.zeros((Cin, Cout, 2 * s)), bias, s, lengths=lengths)
        for b, n in enumerate(lengths or [Lin] * B):
            assert torch.equal(got[b, :, :n * s], bias.reshape(-1, 1).expand(Cout, n * s))
            assert torch.isnan(got[b, :, n * s:]).all()


# --------------------------------------------------------------------------------------
# one ResStack layer: the float64 statement and the fp32 F(4,3) statements (the yardstick of tests/test_resblk4_gpu.py)
# --------------------------------------------------------------------------------------
RB_DILATIONS = [1, 3, 27, 81]


def _rb_operands(C, B, L, seed, bias=True):
    x = _rand((B, C, L), seed)
    w1, w2 = _rand((C, C, 3), seed + 1, (3 * C) ** -0.5), _rand((C, C, 3), seed + 2, (3 * C) ** -0.5)
    b1, b2 = (_rand((C,), seed + 3, 0.3), _rand((C,), seed + 4, 0.3)) if bias else (None, None)
    return x, w1, b1, w2, b2


def _rb_lengths(d):
    return [1, 5, 4 * d + 3]


def _rb_torch(x, w1, b1, w2, b2, d, slope, post, post_slope, dtype):
    """The layer as torch's own operators in `dtype`, one row."""
    c = lambda t: None if t is None else t.to(dtype)
    mid = F.conv1d(F.leaky_relu(c(x), slope), c(w1), c(b1), dilation=d, padding=d)
    y = c(x) + F.conv1d(F.leaky_relu(mid, slope), c(w2), c(b2), padding=1)
    return _post32(y, post, post_slope)


@pytest.mark.parametrize("post", [ref64.POST_NONE, ref64.POST_LRELU, ref64.POST_LRELU_SNAKE])
@pytest.mark.parametrize("d", RB_DILATIONS)
def test_resblock_statement_equals_torch_in_float64(d, post):
    """resblock against a float64 F.conv1d composition to 1e-12 of M, at L = 1, 5 and 4d + 3, plain and ragged (every row
    alone); M is what conv1d(mag1, w2, b2, res=x, magnitude=True) returns and bounds the linear part."""
    C, B = 12, 3
    lens = _rb_lengths(d)
    for bias in (True, False):
        for L in lens:
            x, w1, b1, w2, b2 = _rb_operands(C, B, L, 500 + d + L, bias)
            got = ref64.resblock(x, w1, b1, w2, b2, d, 0.01, post, 0.2)
            M = ref64.resblock(x, w1, b1, w2, b2, d, 0.01, magnitude=True)
            want = _rb_torch(x, w1, b1, w2, b2, d, 0.01, post, 0.2, torch.float64)
            assert got.dtype == torch.float64 and got.shape == want.shape == M.shape
            assert ((got - want).abs() <= 1e-12 * M).all()
            mag1 = ref64.conv1d(x, w1, b1, None, d, pre=ref64.PRE_LRELU, pre_slope=0.01, magnitude=True)
            assert torch.equal(M, ref64.conv1d(mag1, w2, b2, x, 1, magnitude=True))
            lin = ref64.resblock(x, w1, b1, w2, b2, d, 0.01)
            assert (M >= lin.abs() - 1e-12).all()
        Lmax = max(lens)
        x, w1, b1, w2, b2 = _rb_operands(C, B, Lmax, 600 + d, bias)
        for mag in (False, True):
            rag = ref64.resblock(x, w1, b1, w2, b2, d, 0.01, post, 0.2, lengths=lens, magnitude=mag)
            for b, n in enumerate(lens):
                alone = ref64.resblock(x[b:b + 1, :, :n], w1, b1, w2, b2, d, 0.01, post, 0.2, magnitude=mag)
                assert torch.equal(rag[b:b + 1, :, :n], alone) and torch.isnan(rag[b, :, n:]).all()


@pytest.mark.parametrize("ragged", [False, True], ids=["plain", "ragged"])
@pytest.mark.parametrize("d", RB_DILATIONS)
def test_f43_statements_are_the_layer_in_float64(d, ragged):
    """Run with dtype = float64 (U = G w then unrounded), conv1d_f43_f32 meets conv1d and resblock_f43_f32 meets resblock
    to 1e-12 of the magnitude: the statement is algebraically the layer -- quads, taps, matrices, padding at the row's own
    ends, bias and residual after the output transform."""
    C, B = 10, 3
    lens = _rb_lengths(d)
    for L in ([max(lens)] if ragged else lens):
        x, w1, b1, w2, b2 = _rb_operands(C, B, L, 700 + d + L)
        kw = dict(lengths=lens) if ragged else {}
        ok = None
        for post in (ref64.POST_NONE, ref64.POST_LRELU_SNAKE):
            got = ref64.resblock_f43_f32(x, w1, b1, w2, b2, d, 0.01, post, 0.2, dtype=torch.float64, **kw)
            ref = ref64.resblock(x, w1, b1, w2, b2, d, 0.01, post, 0.2, **kw)
            M = ref64.resblock(x, w1, b1, w2, b2, d, 0.01, magnitude=True, **kw)
            ok = ~torch.isnan(ref)
            assert got.dtype == torch.float64 and torch.equal(torch.isnan(got), ~ok) and bool(ok.any())
            assert ((got - ref).abs()[ok] <= 1e-12 * ref64.post_lipschitz(post) * M[ok]).all()
        # one convolution alone, with a residual and no pre-activation
        res = _rand((B, C, L), 9)
        got = ref64.conv1d_f43_f32(x, w1, b1, res, d, dtype=torch.float64, **kw)
        ref = ref64.conv1d(x, w1, b1, res, d, **kw)
        mag = ref64.conv1d(x, w1, b1, res, d, magnitude=True, **kw)
        assert ((got - ref).abs()[ok] <= 1e-12 * mag[ok]).all()


@pytest.mark.parametrize("gains", ["unit", "heavy"])
@pytest.mark.parametrize("d", RB_DILATIONS)
def test_resblock_f43_f32_figure_next_to_torchs_direct_operator(d, gains):
    """At fp32 and C = 64 the statement's figure |. - ref| / (M + |ref|) is printed next to that of torch's direct fp32
    operators; with `heavy` both convolutions carry log-normal output gains and unit-scale biases, as tests/test_resblk4_gpu.py
    draws them.  The statement returns float32, NaN exactly past a row's own end, and is held to what an fp32 evaluation
    can be expected to reach at all: 64 x 2^-23 of M (a wrong tap or constant is off by the order of M)."""
    C, B, L = 64, 3, 4 * d + 3
    lens = [L, 1, 5]
    x, w1, b1, w2, b2 = _rb_operands(C, B, L, 800 + d)
    if gains == "heavy":
        g = torch.Generator().manual_seed(900 + d)
        w1 = w1 * torch.exp(1.5 * torch.randn(C, generator=g) - 2.25).reshape(-1, 1, 1)
        w2 = w2 * torch.exp(1.5 * torch.randn(C, generator=g) - 2.25).reshape(-1, 1, 1)
        b1, b2 = torch.randn(C, generator=g), torch.randn(C, generator=g)
    got = ref64.resblock_f43_f32(x, w1, b1, w2, b2, d, lengths=lens)
    ref = ref64.resblock(x, w1, b1, w2, b2, d, lengths=lens)
    M = ref64.resblock(x, w1, b1, w2, b2, d, lengths=lens, magnitude=True)
    assert got.dtype == torch.float32 and torch.equal(torch.isnan(got), torch.isnan(ref))
    direct = torch.full(ref.shape, float("nan"))
    for b, n in enumerate(lens):
        direct[b:b + 1, :, :n] = _rb_torch(x[b:b + 1, :, :n], w1, b1, w2, b2, d, 0.01, ref64.POST_NONE, 0.0, torch.float32)
    fs, fd = ref64.conv_error(got, ref, M), ref64.conv_error(direct, ref, M)
    print("F43RB d%d %s: statement max %.3e rms %.3e, torch direct max %.3e rms %.3e" % (d, gains, fs[0], _rms(fs), fd[0], _rms(fd)))
    assert fs[2] == fd[2] == C * sum(lens)
    assert fs[0] <= 64 * ULP and fd[0] <= 64 * ULP


def test_f43_weights_1d_are_the_packed_ones():
    """U = G w of the statement holds bit for bit the values packing.pack_wino4 hands the kernels, once its blob
    [6 planes][Cin / 8][Cout][8] is un-permuted (packing.pack_direct: position e of a group of 8 input channels is
    channel (0, 2, 4, 6, 1, 3, 5, 7)[e])."""
    from voicefixer_amd import packing
    C = 16
    w = _rand((C, C, 3), 41, 0.1)
    U = ref64._f43_weights_1d(w, torch.float32)                            # (6, Cout, Cin)
    blob = packing.pack_wino4(packing.pack_conv1d(w))                      # [6][Cin / 8][Cout][8]
    assert blob.shape == (6, C // 8, C, 8)
    lane_ci = torch.tensor([0, 2, 4, 6, 1, 3, 5, 7])
    un = torch.empty_like(U)
    for grp in range(C // 8):
        un[:, :, grp * 8 + lane_ci] = blob[:, grp]
    assert torch.equal(un, U)


# --------------------------------------------------------------------------------------
# the bf16x3 statement (split="bf16x3": the reference of tests/test_conv_x3_gpu.py)
# --------------------------------------------------------------------------------------
# Round-to-nearest-even to bf16's 8 significant bits: for 2^e <= |v| < 2^(e+1) the spacing is 2^(e-7), so r = v - hi (exact in
# float32) has |r| <= 2^(e-8) <= 2^-8 |v|; lo = bf16(r) is rounded at r's own spacing, at most 2^(e-16), so
# |v - hi - lo| <= 2^(e-17) <= 2^-17 |v| (the kernel header's split residual; |r| = 2^(e-8) itself is representable).
# With x~ = xh + xl + ex and w = wh + wl + ew:  x~ w - (xh wh + xh wl + xl wh) = xl wl + ex w + (xh + xl) ew, and
# |xl wl| <= 2^-16 |x~ w|,  |ex w| <= 2^-17 |x~ w|,  |(x~ - ex) ew| <= (1 + 2^-17) 2^-17 |x~ w|:
X3_SPLIT = 2.0 ** -17
X3_C = 2.0 ** -16 + 2.0 ** -17 + (1.0 + 2.0 ** -17) * 2.0 ** -17             # = 2^-15 (1 + 2^-19) per product
# the plain float64 statement pre-activates in float64, the split one in float32 (conv_pre32): one rounding of the slope and
# one of the product (2^-23 of |x~|); the affine part adds one more rounding of a sum whose terms can cancel, so the affine
# case is pinned on the float32 x~ itself
X3_PRE = 2.0 ** -23

X3_SHAPES = [  # op, Cin, Cout, extent, k / stride, dilation / pitch log2, pre, heavy
    ("conv1d", 32, 64, 300, 3, 1, ref64.PRE_LRELU, False), ("conv1d", 512, 32, 200, 3, 27, ref64.PRE_LRELU, True),
    ("conv1d", 96, 32, 64, 1, 1, ref64.PRE_NONE, True), ("convtr1d", 128, 64, 50, 7, 0, ref64.PRE_NONE, False),
    ("convtr1d", 64, 32, 40, 2, 0, ref64.PRE_LRELU, True), ("conv2d", 64, 32, 5, 3, 3, ref64.PRE_AFFINE_LRELU, False),
    ("conv2d", 160, 32, 3, 1, 2, ref64.PRE_NONE, True),
]
X3_IDS = ["%s-c%d-k%d-%d-pre%d%s" % (s[0], s[1], s[4], s[5], s[6], "-heavy" if s[7] else "") for s in X3_SHAPES]


def _x3_operands(shape, seed):
    op, cin, cout, ext, k, dl, pre, heavy = shape
    B = 2
    if op == "conv1d":
        x, w = _rand((B, cin, ext), seed), _rand((cout, cin, k), seed + 1, (cin * k) ** -0.5)
    elif op == "convtr1d":
        x, w = _rand((B, cin, ext), seed), _rand((cin, cout, 2 * k), seed + 1, (2 * cin) ** -0.5)
    else:
        x, w = _rand((B, cin, ext, (1 << dl) - 1), seed), _rand((cout, cin, k, k), seed + 1, (cin * k * k) ** -0.5)
    if heavy:
        gain = torch.exp(1.5 * _rand((cout,), seed + 2) - 2.25)
        w = w * gain.reshape([-1 if d == (1 if op == "convtr1d" else 0) else 1 for d in range(w.dim())])
    bias = _rand((cout,), seed + 3, 1.0 if heavy else 0.3)
    kw = dict(pre=pre, pre_slope=0.01)
    if pre == ref64.PRE_AFFINE_LRELU:
        kw.update(scale=0.8 + 0.4 * torch.rand(cin, generator=torch.Generator().manual_seed(seed + 4)), shift=_rand((cin,), seed + 5, 0.3))
    return x, w, bias, kw


def _x3_call(shape, x, w, bias, kw, **more):
    op, k, dl = shape[0], shape[4], shape[5]
    if op == "conv1d":
        return ref64.conv1d(x, w, bias, None, dl, **kw, **more)
    if op == "convtr1d":
        return ref64.convtr1d(x, w, bias, k, **kw, **more)
    return ref64.conv2d(x, w, bias, None, **kw, **more)


def _x3_torch(shape, x, w, bias):
    op, k, dl = shape[0], shape[4], shape[5]
    if op == "conv1d":
        return F.conv1d(x, w, bias, dilation=dl, padding=(k - 1) // 2 * dl)
    if op == "convtr1d":
        return F.conv_transpose1d(x, w, bias, stride=k, padding=k // 2 + k % 2, output_padding=k % 2)
    return F.conv2d(x, w, bias, padding=k // 2)


def test_split_bf16_planes_are_the_packed_ones():
    """(a) hi / lo of the split helper are bit-equal to the planes packing.pack_x3 writes ([slab][Cin / 16][plane][k-half][Cout][8]),
    and the split residual is within the derived 2^-17 |v|."""
    from voicefixer_amd import packing
    cout, cin, k = 32, 48, 3
    w = _rand((cout, cin, k), 51, 0.1) * torch.exp(3.0 * _rand((cout, 1, 1), 52))
    hi, lo = ref64.split_bf16(w)
    blob = packing.pack_x3(packing.pack_conv1d(w))
    assert blob.dtype == torch.bfloat16 and tuple(blob.shape) == (k, cin // 16, 2, 2, cout, 8)
    planes = blob.permute(2, 4, 1, 3, 5, 0).reshape(2, cout, cin, k).float()       # [plane][Cout][chunk, k-half, k][slab]
    assert torch.equal(planes[0].view(torch.int32), hi.view(torch.int32))
    assert torch.equal(planes[1].view(torch.int32), lo.view(torch.int32))
    resid = (w.double() - hi.double() - lo.double()).abs()
    assert bool((resid <= X3_SPLIT * w.double().abs()).all())
    assert float((resid / w.double().abs()).max()) > 0.25 * X3_SPLIT               # (the bound is not vacuous)
    v = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 0.0, 2.0 ** -130])   # ties go to even
    h2, l2 = ref64.split_bf16(v)
    assert h2[:4].tolist() == [1.0, 1.0, 1.0 + 2.0 ** -6, -1.0] and l2[:4].tolist() == [0.0, 2.0 ** -8, -(2.0 ** -8), -(2.0 ** -8)]


@pytest.mark.parametrize("shape", X3_SHAPES, ids=X3_IDS)
def test_bf16x3_statement_is_within_the_derived_bound_of_float64(shape):
    """(b) |statement - plain float64| <= c sum |x~| |w| with c = X3_C (+ X3_PRE where a leaky ReLU is formed in float32), the
    derived worst case; the largest ratio seen is printed.  (c) zero weights return the bias.  magnitude=True is the plain
    statement's (on the float32 x~)."""
    x, w, bias, kw = _x3_operands(shape, 600)
    pre = shape[6]
    if pre == ref64.PRE_AFFINE_LRELU:       # pinned on the float32 x~ (see X3_PRE)
        x, kw = ref64.conv_pre32(x, pre, kw["pre_slope"], kw["scale"], kw["shift"]), {}
    stmt = _x3_call(shape, x, w, bias, kw, split="bf16x3")
    plain = _x3_call(shape, x, w, bias, kw)
    mag = _x3_call(shape, x, w, None, kw, magnitude=True)
    mag3 = _x3_call(shape, x, w, bias, kw, magnitude=True, split="bf16x3")
    assert stmt.dtype == torch.float64 and stmt.shape == plain.shape
    c = X3_C + (X3_PRE if kw.get("pre", ref64.PRE_NONE) != ref64.PRE_NONE else 0.0)
    ratio = float(((stmt - plain).abs() / mag).max())
    print("X3-STATEMENT %s: max |statement - float64| / sum|x~||w| = %.3f x 2^-16 (bound %.3f x 2^-16)" % (
        X3_IDS[X3_SHAPES.index(shape)], ratio * 2.0 ** 16, c * 2.0 ** 16))
    assert 0.0 < ratio <= c
    _close(mag3, (mag + bias.double().abs().reshape([1, -1] + [1] * (mag.dim() - 2))).float(), 1e-6)
    zero = _x3_call(shape, x, torch.zeros_like(w), bias, kw, split="bf16x3")
    assert torch.equal(zero, bias.double().reshape([1, -1] + [1] * (zero.dim() - 2)).expand_as(zero))


@pytest.mark.parametrize("shape", X3_SHAPES, ids=X3_IDS)
def test_bf16x3_yardstick_is_fp32_accumulation_of_the_same_sum(shape):
    """(d) the yardstick of the device bound: torch's fp32 CPU operator on the tripled problem (cat[xh, xh, xl], cat[wh, wl, wh]
    along Cin; every product exact in fp32) scored against the statement with conv_error: a few fp32 roundings, far below the
    split's own 2^-16, and exact in float64."""
    x, w, bias, kw = _x3_operands(shape, 700)
    x3, w3 = ref64.bf16x3_tripled(x, w, cin_dim=0 if shape[0] == "convtr1d" else 1, **kw)
    assert x3.dtype == w3.dtype == torch.float32 and x3.shape[1] == 3 * x.shape[1]
    stmt = _x3_call(shape, x, w, bias, kw, split="bf16x3")
    mag = _x3_call(shape, x, w, bias, kw, magnitude=True, split="bf16x3")
    exact = _x3_torch(shape, x3.double(), w3.double(), bias.double())
    assert float(((exact - stmt).abs() / mag).max()) <= 2.0 ** -45, "the tripled problem is not the statement's sum"
    mx, ss, n = ref64.conv_error(_x3_torch(shape, x3, w3, bias), stmt, mag)
    print("X3-YARDSTICK %s: max %.3e rms %.3e" % (X3_IDS[X3_SHAPES.index(shape)], mx, (ss / n) ** 0.5))
    assert n == stmt.numel() and 0.0 < mx <= 16 * ULP
