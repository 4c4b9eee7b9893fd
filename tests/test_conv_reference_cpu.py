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
