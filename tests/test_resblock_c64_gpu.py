"""vfx_resblock_wino4_f32: one C = 64 ResStack layer with both convolutions as Winograd F(4,3) in one launch at every dilation of the
stage (resblk4_kernel for d = 1 .. 27, the strip tile resblk4s_kernel for d = 81 .. 2187), against F.conv1d on the CPU in fp32.
NaN canaries around every buffer catch reads of the guard band and writes outside a row."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from voicefixer_amd import ops, packing, _lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
C64 = 64
DILATIONS = [3 ** i for i in range(8)]
GUARD = 16


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def _weights(seed):
    w1 = _rand((C64, C64, 3), seed, (C64 * 3) ** -0.5)
    b1 = _rand((C64,), seed + 1, 0.1)
    w2 = _rand((C64, C64, 3), seed + 2, (C64 * 3) ** -0.5)
    b2 = _rand((C64,), seed + 3, 0.1)
    return w1, b1, w2, b2


def _dev_weights(w1, b1, w2, b2):
    return (packing.pack_wino4(packing.pack_conv1d(w1)).to(DEV), b1.to(DEV),
            packing.pack_wino4(packing.pack_conv1d(w2)).to(DEV), b2.to(DEV))


def _ref(x, w1, b1, w2, b2, dil, post):
    mid = F.conv1d(F.leaky_relu(x, 0.01), w1, b1, dilation=dil, padding=dil)
    y = x + F.conv1d(F.leaky_relu(mid, 0.01), w2, b2, padding=1)
    if post == _lib.POST_LRELU:
        return F.leaky_relu(y, 0.2)
    if post == _lib.POST_LRELU_SNAKE:
        u = F.leaky_relu(y, 0.2)
        return u + torch.sin(u)
    return y


def _close(got, want, tol=2e-5):
    got = got.cpu()
    assert got.shape == want.shape
    assert torch.isfinite(got).all()
    err = (got - want).abs().max().item()
    scale = want.abs().max().item() + 1e-12
    assert err <= tol * max(1.0, scale), "max err %g (scale %g)" % (err, scale)


def _nan_guarded(B, L):
    v = ops.guarded(B, C64, L, GUARD, DEV)
    v._vfx_base.fill_(float("nan"))
    return v


def _expected_code(dil):
    return 96 if dil <= 27 else 97


def _run(x, dil, post, seed=301):
    """x: CPU (B, 64, L).  Runs the layer on the device, checks the kernel code, the result and the canaries; returns y."""
    B, _, L = x.shape
    w1, b1, w2, b2 = _weights(seed)
    xd = _nan_guarded(B, L)
    xd[:, :, :L] = x.to(DEV)
    yd = _nan_guarded(B, L)
    before = _lib.lib().vfx_launch_count()
    ops.resblock_wino4(xd, yd, *_dev_weights(w1, b1, w2, b2), L, dil, 0.01, post, 0.2)
    torch.cuda.synchronize()
    assert _lib.lib().vfx_launch_count() == before + 1
    assert _lib.lib().vfx_last_conv_tile() % 100 == _expected_code(dil)
    _close(yd[:, :, :L], _ref(x, w1, b1, w2, b2, dil, post))
    base, g = yd._vfx_base, yd._vfx_guard
    assert torch.isnan(base[:, :, :g]).all() and torch.isnan(base[:, :, g + L:]).all()   # nothing written outside [0, L)
    return yd


def _lengths(d):
    """Row ends at every kind of place: length 1, shorter than d, mid-strip, one segment exactly (W = 28 / 60), one and a half
    blocks, whole blocks."""
    out = {1, max(1, d // 2), d + 13, 3 * d + 28, 3 * d + 60, 6 * d + 5, 12 * d}
    return sorted(out)


@pytest.mark.parametrize("dil", DILATIONS)
def test_every_dilation_and_row_end(dil):
    for i, L in enumerate(_lengths(dil)):
        x = _rand((2, C64, L), 1000 * dil + i)
        _run(x, dil, _lib.POST_NONE)


@pytest.mark.parametrize("post", [_lib.POST_NONE, _lib.POST_LRELU, _lib.POST_LRELU_SNAKE])
@pytest.mark.parametrize("dil", [27, 81, 2187])
def test_post_variants(dil, post):
    _run(_rand((2, C64, 5 * dil + 3), 7 + post), dil, post)


@pytest.mark.parametrize("dil", [81, 2187])
def test_single_row(dil):
    _run(_rand((1, C64, 40 * dil + 1), 11), dil, _lib.POST_LRELU)


def test_thirty_second_rows():
    """B = 8 rows of 1 323 000 positions (a 30 s segment at the last stage); rows 0, 5 and 7 are checked."""
    B, L = 8, 1323000
    w1, b1, w2, b2 = _weights(17)
    g = torch.Generator(device=DEV).manual_seed(19)
    xd = _nan_guarded(B, L)
    xd[:, :, :L] = torch.randn((B, C64, L), generator=g, device=DEV)
    yd = _nan_guarded(B, L)
    dw = _dev_weights(w1, b1, w2, b2)
    for dil in (81, 2187):
        yd._vfx_base.fill_(float("nan"))
        ops.resblock_wino4(xd, yd, *dw, L, dil, 0.01, _lib.POST_NONE, 0.0)
        torch.cuda.synchronize()
        assert _lib.lib().vfx_last_conv_tile() % 100 == 97
        for b in (0, 5, 7):
            x = xd[b:b + 1, :, :L].cpu()
            _close(yd[b:b + 1, :, :L], _ref(x, w1, b1, w2, b2, dil, _lib.POST_NONE))
        base, gd = yd._vfx_base, yd._vfx_guard
        assert torch.isnan(base[:, :, :gd]).all() and torch.isnan(base[:, :, gd + L:]).all()


@pytest.mark.parametrize("dil", [9, 81, 243, 729, 2187])
def test_ragged_rows(dil):
    """Per-row lengths: every row equals the layer applied to that row alone, nothing is written past a row's end."""
    lens = [4 * dil * 3 + 17, dil - 5 if dil > 5 else 2, 4 * dil + 2 * dil + 29, 1]
    B, Lmax = len(lens), max(lens)
    w1, b1, w2, b2 = _weights(23)
    rows = torch.tensor(lens, dtype=torch.int32, device=DEV)
    x = _rand((B, C64, Lmax), 29)
    xd = _nan_guarded(B, Lmax)
    for b, n in enumerate(lens):
        xd[b, :, :n] = x[b, :, :n].to(DEV)       # past a row's end the input holds NaN: nothing may read it
    ops.with_rows(xd, rows)
    yd = ops.with_rows(_nan_guarded(B, Lmax), rows)
    ops.resblock_wino4(xd, yd, *_dev_weights(w1, b1, w2, b2), Lmax, dil, 0.01, _lib.POST_LRELU_SNAKE, 0.2)
    torch.cuda.synchronize()
    assert _lib.lib().vfx_last_conv_tile() % 100 == _expected_code(dil)
    base, g = yd._vfx_base, yd._vfx_guard
    for b, n in enumerate(lens):
        _close(yd[b:b + 1, :, :n], _ref(x[b:b + 1, :, :n], w1, b1, w2, b2, dil, _lib.POST_LRELU_SNAKE))
        assert torch.isnan(base[b, :, g + n:]).all() and torch.isnan(base[b, :, :g]).all()


def test_in_place_and_other_shapes_are_refused():
    w1, b1, w2, b2 = _weights(31)
    dw = _dev_weights(w1, b1, w2, b2)
    L = 1000
    xd = _nan_guarded(2, L)
    xd[:, :, :L] = _rand((2, C64, L), 37).to(DEV)
    with pytest.raises(_lib.VfxError):
        ops.resblock_wino4(xd, xd, *dw, L, 243)          # y aliasing x
    yd = _nan_guarded(2, L + 4)
    with pytest.raises(_lib.VfxError):
        ops.resblock_wino4(xd, yd[:, :, 1:1 + L], *dw, L, 243)   # rows not 16-byte aligned
    with pytest.raises(_lib.VfxError):
        ops.resblock_wino4(xd[:, :32], yd[:, :32, :L], *dw, L, 243)   # C = 32
