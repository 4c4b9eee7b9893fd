"""convtw_kernel with channel-major rows (vfx_convtw.inc): the s output phases of the transposed convolution are ONE GEMM with
s Cout rows, row c s + r = (channel c, phase r), so a row block of 128 (or 64) rows cuts through a channel's phases wherever s does
not divide it, and a lane's 16 register rows belong to up to 16 different (channel, phase) pairs.

Reference: torch's direct fp32 conv_transpose1d on the CPU at the direct kernels' 2e-5 (the transform constants are 1 and 1/2), as
test_ops_gpu.test_convtr1d_winograd32.  NaN canaries sit in the input's guard band; y is pre-filled with NaN and must hold no NaN in
[0, s len) and nothing but NaN from s len on, for every row of every batch item.  Shapes are the smallest that can still go wrong:
Cin = 32 (the kernel's minimum, two chunks), input lengths of one tile exactly, one more / less, and two tiles plus one; the kernel
declines launches of fewer than 512 workgroups, which the batch size makes up for (never the length)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from voicefixer_amd import ops, packing, _lib  # noqa: E402

DEV = "cuda"
TOL = 2e-5


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def _guarded_nan(t, guard):
    B, Cn, L = t.shape
    v = ops.guarded(B, Cn, L, guard, DEV)
    v._vfx_base.fill_(float("nan"))
    v[:, :, :L] = t.to(DEV)
    return v


def _batch(B, s, Cout, Lin):
    """The table's batch size, raised where the launch would otherwise have fewer than 512 workgroups."""
    wide = Cout % 128 == 0
    bt = 32 if wide else 64
    ntiles = ((Lin + 3) // 3 + bt - 1) // bt
    nwg = ntiles * s * (Cout // (128 if wide else 64))
    return max(B, (512 + nwg - 1) // nwg)


_CACHE = {}


def _problem(s, Cin, Cout, B, Lin):
    """Inputs, device weights and the CPU reference WITHOUT bias, computed once per shape and never modified."""
    key = (s, Cin, Cout, B, Lin)
    if key not in _CACHE:
        x = _rand((B, Cin, Lin), 1300 + s)
        w = _rand((Cin, Cout, 2 * s), 1310 + s, (2 * Cin) ** -0.5)
        bias = torch.linspace(-1.0, 1.0, Cout) + _rand((Cout,), 1320 + s, 0.05)      # differs per channel
        wp = packing.pack_convtr1d(w)
        dev = (wp.to(DEV), packing.pack_direct(wp).to(DEV), packing.pack_wino32_tr(wp, s).to(DEV), bias.to(DEV))
        ref = F.conv_transpose1d(x, w, None, stride=s, padding=s // 2 + s % 2, output_padding=s % 2)
        _CACHE.clear()                      # (one shape at a time: the parametrised cases of a shape run back to back)
        _CACHE[key] = (x, w, bias, dev, ref)
    return _CACHE[key]


def _check(got, want, what):
    assert got.shape == want.shape
    assert not torch.isnan(got).any(), "%s: NaN inside [0, s len)" % what
    err = (got - want).abs().max().item()
    scale = want.abs().max().item() + 1e-12
    assert err <= TOL * max(1.0, scale), "%s: max err %g (scale %g)" % (what, err, scale)


def _run(s, Cin, Cout, B, Lin, with_bias, lens=None):
    B = _batch(B, s, Cout, Lin)
    x, w, bias, (wp, wd, wt, bd), ref = _problem(s, Cin, Cout, B, Lin)
    xd = _guarded_nan(x, 264)
    if lens is not None:
        rows = [lens[i % len(lens)] for i in range(B)]
        ops.with_rows(xd, torch.tensor(rows, dtype=torch.int32, device=DEV))
    else:
        rows = [Lin] * B
    Lo = Lin * s
    yd = torch.full((B, Cout, (Lo + 67) // 4 * 4), float("nan"), device=DEV)
    ops.convtr1d(xd, wp, bd if with_bias else None, yd, Lin, s, None, wd=wd, wg4=wt)
    torch.cuda.synchronize()
    assert _lib.lib().vfx_last_conv_tile() % 100 == 83, "launch did not run on convtw_kernel"
    y = yd.cpu()
    badd = bias[None, :, None] if with_bias else 0.0
    if lens is None:
        _check(y[:, :, :Lo], ref + badd, "Lin %d" % Lin)
        assert torch.isnan(y[:, :, Lo:]).all(), "written at or past s Lin"
        return
    for n in sorted(set(rows)):
        idx = [i for i, r in enumerate(rows) if r == n]
        want = F.conv_transpose1d(x[idx][:, :, :n], w, None, stride=s, padding=s // 2 + s % 2, output_padding=s % 2)
        _check(y[idx][:, :, :n * s], want + badd, "row length %d" % n)
        assert torch.isnan(y[idx][:, :, n * s:]).all(), "row length %d: written at or past s len" % n


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("Lin", [95, 96, 97, 193])
def test_row_block_cuts_a_channels_phases_s7(Lin, with_bias):
    """s = 7, Cout = 128: 896 rows in blocks of 128 = 18.3 channels each; every wave boundary but one cuts a channel."""
    _run(7, 32, 128, 40, Lin, with_bias)


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("Lin", [191, 192, 193])
def test_row_block_cuts_a_channels_phases_s3_64_rows(Lin, with_bias):
    """s = 3, Cout = 64 (the 64 rows x 64 triples workgroup): 192 rows in blocks of 64 = 21.3 channels each."""
    _run(3, 32, 64, 48, Lin, with_bias)


@pytest.mark.parametrize("with_bias", [True, False])
def test_even_stride_no_straddle(with_bias):
    """s = 2, Cout = 64: 32 whole channels per row block."""
    _run(2, 32, 64, 64, 193, with_bias)


@pytest.mark.parametrize("s,Cin,B", [(7, 32, 40), (7, 224, 40), (3, 32, 48), (3, 544, 48)])
def test_both_work_orders(s, Cin, B):
    """Cout = 128 on either side of the host's 3 MB threshold (16 s Cin Cout bytes of transformed weights): row block fastest
    below it (Cin = 32), tile fastest above (s = 7: Cin = 224 -> 3.06 MB; s = 3: Cin = 544 -> 3.19 MB)."""
    assert (16 * s * Cin * 128 <= (3 << 20)) == (Cin == 32)
    _run(s, Cin, 128, B, 97, True)


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("s,Cout,B", [(7, 128, 40), (3, 64, 48)])
def test_ragged_rows(s, Cout, B, with_bias):
    """Per-row lengths that end inside the first triple, on a tile boundary and one to either side of it."""
    _run(s, 32, Cout, B, 97, with_bias, lens=[1, 2, 95, 96, 97])


def test_bad_arguments_stay_einval_when_the_winograd_planes_are_offered():
    """try_launch_convtw runs before launch_conv validates: it must decline (not launch on) Cin = 0 / Cout = 0 / missing tap slabs, so
    that the caller still gets VFX_EINVAL."""
    import ctypes as C
    s, Cin, Cout, B, Lin = 7, 32, 128, 40, 97
    x, w, bias, (wp, wd, wt, bd), _ = _problem(s, Cin, Cout, B, Lin)
    xd = _guarded_nan(x, 264)
    yd = torch.full((B, Cout, (Lin * s + 67) // 4 * 4), float("nan"), device=DEV)
    xt, yt = ops.tdesc(xd), ops.tdesc(yd)
    act = _lib.vfx_act(w_direct=wd.data_ptr(), w_wino4=wt.data_ptr())
    for cin, cout, taps in [(0, Cout, wp), (Cin, 0, wp), (-32, Cout, wp), (Cin, -128, wp), (Cin, Cout, None)]:
        rc = _lib.lib().vfx_convtr1d_f32(C.byref(xt), C.c_void_p(taps.data_ptr() if taps is not None else 0),
                                         C.c_void_p(bd.data_ptr()), C.byref(yt), B, cin, cout, Lin, s, C.byref(act), ops._stream())
        assert rc == _lib.EINVAL, "Cin %d Cout %d tap slabs %s: %d" % (cin, cout, taps is not None, rc)
    torch.cuda.synchronize()
    assert torch.isnan(yd).all(), "a rejected call wrote output"
