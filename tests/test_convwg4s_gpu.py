"""convwg4s_kernel (voicefixer_amd/csrc/vfx_convwg2d.inc, vfx_last_conv_tile() % 100 == 88: the 3x3 convolutions of the
ResUNet as Winograd F(4,3) along the map rows) at every one of its four instances, against float64.

* ``test_launch_census`` runs the seeded pipeline at the five geometries of tests/test_conv_taps_gpu.py under
  voicefixer_amd.launch_record and asserts that every code-88 launch is a row of ``CASES``.  The key is (BM, Cin, Cout, pitch,
  pre, post, bias, residual none / separate / in place, row tags, tile order); map height and batch are not part of it.
* ``test_case_parity`` launches every row of ``CASES`` once, at the smallest size that still launches on this kernel and
  keeps the row's tile order (see ``size_for``).
* ``test_edge_parity`` does the same for the index arithmetic the product does not reach (``EDGES``).
* ``test_residual_pass_through`` holds the skip connection to the floor of the figure on zero weights, and to the fp32
  F(4,3) statement on weights of 2^-10 (it is why bias and residual are added after the output transform).
* ``test_declined_shapes_fall_back_and_stay_right``: what the kernel's host side refuses runs elsewhere and stays right.

Buffers are built as the engine builds them: the input is a guarded view with NaN in its guard bands, past every row's own
height and -- when a pre-activation runs over it -- in the pad column (a map without pre-activation carries its structural
zero); the output is a channel slice of a wider NaN-filled buffer with guard bands, so its batch stride exceeds Cout x the
channel stride; a separate residual has channel and batch strides of its own; its pad column is zero.  Every launch asserts
the tile code and one launch, the zero pad column inside each row's height, and that NaN is untouched everywhere else.

Two error figures, both against ``f64_reference.conv2d`` and its ``magnitude=True`` twin: ``conv_error`` per output,
|got - ref| / (lip * magnitude + |ref|), and ``quad_figure``, the same with the denominator's maximum over the four
vertically adjacent outputs that share an F(4,3) quad.  The bound is measured on the reference side, on
``f64_reference.conv2d_f43_f32`` -- a plain fp32 statement of the same algorithm: the device may be at most MARGIN = 4 times
worse, maximum and RMS, in both figures, with the floors of tests/test_conv_taps_gpu.py (4 x 2^-23, 4 x 2^-24 / sqrt(3) / 2).
The device forms the same products in another order (8- or 16-channel chunks, the kernel-column loop, fmaf in the
transforms), which moves a rounding error by a small factor, not by its order.  (The direct fp32 operator is no yardstick
for an F(4,3) kernel: a plain fp32 F(4,3) is 4.3 x / 2.2 x the direct operator's maximum / RMS at 64 -> 64 channels.)
Every case prints ``PARITY <id> <figure> <ref max> <dev max> <ratio> <ref rms> <dev rms> <ratio>`` for both figures before
it asserts; profiles/convwg4s_parity.txt is that output.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from voicefixer_amd import ops, packing, _lib  # noqa: E402
from oracle import f64_reference as ref64  # noqa: E402
from test_conv_taps_gpu import GEOMETRIES, MARGIN, RMS_FLOOR, ULP, _Acc, _census, pipe  # noqa: E402,F401

DEV = "cuda"
NAN = float("nan")
PRE_AFF, PRE_NONE = _lib.PRE_AFFINE_LRELU, _lib.PRE_NONE
POST_NONE, POST_LRELU, POST_ELU = _lib.POST_NONE, _lib.POST_LRELU, _lib.POST_ELU
MIN_WGS = 384            # try_launch_convwg4s_2d: fewer workgroups stay on the small tiles / split-K

# BM, Cin, Cout, pitch, pre, post, bias, residual, row tags, tile order: every distinct convwg4s_kernel launch of the five
# census geometries, in launch order, with the product's map height (test_launch_census keeps the table complete; batch 1 x 10 s
# stays below 384 workgroups at every level and puts nothing on this kernel)
CASES = [
    # batch 32 x 10 s (the headline)
    (32, 32, 32, 128, 0, 0, False, 'in place', False, 'xcd'),   # H 1024
    (32, 32, 32, 128, 2, 1, True, 'none', False, 'xcd'),   # H 1024
    (32, 32, 32, 128, 0, 0, False, 'separate', False, 'xcd'),   # H 1024
    (64, 32, 64, 64, 2, 1, True, 'none', False, 'xcd'),   # H 512
    (64, 64, 64, 64, 0, 0, False, 'in place', False, 'xcd'),   # H 512
    (64, 64, 64, 64, 2, 1, True, 'none', False, 'xcd'),   # H 512
    (64, 64, 64, 64, 0, 0, False, 'separate', False, 'xcd'),   # H 512
    (64, 64, 128, 32, 2, 1, True, 'none', False, 'linear'),   # H 256
    (64, 128, 128, 32, 0, 0, False, 'in place', False, 'linear'),   # H 256
    (64, 128, 128, 32, 2, 1, True, 'none', False, 'linear'),   # H 256
    (64, 128, 128, 32, 0, 0, False, 'separate', False, 'linear'),   # H 256
    (64, 128, 256, 16, 2, 1, True, 'none', False, 'linear'),   # H 128
    (64, 256, 256, 16, 0, 0, False, 'in place', False, 'linear'),   # H 128
    (64, 256, 256, 16, 2, 1, True, 'none', False, 'linear'),   # H 128
    (64, 256, 256, 16, 0, 0, False, 'separate', False, 'linear'),   # H 128
    (64, 256, 384, 8, 2, 1, True, 'none', False, 'linear'),   # H 64
    (64, 384, 384, 8, 0, 0, False, 'in place', False, 'linear'),   # H 64
    (64, 384, 384, 8, 2, 1, True, 'none', False, 'linear'),   # H 64
    (64, 384, 384, 8, 0, 0, False, 'separate', False, 'linear'),   # H 64
    (64, 768, 384, 8, 2, 1, True, 'none', False, 'linear'),   # H 64
    (64, 512, 256, 16, 2, 1, True, 'none', False, 'linear'),   # H 128
    (64, 256, 128, 32, 2, 1, True, 'none', False, 'linear'),   # H 256
    (64, 128, 64, 64, 2, 1, True, 'none', False, 'xcd'),   # H 512
    (32, 64, 32, 128, 2, 1, True, 'none', False, 'xcd'),   # H 1024
    # batch 8 x 30 s
    (64, 64, 128, 32, 2, 1, True, 'none', False, 'xcd'),   # H 752
    (64, 128, 128, 32, 0, 0, False, 'in place', False, 'xcd'),   # H 752
    (64, 128, 128, 32, 2, 1, True, 'none', False, 'xcd'),   # H 752
    (64, 128, 128, 32, 0, 0, False, 'separate', False, 'xcd'),   # H 752
    (64, 256, 128, 32, 2, 1, True, 'none', False, 'xcd'),   # H 752
    # ragged mode-0 batch of five rows (10, 1, 4.5, 7.6, 2.3 s)
    (32, 32, 32, 128, 0, 0, False, 'in place', True, 'xcd'),   # H 1024
    (32, 32, 32, 128, 2, 1, True, 'none', True, 'xcd'),   # H 1024
    (32, 32, 32, 128, 0, 0, False, 'separate', True, 'xcd'),   # H 1024
    (64, 32, 64, 64, 2, 1, True, 'none', True, 'xcd'),   # H 512
    (64, 64, 64, 64, 0, 0, False, 'in place', True, 'xcd'),   # H 512
    (64, 64, 64, 64, 2, 1, True, 'none', True, 'xcd'),   # H 512
    (64, 64, 64, 64, 0, 0, False, 'separate', True, 'xcd'),   # H 512
    (64, 128, 64, 64, 2, 1, True, 'none', True, 'xcd'),   # H 512
    (32, 64, 32, 128, 2, 1, True, 'none', True, 'xcd'),   # H 1024
    # mode 2 (train-mode BatchNorm), batch 4 x 10 s
    (32, 32, 32, 128, 0, 0, False, 'none', False, 'xcd'),   # H 1024
    (64, 32, 64, 64, 0, 0, False, 'none', False, 'xcd'),   # H 512
    (64, 64, 64, 64, 0, 0, False, 'none', False, 'xcd'),   # H 512
    (64, 128, 64, 64, 0, 0, False, 'none', False, 'xcd'),   # H 512
    (32, 64, 32, 128, 0, 0, False, 'none', False, 'xcd'),   # H 1024
]


# --------------------------------------------------------------------------------------
# geometry of a launch
# --------------------------------------------------------------------------------------
def tile_of(cout):
    """(BM, BQ, KC) of the instance the host picks: <2,2,16> for 64-channel blocks, <1,4,8> when Cout % 64 != 0."""
    return (64, 64, 16) if cout % 64 == 0 else (32, 128, 8)


def ntiles_of(H, P, BQ):
    return -(-(-(-H // 4) * P) // BQ)


def order_of(H, P, cout):
    """Tile order of the launch: linear below 64 tiles, XCD-aware with folded channel blocks from 64 tiles up."""
    return "xcd" if ntiles_of(H, P, tile_of(cout)[1]) >= 64 else "linear"


def size_for(cout, P, tiles):
    """(B, H): the map height that gives exactly `tiles` tiles with the last quad-row partial (H % 4 == 3) and, where a tile
    holds several quad-rows, the last tile one quad-row short; B the least batch that reaches MIN_WGS workgroups."""
    BM, BQ, _ = tile_of(cout)
    r = BQ // P
    nq = tiles * r - (1 if r > 1 else 0)
    H = 4 * nq - 1
    assert ntiles_of(H, P, BQ) == tiles
    return -(-MIN_WGS // (tiles * (cout // BM))), H


def expected_tile(cout):
    BM, BQ, _ = tile_of(cout)
    return BM * 100000 + (4 * BQ % 1000) * 100 + 88


def ragged_heights(B, H):
    """Per-row map heights of a ragged launch, cycled over the batch; row 0 fills the capacity."""
    hs = [H, 1, 2, 3, 4, 5, H - 1, max(1, H // 2), 6, 7, max(1, H - 4), 8, max(1, H // 3), 9]
    return [min(H, hs[b % len(hs)]) for b in range(B)]


def make_spec(cin, cout, P, pre, post, bias, res, rows, tiles=3, **extra):
    spec = dict(cin=cin, cout=cout, P=P, pre=pre, post=post, bias=bias, res=res, rows=rows, pre_slope=0.01, post_slope=0.01,
                heavy=False, w_scale=1.0, res_dist="gauss")
    if "H" not in extra or "B" not in extra:
        spec["B"], spec["H"] = size_for(cout, P, tiles)
    spec.update(extra)
    if spec.get("lengths") is None:
        spec["lengths"] = ragged_heights(spec["B"], spec["H"]) if rows else None
    return spec


def case_key_id(key):
    BM, cin, cout, P, pre, post, bias, res, rows, order = key
    return "BM%d-%dto%d-P%d-pre%d-post%d%s%s%s-%s" % (
        BM, cin, cout, P, pre, post, "-bias" if bias else "", {"none": "", "separate": "-res", "in place": "-resinplace"}[res],
        "-rows" if rows else "", order)


# --------------------------------------------------------------------------------------
# one launch
# --------------------------------------------------------------------------------------
def _rand(shape, gen, scale=1.0):
    return torch.randn(shape, generator=gen) * scale


def _up4(n):
    return (n + 3) // 4 * 4


def _inputs(spec, seed):
    """CPU fp32 operands, dense maps: unit-variance activations, weights scaled by fan-in^-1/2 (`heavy`: times a log-normal
    gain per output channel, exp(1.5 z - 2.25), as tests/test_conv_taps_gpu.py draws them, and the BatchNorm scales times
    exp(1.5 z)), a bias of 0.3, a unit-variance residual (`res_dist` lognormal: every element times exp(1.5 z))."""
    g = torch.Generator().manual_seed(seed)
    B, cin, cout, H, W = spec["B"], spec["cin"], spec["cout"], spec["H"], spec["P"] - 1
    t = {"w": _rand((cout, cin, 3, 3), g, (cin * 9) ** -0.5) * spec["w_scale"]}
    if spec["heavy"]:
        t["w"] = t["w"] * torch.exp(1.5 * _rand((cout,), g) - 2.25).reshape(-1, 1, 1, 1)
    t["bias"] = (_rand((cout,), g, 0.3) * (0.0 if spec["w_scale"] == 0.0 else 1.0)) if spec["bias"] else None
    t["scale"] = t["shift"] = None
    if spec["pre"] == PRE_AFF:
        t["scale"] = 0.8 + 0.4 * torch.rand(cin, generator=g)
        if spec["heavy"]:
            t["scale"] = t["scale"] * torch.exp(1.5 * _rand((cin,), g))
        t["shift"] = _rand((cin,), g, 0.3)
    t["x"] = _rand((B, cin, H, W), g)
    t["res"] = None
    if spec["res"] != "none":
        t["res"] = _rand((B, cout, H, W), g)
        if spec["res_dist"] == "lognormal":
            t["res"] = t["res"] * torch.exp(1.5 * _rand((B, cout, H, W), g))
    return t


def _alloc(B, Cn, L, guard, cpad):
    """NaN-filled (B, cpad + Cn + cpad, guard + L' + guard) allocation; returns (base, the (B, Cn, L') view in its middle)."""
    g4, Lp = _up4(guard), _up4(L)
    base = torch.full((B, Cn + 2 * cpad, g4 + Lp + g4), NAN, device=DEV)
    return base, base[:, cpad:cpad + Cn, g4:g4 + Lp]


def launch(spec, seed, expect88=True, wg4_misaligned=False):
    """Launch `spec` once on buffers laid out as the header says and hold it to the tile code, the launch count and the
    canaries.  Returns (device output as a dense (B, Cout, H, W) fp32 CPU tensor, the operands)."""
    B, cin, cout, H, P = spec["B"], spec["cin"], spec["cout"], spec["H"], spec["P"]
    lp = P.bit_length() - 1
    lengths = spec["lengths"]
    hs = lengths if lengths is not None else [H] * B
    t = _inputs(spec, seed)
    guard = P + 1 + 264
    xbase, xv = _alloc(B, cin, H * P, guard, 0)
    xflat = ref64.to_pitch(t["x"], lp, fill=NAN if spec["pre"] != PRE_NONE else 0.0)
    for b in range(B):
        xv[b, :, :hs[b] * P] = xflat[b, :, :hs[b] * P].to(DEV)
    xv._vfx_guard = _up4(guard)
    xv._vfx_base = xbase
    if lengths is not None:
        ops.with_rows(xv, torch.tensor([h * P for h in hs], dtype=torch.int32, device=DEV))
    ybase, yv = _alloc(B, cout, H * P, 8, 4)            # a channel slice of a wider buffer: y_bs > Cout * y_cs
    assert yv.stride(0) > cout * yv.stride(1)
    rv = None
    if t["res"] is not None:
        rflat = ref64.to_pitch(t["res"], lp, fill=0.0)
        if spec["res"] == "in place":
            rv = yv
        else:
            rbase, rv = _alloc(B, cout, H * P, 12, 1)
            assert rv.stride(1) != yv.stride(1) and rv.stride(0) != yv.stride(0)
        for b in range(B):
            rv[b, :, :hs[b] * P] = rflat[b, :, :hs[b] * P].to(DEV)
    wp = packing.pack_conv2d(t["w"])
    wg4 = packing.pack_wino4_2d(wp)
    if wg4_misaligned:
        wg4 = torch.cat([torch.zeros(1), wg4.flatten()]).to(DEV)[1:].reshape(wg4.shape)
        assert wg4.data_ptr() % 16 != 0
    else:
        wg4 = wg4.to(DEV)
    wp = wp.to(DEV)
    bias = t["bias"].to(DEV) if t["bias"] is not None else None
    act = ops.Act(pre=spec["pre"], pre_slope=spec["pre_slope"], scale=t["scale"].to(DEV) if t["scale"] is not None else None,
                  shift=t["shift"].to(DEV) if t["shift"] is not None else None, post=spec["post"], post_slope=spec["post_slope"])
    lib = _lib.lib()
    torch.cuda.synchronize()
    before = lib.vfx_launch_count()
    ops.conv2d(xv, wp, bias, yv, H, lp, 3, act, rv, wg4=wg4)
    torch.cuda.synchronize()
    tile, launches = lib.vfx_last_conv_tile(), int(lib.vfx_launch_count() - before)
    if expect88:
        assert tile == expected_tile(cout), "ran as %d, expected %d" % (tile, expected_tile(cout))
        assert launches == 1
    else:
        assert tile % 100 != 88 and launches >= 1, "ran as %d" % tile
    # ---- canaries: NaN past each row's own height, past the capacity, in the guard bands and the neighbouring channels
    allowed = torch.zeros(ybase.shape, dtype=torch.bool, device=DEV)
    av = allowed[:, 4:4 + cout, 8:8 + _up4(H * P)]
    for b in range(B):
        av[b, :, :hs[b] * P] = True
    if not expect88 and launches > 1:                   # a split-K fallback reduces the whole capacity (include/vfx_hip.h)
        av[:, :, :H * P] = True
    stray = ~(torch.isnan(ybase) | allowed)
    assert not bool(stray.any()), "%d elements outside the valid output were written" % int(stray.sum())
    got = ref64.from_pitch(yv.detach().cpu(), H, lp)
    for b in range(B):
        assert bool((got[b, :, :hs[b], P - 1] == 0).all()), "output pad column is not exactly 0"
    return got[..., :P - 1].contiguous(), t


def _kw(spec, t):
    return dict(pre=spec["pre"], pre_slope=spec["pre_slope"], scale=t["scale"], shift=t["shift"], post=spec["post"],
                post_slope=spec["post_slope"], lengths=spec["lengths"])


def score(spec, t, got, yardstick):
    """`got` and the fp32 yardstick (`f43`: conv2d_f43_f32, `direct`: torch's CPU operator), each against the float64
    statement -- every row of a ragged batch against the convolution of that map alone.  Returns {figure: (dev, ref)} of
    _Acc for the per-output and the per-quad figure."""
    kw = _kw(spec, t)
    with torch.no_grad():
        ref = ref64.conv2d(t["x"], t["w"], t["bias"], t["res"], **kw)
        mag = ref64.conv2d(t["x"], t["w"], t["bias"], t["res"], magnitude=True, **kw)
        if yardstick == "f43":
            y32 = ref64.conv2d_f43_f32(t["x"], t["w"], t["bias"], t["res"], **kw)
        else:
            y32 = _direct32(spec, t)
    out = {}
    for name, fig in (("output", ref64.conv_error), ("quad", ref64.quad_figure)):
        dev, cpu = _Acc(), _Acc()
        dev.add(fig(got, ref, mag))
        cpu.add(fig(y32, ref, mag))
        out[name] = (dev, cpu)
    return out


def _direct32(spec, t):
    """torch's direct fp32 CPU operator, every row of a ragged batch alone."""
    def one(x, res):
        xa = x
        if spec["pre"] == PRE_AFF:
            xa = F.leaky_relu(x * t["scale"].reshape(1, -1, 1, 1) + t["shift"].reshape(1, -1, 1, 1), spec["pre_slope"])
        y = F.conv2d(xa, t["w"], t["bias"], padding=1)
        y = y + res if res is not None else y
        return F.leaky_relu(y, spec["post_slope"]) if spec["post"] == POST_LRELU else (F.elu(y) if spec["post"] == POST_ELU else y)
    if spec["lengths"] is None:
        return one(t["x"], t["res"])
    full = torch.full((spec["B"], spec["cout"], spec["H"], spec["P"] - 1), NAN)
    for b, h in enumerate(spec["lengths"]):
        full[b:b + 1, :, :h] = one(t["x"][b:b + 1, :, :h], None if t["res"] is None else t["res"][b:b + 1, :, :h])
    return full


def check(name, figs, assert_figures=("output", "quad")):
    """Print every figure, then assert: the device at most MARGIN x the yardstick, maximum and RMS, with the floors."""
    for fig, (dev, cpu) in figs.items():
        print("PARITY %s %s %.3e %.3e %.2f %.3e %.3e %.2f" % (name, fig, cpu.mx, dev.mx, dev.mx / max(cpu.mx, ULP), cpu.rms, dev.rms,
                                                             dev.rms / max(cpu.rms, RMS_FLOOR)))
    for fig in assert_figures:
        dev, cpu = figs[fig]
        assert dev.n > 0 and dev.n == cpu.n
        assert dev.mx <= MARGIN * max(cpu.mx, ULP), "%s: max %s figure %.3e exceeds %.0f x the fp32 statement's %.3e" % (name, fig, dev.mx, MARGIN, cpu.mx)
        assert dev.rms <= MARGIN * max(cpu.rms, RMS_FLOOR), "%s: RMS %s figure %.3e exceeds %.0f x the fp32 statement's %.3e" % (name, fig, dev.rms, MARGIN, cpu.rms)


def run_case(spec, seed, name):
    got, t = launch(spec, seed)
    check(name, score(spec, t, got, "f43"))
    return got


# --------------------------------------------------------------------------------------
# the product's launches
# --------------------------------------------------------------------------------------
def record_key(r):
    return (r["BM"], r["cin"], r["cout"], r["pitch"], r["pre"], r["post"], r["bias"], r["res"], r["rows"],
            order_of(r["H"], r["pitch"], r["cout"]))


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_launch_census(pipe, geometry):  # noqa: F811
    """Every convwg4s_kernel launch of the seeded pipeline at this geometry is a row of CASES, and the census sees the launch
    kinds the product is known to put on this kernel."""
    table = set(CASES)
    rec = _census(pipe, geometry)
    wg = rec.wg4s()
    unmatched = []
    for r in wg:
        assert r["op"] == "conv2d" and r["k"] == 3 and r["guarded"] and r["unit"] and r["launches"] == 1, r
        assert (r["BM"], r["BL"]) == (tile_of(r["cout"])[0], 4 * tile_of(r["cout"])[1] % 1000), r
        if record_key(r) not in table:
            unmatched.append(record_key(r))
    print("CENSUS %s: %d conv-family calls, %d on convwg4s_kernel, %d distinct keys, %d unmatched" % (
        geometry, len(rec.records), len(wg), len({record_key(r) for r in wg}), len(unmatched)))
    assert not unmatched, "convwg4s_kernel launches that are not rows of CASES:\n%s" % "\n".join(map(repr, sorted(set(unmatched))))
    keys = {record_key(r) for r in wg}
    if geometry == "b32x10":
        assert {k[0] for k in keys} == {32, 64}, "both instances"
        assert {k[4] for k in keys} == {PRE_NONE, PRE_AFF}, "with and without pre-activation (AFF)"
        assert any(k[9] == "xcd" for k in keys), "the XCD-aware tile order"
        assert any(k[7] == "in place" for k in keys), "an in-place residual"
    if geometry == "ragged5":
        assert wg and all(k[8] for k in keys), "row tags on every launch of a ragged batch"
    if geometry == "train4x10":
        assert any(k[4] == PRE_NONE and k[7] == "none" and not k[6] for k in keys), "the pre-activation-free first convolution"


def _heavy(i):
    return i % 4 == 0       # every fourth row draws log-normal gains on the BatchNorm scales and the output channels


def _case_spec(key, heavy):
    BM, cin, cout, P, pre, post, bias, res, rows, order = key
    spec = make_spec(cin, cout, P, pre, post, bias, res, rows, tiles=3 if order == "linear" else 67, heavy=heavy)
    assert tile_of(cout)[0] == BM and order_of(spec["H"], P, cout) == order
    return spec


@pytest.mark.parametrize("i", range(len(CASES)), ids=[case_key_id(k) for k in CASES])
def test_case_parity(i):
    """Every row of CASES at the reduced size of its tile order: 3 tiles (linear) or 67 (XCD order, idle workgroups), the
    last quad-row partial, the least batch that reaches 384 workgroups.

    Findings (profiles/convwg4s_parity.txt).  Every row with a residual was 3.2 - 4.8 x the fp32 statement, and 70 - 470 x
    in the per-output figure on the rows with heavy-tailed gains, while the residual entered through the accumulators'
    start values; fixed in the kernel (bias and residual are added after the output transform), 0.9 - 2.0 x now.
    BM64-768to384-P8-pre2-post1-bias-linear, the longest contraction of the product (1152 sequentially accumulated MFMAs
    per plane), measured a maximum of 9.38e-07 against the statement's 2.01e-07: 4.66 x (384 channels: 3.0 - 3.6 x, 512:
    3.9 - 4.1 x): one fp32 chain per accumulator against the statement's blocked sums.  Contractions longer than 384
    channels now run an instance with a two-level sum (partial sums of 64 channels): 1.09 x, 512 -> 256 0.71 x."""
    run_case(_case_spec(CASES[i], _heavy(i)), 2000 + i, case_key_id(CASES[i]))


def test_cases_are_distinct():
    assert len(set(CASES)) == len(CASES)
    for key in CASES:
        assert key[0] == tile_of(key[2])[0] and key[9] in ("linear", "xcd") and key[7] in ("none", "separate", "in place")


# --------------------------------------------------------------------------------------
# edges the product does not reach
# --------------------------------------------------------------------------------------
# The two shapes of a ConvBlockRes' convolutions, on either instance: A = BatchNorm pre-activation, bias, leaky ReLU (AFF
# true); N = no pre-activation, no bias, in-place residual (AFF false: padding through out-of-range offsets alone).
A = dict(pre=PRE_AFF, post=POST_LRELU, bias=True, res="none", rows=False)
N = dict(pre=PRE_NONE, post=POST_NONE, bias=False, res="in place", rows=False)
FULL = dict(post=POST_LRELU, bias=True, res="in place", rows=True)      # bias + in-place residual + leaky ReLU on ragged rows
WIDE, NARROW = 64, 32       # Cout of <2,2,16> / <1,4,8>


def _e(name, cin, cout, P, kind, tiles=3, **extra):
    d = dict(kind)
    d.update(extra)
    return (name, dict(cin=cin, cout=cout, P=P, tiles=tiles, **d))


def _edges():
    e = []
    # map pitches: P <= BQ, several map rows per tile down to P = 2
    for j, P in enumerate((2, 4, 8, 16, 32, 64)):
        e.append(_e("wide-P%d-%s" % (P, "AN"[j % 2]), 32, WIDE, P, (A, N)[j % 2]))
    for j, P in enumerate((2, 16, 64, 128)):
        e.append(_e("narrow-P%d-%s" % (P, "NA"[j % 2]), 16, NARROW, P, (N, A)[j % 2]))
    # chunk counts S = Cin / KC in {2, 4, 6}
    for j, cin in enumerate((32, 64, 96)):
        e.append(_e("wide-S%d-%s" % (cin // 16, "NA"[j % 2]), cin, WIDE, 32, (N, A)[j % 2]))
    for j, cin in enumerate((16, 32, 48)):
        e.append(_e("narrow-S%d-%s" % (cin // 8, "AN"[j % 2]), cin, NARROW, 64, (A, N)[j % 2]))
    # H % 4 in {0, 1, 2, 3} on a capacity whose last tile holds a single quad-row (9 quad-rows of 4 per tile, 17 of 8)
    for j, H in enumerate((36, 35, 34, 33)):
        e.append(_e("wide-H%d-%s" % (H, "AN"[j % 2]), 32, WIDE, 16, (A, N)[j % 2], H=H, B=128))
    for j, H in enumerate((68, 67, 66, 65)):
        e.append(_e("narrow-H%d-%s" % (H, "NA"[j % 2]), 16, NARROW, 16, (N, A)[j % 2], H=H, B=128))
    # the order switch (63 -> 64 tiles) and a multiple of 8 (no idle workgroups)
    for j, tiles in enumerate((63, 64, 72)):
        e.append(_e("wide-tiles%d-%s" % (tiles, "AN"[j % 2]), 32, WIDE, 64, (A, N)[j % 2], tiles=tiles))
        e.append(_e("narrow-tiles%d-%s" % (tiles, "NA"[j % 2]), 16, NARROW, 128, (N, A)[j % 2], tiles=tiles))
    # six folded channel blocks, both orders
    e.append(_e("cout384-linear-A", 32, 384, 4, A))
    e.append(_e("cout384-linear-N", 64, 384, 8, N))
    e.append(_e("cout384-xcd-A", 32, 384, 64, A, tiles=67))
    e.append(_e("cout384-xcd-N", 64, 384, 32, N, tiles=65))
    # ragged rows on every instance with bias, in-place residual and leaky ReLU together; P < BQ; a row of height 1 in the
    # XCD order (ragged_heights: row 1)
    for pre, tag in ((PRE_AFF, "A"), (PRE_NONE, "N")):
        e.append(_e("wide-rows-full-%s" % tag, 32, WIDE, 16, FULL, pre=pre))
        e.append(_e("narrow-rows-full-%s" % tag, 16, NARROW, 32, FULL, pre=pre))
        e.append(_e("wide-rows-full-xcd-%s" % tag, 32, WIDE, 32, FULL, pre=pre, tiles=69))
        e.append(_e("narrow-rows-full-xcd-%s" % tag, 16, NARROW, 128, FULL, pre=pre, tiles=71))
    # post-activations: none, leaky ReLU, the generic branch (ELU)
    e.append(_e("wide-post-none-A", 32, WIDE, 64, A, post=POST_NONE))
    e.append(_e("wide-post-elu-N", 32, WIDE, 64, N, post=POST_ELU))
    e.append(_e("narrow-post-elu-A", 16, NARROW, 128, A, post=POST_ELU))
    e.append(_e("narrow-post-lrelu-N", 16, NARROW, 128, N, post=POST_LRELU))
    # slopes at the ends of their ranges
    e.append(_e("wide-preslope0-postslope0", 32, WIDE, 64, A, pre_slope=0.0, post_slope=0.0))
    e.append(_e("wide-preslope1", 32, WIDE, 64, A, pre_slope=1.0))
    e.append(_e("narrow-preslope1-postslope0", 16, NARROW, 128, A, pre_slope=1.0, post_slope=0.0))
    e.append(_e("narrow-preslope0", 16, NARROW, 128, A, pre_slope=0.0))
    # a separate residual whose channel and batch strides differ from the output's
    e.append(_e("wide-res-separate-A", 32, WIDE, 64, A, res="separate"))
    e.append(_e("wide-res-separate-N", 32, WIDE, 32, N, res="separate"))
    e.append(_e("narrow-res-separate-A", 16, NARROW, 128, A, res="separate"))
    e.append(_e("narrow-res-separate-N", 16, NARROW, 64, N, res="separate", rows=True))
    # the two-level sum: contractions longer than 384 channels take an instance of their own (partial sums of 64 channels,
    # here also with a last partial of 32 / 16 channels); 384 stays on the one-level instance
    e.append(_e("wide-two-cin576-A", 576, WIDE, 64, A))
    e.append(_e("wide-two-cin544-N", 544, WIDE, 32, N))
    e.append(_e("narrow-two-cin576-A", 576, NARROW, 128, A))
    e.append(_e("narrow-two-cin528-N", 528, NARROW, 64, N, rows=True))
    e.append(_e("wide-two-cin512-N", 512, WIDE, 64, N))
    e.append(_e("narrow-two-cin512-A", 512, NARROW, 128, A))
    e.append(_e("wide-two-cin416-A", 416, WIDE, 16, A))
    e.append(_e("narrow-two-cin400-N", 400, NARROW, 128, N))
    e.append(_e("wide-one-cin384-N", 384, WIDE, 64, N))
    e.append(_e("narrow-one-cin384-A", 384, NARROW, 128, A))
    return e


EDGES = _edges()


def _edge_spec(i):
    d = dict(EDGES[i][1])
    return make_spec(d.pop("cin"), d.pop("cout"), d.pop("P"), d.pop("pre"), d.pop("post"), d.pop("bias"), d.pop("res"),
                     d.pop("rows"), d.pop("tiles"), heavy=_heavy(i), **d)


@pytest.mark.parametrize("i", range(len(EDGES)), ids=[e[0] for e in EDGES])
def test_edge_parity(i):
    run_case(_edge_spec(i), 6000 + i, EDGES[i][0])


def test_edges_reach_every_instance_in_every_group():
    assert len({e[0] for e in EDGES}) == len(EDGES)
    specs = [_edge_spec(i) for i in range(len(EDGES))]
    inst = lambda s: (tile_of(s["cout"])[0], s["pre"] != PRE_NONE)
    every = {(64, True), (64, False), (32, True), (32, False)}
    groups = {"P": lambda n: "-P" in n, "S": lambda n: "-S" in n, "H": lambda n: "-H" in n, "tiles": lambda n: "-tiles" in n,
              "rows": lambda n: "rows-full" in n and "xcd" not in n, "rows-xcd": lambda n: "rows-full-xcd" in n,
              "res": lambda n: "res-separate" in n, "two": lambda n: "-two-" in n}
    for g, pred in groups.items():
        assert {inst(s) for (n, _), s in zip(EDGES, specs) if pred(n)} == every, g
    assert {s["P"] for s in specs if s["cout"] == WIDE} >= {2, 4, 8, 16, 32, 64}
    assert {s["P"] for s in specs if s["cout"] == NARROW} >= {2, 16, 64, 128}
    assert {s["cin"] // tile_of(s["cout"])[2] for s in specs if s["cout"] == WIDE} >= {2, 4, 6}
    assert {s["cin"] // tile_of(s["cout"])[2] for s in specs if s["cout"] == NARROW} >= {2, 4, 6}
    tiles = lambda s: ntiles_of(s["H"], s["P"], tile_of(s["cout"])[1])
    assert {tiles(s) for s in specs} >= {3, 63, 64, 72}
    assert {s["H"] % 4 for s in specs} == {0, 1, 2, 3}
    assert {s["cin"] for s in specs} >= {384, 400, 416, 512, 528, 544, 576}      # either side of the two-level instance's threshold
    assert {order_of(s["H"], s["P"], 384) for s in specs if s["cout"] == 384} == {"linear", "xcd"}
    for s in specs:
        assert tiles(s) * (s["cout"] // tile_of(s["cout"])[0]) * s["B"] >= MIN_WGS and s["P"] <= tile_of(s["cout"])[1]
        assert s["cin"] % (2 * tile_of(s["cout"])[2]) == 0
        if s["rows"] and order_of(s["H"], s["P"], s["cout"]) == "xcd":
            assert 1 in s["lengths"]


# --------------------------------------------------------------------------------------
# the skip connection through the accumulators
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [False, True], ids=["plain", "rows"])
@pytest.mark.parametrize("cout", [WIDE, NARROW], ids=["wide", "narrow"])
@pytest.mark.parametrize("res", ["separate", "in place"], ids=["separate", "inplace"])
@pytest.mark.parametrize("dist", ["gauss", "lognormal"])
def test_residual_pass_through(dist, res, cout, rows):
    """Zero weights and bias: the output must be post(residual) within the floor of the per-quad figure (4 x 2^-23 maximum,
    4 x 2^-24 / sqrt(3) / 2 RMS); the fp32 statement scores (nearly) 0 here, so the floor is the bound.  Then weights of 2^-10
    of their usual scale, with a bias: the convolution is present, the residual dominates; bounded by the fp32 F(4,3)
    statement with the floor.  The per-output figure is printed and not asserted.

    This test is why the kernel adds bias and residual after the output transform.  While they entered through the
    accumulators' start values (planes 0, 1, 3, 5, as convwg4_kernel's) the zero-weight pass-through measured 2.9 x 2^-23 in
    the per-quad figure and up to 2.2 in the per-output one (a small residual between large vertical neighbours); the
    better-conditioned planes 0, 1, 2, 5 gave 0.96 x 2^-23, but the 2^-10 variant stayed at 7 - 10 x the statement: every
    product was rounded at 2^-24 of the residual held by the accumulator.  With the epilogue add the pass-through is exact.
    profiles/convwg4s_parity.txt has the three sets of figures."""
    cin, P = (32, 64) if cout == WIDE else (16, 128)
    name = "passthrough-%s-%s-%s-%s" % (dist, res.replace(" ", ""), "wide" if cout == WIDE else "narrow", "rows" if rows else "plain")
    for tag, w_scale in (("zero", 0.0), ("w2^-10", 2.0 ** -10)):
        spec = make_spec(cin, cout, P, PRE_AFF if rows else PRE_NONE, POST_LRELU if res == "in place" else POST_NONE, True, res,
                         rows, w_scale=w_scale, res_dist=dist)
        got, t = launch(spec, 9000 + 8 * (dist == "lognormal") + 4 * (res == "in place") + 2 * (cout == NARROW) + rows)
        figs = score(spec, t, got, "f43")
        check(name + "-" + tag, figs, assert_figures=("quad",))


# --------------------------------------------------------------------------------------
# what the host side declines
# --------------------------------------------------------------------------------------
DECLINED = [
    ("P128-cout64", dict(cin=32, cout=64, P=128, B=6, H=267), {}),            # P > BQ
    ("cin48-wide", dict(cin=48, cout=64, P=64, B=128, H=11), {}),             # Cin % 32 != 0 on 16-channel chunks
    ("one-workgroup-short", dict(cin=32, cout=64, P=64, B=127, H=11), {}),    # 381 workgroups
    ("misaligned-w_wino4", dict(cin=32, cout=64, P=64, B=128, H=11), dict(wg4_misaligned=True)),
]


@pytest.mark.parametrize("i", range(len(DECLINED)), ids=[d[0] for d in DECLINED])
def test_declined_shapes_fall_back_and_stay_right(i):
    """Launches that offer w_wino4 and that try_launch_convwg4s_2d refuses do not report code 88, write nothing outside
    their output, and meet the direct bound of tests/test_conv_taps_gpu.py: 4 x torch's fp32 CPU operator, same floors."""
    name, shape, kw = DECLINED[i]
    spec = make_spec(shape["cin"], shape["cout"], shape["P"], PRE_AFF, POST_LRELU, True, "separate", False, B=shape["B"], H=shape["H"])
    got, t = launch(spec, 9500 + i, expect88=False, **kw)
    check("declined-" + name, score(spec, t, got, "direct"), assert_figures=("output",))


def test_declined_cout48_is_refused_by_the_library():
    """Cout = 48 is no multiple of 32: no kernel of the family takes it (VFX_EINVAL from the entry point, before
    try_launch_convwg4s_2d is asked), nothing is launched and nothing written -- there is no result to hold to a bound."""
    x = torch.zeros((1, 32, 64 * 11), device=DEV)
    y = torch.full((1, 48, 64 * 11), NAN, device=DEV)
    w = torch.zeros((9, 32, 48), device=DEV)
    wg4 = torch.zeros((18, 4, 48, 8), device=DEV)
    lib = _lib.lib()
    before = lib.vfx_launch_count()
    with pytest.raises(_lib.VfxError, match="code -1"):
        ops.conv2d(x, w, None, y, 11, 6, 3, None, None, wg4=wg4)
    torch.cuda.synchronize()
    assert lib.vfx_launch_count() == before and torch.isnan(y).all()


def test_declined_reflect_padding_stays_off_this_kernel():
    """Reflect padding exists only on the 1-D entry point (vfx_conv2d_f32 pads maps with zeros): a k = 3 launch that offers
    w_wino4 with reflect padding does not report code 88 and meets the direct bound."""
    g = torch.Generator().manual_seed(77)
    B, C, L = 8, 64, 1000
    x, w, bias = _rand((B, C, L), g), _rand((C, C, 3), g, (3 * C) ** -0.5), _rand((C,), g, 0.3)
    xbase = torch.full((B, C, 264 + L + 264), NAN, device=DEV)
    xv = xbase[:, :, 264:264 + L]
    xv.copy_(x.to(DEV))
    xv._vfx_guard = 264
    ybase = torch.full((B, C, 8 + L + 8), NAN, device=DEV)
    yv = ybase[:, :, 8:8 + L]
    wp = packing.pack_conv1d(w)
    ops.conv1d(xv, wp.to(DEV), bias.to(DEV), yv, L, 3, 1, _lib.PAD_REFLECT, None, None, wg4=packing.pack_wino4(wp).to(DEV))
    torch.cuda.synchronize()
    assert _lib.lib().vfx_last_conv_tile() % 100 != 88
    assert torch.isnan(ybase[:, :, :8]).all() and torch.isnan(ybase[:, :, 8 + L:]).all()
    ref = ref64.conv1d(x, w, bias, reflect=True)
    mag = ref64.conv1d(x, w, bias, reflect=True, magnitude=True)
    dev, cpu = _Acc(), _Acc()
    dev.add(ref64.conv_error(yv.cpu(), ref, mag))
    cpu.add(ref64.conv_error(F.conv1d(F.pad(x, (1, 1), mode="reflect"), w, bias), ref, mag))
    check("declined-reflect-1d", {"output": (dev, cpu)}, assert_figures=("output",))
