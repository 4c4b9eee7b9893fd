"""conv_x3_kernel (voicefixer_amd/csrc/vfx_conv.hip, vfx_last_conv_tile() % 100 == 16: the opt-in VFX_MATH_BF16X3 arithmetic of
set_math("bf16x3")) at every launch the product makes, against the float64 statement of its stated arithmetic.

The reference is ``f64_reference.conv1d / convtr1d / conv2d(..., split="bf16x3")``: x~ (the pre-activated input in fp32, the affine
part one fused multiply-add) and w split into bf16 planes (hi = bf16(v), lo = bf16(v - hi), round to nearest even), the sum of
xh wh + xh wl + xl wh exact, bias and residual added after it.  The yardstick is torch's fp32 CPU operator on the tripled problem
(cat[xh, xh, xl] against cat[wh, wl, wh] along Cin: every product exact in fp32, so it scores fp32 accumulation of the same 3 K-term
sum); the device may be at most MARGIN = 4 times worse, maximum and RMS, with the floors of tests/test_conv_taps_gpu.py.

The machinery -- census, launch with NaN canaries over the whole allocation, channel subset, figures -- is that of
tests/test_convw_gpu.py (see its docstring); the host rule restated is plan_x3 of tests/test_convw_x3_geometry_cpu.py, which names
the template instance conv_x3_kernel<BM, BL, NT, MODE, ROWS> of every case.

* ``test_launch_census``: every code-16 launch of the seeded pipeline under set_math("bf16x3") at 32 x 10 s and 1 x 10 s is a row
  of ``CASES``; the ragged five-row batch shows none (the host declines per-row lengths: its launches are rows of
  test_convw_gpu.CASES or run on conv_taps_kernel / convwg4s_kernel).
* ``test_case_parity``: every row at a reduced size (both sides of Lq >= 4096 select the 64 x 256 / 64 x 128 tile; launches
  with K >= 1024 just past 96 workgroups), unit and heavy-tailed gains.
* ``test_edge_parity`` / ``test_declined``: what the product does not reach; exact properties."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from voicefixer_amd import _lib  # noqa: E402
from test_conv_taps_gpu import pipe  # noqa: E402,F401
import test_convw_x3_geometry_cpu as geo  # noqa: E402
import test_convw_gpu as cw  # noqa: E402
from test_convw_gpu import (CENSUS_RUNS, ELU, LRELU, NONE, SIGMOID, SNAKE, TANH, case_id, case_spec, census, census_check, launch,  # noqa: E402
                            make_spec, plan, record_key, run_case, statement64, _inputs)

A = _lib.PRE_AFFINE_LRELU
PL = _lib.PRE_LRELU

# code, BM, BL, op, Cin, Cout, pitch, k, dilation / stride, pre, post, post slope, bias, residual, row tags
# (every distinct code-16 launch of the census runs; test_launch_census keeps the table complete)
CASES = [
    (16, 64, 256, 'conv1d', 64, 64, 0, 3, 1, 0, 0, 0.0, True, 'in place', False),
    (16, 64, 256, 'conv1d', 64, 64, 0, 3, 1, 0, 1, 0.2, True, 'in place', False),
    (16, 64, 256, 'conv1d', 64, 64, 0, 3, 1, 1, 1, 0.01, True, 'none', False),
    (16, 64, 256, 'conv1d', 64, 64, 0, 3, 3, 1, 1, 0.01, True, 'none', False),
    (16, 64, 256, 'conv1d', 64, 64, 0, 3, 9, 1, 1, 0.01, True, 'none', False),
    (16, 64, 256, 'conv1d', 64, 64, 0, 3, 27, 1, 1, 0.01, True, 'none', False),
    (16, 64, 256, 'conv1d', 64, 64, 0, 3, 81, 1, 1, 0.01, True, 'none', False),
    (16, 64, 256, 'conv1d', 64, 64, 0, 3, 243, 1, 1, 0.01, True, 'none', False),
    (16, 64, 256, 'conv1d', 64, 64, 0, 3, 729, 1, 1, 0.01, True, 'none', False),
    (16, 64, 256, 'conv1d', 64, 64, 0, 3, 2187, 1, 1, 0.01, True, 'none', False),
    (16, 128, 128, 'conv1d', 128, 128, 0, 3, 1, 0, 0, 0.0, True, 'in place', False),
    (16, 128, 128, 'conv1d', 128, 128, 0, 3, 1, 0, 5, 0.2, True, 'in place', False),
    (16, 128, 128, 'conv1d', 128, 128, 0, 3, 1, 1, 1, 0.01, True, 'none', False),
    (16, 128, 128, 'conv1d', 128, 128, 0, 3, 3, 1, 1, 0.01, True, 'none', False),
    (16, 128, 128, 'conv1d', 128, 128, 0, 3, 9, 1, 1, 0.01, True, 'none', False),
    (16, 128, 128, 'conv1d', 128, 128, 0, 3, 27, 1, 1, 0.01, True, 'none', False),
    (16, 128, 128, 'conv1d', 128, 128, 0, 3, 81, 1, 1, 0.01, True, 'none', False),
    (16, 128, 128, 'conv1d', 128, 128, 0, 3, 243, 1, 1, 0.01, True, 'none', False),
    (16, 128, 128, 'conv1d', 128, 128, 0, 3, 729, 1, 1, 0.01, True, 'none', False),
    (16, 128, 128, 'conv1d', 128, 128, 0, 3, 2187, 1, 1, 0.01, True, 'none', False),
    (16, 128, 128, 'conv1d', 128, 512, 0, 3, 1, 0, 2, 0.0, True, 'none', False),
    (16, 128, 128, 'conv1d', 256, 256, 0, 3, 1, 0, 0, 0.0, True, 'in place', False),
    (16, 128, 128, 'conv1d', 256, 256, 0, 3, 1, 0, 5, 0.2, True, 'in place', False),
    (16, 128, 128, 'conv1d', 256, 256, 0, 3, 1, 1, 1, 0.01, True, 'none', False),
    (16, 128, 128, 'conv1d', 256, 256, 0, 3, 3, 1, 1, 0.01, True, 'none', False),
    (16, 128, 128, 'conv1d', 256, 256, 0, 3, 9, 1, 1, 0.01, True, 'none', False),
    (16, 128, 128, 'conv1d', 256, 256, 0, 3, 27, 1, 1, 0.01, True, 'none', False),
    (16, 128, 128, 'conv1d', 256, 256, 0, 3, 81, 1, 1, 0.01, True, 'none', False),
    (16, 128, 128, 'conv1d', 256, 256, 0, 3, 243, 1, 1, 0.01, True, 'none', False),
    (16, 128, 128, 'conv1d', 256, 256, 0, 3, 729, 1, 1, 0.01, True, 'none', False),
    (16, 128, 128, 'conv1d', 256, 256, 0, 3, 2187, 1, 1, 0.01, True, 'none', False),
    (16, 128, 128, 'conv1d', 512, 512, 0, 3, 1, 0, 0, 0.0, True, 'in place', False),
    (16, 128, 128, 'conv1d', 512, 512, 0, 3, 1, 0, 2, 0.0, True, 'none', False),
    (16, 128, 128, 'conv1d', 512, 512, 0, 3, 1, 0, 5, 0.2, True, 'in place', False),
    (16, 128, 128, 'conv1d', 512, 512, 0, 3, 1, 1, 1, 0.01, True, 'none', False),
    (16, 128, 128, 'conv1d', 512, 512, 0, 3, 3, 1, 1, 0.01, True, 'none', False),
    (16, 128, 128, 'conv1d', 512, 512, 0, 3, 9, 1, 1, 0.01, True, 'none', False),
    (16, 128, 128, 'conv1d', 512, 512, 0, 3, 27, 1, 1, 0.01, True, 'none', False),
    (16, 128, 128, 'conv1d', 512, 512, 0, 3, 81, 1, 1, 0.01, True, 'none', False),
    (16, 128, 128, 'conv1d', 512, 512, 0, 3, 243, 1, 1, 0.01, True, 'none', False),
    (16, 128, 128, 'conv1d', 512, 512, 0, 3, 729, 1, 1, 0.01, True, 'none', False),
    (16, 128, 128, 'conv1d', 512, 512, 0, 3, 2187, 1, 1, 0.01, True, 'none', False),
    (16, 64, 256, 'convtr1d', 128, 64, 0, 6, 3, 0, 0, 0.0, True, 'none', False),
    (16, 128, 128, 'convtr1d', 256, 128, 0, 6, 3, 0, 0, 0.0, True, 'none', False),
    (16, 128, 128, 'convtr1d', 512, 256, 0, 14, 7, 0, 0, 0.0, True, 'none', False),
    (16, 128, 128, 'convtr1d', 1024, 512, 0, 14, 7, 0, 0, 0.0, True, 'none', False),
    (16, 128, 128, 'conv2d', 384, 384, 4, 3, 1, 0, 0, 0.0, False, 'in place', False),
    (16, 128, 128, 'conv2d', 384, 384, 4, 3, 1, 0, 0, 0.0, False, 'separate', False),
    (16, 128, 128, 'conv2d', 384, 384, 4, 3, 1, 2, 1, 0.01, True, 'none', False),
    (16, 128, 128, 'conv2d', 768, 384, 4, 1, 1, 0, 0, 0.0, True, 'none', False),
    (16, 128, 128, 'conv2d', 768, 384, 4, 3, 1, 2, 1, 0.01, True, 'none', False),
    (16, 128, 128, 'conv2d', 256, 384, 8, 1, 1, 0, 0, 0.0, True, 'none', False),
    (16, 128, 128, 'conv2d', 256, 384, 8, 3, 1, 2, 1, 0.01, True, 'none', False),
    (16, 128, 128, 'conv2d', 384, 384, 8, 3, 1, 0, 0, 0.0, False, 'in place', False),
    (16, 128, 128, 'conv2d', 384, 384, 8, 3, 1, 0, 0, 0.0, False, 'separate', False),
    (16, 128, 128, 'conv2d', 384, 384, 8, 3, 1, 2, 1, 0.01, True, 'none', False),
    (16, 128, 128, 'conv2d', 768, 384, 8, 1, 1, 0, 0, 0.0, True, 'none', False),
    (16, 128, 128, 'conv2d', 768, 384, 8, 3, 1, 2, 1, 0.01, True, 'none', False),
    (16, 128, 128, 'conv2d', 128, 256, 16, 1, 1, 0, 0, 0.0, True, 'none', False),
    (16, 128, 128, 'conv2d', 128, 256, 16, 3, 1, 2, 1, 0.01, True, 'none', False),
    (16, 128, 128, 'conv2d', 256, 256, 16, 3, 1, 0, 0, 0.0, False, 'in place', False),
    (16, 128, 128, 'conv2d', 256, 256, 16, 3, 1, 0, 0, 0.0, False, 'separate', False),
    (16, 128, 128, 'conv2d', 256, 256, 16, 3, 1, 2, 1, 0.01, True, 'none', False),
    (16, 128, 128, 'conv2d', 512, 256, 16, 1, 1, 0, 0, 0.0, True, 'none', False),
    (16, 128, 128, 'conv2d', 512, 256, 16, 3, 1, 2, 1, 0.01, True, 'none', False),
    (16, 128, 128, 'conv2d', 64, 128, 32, 1, 1, 0, 0, 0.0, True, 'none', False),
    (16, 128, 128, 'conv2d', 64, 128, 32, 3, 1, 2, 1, 0.01, True, 'none', False),
    (16, 128, 128, 'conv2d', 128, 128, 32, 3, 1, 0, 0, 0.0, False, 'in place', False),
    (16, 128, 128, 'conv2d', 128, 128, 32, 3, 1, 0, 0, 0.0, False, 'separate', False),
    (16, 128, 128, 'conv2d', 128, 128, 32, 3, 1, 2, 1, 0.01, True, 'none', False),
    (16, 128, 128, 'conv2d', 256, 128, 32, 1, 1, 0, 0, 0.0, True, 'none', False),
    (16, 128, 128, 'conv2d', 256, 128, 32, 3, 1, 2, 1, 0.01, True, 'none', False),
    (16, 64, 256, 'conv2d', 32, 64, 64, 1, 1, 0, 0, 0.0, True, 'none', False),
    (16, 64, 256, 'conv2d', 32, 64, 64, 3, 1, 2, 1, 0.01, True, 'none', False),
    (16, 64, 256, 'conv2d', 64, 64, 64, 3, 1, 0, 0, 0.0, False, 'in place', False),
    (16, 64, 256, 'conv2d', 64, 64, 64, 3, 1, 0, 0, 0.0, False, 'separate', False),
    (16, 64, 256, 'conv2d', 64, 64, 64, 3, 1, 2, 1, 0.01, True, 'none', False),
    (16, 64, 256, 'conv2d', 128, 64, 64, 1, 1, 0, 0, 0.0, True, 'none', False),
    (16, 64, 256, 'conv2d', 128, 64, 64, 3, 1, 2, 1, 0.01, True, 'none', False),
    (16, 32, 256, 'conv2d', 32, 32, 128, 3, 1, 0, 0, 0.0, False, 'in place', False),
    (16, 32, 256, 'conv2d', 32, 32, 128, 3, 1, 0, 0, 0.0, False, 'separate', False),
    (16, 32, 256, 'conv2d', 32, 32, 128, 3, 1, 2, 1, 0.01, True, 'none', False),
    (16, 32, 256, 'conv2d', 64, 32, 128, 1, 1, 0, 0, 0.0, True, 'none', False),
    (16, 32, 256, 'conv2d', 64, 32, 128, 3, 1, 2, 1, 0.01, True, 'none', False),
]


def X(op, cin, cout, ext, B, **kw):
    return make_spec(op, cin, cout, ext, B, math="x3", **kw)


@pytest.mark.parametrize("mode,geometry", CENSUS_RUNS, ids=["%s-%s" % r for r in CENSUS_RUNS])
def test_launch_census(pipe, mode, geometry):  # noqa: F811
    """Every code-16 launch of the run is a row of CASES (only set_math("bf16x3") makes any), with the pinned count.  A ragged
    batch under bf16x3 shows no code 16 at all: every one of its launches carries row tags, which the host declines."""
    rec = census_check(pipe, mode, geometry, (16,), set(CASES))
    x3 = [r for r in rec.records if r["code"] == 16]
    assert (len(x3) > 0) == (mode == "bf16x3" and geometry != "ragged5")
    assert not any(r["rows"] for r in x3), "a launch with row tags ran on conv_x3_kernel"


def test_every_case_is_a_product_launch(pipe):  # noqa: F811
    seen = {record_key(r) for run in CENSUS_RUNS if run[0] == "bf16x3" for r in census(pipe, *run).records}
    missing = [case_id(k) for k in CASES if k not in seen]
    assert not missing, "rows of CASES that no census run launches: %r" % missing


@pytest.mark.parametrize("gains", ["unit", "heavy"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=[case_id(k) for k in CASES])
def test_case_parity(i, gains):
    """Every row of CASES at its reduced size, with unit gains and with heavy-tailed ones (profiles/convw_x3_parity.txt).

    Finding, fixed in the kernel; these are its regression cases.  While conv_x3_kernel started its accumulators at the bias and,
    with a residual on a plain output map, at bias + residual, every partial sum of the 3 K-term chain rounded at their magnitude:
    55 of the 84 rows with heavy-tailed gains were above the bound, at up to 20.1 x the yardstick's maximum and 14.9 x its RMS
    (unit gains: 0.2 - 3.0 x / 0.3 - 1.7 x).  The accumulators now start at zero and bias and residual are added to the finished sum,
    in torch's order (conv_epilogue with SUM_FIRST): all 168 rows at 0.2 - 2.2 x / 0.3 - 1.1 x."""
    key = CASES[i]
    p = run_case(case_spec(key, gains == "heavy", "x3"), 21000 + 2 * i + (gains == "heavy"), case_id(key) + "-" + gains)
    assert (p["BM"], p["BL"]) == key[1:3]


# --------------------------------------------------------------------------------------
# edges the product does not reach
# --------------------------------------------------------------------------------------
L1 = dict(pre=PL, post=LRELU, post_slope=0.2)
# name -> spec; every second edge draws heavy-tailed gains.  What each group is for:
#  tile-*          all four tiles: 128 x 128, 64 x 256 (Lq >= 4096), 64 x 128 (below), 32 x 256 (Cout % 64 != 0: 3x3 and 1x1 only)
#  d4 / d5         staging mode 0 (halo inside the BL columns: BL - span outputs) / 1 (BL + span columns); d60 / d61: mode 1 / one
#                  tap per K-step (ROWS 3, NT 1); d2187: the same with the dilation beyond L
#  lq-*            Lq = n bl_eff - 1, n bl_eff, n bl_eff + 1 (bl_eff = BL - span)
#  cin*            Cin = 32, 64, 96, 160 (two to ten K-steps: the loop body runs pairs)
#  wg97            K >= 1024 just past the 96 workgroups below which the host declines (test_declined: 96)
#  tr-s*           transposed strides 2, 3, 7, 8, Cout = 64 (a 64-row block per phase) and 256 (two 128-row blocks per phase)
#  map-P4-*        the 3x3 at pitch 4, the minimum, H = 1, 2, 7; map-affine: PRE_AFFINE_LRELU with its 16 KB table in LDS, and at
#                  Cin = 12288 with 96 KB of it: exactly the 160 KB of dynamic LDS the host accepts, one workgroup per CU (12320 is
#                  declined: test_declined)
#  res-* / y-ls2   residual in place / separate / with strides of its own, an output of element stride 2
#  post-*          every post-activation
EDGES = [
    ("tile-128x128", X("conv1d", 64, 128, 1001, 2, **L1)),
    ("tile-64x256", X("conv1d", 64, 64, 4096, 1, **L1)),
    ("tile-64x128", X("conv1d", 64, 64, 4095, 1, **L1)),
    ("tile-32x256-3x3", X("conv2d", 32, 32, 9, 2, pitch=64, pre=A, post=LRELU, post_slope=0.01)),
    ("tile-32x256-1x1", X("conv2d", 64, 32, 9, 2, k=1, pitch=64)),
    ("d4-mode0", X("conv1d", 64, 128, 1001, 2, step=4, **L1)),
    ("d5-mode1", X("conv1d", 64, 128, 1001, 2, step=5, **L1)),
    ("d60-mode1", X("conv1d", 64, 128, 1001, 2, step=60, **L1)),
    ("d61-tapsplit", X("conv1d", 64, 128, 1001, 2, step=61, **L1)),
    ("d2187-tapsplit-beyond-L", X("conv1d", 64, 64, 743, 2, step=2187, **L1)),
    ("lq-8x126-1", X("conv1d", 32, 128, 8 * 126 - 1, 2, **L1)),
    ("lq-8x126", X("conv1d", 32, 128, 8 * 126, 2, **L1)),
    ("lq-8x126+1", X("conv1d", 32, 128, 8 * 126 + 1, 2, **L1)),
    ("lq-d9-8x128+1", X("conv1d", 32, 128, 8 * 128 + 1, 2, step=9, **L1)),
] + [("cin%d" % c, X("conv1d", c, 128, 1001, 2, **L1)) for c in (32, 64, 96, 160)] + [
    ("wg97-k1056", X("conv1d", 352, 128, 96 * 126 + 1, 1, **L1)),
] + [("tr-s%d-cout%d" % (s, c), X("convtr1d", 64, c, 531, 2, k=2 * s, step=s)) for s in (2, 3, 7, 8) for c in (64, 256)] + [
    ("map-P4-H1", X("conv2d", 64, 128, 1, 3, pitch=4, pre=A, post=LRELU, post_slope=0.01)),
    ("map-P4-H2", X("conv2d", 64, 64, 2, 3, pitch=4, bias=False, res="in place")),
    ("map-P4-H7", X("conv2d", 64, 32, 7, 3, pitch=4, pre=A, post=LRELU, post_slope=0.01)),
    ("map-affine-cin2048", X("conv2d", 2048, 128, 7, 97, pitch=4, pre=A, post=LRELU, post_slope=0.01)),
    ("map-affine-cin12288-lds160k", X("conv2d", 12288, 128, 2, 97, pitch=4, pre=A, post=LRELU, post_slope=0.01)),
    ("map-1x1-P8", X("conv2d", 96, 128, 37, 2, k=1, pitch=8)),
    ("res-inplace", X("conv1d", 64, 128, 1001, 2, res="in place")),
    ("res-separate-snake", X("conv1d", 64, 128, 1001, 2, res="separate", post=SNAKE, post_slope=0.2)),
    ("res-own-strides", X("conv1d", 64, 64, 4100, 1, res="separate", r_own=True, post=LRELU, post_slope=0.2)),
    ("y-ls2-res-inplace", X("conv1d", 64, 128, 1001, 2, res="in place", y_ls=2)),
    ("map-res-own-strides", X("conv2d", 64, 64, 70, 2, pitch=64, bias=False, res="separate", r_own=True)),
] + [("post-%d" % post, X("conv1d", 64, 128, 1001, 2, pre=PL, post=post, post_slope=0.2, res="in place")) for post in
     (NONE, LRELU, ELU, TANH, SIGMOID, SNAKE)]
EDGE_IDS = [e[0] for e in EDGES]


@pytest.mark.parametrize("i", range(len(EDGES)), ids=EDGE_IDS)
def test_edge_parity(i):
    name, spec = EDGES[i]
    p = run_case(dict(spec, heavy=i % 2 == 1), 22000 + i, "x3-" + name)
    print("EDGE x3-%s ran as %s, %d tiles of %d" % (name, p["name"], p["ntiles"], p["bl_eff"]))


def test_edges_reach_what_they_are_named_for():
    pl = {name: plan(spec) for name, spec in EDGES}
    assert [pl[n]["instance"] for n in ("tile-128x128", "tile-64x256", "tile-64x128", "tile-32x256-3x3", "tile-32x256-1x1")] == [
        (128, 128, 3, 0, 1), (64, 256, 3, 0, 1), (64, 128, 3, 0, 1), (32, 256, 3, 0, 3), (32, 256, 1, 0, 1)]
    assert [pl[n]["instance"][2:] for n in ("d4-mode0", "d5-mode1", "d60-mode1", "d61-tapsplit", "d2187-tapsplit-beyond-L")] == [
        (3, 0, 1), (3, 1, 1), (3, 1, 1), (1, 0, 3), (1, 0, 3)]
    assert [pl[n]["ntiles"] for n in ("lq-8x126-1", "lq-8x126", "lq-8x126+1", "lq-d9-8x128+1")] == [8, 8, 9, 9]
    assert pl["wg97-k1056"]["grid"] == (97, 1, 1)
    for s in (2, 3, 7, 8):
        assert pl["tr-s%d-cout64" % s]["grid"][1] == s and pl["tr-s%d-cout256" % s]["grid"][1] == 2 * s
        assert pl["tr-s%d-cout64" % s]["instance"][2:] == (2, 0, 1)
    assert all(pl[n]["instance"][4] == 3 for n in pl if n.startswith("map-P4") or n.startswith("map-affine"))
    assert pl["map-affine-cin2048"]["lds"] == 65536 + 16384 and pl["map-affine-cin12288-lds160k"]["lds"] == 160 * 1024


# name -> a launch conv_x3_kernel must NOT take: the fp32 fallback (conv_taps_kernel here), asserted and held to its own bound
DECLINED = [
    ("wg96-k1056", X("conv1d", 352, 128, 96 * 126, 1, **L1)),
    ("cout32-k3", X("conv1d", 64, 32, 1001, 2, **L1)),
    ("cout32-transposed", X("convtr1d", 64, 32, 531, 2, k=4, step=2)),
    ("guard-one-short", X("conv1d", 64, 128, 1000, 2, step=9, guard=7 * 128 + 9 + 128 - 1000 - 1, **L1)),
    ("rows", X("conv1d", 64, 128, 1001, 2, lengths=[1001, 300], **L1)),
    ("cin48", X("conv1d", 48, 128, 1001, 2, **L1)),
    ("map-P2", X("conv2d", 64, 64, 9, 2, pitch=2)),
    ("map-affine-cin12320-lds", X("conv2d", 12320, 128, 2, 97, pitch=4, pre=A, post=LRELU, post_slope=0.01)),
]


@pytest.mark.parametrize("i", range(len(DECLINED)), ids=[d[0] for d in DECLINED])
def test_declined(i):
    """The bf16 planes are offered and the host declines: K >= 1024 on 96 workgroups (97 is the `wg97-k1056` edge), Cout % 64 != 0
    with three taps or transposed phases, a guard one short of interior, per-row lengths, Cin % 32 != 0, pitch 2, and an affine
    table that takes the dynamic LDS past 160 KB (Cin = 12320; 12288 is the `map-affine-cin12288-lds160k` edge).  The launch
    runs in fp32 and is scored as such."""
    name, spec = DECLINED[i]
    spec = dict(spec, heavy=i % 2 == 1)
    got, t, _ = launch(spec, 22500 + i, expect=None)
    dev, cpu = cw.score(dict(spec, math="f32"), t, got, 22500 + i)
    cw.check("x3-declined-" + name, dev, cpu)


# --------------------------------------------------------------------------------------
# exact properties
# --------------------------------------------------------------------------------------
EXACT = [("k3-128x128", X("conv1d", 64, 128, 1001, 4, res="in place", post=LRELU, post_slope=0.2)),
         ("k3-d61-64x256", X("conv1d", 32, 64, 4100, 4, step=61, **L1)),
         ("tr-s3", X("convtr1d", 64, 128, 531, 4, k=6, step=3)),
         ("map-32x256", X("conv2d", 32, 32, 9, 4, pitch=64, res="in place", post=LRELU, post_slope=0.01))]
EXACT_IDS = [e[0] for e in EXACT]


@pytest.mark.parametrize("e", EXACT, ids=EXACT_IDS)
def test_zero_weights_return_bias_plus_residual(e):
    """With zero weights every output is post(bias + residual) bit for bit."""
    spec = dict(e[1], w_scale=0.0, heavy=True)
    got, t, _ = launch(spec, 23000)
    want = t["bias"].reshape([1, -1] + [1] * (got.dim() - 2)).expand_as(got)
    if t["res"] is not None:
        want = want + t["res"]
    assert torch.equal(got, cw._post_f32(want, spec))


@pytest.mark.parametrize("e", EXACT, ids=EXACT_IDS)
def test_batch_items_are_independent(e):
    spec = dict(e[1], heavy=True)
    t = _inputs(spec, 23100)
    t["x"][3] = t["x"][0]
    if t["res"] is not None:
        t["res"][3] = t["res"][0]
    got, _, _ = launch(spec, 0, t=t)
    assert torch.equal(got[0], got[3]) and not torch.equal(got[0], got[1])


@pytest.mark.parametrize("e", [X("conv1d", 64, 128, 1001, 2, step=5), X("convtr1d", 64, 64, 531, 2, k=6, step=3),
                               X("conv2d", 32, 32, 9, 2, pitch=64), X("conv1d", 64, 64, 4100, 1, step=61)],
                         ids=["k3-d5", "tr-s3", "map-3x3", "k3-d61"])
def test_bf16_exact_operands_give_the_plain_float64_sum(e, request):
    """Weights and inputs exactly representable in bf16 (no pre-activation): every `lo` plane is zero, so the statement IS the
    plain float64 convolution, and the device -- whose xh wl and xl wh products must then all vanish -- is within the fp32
    accumulation bound of it: a direct check that the `lo` products read the right operands."""
    spec = dict(e, bf16_exact=True, heavy=True)
    got, t, _ = launch(spec, 23200)
    assert torch.equal(statement64(spec, t, list(range(spec["cout"])), False, "bf16x3"), statement64(spec, t, list(range(spec["cout"])), False))
    dev, cpu = cw.score(spec, t, got, 23200)
    cw.check("x3-bf16-exact-" + request.node.callspec.id, dev, cpu)
