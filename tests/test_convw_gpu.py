"""convw_kernel (voicefixer_amd/csrc/vfx_convw.inc, unfused: vfx_last_conv_tile() % 100 == 51 / 52 / 54, and 59 for the 3x3 on a
pitch map) at every launch the product makes, against float64.  convw_kernel is the "direct" variant of the product's self-check
(engine.set_winograd(False)), takes one 3x3 launch of every default step and whatever the Winograd F(4,3) kernels decline while the
launch still has 384 workgroups.

* ``test_launch_census`` runs the seeded pipeline at 32 x 10 s, 1 x 10 s and the ragged five-row batch under
  voicefixer_amd.launch_record, in default fp32, under set_winograd(False) and under set_math("bf16x3"), and asserts that every
  launch on codes 51 / 52 / 54 / 59 is a row of ``CASES``: the key is (code, BM, BL, op, Cin, Cout, pitch, k, dilation / stride, pre,
  post, post slope, bias, residual none / in place / separate, row tags).  The launches per code are pinned per run, those of the
  fused direct layer (codes 61 / 62 / 64) included, so the record says how much of "direct" runs there.
* ``test_case_parity`` launches every row of ``CASES`` with the product's Cin, Cout and geometry, B and the extent cut down to the
  least at which the host still selects the row's instance (just past 384 workgroups), once with unit gains and once with
  heavy-tailed weight-norm gains exp(1.5 z - 2.25) and a unit-scale bias.
* ``test_edge_parity`` does the same for what the product does not reach (``EDGES``); ``test_declined`` asserts what must run
  elsewhere, at the direct kernels' 2e-5.
* exact properties: zero weights, batch independence, ragged rows against the rows alone, folded against unfolded phase order.

Every spec is first walked by the restated host rule (tests/test_convw_x3_geometry_cpu.py: plan_convw / plan_x3), which names the
instance; the tile code is asserted against it after the launch.  Buffers are laid out as the engine lays them out: guarded views,
NaN in the guard bands, past every row's own end, in the pad column of pitch maps and in the whole output allocation.  Every launch
asserts one launch, no NaN inside a row's valid output, nothing but NaN outside it, an output pad column of exactly 0, and x (and
a separate residual) unchanged bit for bit.

The figure is ``conv_error`` against the float64 statement and its ``magnitude=True`` twin: |got - ref| / (lip M + |ref|).  The
bound is measured on the reference side: torch's fp32 CPU operator on the same operands may be exceeded at most MARGIN = 4 times,
maximum and RMS, with the floors of tests/test_conv_taps_gpu.py.  Where float64 over the whole launch would take more than a few
seconds both are scored on a SUBSET of the output channels over all positions (the first and last row of every 32-row wave block,
seeded others up to one in eight, and under heavy gains the four channels with the largest |bias| / rms(sum)); every other channel
is compared with the fp32 operator at 2e-5 of the launch's peak.  Every case prints
``PARITY <id> <cpu max> <dev max> <ratio> <cpu rms> <dev rms> <ratio>`` before it asserts; profiles/convw_x3_parity.txt is that
output."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from voicefixer_amd import ops, packing, _lib, launch_record  # noqa: E402
from oracle import f64_reference as ref64  # noqa: E402
from test_conv_taps_gpu import MARGIN, RMS_FLOOR, ULP, RAGGED_SAMPLES, _Acc, _post32, pipe  # noqa: E402,F401
import test_convw_x3_geometry_cpu as geo  # noqa: E402

DEV = "cuda"
NAN = float("nan")
DIRECT_TOL = 2e-5            # channels outside the float64 subset: the fp32 CPU operator, of the launch's peak
F64_BUDGET = 2.5e9           # multiply-adds of one float64 pass above which the channel subset is scored
NONE, LRELU, ELU, TANH, SIGMOID, SNAKE = (_lib.POST_NONE, _lib.POST_LRELU, _lib.POST_ELU, _lib.POST_TANH, _lib.POST_SIGMOID,
                                          _lib.POST_LRELU_SNAKE)
assert (_lib.PRE_NONE, _lib.PRE_LRELU, _lib.PRE_AFFINE_LRELU) == (geo.PRE_NONE, geo.PRE_LRELU, geo.PRE_AFFINE_LRELU)

# code, BM, BL, op, Cin, Cout, pitch, k, dilation / stride, pre, post, post slope, bias, residual, row tags
# (every distinct launch on codes 51 / 52 / 54 / 59 of the nine census runs; test_launch_census keeps the table complete)
CASES = [
    (52, 64, 256, 'conv1d', 64, 64, 0, 3, 1, 0, 0, 0.0, True, 'in place', True),
    (52, 64, 256, 'conv1d', 64, 64, 0, 3, 1, 0, 1, 0.2, True, 'in place', True),
    (52, 64, 256, 'conv1d', 64, 64, 0, 3, 1, 1, 1, 0.01, True, 'none', True),
    (52, 64, 256, 'conv1d', 64, 64, 0, 3, 3, 1, 1, 0.01, True, 'none', True),
    (52, 64, 256, 'conv1d', 64, 64, 0, 3, 9, 1, 1, 0.01, True, 'none', True),
    (52, 64, 256, 'conv1d', 64, 64, 0, 3, 27, 1, 1, 0.01, True, 'none', True),
    (51, 64, 256, 'conv1d', 64, 64, 0, 3, 81, 1, 1, 0.01, True, 'none', True),
    (51, 64, 256, 'conv1d', 64, 64, 0, 3, 243, 1, 1, 0.01, True, 'none', True),
    (51, 64, 256, 'conv1d', 64, 64, 0, 3, 729, 1, 1, 0.01, True, 'none', True),
    (51, 64, 256, 'conv1d', 64, 64, 0, 3, 2187, 1, 1, 0.01, True, 'none', True),
    (54, 128, 128, 'conv1d', 128, 128, 0, 3, 1, 0, 0, 0.0, True, 'in place', True),
    (54, 128, 128, 'conv1d', 128, 128, 0, 3, 1, 0, 5, 0.2, True, 'in place', True),
    (54, 128, 128, 'conv1d', 128, 128, 0, 3, 1, 1, 1, 0.01, True, 'none', True),
    (54, 128, 128, 'conv1d', 128, 128, 0, 3, 3, 1, 1, 0.01, True, 'none', True),
    (54, 128, 128, 'conv1d', 128, 128, 0, 3, 9, 1, 1, 0.01, True, 'none', True),
    (54, 128, 128, 'conv1d', 128, 128, 0, 3, 27, 1, 1, 0.01, True, 'none', True),
    (52, 128, 128, 'conv1d', 128, 128, 0, 3, 81, 1, 1, 0.01, True, 'none', True),
    (52, 128, 128, 'conv1d', 128, 128, 0, 3, 243, 1, 1, 0.01, True, 'none', True),
    (52, 128, 128, 'conv1d', 128, 128, 0, 3, 729, 1, 1, 0.01, True, 'none', True),
    (52, 128, 128, 'conv1d', 128, 128, 0, 3, 2187, 1, 1, 0.01, True, 'none', True),
    (54, 128, 128, 'conv1d', 128, 512, 0, 3, 1, 0, 2, 0.0, True, 'none', False),
    (54, 128, 128, 'conv1d', 256, 256, 0, 3, 1, 0, 0, 0.0, True, 'in place', False),
    (54, 128, 128, 'conv1d', 256, 256, 0, 3, 1, 0, 0, 0.0, True, 'in place', True),
    (54, 128, 128, 'conv1d', 256, 256, 0, 3, 1, 0, 5, 0.2, True, 'in place', False),
    (54, 128, 128, 'conv1d', 256, 256, 0, 3, 1, 0, 5, 0.2, True, 'in place', True),
    (54, 128, 128, 'conv1d', 256, 256, 0, 3, 1, 1, 1, 0.01, True, 'none', False),
    (54, 128, 128, 'conv1d', 256, 256, 0, 3, 1, 1, 1, 0.01, True, 'none', True),
    (54, 128, 128, 'conv1d', 256, 256, 0, 3, 3, 1, 1, 0.01, True, 'none', False),
    (54, 128, 128, 'conv1d', 256, 256, 0, 3, 3, 1, 1, 0.01, True, 'none', True),
    (54, 128, 128, 'conv1d', 256, 256, 0, 3, 9, 1, 1, 0.01, True, 'none', False),
    (54, 128, 128, 'conv1d', 256, 256, 0, 3, 9, 1, 1, 0.01, True, 'none', True),
    (54, 128, 128, 'conv1d', 256, 256, 0, 3, 27, 1, 1, 0.01, True, 'none', False),
    (54, 128, 128, 'conv1d', 256, 256, 0, 3, 27, 1, 1, 0.01, True, 'none', True),
    (52, 128, 128, 'conv1d', 256, 256, 0, 3, 81, 1, 1, 0.01, True, 'none', False),
    (52, 128, 128, 'conv1d', 256, 256, 0, 3, 81, 1, 1, 0.01, True, 'none', True),
    (52, 128, 128, 'conv1d', 256, 256, 0, 3, 243, 1, 1, 0.01, True, 'none', False),
    (52, 128, 128, 'conv1d', 256, 256, 0, 3, 243, 1, 1, 0.01, True, 'none', True),
    (52, 128, 128, 'conv1d', 256, 256, 0, 3, 729, 1, 1, 0.01, True, 'none', False),
    (52, 128, 128, 'conv1d', 256, 256, 0, 3, 729, 1, 1, 0.01, True, 'none', True),
    (52, 128, 128, 'conv1d', 256, 256, 0, 3, 2187, 1, 1, 0.01, True, 'none', False),
    (52, 128, 128, 'conv1d', 256, 256, 0, 3, 2187, 1, 1, 0.01, True, 'none', True),
    (54, 128, 128, 'conv1d', 512, 512, 0, 3, 1, 0, 0, 0.0, True, 'in place', False),
    (54, 128, 128, 'conv1d', 512, 512, 0, 3, 1, 0, 0, 0.0, True, 'in place', True),
    (54, 128, 128, 'conv1d', 512, 512, 0, 3, 1, 0, 2, 0.0, True, 'none', False),
    (54, 128, 128, 'conv1d', 512, 512, 0, 3, 1, 0, 5, 0.2, True, 'in place', False),
    (54, 128, 128, 'conv1d', 512, 512, 0, 3, 1, 0, 5, 0.2, True, 'in place', True),
    (54, 128, 128, 'conv1d', 512, 512, 0, 3, 1, 1, 1, 0.01, True, 'none', False),
    (54, 128, 128, 'conv1d', 512, 512, 0, 3, 1, 1, 1, 0.01, True, 'none', True),
    (54, 128, 128, 'conv1d', 512, 512, 0, 3, 3, 1, 1, 0.01, True, 'none', False),
    (54, 128, 128, 'conv1d', 512, 512, 0, 3, 3, 1, 1, 0.01, True, 'none', True),
    (54, 128, 128, 'conv1d', 512, 512, 0, 3, 9, 1, 1, 0.01, True, 'none', False),
    (54, 128, 128, 'conv1d', 512, 512, 0, 3, 9, 1, 1, 0.01, True, 'none', True),
    (54, 128, 128, 'conv1d', 512, 512, 0, 3, 27, 1, 1, 0.01, True, 'none', False),
    (54, 128, 128, 'conv1d', 512, 512, 0, 3, 27, 1, 1, 0.01, True, 'none', True),
    (52, 128, 128, 'conv1d', 512, 512, 0, 3, 81, 1, 1, 0.01, True, 'none', False),
    (52, 128, 128, 'conv1d', 512, 512, 0, 3, 81, 1, 1, 0.01, True, 'none', True),
    (52, 128, 128, 'conv1d', 512, 512, 0, 3, 243, 1, 1, 0.01, True, 'none', False),
    (52, 128, 128, 'conv1d', 512, 512, 0, 3, 243, 1, 1, 0.01, True, 'none', True),
    (52, 128, 128, 'conv1d', 512, 512, 0, 3, 729, 1, 1, 0.01, True, 'none', False),
    (52, 128, 128, 'conv1d', 512, 512, 0, 3, 729, 1, 1, 0.01, True, 'none', True),
    (52, 128, 128, 'conv1d', 512, 512, 0, 3, 2187, 1, 1, 0.01, True, 'none', False),
    (52, 128, 128, 'conv1d', 512, 512, 0, 3, 2187, 1, 1, 0.01, True, 'none', True),
    (52, 64, 256, 'convtr1d', 128, 64, 0, 6, 3, 0, 0, 0.0, True, 'none', False),
    (52, 64, 256, 'convtr1d', 128, 64, 0, 6, 3, 0, 0, 0.0, True, 'none', True),
    (54, 128, 128, 'convtr1d', 256, 128, 0, 6, 3, 0, 0, 0.0, True, 'none', False),
    (54, 128, 128, 'convtr1d', 256, 128, 0, 6, 3, 0, 0, 0.0, True, 'none', True),
    (54, 128, 128, 'convtr1d', 512, 256, 0, 14, 7, 0, 0, 0.0, True, 'none', False),
    (54, 128, 128, 'convtr1d', 512, 256, 0, 14, 7, 0, 0, 0.0, True, 'none', True),
    (54, 128, 128, 'convtr1d', 1024, 512, 0, 14, 7, 0, 0, 0.0, True, 'none', False),
    (54, 128, 128, 'convtr1d', 1024, 512, 0, 14, 7, 0, 0, 0.0, True, 'none', True),
    (59, 128, 64, 'conv2d', 256, 384, 8, 3, 1, 2, 1, 0.01, True, 'none', False),
    (59, 128, 64, 'conv2d', 384, 384, 8, 3, 1, 0, 0, 0.0, False, 'in place', False),
    (59, 128, 64, 'conv2d', 384, 384, 8, 3, 1, 0, 0, 0.0, False, 'separate', False),
    (59, 128, 64, 'conv2d', 384, 384, 8, 3, 1, 2, 1, 0.01, True, 'none', False),
    (59, 128, 64, 'conv2d', 768, 384, 8, 3, 1, 2, 1, 0.01, True, 'none', False),
    (59, 128, 128, 'conv2d', 128, 256, 16, 3, 1, 2, 1, 0.01, True, 'none', False),
    (59, 128, 128, 'conv2d', 256, 256, 16, 3, 1, 0, 0, 0.0, False, 'in place', False),
    (59, 128, 128, 'conv2d', 256, 256, 16, 3, 1, 0, 0, 0.0, False, 'separate', False),
    (59, 128, 128, 'conv2d', 256, 256, 16, 3, 1, 2, 1, 0.01, True, 'none', False),
    (59, 128, 128, 'conv2d', 512, 256, 16, 3, 1, 2, 1, 0.01, True, 'none', False),
    (59, 128, 128, 'conv2d', 64, 128, 32, 3, 1, 2, 1, 0.01, True, 'none', False),
    (59, 128, 64, 'conv2d', 64, 128, 32, 3, 1, 2, 1, 0.01, True, 'none', True),
    (59, 128, 128, 'conv2d', 128, 128, 32, 3, 1, 0, 0, 0.0, False, 'in place', False),
    (59, 128, 64, 'conv2d', 128, 128, 32, 3, 1, 0, 0, 0.0, False, 'in place', True),
    (59, 128, 128, 'conv2d', 128, 128, 32, 3, 1, 0, 0, 0.0, False, 'separate', False),
    (59, 128, 64, 'conv2d', 128, 128, 32, 3, 1, 0, 0, 0.0, False, 'separate', True),
    (59, 128, 128, 'conv2d', 128, 128, 32, 3, 1, 2, 1, 0.01, True, 'none', False),
    (59, 128, 64, 'conv2d', 128, 128, 32, 3, 1, 2, 1, 0.01, True, 'none', True),
    (59, 128, 128, 'conv2d', 256, 128, 32, 3, 1, 2, 1, 0.01, True, 'none', False),
    (59, 128, 64, 'conv2d', 256, 128, 32, 3, 1, 2, 1, 0.01, True, 'none', True),
    (59, 64, 128, 'conv2d', 32, 64, 64, 3, 1, 2, 1, 0.01, True, 'none', False),
    (59, 64, 128, 'conv2d', 32, 64, 64, 3, 1, 2, 1, 0.01, True, 'none', True),
    (59, 64, 128, 'conv2d', 64, 64, 64, 3, 1, 0, 0, 0.0, False, 'in place', False),
    (59, 64, 128, 'conv2d', 64, 64, 64, 3, 1, 0, 0, 0.0, False, 'in place', True),
    (59, 64, 128, 'conv2d', 64, 64, 64, 3, 1, 0, 0, 0.0, False, 'separate', False),
    (59, 64, 128, 'conv2d', 64, 64, 64, 3, 1, 0, 0, 0.0, False, 'separate', True),
    (59, 64, 128, 'conv2d', 64, 64, 64, 3, 1, 2, 1, 0.01, True, 'none', False),
    (59, 64, 128, 'conv2d', 64, 64, 64, 3, 1, 2, 1, 0.01, True, 'none', True),
    (59, 64, 128, 'conv2d', 128, 64, 64, 3, 1, 2, 1, 0.01, True, 'none', False),
    (59, 64, 128, 'conv2d', 128, 64, 64, 3, 1, 2, 1, 0.01, True, 'none', True),
    (59, 32, 256, 'conv2d', 8, 32, 128, 3, 1, 2, 1, 0.01, True, 'none', False),
    (59, 32, 256, 'conv2d', 8, 32, 128, 3, 1, 2, 1, 0.01, True, 'none', True),
    (59, 32, 256, 'conv2d', 32, 32, 128, 3, 1, 0, 0, 0.0, False, 'in place', False),
    (59, 32, 256, 'conv2d', 32, 32, 128, 3, 1, 0, 0, 0.0, False, 'in place', True),
    (59, 32, 256, 'conv2d', 32, 32, 128, 3, 1, 0, 0, 0.0, False, 'separate', False),
    (59, 32, 256, 'conv2d', 32, 32, 128, 3, 1, 0, 0, 0.0, False, 'separate', True),
    (59, 32, 256, 'conv2d', 32, 32, 128, 3, 1, 2, 1, 0.01, True, 'none', False),
    (59, 32, 256, 'conv2d', 32, 32, 128, 3, 1, 2, 1, 0.01, True, 'none', True),
    (59, 32, 256, 'conv2d', 64, 32, 128, 3, 1, 2, 1, 0.01, True, 'none', False),
    (59, 32, 256, 'conv2d', 64, 32, 128, 3, 1, 2, 1, 0.01, True, 'none', True),
]

# launches per code of each census run (mode, geometry)
COUNTS = {
    ('f32', 'b32x10'): {59: 1},
    ('f32', 'b1x10'): {59: 18},
    ('f32', 'ragged5'): {59: 17},
    ('direct', 'b32x10'): {52: 9, 54: 32, 59: 82, 61: 4, 62: 8, 64: 4},
    ('direct', 'b1x10'): {52: 5, 54: 14, 59: 18, 61: 4, 62: 8, 64: 4},
    ('direct', 'ragged5'): {52: 9, 54: 27, 59: 50, 61: 4, 62: 8, 64: 4},
    ('bf16x3', 'b32x10'): {16: 180, 59: 1},
    ('bf16x3', 'b1x10'): {16: 113, 59: 1},
    ('bf16x3', 'ragged5'): {51: 4, 52: 25, 54: 39, 59: 17},
}
CENSUS_CODES = (16, 51, 52, 54, 59, 61, 62, 64)
POST_NAMES = {NONE: "nopost", LRELU: "lrelu", ELU: "elu", TANH: "tanh", SIGMOID: "sigmoid", SNAKE: "snake"}


def case_id(key):
    code, BM, BL, op, cin, cout, pitch, k, step, pre, post, ps, bias, res, rows = key
    s = "k%d-%dx%d-%s-%dto%d" % (code, BM, BL, op, cin, cout) + ("-P%d" % pitch if pitch else "") + "-k%d" % k
    s += ("-%s%d" % ("s" if op == "convtr1d" else "d", step) if step != 1 else "") + "-pre%d-%s" % (pre, POST_NAMES[post])
    s += ("%g" % ps if post in (LRELU, SNAKE) else "") + ("-bias" if bias else "")
    return s + {"none": "", "separate": "-res", "in place": "-resinplace"}[res] + ("-rows" if rows else "")


# --------------------------------------------------------------------------------------
# one launch
# --------------------------------------------------------------------------------------
def engine_guard(op, k, step, pitch):
    """The guard band the engine gives an input: largest tap offset + 264 (engine.G_TILE)."""
    if pitch:
        return pitch + 1 + geo.G_TILE
    return (k - 1) // 2 * step + geo.G_TILE if op == "conv1d" else geo.G_TILE


def make_spec(op, cin, cout, ext, B, k=3, step=1, pitch=0, pre=_lib.PRE_NONE, pre_slope=0.01, post=NONE, post_slope=0.0, bias=True,
              res="none", lengths=None, guard=None, heavy=False, w_scale=1.0, math="f32", y_ls=1, r_own=False, r_ls=1, bf16_exact=False):
    """math: "f32" offers the launch packing.pack_direct (convw_kernel), "x3" packing.pack_x3 (conv_x3_kernel).  lengths: per-row
    extents (samples, or map rows).  y_ls: element stride of the output view.  r_own: a separate residual with strides of its own
    (more channels and a longer pitch than y), r_ls its element stride.  bf16_exact: operands exactly representable in bf16."""
    return dict(op=op, cin=cin, cout=cout, ext=ext, B=B, k=k, step=step, pitch=pitch, pre=pre, pre_slope=pre_slope, post=post,
                post_slope=post_slope, bias=bias, res=res, lengths=lengths, guard=engine_guard(op, k, step, pitch) if guard is None else guard,
                heavy=heavy, w_scale=w_scale, math=math, y_ls=y_ls, r_own=r_own, r_ls=r_ls, bf16_exact=bf16_exact)


def plan(spec):
    """The restated host rule for `spec`: None = the launch runs on conv_taps_kernel."""
    a = (spec["op"], spec["B"], spec["cin"], spec["cout"], spec["ext"], spec["k"], spec["step"], spec["guard"])
    if spec["math"] == "x3":
        return geo.plan_x3(*a, pitch=spec["pitch"], pre=spec["pre"], rows=spec["lengths"] is not None)
    return geo.plan_convw(*a, pitch=spec["pitch"], pre=spec["pre"], pre_slope=spec["pre_slope"])


def _rand(shape, gen, scale=1.0):
    return torch.randn(shape, generator=gen) * scale


def _lens(spec):
    return list(spec["lengths"]) if spec["lengths"] is not None else [spec["ext"]] * spec["B"]


def out_shape(spec, n=None):
    """(Cout, ...) of one row's dense output at extent n."""
    n = spec["ext"] if n is None else n
    if spec["op"] == "conv2d":
        return (spec["cout"], n, spec["pitch"] - 1)
    return (spec["cout"], n * (spec["step"] if spec["op"] == "convtr1d" else 1))


def _inputs(spec, seed):
    """CPU fp32 operands in torch's layouts: unit-variance activations and residual, weights scaled by fan-in^-1/2 and a bias of
    0.3; `heavy`: the weights times a log-normal gain per output channel, exp(1.5 z - 2.25) (trained weight-norm gains), and a
    unit-scale bias, so that some channels are all bias or all residual.  The weights and the bias come from one generator, every
    batch row from its own: row b does not depend on how many rows the batch has."""
    g = torch.Generator().manual_seed(seed)
    op, B, cin, cout, ext, k, s = spec["op"], spec["B"], spec["cin"], spec["cout"], spec["ext"], spec["k"], spec["step"]
    t = {}
    if op == "conv1d":
        xshape, t["w"] = (cin, ext), _rand((cout, cin, k), g, (cin * k) ** -0.5)
    elif op == "convtr1d":
        xshape, t["w"] = (cin, ext), _rand((cin, cout, 2 * s), g, (2 * cin) ** -0.5)
    else:
        xshape, t["w"] = (cin, ext, spec["pitch"] - 1), _rand((cout, cin, k, k), g, (cin * k * k) ** -0.5)
    if spec["heavy"]:
        gain = torch.exp(1.5 * _rand((cout,), g) - 2.25)
        t["w"] = t["w"] * gain.reshape([-1 if d == (1 if op == "convtr1d" else 0) else 1 for d in range(t["w"].dim())])
    t["w"] = t["w"] * spec["w_scale"]
    b = _rand((cout,), g, 1.0 if spec["heavy"] else 0.3)
    t["bias"] = b if spec["bias"] else None
    aff = spec["pre"] == _lib.PRE_AFFINE_LRELU
    t["scale"] = 0.8 + 0.4 * torch.rand(cin, generator=g) if aff else None
    t["shift"] = _rand((cin,), g, 0.3) if aff else None
    rows = [torch.Generator().manual_seed(seed * 4099 + 1 + b) for b in range(B)]
    t["x"] = torch.stack([_rand(xshape, rg) for rg in rows])
    t["res"] = torch.stack([_rand(out_shape(spec), rg) for rg in rows]) if spec["res"] != "none" else None
    if spec["bf16_exact"]:
        for name in ("w", "x"):
            t[name] = t[name].to(torch.bfloat16).float()
    return t


def _alloc(B, Cn, L, guard, cpad=0, wpad=0, ls=1):
    """NaN-filled allocation and the (B, Cn, up4(L)) view inside it: `guard` elements (rounded up to 4) around every row, `wpad`
    more behind it, `cpad` channels on both sides, element stride `ls`."""
    g4, Lp = geo.up4(guard), geo.up4(L)
    base = torch.full((B, Cn + 2 * cpad, (g4 + Lp + g4 + wpad) * ls), NAN, device=DEV)
    v = base[:, cpad:cpad + Cn, g4 * ls:(g4 + Lp) * ls:ls]
    return base, v


def _to_flat(spec, a, fill):
    return ref64.to_pitch(a, spec["pitch"].bit_length() - 1, fill=fill) if spec["op"] == "conv2d" else a


def launch(spec, seed=0, t=None, expect="plan"):
    """Launch `spec` once.  expect "plan": the restated host rule must take the launch, and the tile the library reports must be
    the one it names; None: it must decline it, and the launch must run on conv_taps_kernel.  Returns (device output as a dense
    fp32 CPU tensor in torch's layout, NaN past every row's own end; the operands; the plan)."""
    p = plan(spec)
    assert (p is not None) == (expect == "plan"), "the restated host rule %s this launch" % ("declines" if p is None else "takes")
    op, B, cin, cout, ext, pitch, k, s = (spec[n] for n in ("op", "B", "cin", "cout", "ext", "pitch", "k", "step"))
    t = _inputs(spec, seed) if t is None else t
    lens = _lens(spec)
    maps = op == "conv2d"
    unit = pitch if maps else 1
    omul = s if op == "convtr1d" else 1
    Lin, Lout = ext * unit, ext * unit * omul
    # ---- input: NaN in the guard bands, past every row's own end and (where one of the two kernels is to run) in the pad column
    xbase, xv = _alloc(B, cin, Lin, spec["guard"])
    xflat = _to_flat(spec, t["x"], NAN if (p is not None or spec["pre"] != _lib.PRE_NONE) else 0.0)
    for b in range(B):
        xv[b, :, :lens[b] * unit] = xflat[b, :, :lens[b] * unit].to(DEV)
    xv._vfx_guard, xv._vfx_base = spec["guard"], xbase
    ybase, yv = _alloc(B, cout, Lout, 8, ls=spec["y_ls"])
    rv = rbase = None
    if t["res"] is not None:
        rflat = _to_flat(spec, t["res"], 0.0)
        if spec["res"] == "in place":
            rv = yv
        else:
            rbase, rv = _alloc(B, cout, Lout, 8, cpad=3 if spec["r_own"] else 0, wpad=20 if spec["r_own"] else 0, ls=spec["r_ls"])
        for b in range(B):
            rv[b, :, :lens[b] * unit * omul] = rflat[b, :, :lens[b] * unit * omul].to(DEV)
    if spec["lengths"] is not None:
        ops.with_rows(xv, torch.tensor([n * unit for n in lens], dtype=torch.int32, device=DEV))
    pack = {"conv1d": packing.pack_conv1d, "convtr1d": packing.pack_convtr1d, "conv2d": packing.pack_conv2d}[op]
    wp = pack(t["w"])
    offer = dict(w3=packing.pack_x3(wp).to(DEV)) if spec["math"] == "x3" else dict(wd=packing.pack_direct(wp).to(DEV))
    bias = t["bias"].to(DEV) if t["bias"] is not None else None
    act = ops.Act(pre=spec["pre"], pre_slope=spec["pre_slope"], scale=t["scale"].to(DEV) if t["scale"] is not None else None,
                  shift=t["shift"].to(DEV) if t["shift"] is not None else None, post=spec["post"], post_slope=spec["post_slope"])
    xkeep = xbase.clone()
    rkeep = rbase.clone() if rbase is not None else None
    lib = _lib.lib()
    torch.cuda.synchronize()
    before = lib.vfx_launch_count()
    if op == "conv1d":
        ops.conv1d(xv, wp.to(DEV), bias, yv, ext, k, s, _lib.PAD_ZERO, act, rv, **offer)
    elif op == "convtr1d":
        ops.convtr1d(xv, wp.to(DEV), bias, yv, ext, s, act, **offer)
    else:
        ops.conv2d(xv, wp.to(DEV), bias, yv, ext, pitch.bit_length() - 1, k, act, rv, **offer)
    torch.cuda.synchronize()
    tile, launches = lib.vfx_last_conv_tile(), int(lib.vfx_launch_count() - before)
    if p is not None:
        assert (tile // 100000, tile // 100 % 1000, tile % 100) == (p["BM"], p["BL"], p["code"]), \
            "ran as %d, the restated host rule names %s (code %d)" % (tile, p["name"], p["code"])
        assert launches == 1
    else:
        assert tile % 100 in (4, 8), "a launch the restated host rule declines ran as %d" % tile
    # ---- canaries
    allowed = torch.zeros(ybase.shape, dtype=torch.bool, device=DEV)
    g4 = geo.up4(8)
    av = allowed[:, :, g4 * spec["y_ls"]:(g4 + geo.up4(Lout)) * spec["y_ls"]:spec["y_ls"]]
    split_k = p is None and launches > 1          # (conv_taps_kernel's split-K reduce covers the capacity)
    for b in range(B):
        hi = lens[b] * unit * omul
        if op == "convtr1d" and spec["lengths"] is not None:
            hi = min(Lout, hi + s)                # the lq_extra block of a ragged row
        av[b, :, :Lout if split_k else hi] = True
    stray = ~(torch.isnan(ybase) | allowed)
    assert not bool(stray.any()), "%d elements outside the valid output were written" % int(stray.sum())
    assert torch.equal(xbase.view(torch.int32), xkeep.view(torch.int32)), "x was written"
    if rbase is not None:
        assert torch.equal(rbase.view(torch.int32), rkeep.view(torch.int32)), "the residual was written"
    flat = yv.detach().cpu()[:, :, :Lout].contiguous()
    for b in range(B):
        n = lens[b] * unit * omul
        assert not bool(torch.isnan(flat[b, :, :n]).any()), "NaN inside row %d's valid output" % b
        flat[b, :, n:] = NAN
    if maps:
        got = ref64.from_pitch(flat, ext, pitch.bit_length() - 1)
        for b in range(B):
            assert bool((got[b, :, :lens[b], pitch - 1] == 0).all()), "output pad column is not exactly 0"
        return got[..., :pitch - 1].contiguous(), t, p
    return flat, t, p


# --------------------------------------------------------------------------------------
# the figures
# --------------------------------------------------------------------------------------
def _groups(spec):
    lens = _lens(spec)
    return [(n, [b for b in range(spec["B"]) if lens[b] == n]) for n in sorted(set(lens))]


def _op32(spec, x, w, bias):
    op, k, s = spec["op"], spec["k"], spec["step"]
    if op == "conv1d":
        return F.conv1d(x, w, bias, dilation=s, padding=(k - 1) // 2 * s)
    if op == "convtr1d":
        return F.conv_transpose1d(x, w, bias, stride=s, padding=s // 2 + s % 2, output_padding=s % 2)
    return F.conv2d(x, w, bias, padding=k // 2)


def yardstick32(spec, t):
    """The fp32 CPU yardstick, every row of a ragged batch alone: (the bare convolution, the launch's result), dense with NaN
    past a row's own end.  math "f32": torch's operator on the pre-activated input.  math "x3": torch's operator on the tripled
    problem (f64_reference.bf16x3_tripled): fp32 accumulation of the 3 K exact products the bf16x3 statement adds."""
    B = spec["B"]
    conv = torch.full((B,) + out_shape(spec), NAN)
    kw = dict(pre=spec["pre"], pre_slope=spec["pre_slope"], scale=t["scale"], shift=t["shift"])
    omul = spec["step"] if spec["op"] == "convtr1d" else 1
    for n, idx in _groups(spec):
        x = t["x"][idx][:, :, :n]
        if spec["math"] == "x3":
            x3, w3 = ref64.bf16x3_tripled(x, t["w"], cin_dim=0 if spec["op"] == "convtr1d" else 1, **kw)
            conv[idx, :, :n * omul] = _op32(spec, x3, w3, None)
        else:
            conv[idx, :, :n * omul] = _op32(spec, ref64.conv_pre32(x, spec["pre"], spec["pre_slope"], t["scale"], t["shift"]), t["w"], None)
    y = conv
    if t["bias"] is not None:
        y = y + t["bias"].reshape([1, -1] + [1] * (y.dim() - 2))
    if t["res"] is not None:
        y = y + t["res"]
    return conv, _post32(y, spec["post"], spec["post_slope"])


def subset(spec, t, conv, seed):
    """The output channels scored in float64 (module docstring), sorted; all of them while one float64 pass stays in F64_BUDGET."""
    cout = spec["cout"]
    taps = {"conv1d": spec["k"], "convtr1d": 2, "conv2d": spec["k"] ** 2}[spec["op"]]
    if float(conv[0].numel()) * spec["B"] * spec["cin"] * taps <= F64_BUDGET:
        return list(range(cout))
    sub = {c for c in range(cout) if c % 32 in (0, 31)}
    g = torch.Generator().manual_seed(seed)
    for c in torch.randperm(cout, generator=g).tolist():
        if len(sub) >= max(cout // 8, 8):
            break
        sub.add(c)
    if spec["heavy"] and t["bias"] is not None:
        rms = torch.nan_to_num(conv, nan=0.0).double().pow(2).sum(dim=[d for d in range(conv.dim()) if d != 1]).sqrt()
        sub |= set(torch.topk(t["bias"].double().abs() / rms.clamp(min=1e-300), 4).indices.tolist())
    return sorted(sub)


def statement64(spec, t, sub, magnitude, split=None, x=None):
    w = t["w"][:, sub] if spec["op"] == "convtr1d" else t["w"][sub]
    bias = t["bias"][sub] if t["bias"] is not None else None
    res = t["res"][:, sub] if t["res"] is not None else None
    kw = dict(pre=spec["pre"], pre_slope=spec["pre_slope"], scale=t["scale"], shift=t["shift"], post=spec["post"],
              post_slope=spec["post_slope"], lengths=spec["lengths"], magnitude=magnitude, split=split)
    x = t["x"] if x is None else x
    if spec["op"] == "conv1d":
        return ref64.conv1d(x, w, bias, res, dilation=spec["step"], **kw)
    if spec["op"] == "convtr1d":
        return ref64.convtr1d(x, w, bias, spec["step"], **kw)
    return ref64.conv2d(x, w, bias, res, **kw)


def score(spec, t, got, seed):
    """`got` and the fp32 yardstick, each against the float64 statement (math "x3": the bf16x3 statement) on the channel subset;
    the other channels against the yardstick.  Returns two _Acc (device, yardstick)."""
    with torch.no_grad():
        conv, yard = yardstick32(spec, t)
        sub = subset(spec, t, conv, seed)
        del conv
        split = "bf16x3" if spec["math"] == "x3" else None
        ref = statement64(spec, t, sub, False, split)
        mag = statement64(spec, t, sub, True, split)
    assert got.shape == yard.shape and ref.shape == got[:, sub].shape, (got.shape, yard.shape, ref.shape)
    lip = ref64.post_lipschitz(spec["post"])
    dev, cpu = _Acc(), _Acc()
    dev.add(ref64.conv_error(got[:, sub], ref, mag, lip))
    cpu.add(ref64.conv_error(yard[:, sub], ref, mag, lip))
    ok = ~torch.isnan(yard)
    assert torch.equal(torch.isnan(got), ~ok), "NaN pattern of the output"
    peak = float(yard[ok].abs().max())
    worst = float((got - yard)[ok].abs().max())
    assert worst <= DIRECT_TOL * peak, "fp32 operator comparison: %.3e of the peak" % (worst / peak)
    return dev, cpu


def check(name, dev, cpu):
    """Print the figures, then assert: the device at most MARGIN x the yardstick, maximum and RMS, with the floors."""
    print("PARITY %s %.3e %.3e %.2f %.3e %.3e %.2f" % (name, cpu.mx, dev.mx, dev.mx / max(cpu.mx, ULP), cpu.rms, dev.rms,
                                                      dev.rms / max(cpu.rms, RMS_FLOOR)))
    assert dev.n > 0 and dev.n == cpu.n
    assert dev.mx <= MARGIN * max(cpu.mx, ULP), "%s: max figure %.3e exceeds %.0f x the yardstick's %.3e" % (name, dev.mx, MARGIN, cpu.mx)
    assert dev.rms <= MARGIN * max(cpu.rms, RMS_FLOOR), "%s: RMS figure %.3e exceeds %.0f x the yardstick's %.3e" % (name, dev.rms, MARGIN, cpu.rms)


def run_case(spec, seed, name, expect="plan"):
    got, t, p = launch(spec, seed, expect=expect)
    dev, cpu = score(spec, t, got, seed)
    check(name, dev, cpu)
    return p


# --------------------------------------------------------------------------------------
# the product's launches
# --------------------------------------------------------------------------------------
def record_key(r):
    return (r["code"], r["BM"], r["BL"], r["op"], r["cin"], r["cout"], r.get("pitch", 0), r["k"], r["step"], r["pre"], r["post"],
            round(r["post_slope"], 6) if r["post"] in (LRELU, SNAKE) else 0.0, r["bias"], r["res"], r["rows"])


_RECS = {}


def census(pipe, mode, geometry):  # noqa: F811
    """The launch records of one seeded run: mode "f32" (default), "direct" (set_winograd(False)) or "bf16x3" (set_math)."""
    if (mode, geometry) in _RECS:
        return _RECS[(mode, geometry)]
    import bench
    from voicefixer_amd import engine
    n = 441000
    if geometry == "ragged5":
        wav = bench.synth_batch(5, n, 1002, DEV)
        fn = lambda: pipe.restore_rows(wav, RAGGED_SAMPLES)
    else:
        wav = bench.synth_batch(32 if geometry == "b32x10" else 1, n, 1000, DEV)
        fn = lambda: pipe.restore(wav, n)
    try:
        engine.set_winograd(mode != "direct")
        pipe.set_math("bf16x3" if mode == "bf16x3" else "f32")
        with launch_record.LaunchRecorder() as rec:
            fn()
            torch.cuda.synchronize()
    finally:
        engine.set_winograd(True)
        pipe.set_math("f32")
    _RECS[(mode, geometry)] = rec
    return rec


CENSUS_RUNS = sorted(COUNTS)


def census_check(pipe, mode, geometry, codes, table):  # noqa: F811
    rec = census(pipe, mode, geometry)
    mine = [r for r in rec.records if r["code"] in codes]
    keys = [record_key(r) for r in mine]
    unmatched = sorted({k for k in keys if k not in table}, key=repr)
    counts = {c: sum(1 for r in rec.records if r["code"] == c) for c in CENSUS_CODES}
    counts = {c: n for c, n in counts.items() if n}
    print("CENSUS %s %s: %d conv-family calls, %r, %d distinct keys on %r, %d unmatched" % (
        mode, geometry, len(rec.records), counts, len(set(keys)), codes, len(unmatched)))
    for k in sorted(set(keys), key=repr):
        print("CENSUS-KEY %s %s %s x%d" % (mode, geometry, case_id(k) if k[10] in POST_NAMES else repr(k), keys.count(k)))
    assert not unmatched, "launches on codes %r that are not rows of CASES:\n%s" % (codes, "\n".join(map(repr, unmatched)))
    for r in mine:
        assert r["launches"] == 1 and r["guarded"] and r["unit"] and r["pad"] == "zero", r
    assert counts == COUNTS[(mode, geometry)]
    return rec


RAGGED_FRACTIONS = (1.0, 0.1, 0.45, 0.76, 0.23, 0.6, 0.05, 0.9)   # row 0 fills the capacity, as the longest row of a batch does
_SHAPES = {}


def reduced_shape(key, math):
    """The least (B, extent) at which the restated host rule still gives the row's (code, BM, BL): odd extents, B >= 3 with row tags."""
    if (key, math) in _SHAPES:
        return _SHAPES[(key, math)]
    code, BM, BL, op, cin, cout, pitch, k, step, pre, post, ps, bias, res, rows = key
    best = None
    for B in ((3, 4, 5, 8, 16, 32) if rows else (1, 2, 3, 4, 8, 16, 32)):
        for ext in (range(1, 1025) if pitch else range(97, 60000, 131)):
            if best is not None and B * ext * max(pitch, 1) >= best[0]:
                break
            p = plan(make_spec(op, cin, cout, ext, B, k, step, pitch, pre, math=math, lengths=[ext] * B if rows else None))
            if p is not None and (p["code"], p["BM"], p["BL"]) == (code, BM, BL):
                best = (B * ext * max(pitch, 1), B, ext)
                break
    assert best is not None, "no shape selects %r" % (key,)
    _SHAPES[(key, math)] = best[1:]
    return best[1:]


def ragged_lengths(ext, B):
    return [max(1, int(round(ext * RAGGED_FRACTIONS[b % len(RAGGED_FRACTIONS)]))) for b in range(B)]


def case_spec(key, heavy, math="f32"):
    code, BM, BL, op, cin, cout, pitch, k, step, pre, post, ps, bias, res, rows = key
    B, ext = reduced_shape(key, math)
    return make_spec(op, cin, cout, ext, B, k, step, pitch, pre, 0.01, post, ps, bias, res, ragged_lengths(ext, B) if rows else None,
                     heavy=heavy, math=math)


@pytest.mark.parametrize("mode,geometry", CENSUS_RUNS, ids=["%s-%s" % r for r in CENSUS_RUNS])
def test_launch_census(pipe, mode, geometry):  # noqa: F811
    """Every launch on codes 51 / 52 / 54 / 59 of the seeded pipeline in this run is a row of CASES, and the launches per code --
    those of conv_x3_kernel (16) and of the fused direct layer (61 / 62 / 64) included -- are the pinned ones.  Under
    set_winograd(False) the sixteen C = 64 / C = 128 ResStack layers run fused (codes 61 / 62 / 64), everything else of "direct"
    on this kernel."""
    census_check(pipe, mode, geometry, (51, 52, 54, 59), set(CASES))


def test_every_case_is_a_product_launch(pipe):  # noqa: F811
    seen = {record_key(r) for run in CENSUS_RUNS for r in census(pipe, *run).records}
    missing = [case_id(k) for k in CASES if k not in seen]
    assert not missing, "rows of CASES that no census run launches: %r" % missing


@pytest.mark.parametrize("gains", ["unit", "heavy"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=[case_id(k) for k in CASES])
def test_case_parity(i, gains):
    """Every row of CASES at its reduced size, with unit gains and with heavy-tailed ones (profiles/convw_x3_parity.txt).

    Finding, fixed in the kernel; these are its regression cases.  While the unfused convw_kernel started its accumulators at the
    bias (and, on plain output maps, at the residual), every partial sum of the K loop rounded at their magnitude: 108 of the
    110 rows with heavy-tailed gains were above the bound, at 2.4 - 44.3 x the CPU operator's maximum and 2.6 - 18.5 x its RMS, and
    10 of the 110 with unit gains (up to 5.6 x).  The accumulators now start at zero and bias and residual are added to the
    finished sum, in torch's order (acc_store_rows / conv_epilogue with SUM_FIRST).  That left three 3x3 unit-gain rows at 4.1 - 4.5 x
    (k59-128x128-conv2d-512to256-P16, k59-128x128-conv2d-256to128-P32, k59-32x256-conv2d-64to32-P128-rows: K = 9 Cin terms in
    one sequential chain against a floor of 4 x 2^-23); the 3x3 instances now add their accumulators into a second set every 32
    input channels (TWO_LEVEL).  All 220 rows: 0.3 - 3.5 x / 0.3 - 1.6 x."""
    key = CASES[i]
    run_case(case_spec(key, gains == "heavy"), 11000 + 2 * i + (gains == "heavy"), case_id(key) + "-" + gains)


# --------------------------------------------------------------------------------------
# edges the product does not reach
# --------------------------------------------------------------------------------------
A = _lib.PRE_AFFINE_LRELU
L1 = dict(pre=_lib.PRE_LRELU, post=LRELU, post_slope=0.2)
# name -> spec; every second edge draws heavy-tailed gains.  What each group is for:
#  cin*            chunk depths 8 / 16 / 32 and a single trip of the K loop (Cin = 8 .. 96), on the 128 x 128 tile
#  tile64x256      the other 1-D tile
#  span8 / span10  dilation 4 stages BL columns for BL - 8 outputs, dilation 5 a halo tile; d27 a wide halo; d243 / d2187
#                  one segment per tap (2187 > L)
#  lq-*            Lq = n bl_step - 1, n bl_step, n bl_step + 1
#  tiles63/64/65   linear order, XCD order, XCD order on a rounded-up grid with idle workgroups
#  res-* / y-ls2   residual in place and separate with batch / channel strides of its own (both on the lean store path, acc_store_rows:
#                  res_init = 1); a residual of element stride 2 (res_init = 0) and an output view of element stride 2 (no plain
#                  output map), which take conv_epilogue.  (res_init = 0 through residual offsets of 2^31 or more is not reached.)
#  ragged-*        per-row lengths: a row shorter than one tile, a row that ends inside a tile's halo, a row of one sample
#  tr-s*           transposed convolutions at strides 2, 3, 7, 8 with the phases folded into the tile order (64 tiles) and not (63)
#  map-*           all four 3x3 tiles (128 x 64 below 768 workgroups), H = 1, 2, 7, ragged map rows, the affine pre-activation;
#                  *-two-level-*: the instances with a second accumulator set (from Cin = 64, on the 128 x 128 tile from 256), with
#                  two flushes and a chunk behind the last (Cin = 72), three (96), eight (264), and the last Cin below the switch
EDGES = [("cin%d" % c, make_spec("conv1d", c, 128, 6201, 8, **L1)) for c in (8, 24, 40, 64, 96)] + [
    ("tile64x256", make_spec("conv1d", 64, 64, 12301, 8, **L1)),
    ("span8-d4", make_spec("conv1d", 64, 128, 6201, 8, step=4, **L1)),
    ("span10-d5", make_spec("conv1d", 64, 128, 6201, 8, step=5, **L1)),
    ("halo-d27", make_spec("conv1d", 64, 128, 6201, 8, step=27, **L1)),
    ("segments-d243", make_spec("conv1d", 64, 128, 6201, 8, step=243, **L1)),
    ("segments-d2187-beyond-L", make_spec("conv1d", 64, 128, 1601, 32, step=2187, **L1)),
    ("lq-48x126-1", make_spec("conv1d", 32, 128, 48 * 126 - 1, 8, **L1)),
    ("lq-48x126", make_spec("conv1d", 32, 128, 48 * 126, 8, **L1)),
    ("lq-48x126+1", make_spec("conv1d", 32, 128, 48 * 126 + 1, 8, **L1)),
    ("tiles63", make_spec("conv1d", 32, 128, 63 * 126, 7, **L1)),
    ("tiles64", make_spec("conv1d", 32, 128, 64 * 126, 7, **L1)),
    ("tiles65", make_spec("conv1d", 32, 128, 64 * 126 + 1, 7, **L1)),
    ("res-inplace", make_spec("conv1d", 64, 128, 6201, 8, res="in place")),
    ("res-inplace-snake", make_spec("conv1d", 64, 128, 6201, 8, res="in place", post=SNAKE, post_slope=0.2)),
    ("res-own-strides", make_spec("conv1d", 64, 128, 6201, 8, res="separate", r_own=True, post=ELU)),
    ("y-ls2-res-separate", make_spec("conv1d", 64, 128, 6201, 8, res="separate", y_ls=2, post=LRELU, post_slope=0.01)),
    ("y-ls2", make_spec("conv1d", 64, 64, 12301, 8, y_ls=2, **L1)),
    ("res-ls2", make_spec("conv1d", 64, 128, 6201, 8, res="separate", r_ls=2, post=LRELU, post_slope=0.2)),
    ("res-ls2-own-strides-64x256", make_spec("conv1d", 32, 64, 12301, 8, res="separate", r_own=True, r_ls=2)),
    ("map-res-ls2", make_spec("conv2d", 16, 64, 7, 96, pitch=64, bias=False, res="separate", r_ls=2)),
    ("ragged-short-rows", make_spec("conv1d", 64, 128, 6201, 8, lengths=[6201, 50, 3 * 126 + 1, 1, 126, 4000, 127, 6200], res="in place")),
    ("ragged-d27-row-ends-in-halo", make_spec("conv1d", 64, 128, 6201, 8, step=27, lengths=[6201, 128 + 13, 20, 256, 6000, 1, 129, 3000], **L1)),
    ("ragged-64x256", make_spec("conv1d", 64, 64, 12301, 8, lengths=[12301, 200, 254, 255, 1, 9000, 508, 12300], **L1)),
] + [("tr-s%d-folded" % s, make_spec("convtr1d", 64, 128, 64 * 127 - 1, 3, 2 * s, s)) for s in (2, 3, 7, 8)] + [
    ("tr-s%d-unfolded" % s, make_spec("convtr1d", 64, 128, 63 * 127 - 1, 4, 2 * s, s)) for s in (2, 3, 7, 8)] + [
    ("tr-s3-64x256-ragged", make_spec("convtr1d", 32, 64, 40 * 255 - 1, 4, 6, 3, lengths=[40 * 255 - 1, 17, 255, 5000])),
    ("map-128x128-H16", make_spec("conv2d", 8, 128, 16, 96, pitch=64, pre=A, post=LRELU, post_slope=0.01)),
    ("map-128x64-H7", make_spec("conv2d", 8, 128, 7, 55, pitch=64, pre=A, post=LRELU, post_slope=0.01)),
    ("map-128x64-H1", make_spec("conv2d", 8, 128, 1, 192, pitch=128, bias=False, res="in place")),
    ("map-128x64-H2", make_spec("conv2d", 8, 128, 2, 96, pitch=128, bias=False, res="separate", r_own=True)),
    ("map-64x128-H7", make_spec("conv2d", 64, 64, 7, 96, pitch=64, pre=A, post=LRELU, post_slope=0.01)),
    ("map-32x256-H7", make_spec("conv2d", 8, 32, 7, 96, pitch=128, pre=A, post=LRELU, post_slope=0.01)),
    ("map-32x256-ragged", make_spec("conv2d", 8, 32, 7, 96, pitch=128, pre=A, post=LRELU, post_slope=0.01,
                                    lengths=[7, 1, 2, 6, 3, 5, 4, 7] * 12)),
    ("map-128x64-ragged-resinplace", make_spec("conv2d", 16, 128, 7, 56, pitch=64, bias=False, res="in place", lengths=[7, 1, 2, 6, 3, 5, 4] * 8)),
    ("map-32x256-two-level-cin72", make_spec("conv2d", 72, 32, 7, 96, pitch=128, pre=A, post=LRELU, post_slope=0.01)),
    ("map-128x64-two-level-cin96", make_spec("conv2d", 96, 128, 7, 55, pitch=64, bias=False, res="in place")),
    ("map-128x128-two-level-cin264", make_spec("conv2d", 264, 128, 16, 96, pitch=64, pre=A, post=LRELU, post_slope=0.01)),
    ("map-128x128-one-level-cin248", make_spec("conv2d", 248, 128, 16, 96, pitch=64, pre=A, post=LRELU, post_slope=0.01)),
]
EDGE_IDS = [e[0] for e in EDGES]


@pytest.mark.parametrize("i", range(len(EDGES)), ids=EDGE_IDS)
def test_edge_parity(i):
    name, spec = EDGES[i]
    p = run_case(dict(spec, heavy=i % 2 == 1), 12000 + i, name)
    print("EDGE %s ran as %s, %d tiles, chunk depth %d, nph_fold %d" % (name, p["name"], p["ntiles"], p["kcx"], p["nph_fold"]))


def test_edges_reach_what_they_are_named_for():
    """The restated host rule on the edge table: chunk depths, staging modes, tile orders and folds are the ones the names say."""
    pl = {name: plan(spec) for name, spec in EDGES}
    assert [pl["cin%d" % c]["kcx"] for c in (8, 24, 40, 64, 96)] == [8, 8, 8, 32, 32]
    assert {pl["cin%d" % c]["code"] for c in (8, 24, 40, 64, 96)} == {51, 54}
    assert pl["halo-d27"]["code"] == 54 and pl["halo-d27"]["staging"] == "halo"
    assert (pl["span8-d4"]["staging"], pl["span10-d5"]["staging"], pl["segments-d243"]["staging"]) == ("shrink", "halo", "segments")
    assert pl["segments-d2187-beyond-L"]["nseg"] == 3
    assert [pl[n]["ntiles"] for n in ("lq-48x126-1", "lq-48x126", "lq-48x126+1")] == [48, 48, 49]
    assert [(pl[n]["ntiles"], pl[n]["xcd_chunk"], pl[n]["grid"][0]) for n in ("tiles63", "tiles64", "tiles65")] == [(63, 0, 63), (64, 8, 64), (65, 9, 72)]
    for s in (2, 3, 7, 8):
        assert pl["tr-s%d-folded" % s]["nph_fold"] == s and pl["tr-s%d-unfolded" % s]["nph_fold"] == 0
    assert {(pl[n]["BM"], pl[n]["BL"]) for n in pl if n.startswith("map-")} == {(128, 128), (128, 64), (64, 128), (32, 256)}
    assert pl["tile64x256"]["BL"] == 256 and pl["y-ls2"]["BL"] == 256
    assert {n for n in pl if pl[n].get("two_level")} == {"map-64x128-H7", "map-32x256-two-level-cin72", "map-128x64-two-level-cin96",
                                                         "map-128x128-two-level-cin264"}


# name -> a launch the kernel must NOT take: it runs on conv_taps_kernel, and is held to the same bound
DECLINED = [
    ("wg383", make_spec("conv1d", 32, 128, 383 * 126, 1, **L1)),
    ("guard-one-short", make_spec("conv1d", 64, 128, 8192, 8, step=27, guard=63 * 128 - 27 + geo.up4(128 + 54) - 8192 - 1, **L1)),
    ("pre-slope-1.5", make_spec("conv1d", 64, 128, 6201, 8, pre=_lib.PRE_LRELU, pre_slope=1.5)),
    ("pre-slope-negative", make_spec("conv1d", 64, 128, 6201, 8, pre=_lib.PRE_LRELU, pre_slope=-0.25)),
    ("cout96", make_spec("conv1d", 64, 96, 6201, 8, **L1)),
    ("map-8-workgroups", make_spec("conv2d", 8, 128, 8, 1, pitch=64, pre=A)),
]


@pytest.mark.parametrize("i", range(len(DECLINED)), ids=[d[0] for d in DECLINED])
def test_declined(i):
    """What convw_kernel declines runs on conv_taps_kernel with the same operands: 383 workgroups (384 is the `wg384` edge
    below), a guard one short of interior, pre-activation slopes outside [0, 1] (the kernel evaluates leaky ReLU as max(v, s v)),
    a Cout that is no multiple of 64."""
    name, spec = DECLINED[i]
    run_case(dict(spec, heavy=i % 2 == 1), 12500 + i, "declined-" + name, expect=None)


def test_wg384_is_taken():
    run_case(make_spec("conv1d", 32, 128, 384 * 126, 1, heavy=True, **L1), 12600, "wg384")


# --------------------------------------------------------------------------------------
# exact properties
# --------------------------------------------------------------------------------------
EXACT = [("k3-128x128", make_spec("conv1d", 64, 128, 6201, 8, res="in place", post=LRELU, post_slope=0.2)),
         ("k3-d9-64x256", make_spec("conv1d", 32, 64, 12301, 8, step=9, **L1)),
         ("k3-y-ls2-res", make_spec("conv1d", 32, 128, 6201, 8, res="separate", y_ls=2)),
         ("tr-s3", make_spec("convtr1d", 32, 128, 64 * 127 - 1, 4, 6, 3)),
         ("map-64x128", make_spec("conv2d", 16, 64, 7, 96, pitch=64, bias=True, res="in place", post=LRELU, post_slope=0.01))]
EXACT_IDS = [e[0] for e in EXACT]


def _post_f32(v, spec):
    return torch.where(v > 0, v, v * torch.tensor(spec["post_slope"], dtype=torch.float32)) if spec["post"] == LRELU else v


@pytest.mark.parametrize("e", EXACT, ids=EXACT_IDS)
def test_zero_weights_return_bias_plus_residual(e):
    """With zero weights every output is post(bias + residual) bit for bit: both are added to the finished sum, once, in torch's
    order (an accumulator started at the bias gives the same bits here; one that adds them in the other order does not)."""
    spec = dict(e[1], w_scale=0.0, heavy=True)
    got, t, _ = launch(spec, 13000)
    want = t["bias"].reshape([1, -1] + [1] * (got.dim() - 2)).expand_as(got)
    if t["res"] is not None:
        want = want + t["res"]
    assert torch.equal(got, _post_f32(want, spec))


@pytest.mark.parametrize("e", EXACT, ids=EXACT_IDS)
def test_batch_items_are_independent(e):
    """The same row at batch index 0 and 3 of a launch, with different neighbours, is bit-equal."""
    spec = dict(e[1], heavy=True)
    t = _inputs(spec, 13100)
    t["x"][3] = t["x"][0]
    if t["res"] is not None:
        t["res"][3] = t["res"][0]
    got, _, _ = launch(spec, 0, t=t)
    assert torch.equal(got[0], got[3]) and not torch.equal(got[0], got[1])


@pytest.mark.parametrize("name", ["ragged-short-rows", "ragged-d27-row-ends-in-halo", "ragged-64x256"])
def test_ragged_rows_equal_the_rows_alone(name):
    """Row b of a ragged launch is bit-equal to that row launched alone at its own length (as many copies of it as the 384-workgroup
    floor asks for): every output is one chain over the input channels and taps in the same order wherever its tile lies."""
    spec = dict(dict(EDGES)[name], heavy=True)
    got, t, _ = launch(spec, 13200)
    for b, n in enumerate(spec["lengths"]):
        if b == 0:
            continue
        copies = 1
        while plan(dict(spec, B=copies, ext=n, lengths=None)) is None:
            copies *= 2
        rep = lambda a: None if a is None else a[b:b + 1, :, :n].expand(copies, -1, -1).contiguous()
        alone, _, _ = launch(dict(spec, B=copies, ext=n, lengths=None), 0, t=dict(t, x=rep(t["x"]), res=rep(t["res"])))
        assert torch.equal(alone, alone[:1].expand_as(alone)), "copies of one row differ"
        assert torch.equal(got[b, :, :n], alone[0]), "row %d of length %d" % (b, n)


@pytest.mark.parametrize("s", [2, 3, 7, 8])
def test_folded_and_unfolded_phase_order_give_the_same_bits(s):
    """The same rows as 64 tiles (phases folded into the tile order) and, cut by one tile, as 63 (phase in blockIdx.y): the
    outputs both launches own -- those that do not see the cut -- are bit-equal."""
    long = make_spec("convtr1d", 64, 128, 64 * 127 - 1, 4, 2 * s, s, heavy=True)
    got, t, p = launch(long, 13300 + s)
    n = 63 * 127 - 1
    cut, _, q = launch(dict(long, ext=n), 0, t=dict(t, x=t["x"][:, :, :n].contiguous()))
    assert p["nph_fold"] == s and q["nph_fold"] == 0
    keep = s * (n - 1) - s
    assert torch.equal(got[:, :, :keep], cut[:, :, :keep])
