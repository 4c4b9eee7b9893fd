"""conv_taps_kernel (the first-generation implicit-GEMM kernel, vfx_last_conv_tile() codes 4 / 8) at every launch shape the
product uses, against float64.

* ``test_launch_census`` runs the seeded pipeline at five geometries under voicefixer_amd.launch_record and asserts that every
  launch that lands on conv_taps_kernel is a row of ``CASES`` -- tile, K-chunk depth and split-K included -- so a dispatch
  change that moves a product launch onto an untested configuration fails here.
* ``test_case_parity`` launches every row of ``CASES`` once at its product size, on buffers built as the engine builds them
  (guard bands, pad columns of pre-activated maps and the whole output buffer hold NaN), asserts the configuration the row
  names, that nothing outside the valid output was written, and every output against oracle/f64_reference.py.
* ``test_edge_parity`` does the same for the index arithmetic the product does not reach (``EDGES``): every split-K count,
  tile edges of all six tiles, short guards, transposed shapes, reflect padding at its minimum, channel tails.

The error figure is |got - ref| / (lip * magnitude + |ref|) per output (magnitude = sum |x~| |w| + |bias| + |res|, lip the
Lipschitz constant of the post-activation).  Its bound is measured on the reference side: torch's fp32 CPU operator on the
same inputs is scored against the same float64 statement, and the device may be at most 4 x worse, maximum and RMS: the
device adds the same products in another order (K-chunks of 4 or 8 channels, up to eight split-K partials), which moves a
rounding error by a small factor, not by its order.  Where the CPU operator happens to be (nearly) exact the bound has a
floor: 4 x 2^-23 for the maximum (a few fp32 ulps), and for the RMS 4 x 2^-24 / sqrt(3) / 2 -- the correctly rounded fp32
value of an exact sum is off by a uniform +-2^-24 |ref|, RMS 2^-24 / sqrt(3), and |ref| is at most half of magnitude + |ref|.  Every case prints ``PARITY <id> <cpu max> <dev max> <ratio> <cpu rms> <dev rms> <ratio>`` before it asserts;
profiles/conv_taps_parity.txt is that output.

A row of CASES / EDGES expects (BM, BL, K-chunk, grids, split-K): ``grids`` is the number of conv_taps_kernel grids (1 when
every tile takes the same instance -- guarded zero-padded inputs: interior; channel tails, ragged reflect padding: general --
2 when interior and boundary tiles both exist), and the vfx_launch_count() delta must be grids + split-K
(splitk_reduce_kernel is the extra launch).

Where a row's own end lies before the capacity of the launch (ragged batches), outputs past it are unspecified by
include/vfx_hip.h.  The non-split kernel writes nothing there and the tests hold it to that (NaN stays); a split-K launch
reduces the whole capacity, so for those only the positions past the capacity, the guard bands and the other channels are
canaries.  A ragged transposed 1-D launch may write the `stride` positions that follow a row's end (its lq_extra block)."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from voicefixer_amd import ops, packing, _lib, launch_record  # noqa: E402
from oracle import f64_reference as ref64  # noqa: E402

DEV = "cuda"
NAN = float("nan")
ULP = 2.0 ** -23
RMS_FLOOR = 2.0 ** -24 / math.sqrt(3.0) / 2.0
MARGIN = 4.0

# op, B, Cin, Cout, L (1-D) or H (maps: rows of the INPUT map), pitch of the input map (0: 1-D), k, dilation / stride, padding,
# pre-activation, post-activation, residual, row tags on the input, unit-stride output  ->  BM, BL, K-chunk, grids, split-K
# (every distinct conv_taps_kernel launch of the five census geometries, in launch order; test_launch_census keeps it complete)
CASES = [
    # batch 32 x 10 s (the headline)
    (('conv1d', 32, 128, 256, 1001, 0, 1, 1, 'zero', 0, 1, 'none', False, True), (128, 128, 8, 1, 0)),
    (('conv1d', 32, 256, 512, 1001, 0, 1, 1, 'zero', 0, 1, 'none', False, True), (128, 128, 8, 1, 0)),
    (('conv1d', 32, 512, 1536, 1001, 0, 1, 1, 'zero', 0, 0, 'none', False, False), (128, 128, 8, 1, 0)),
    (('conv1d', 32, 512, 512, 1001, 0, 1, 1, 'zero', 2, 1, 'none', False, True), (128, 128, 8, 1, 0)),
    (('conv1d', 32, 512, 128, 1001, 0, 1, 1, 'zero', 0, 4, 'none', False, True), (128, 64, 8, 1, 0)),
    (('conv2d', 32, 8, 32, 1024, 128, 1, 1, 'zero', 0, 0, 'none', False, True), (32, 256, 8, 1, 0)),
    (('conv2d', 32, 32, 64, 512, 64, 1, 1, 'zero', 0, 0, 'none', False, True), (64, 256, 8, 1, 0)),
    (('conv2d', 32, 64, 128, 256, 32, 1, 1, 'zero', 0, 0, 'none', False, True), (128, 128, 8, 1, 0)),
    (('conv2d', 32, 128, 256, 128, 16, 1, 1, 'zero', 0, 0, 'none', False, True), (128, 128, 8, 1, 0)),
    (('conv2d', 32, 256, 384, 64, 8, 1, 1, 'zero', 0, 0, 'none', False, True), (128, 128, 8, 1, 0)),
    (('conv2d', 32, 384, 384, 32, 4, 3, 1, 'zero', 2, 1, 'none', False, True), (64, 64, 4, 1, 0)),
    (('conv2d', 32, 384, 384, 32, 4, 3, 1, 'zero', 0, 0, 'separate', False, True), (64, 64, 4, 1, 0)),
    (('conv2d', 32, 384, 384, 32, 4, 3, 1, 'zero', 0, 0, 'in place', False, True), (64, 64, 4, 1, 0)),
    (('conv2d', 32, 384, 384, 16, 2, 3, 1, 'zero', 2, 1, 'none', False, True), (64, 64, 4, 1, 1)),
    (('conv2d', 32, 384, 384, 16, 2, 3, 1, 'zero', 0, 0, 'in place', False, True), (64, 64, 4, 1, 1)),
    (('convtr2d_3x3s2', 32, 384, 384, 16, 2, 3, 2, 'zero', 2, 0, 'none', False, True), (128, 64, 8, 1, 0)),
    (('conv2d', 32, 768, 384, 32, 4, 1, 1, 'zero', 0, 0, 'none', False, True), (64, 64, 8, 1, 0)),
    (('conv2d', 32, 768, 384, 32, 4, 3, 1, 'zero', 2, 1, 'none', False, True), (64, 64, 4, 1, 0)),
    (('convtr2d_3x3s2', 32, 384, 384, 32, 4, 3, 2, 'zero', 2, 0, 'none', False, True), (128, 128, 8, 1, 0)),
    (('conv2d', 32, 768, 384, 64, 8, 1, 1, 'zero', 0, 0, 'none', False, True), (128, 128, 8, 1, 0)),
    (('convtr2d_3x3s2', 32, 384, 256, 64, 8, 3, 2, 'zero', 2, 0, 'none', False, True), (128, 128, 8, 1, 0)),
    (('conv2d', 32, 512, 256, 128, 16, 1, 1, 'zero', 0, 0, 'none', False, True), (128, 128, 8, 1, 0)),
    (('convtr2d_3x3s2', 32, 256, 128, 128, 16, 3, 2, 'zero', 2, 0, 'none', False, True), (128, 128, 8, 1, 0)),
    (('conv2d', 32, 256, 128, 256, 32, 1, 1, 'zero', 0, 0, 'none', False, True), (128, 128, 8, 1, 0)),
    (('convtr2d_3x3s2', 32, 128, 64, 256, 32, 3, 2, 'zero', 2, 0, 'none', False, True), (64, 256, 8, 1, 0)),
    (('conv2d', 32, 128, 64, 512, 64, 1, 1, 'zero', 0, 0, 'none', False, True), (64, 256, 8, 1, 0)),
    (('convtr2d_3x3s2', 32, 64, 32, 512, 64, 3, 2, 'zero', 2, 0, 'none', False, True), (32, 256, 8, 1, 0)),
    (('conv2d', 32, 64, 32, 1024, 128, 1, 1, 'zero', 0, 0, 'none', False, True), (32, 256, 8, 1, 0)),
    (('conv1d', 32, 512, 1024, 1006, 0, 7, 1, 'reflect', 0, 5, 'none', False, True), (128, 128, 4, 2, 0)),
    # batch 1 x 10 s
    (('conv1d', 1, 128, 256, 1001, 0, 1, 1, 'zero', 0, 1, 'none', False, True), (64, 64, 8, 1, 0)),
    (('conv1d', 1, 256, 512, 1001, 0, 1, 1, 'zero', 0, 1, 'none', False, True), (64, 64, 8, 1, 1)),
    (('conv1d', 1, 512, 1536, 1001, 0, 1, 1, 'zero', 0, 0, 'none', False, False), (64, 64, 8, 1, 0)),
    (('conv1d', 1, 512, 512, 1001, 0, 1, 1, 'zero', 2, 1, 'none', False, True), (64, 64, 8, 1, 1)),
    (('conv1d', 1, 512, 128, 1001, 0, 1, 1, 'zero', 0, 4, 'none', False, True), (64, 64, 8, 1, 1)),
    (('conv2d', 1, 8, 32, 1024, 128, 1, 1, 'zero', 0, 0, 'none', False, True), (32, 256, 8, 1, 0)),
    (('conv2d', 1, 32, 64, 512, 64, 1, 1, 'zero', 0, 0, 'none', False, True), (64, 64, 8, 1, 0)),
    (('conv2d', 1, 32, 64, 512, 64, 3, 1, 'zero', 2, 1, 'none', False, True), (64, 64, 4, 1, 0)),
    (('conv2d', 1, 64, 64, 512, 64, 3, 1, 'zero', 0, 0, 'in place', False, True), (64, 64, 4, 1, 0)),
    (('conv2d', 1, 64, 64, 512, 64, 3, 1, 'zero', 2, 1, 'none', False, True), (64, 64, 4, 1, 0)),
    (('conv2d', 1, 64, 64, 512, 64, 3, 1, 'zero', 0, 0, 'separate', False, True), (64, 64, 4, 1, 0)),
    (('conv2d', 1, 64, 128, 256, 32, 1, 1, 'zero', 0, 0, 'none', False, True), (64, 64, 8, 1, 0)),
    (('conv2d', 1, 64, 128, 256, 32, 3, 1, 'zero', 2, 1, 'none', False, True), (64, 64, 4, 1, 0)),
    (('conv2d', 1, 128, 128, 256, 32, 3, 1, 'zero', 0, 0, 'in place', False, True), (64, 64, 4, 1, 0)),
    (('conv2d', 1, 128, 128, 256, 32, 3, 1, 'zero', 2, 1, 'none', False, True), (64, 64, 4, 1, 0)),
    (('conv2d', 1, 128, 128, 256, 32, 3, 1, 'zero', 0, 0, 'separate', False, True), (64, 64, 4, 1, 0)),
    (('conv2d', 1, 128, 256, 128, 16, 1, 1, 'zero', 0, 0, 'none', False, True), (64, 64, 8, 1, 0)),
    (('conv2d', 1, 128, 256, 128, 16, 3, 1, 'zero', 2, 1, 'none', False, True), (64, 64, 4, 1, 1)),
    (('conv2d', 1, 256, 256, 128, 16, 3, 1, 'zero', 0, 0, 'in place', False, True), (64, 64, 4, 1, 1)),
    (('conv2d', 1, 256, 256, 128, 16, 3, 1, 'zero', 2, 1, 'none', False, True), (64, 64, 4, 1, 1)),
    (('conv2d', 1, 256, 256, 128, 16, 3, 1, 'zero', 0, 0, 'separate', False, True), (64, 64, 4, 1, 1)),
    (('conv2d', 1, 256, 384, 64, 8, 1, 1, 'zero', 0, 0, 'none', False, True), (64, 64, 8, 1, 1)),
    (('conv2d', 1, 256, 384, 64, 8, 3, 1, 'zero', 2, 1, 'none', False, True), (64, 64, 4, 1, 1)),
    (('conv2d', 1, 384, 384, 64, 8, 3, 1, 'zero', 0, 0, 'in place', False, True), (64, 64, 4, 1, 1)),
    (('conv2d', 1, 384, 384, 64, 8, 3, 1, 'zero', 2, 1, 'none', False, True), (64, 64, 4, 1, 1)),
    (('conv2d', 1, 384, 384, 64, 8, 3, 1, 'zero', 0, 0, 'separate', False, True), (64, 64, 4, 1, 1)),
    (('conv2d', 1, 384, 384, 32, 4, 3, 1, 'zero', 2, 1, 'none', False, True), (64, 64, 4, 1, 1)),
    (('conv2d', 1, 384, 384, 32, 4, 3, 1, 'zero', 0, 0, 'separate', False, True), (64, 64, 4, 1, 1)),
    (('conv2d', 1, 384, 384, 32, 4, 3, 1, 'zero', 0, 0, 'in place', False, True), (64, 64, 4, 1, 1)),
    (('conv2d', 1, 384, 384, 16, 2, 3, 1, 'zero', 2, 1, 'none', False, True), (64, 64, 4, 1, 1)),
    (('conv2d', 1, 384, 384, 16, 2, 3, 1, 'zero', 0, 0, 'in place', False, True), (64, 64, 4, 1, 1)),
    (('convtr2d_3x3s2', 1, 384, 384, 16, 2, 3, 2, 'zero', 2, 0, 'none', False, True), (64, 64, 8, 1, 0)),
    (('conv2d', 1, 768, 384, 32, 4, 1, 1, 'zero', 0, 0, 'none', False, True), (64, 64, 8, 1, 1)),
    (('conv2d', 1, 768, 384, 32, 4, 3, 1, 'zero', 2, 1, 'none', False, True), (64, 64, 4, 1, 1)),
    (('convtr2d_3x3s2', 1, 384, 384, 32, 4, 3, 2, 'zero', 2, 0, 'none', False, True), (64, 64, 8, 1, 0)),
    (('conv2d', 1, 768, 384, 64, 8, 1, 1, 'zero', 0, 0, 'none', False, True), (64, 64, 8, 1, 1)),
    (('conv2d', 1, 768, 384, 64, 8, 3, 1, 'zero', 2, 1, 'none', False, True), (64, 64, 4, 1, 1)),
    (('convtr2d_3x3s2', 1, 384, 256, 64, 8, 3, 2, 'zero', 2, 0, 'none', False, True), (64, 64, 8, 1, 0)),
    (('conv2d', 1, 512, 256, 128, 16, 1, 1, 'zero', 0, 0, 'none', False, True), (64, 64, 8, 1, 1)),
    (('conv2d', 1, 512, 256, 128, 16, 3, 1, 'zero', 2, 1, 'none', False, True), (64, 64, 4, 1, 1)),
    (('convtr2d_3x3s2', 1, 256, 128, 128, 16, 3, 2, 'zero', 2, 0, 'none', False, True), (64, 64, 8, 1, 0)),
    (('conv2d', 1, 256, 128, 256, 32, 1, 1, 'zero', 0, 0, 'none', False, True), (64, 64, 8, 1, 0)),
    (('conv2d', 1, 256, 128, 256, 32, 3, 1, 'zero', 2, 1, 'none', False, True), (64, 64, 4, 1, 0)),
    (('convtr2d_3x3s2', 1, 128, 64, 256, 32, 3, 2, 'zero', 2, 0, 'none', False, True), (64, 64, 8, 1, 0)),
    (('conv2d', 1, 128, 64, 512, 64, 1, 1, 'zero', 0, 0, 'none', False, True), (64, 64, 8, 1, 0)),
    (('conv2d', 1, 128, 64, 512, 64, 3, 1, 'zero', 2, 1, 'none', False, True), (64, 64, 4, 1, 0)),
    (('convtr2d_3x3s2', 1, 64, 32, 512, 64, 3, 2, 'zero', 2, 0, 'none', False, True), (32, 256, 8, 1, 0)),
    (('conv2d', 1, 64, 32, 1024, 128, 1, 1, 'zero', 0, 0, 'none', False, True), (32, 256, 8, 1, 0)),
    (('conv1d', 1, 128, 512, 1006, 0, 3, 1, 'zero', 0, 2, 'none', False, True), (64, 64, 8, 1, 0)),
    (('conv1d', 1, 512, 512, 1006, 0, 3, 1, 'zero', 0, 2, 'none', False, True), (64, 64, 8, 1, 1)),
    (('conv1d', 1, 512, 1024, 1006, 0, 7, 1, 'reflect', 0, 5, 'none', False, True), (64, 64, 8, 2, 0)),
    (('convtr1d', 1, 1024, 512, 1006, 0, 14, 7, 'zero', 0, 0, 'none', False, True), (128, 64, 8, 1, 0)),
    (('conv1d', 1, 512, 512, 7042, 0, 3, 1, 'zero', 1, 1, 'none', False, True), (128, 64, 8, 1, 0)),
    (('conv1d', 1, 512, 512, 7042, 0, 3, 1, 'zero', 0, 0, 'in place', False, True), (128, 64, 8, 1, 0)),
    (('conv1d', 1, 512, 512, 7042, 0, 3, 3, 'zero', 1, 1, 'none', False, True), (128, 64, 8, 1, 0)),
    (('conv1d', 1, 512, 512, 7042, 0, 3, 9, 'zero', 1, 1, 'none', False, True), (128, 64, 8, 1, 0)),
    (('conv1d', 1, 512, 512, 7042, 0, 3, 27, 'zero', 1, 1, 'none', False, True), (128, 64, 8, 1, 0)),
    (('conv1d', 1, 512, 512, 7042, 0, 3, 81, 'zero', 1, 1, 'none', False, True), (128, 64, 8, 1, 0)),
    (('conv1d', 1, 512, 512, 7042, 0, 3, 243, 'zero', 1, 1, 'none', False, True), (128, 64, 8, 1, 0)),
    (('conv1d', 1, 512, 512, 7042, 0, 3, 729, 'zero', 1, 1, 'none', False, True), (128, 64, 8, 1, 0)),
    (('conv1d', 1, 512, 512, 7042, 0, 3, 2187, 'zero', 1, 1, 'none', False, True), (128, 64, 8, 1, 0)),
    (('conv1d', 1, 512, 512, 7042, 0, 3, 1, 'zero', 0, 5, 'in place', False, True), (128, 64, 8, 1, 0)),
    # batch 8 x 30 s
    (('conv1d', 8, 128, 256, 3001, 0, 1, 1, 'zero', 0, 1, 'none', False, True), (128, 128, 8, 1, 0)),
    (('conv1d', 8, 256, 512, 3001, 0, 1, 1, 'zero', 0, 1, 'none', False, True), (128, 64, 8, 1, 0)),
    (('conv1d', 8, 512, 1536, 3001, 0, 1, 1, 'zero', 0, 0, 'none', False, False), (128, 128, 8, 1, 0)),
    (('conv1d', 8, 512, 512, 3001, 0, 1, 1, 'zero', 2, 1, 'none', False, True), (128, 64, 8, 1, 0)),
    (('conv1d', 8, 512, 128, 3001, 0, 1, 1, 'zero', 0, 4, 'none', False, True), (128, 64, 8, 1, 0)),
    (('conv2d', 8, 8, 32, 3008, 128, 1, 1, 'zero', 0, 0, 'none', False, True), (32, 256, 8, 1, 0)),
    (('conv2d', 8, 32, 64, 1504, 64, 1, 1, 'zero', 0, 0, 'none', False, True), (64, 256, 8, 1, 0)),
    (('conv2d', 8, 64, 128, 752, 32, 1, 1, 'zero', 0, 0, 'none', False, True), (128, 128, 8, 1, 0)),
    (('conv2d', 8, 128, 256, 376, 16, 1, 1, 'zero', 0, 0, 'none', False, True), (128, 64, 8, 1, 0)),
    (('conv2d', 8, 256, 384, 188, 8, 1, 1, 'zero', 0, 0, 'none', False, True), (128, 128, 8, 1, 0)),
    (('conv2d', 8, 384, 384, 94, 4, 3, 1, 'zero', 2, 1, 'none', False, True), (64, 64, 4, 1, 0)),
    (('conv2d', 8, 384, 384, 94, 4, 3, 1, 'zero', 0, 0, 'separate', False, True), (64, 64, 4, 1, 0)),
    (('conv2d', 8, 384, 384, 94, 4, 3, 1, 'zero', 0, 0, 'in place', False, True), (64, 64, 4, 1, 0)),
    (('conv2d', 8, 384, 384, 47, 2, 3, 1, 'zero', 2, 1, 'none', False, True), (64, 64, 4, 1, 1)),
    (('conv2d', 8, 384, 384, 47, 2, 3, 1, 'zero', 0, 0, 'in place', False, True), (64, 64, 4, 1, 1)),
    (('convtr2d_3x3s2', 8, 384, 384, 47, 2, 3, 2, 'zero', 2, 0, 'none', False, True), (64, 64, 8, 1, 0)),
    (('conv2d', 8, 768, 384, 94, 4, 1, 1, 'zero', 0, 0, 'none', False, True), (64, 64, 8, 1, 0)),
    (('conv2d', 8, 768, 384, 94, 4, 3, 1, 'zero', 2, 1, 'none', False, True), (64, 64, 4, 1, 0)),
    (('convtr2d_3x3s2', 8, 384, 384, 94, 4, 3, 2, 'zero', 2, 0, 'none', False, True), (128, 128, 8, 1, 0)),
    (('conv2d', 8, 768, 384, 188, 8, 1, 1, 'zero', 0, 0, 'none', False, True), (128, 128, 8, 1, 0)),
    (('convtr2d_3x3s2', 8, 384, 256, 188, 8, 3, 2, 'zero', 2, 0, 'none', False, True), (128, 64, 8, 1, 0)),
    (('conv2d', 8, 512, 256, 376, 16, 1, 1, 'zero', 0, 0, 'none', False, True), (128, 64, 8, 1, 0)),
    (('convtr2d_3x3s2', 8, 256, 128, 376, 16, 3, 2, 'zero', 2, 0, 'none', False, True), (128, 128, 8, 1, 0)),
    (('conv2d', 8, 256, 128, 752, 32, 1, 1, 'zero', 0, 0, 'none', False, True), (128, 128, 8, 1, 0)),
    (('convtr2d_3x3s2', 8, 128, 64, 752, 32, 3, 2, 'zero', 2, 0, 'none', False, True), (64, 256, 8, 1, 0)),
    (('conv2d', 8, 128, 64, 1504, 64, 1, 1, 'zero', 0, 0, 'none', False, True), (64, 256, 8, 1, 0)),
    (('convtr2d_3x3s2', 8, 64, 32, 1504, 64, 3, 2, 'zero', 2, 0, 'none', False, True), (32, 256, 8, 1, 0)),
    (('conv2d', 8, 64, 32, 3008, 128, 1, 1, 'zero', 0, 0, 'none', False, True), (32, 256, 8, 1, 0)),
    (('conv1d', 8, 512, 1024, 3006, 0, 7, 1, 'reflect', 0, 5, 'none', False, True), (128, 128, 4, 2, 0)),
    # ragged mode-0 batch of five rows (10, 1, 4.5, 7.6, 2.3 s)
    (('conv1d', 5, 128, 256, 1001, 0, 1, 1, 'zero', 0, 1, 'none', False, True), (64, 64, 8, 1, 0)),
    (('conv1d', 5, 256, 512, 1001, 0, 1, 1, 'zero', 0, 1, 'none', False, True), (128, 64, 8, 1, 0)),
    (('conv1d', 5, 512, 1536, 1001, 0, 1, 1, 'zero', 0, 0, 'none', False, False), (128, 128, 8, 1, 0)),
    (('conv1d', 5, 512, 512, 1001, 0, 1, 1, 'zero', 2, 1, 'none', False, True), (128, 64, 8, 1, 0)),
    (('conv1d', 5, 512, 128, 1001, 0, 1, 1, 'zero', 0, 4, 'none', False, True), (64, 64, 8, 1, 1)),
    (('conv2d', 5, 8, 32, 1024, 128, 1, 1, 'zero', 0, 0, 'none', True, True), (32, 256, 8, 1, 0)),
    (('conv2d', 5, 32, 64, 512, 64, 1, 1, 'zero', 0, 0, 'none', True, True), (32, 256, 8, 1, 0)),
    (('conv2d', 5, 64, 128, 256, 32, 1, 1, 'zero', 0, 0, 'none', True, True), (128, 128, 8, 1, 0)),
    (('conv2d', 5, 128, 256, 128, 16, 1, 1, 'zero', 0, 0, 'none', True, True), (128, 64, 8, 1, 0)),
    (('conv2d', 5, 128, 256, 128, 16, 3, 1, 'zero', 2, 1, 'none', True, True), (128, 64, 4, 1, 0)),
    (('conv2d', 5, 256, 256, 128, 16, 3, 1, 'zero', 0, 0, 'in place', True, True), (128, 64, 4, 1, 0)),
    (('conv2d', 5, 256, 256, 128, 16, 3, 1, 'zero', 2, 1, 'none', True, True), (128, 64, 4, 1, 0)),
    (('conv2d', 5, 256, 256, 128, 16, 3, 1, 'zero', 0, 0, 'separate', True, True), (128, 64, 4, 1, 0)),
    (('conv2d', 5, 256, 384, 64, 8, 1, 1, 'zero', 0, 0, 'none', True, True), (64, 64, 8, 1, 0)),
    (('conv2d', 5, 256, 384, 64, 8, 3, 1, 'zero', 2, 1, 'none', True, True), (64, 64, 4, 1, 0)),
    (('conv2d', 5, 384, 384, 64, 8, 3, 1, 'zero', 0, 0, 'in place', True, True), (64, 64, 4, 1, 0)),
    (('conv2d', 5, 384, 384, 64, 8, 3, 1, 'zero', 2, 1, 'none', True, True), (64, 64, 4, 1, 0)),
    (('conv2d', 5, 384, 384, 64, 8, 3, 1, 'zero', 0, 0, 'separate', True, True), (64, 64, 4, 1, 0)),
    (('conv2d', 5, 384, 384, 32, 4, 3, 1, 'zero', 2, 1, 'none', True, True), (64, 64, 4, 1, 1)),
    (('conv2d', 5, 384, 384, 32, 4, 3, 1, 'zero', 0, 0, 'separate', True, True), (64, 64, 4, 1, 1)),
    (('conv2d', 5, 384, 384, 32, 4, 3, 1, 'zero', 0, 0, 'in place', True, True), (64, 64, 4, 1, 1)),
    (('conv2d', 5, 384, 384, 16, 2, 3, 1, 'zero', 2, 1, 'none', True, True), (64, 64, 4, 1, 1)),
    (('conv2d', 5, 384, 384, 16, 2, 3, 1, 'zero', 0, 0, 'in place', True, True), (64, 64, 4, 1, 1)),
    (('convtr2d_3x3s2', 5, 384, 384, 16, 2, 3, 2, 'zero', 2, 0, 'none', True, True), (64, 64, 8, 1, 0)),
    (('conv2d', 5, 768, 384, 32, 4, 1, 1, 'zero', 0, 0, 'none', True, True), (64, 64, 8, 1, 1)),
    (('conv2d', 5, 768, 384, 32, 4, 3, 1, 'zero', 2, 1, 'none', True, True), (64, 64, 4, 1, 1)),
    (('convtr2d_3x3s2', 5, 384, 384, 32, 4, 3, 2, 'zero', 2, 0, 'none', True, True), (64, 64, 8, 1, 0)),
    (('conv2d', 5, 768, 384, 64, 8, 1, 1, 'zero', 0, 0, 'none', True, True), (64, 64, 8, 1, 0)),
    (('conv2d', 5, 768, 384, 64, 8, 3, 1, 'zero', 2, 1, 'none', True, True), (64, 64, 4, 1, 0)),
    (('convtr2d_3x3s2', 5, 384, 256, 64, 8, 3, 2, 'zero', 2, 0, 'none', True, True), (128, 64, 8, 1, 0)),
    (('conv2d', 5, 512, 256, 128, 16, 1, 1, 'zero', 0, 0, 'none', True, True), (128, 64, 8, 1, 0)),
    (('conv2d', 5, 512, 256, 128, 16, 3, 1, 'zero', 2, 1, 'none', True, True), (128, 64, 4, 1, 0)),
    (('convtr2d_3x3s2', 5, 256, 128, 128, 16, 3, 2, 'zero', 2, 0, 'none', True, True), (128, 128, 8, 1, 0)),
    (('conv2d', 5, 256, 128, 256, 32, 1, 1, 'zero', 0, 0, 'none', True, True), (128, 128, 8, 1, 0)),
    (('convtr2d_3x3s2', 5, 128, 64, 256, 32, 3, 2, 'zero', 2, 0, 'none', True, True), (32, 256, 8, 1, 0)),
    (('conv2d', 5, 128, 64, 512, 64, 1, 1, 'zero', 0, 0, 'none', True, True), (32, 256, 8, 1, 0)),
    (('convtr2d_3x3s2', 5, 64, 32, 512, 64, 3, 2, 'zero', 2, 0, 'none', True, True), (32, 256, 8, 1, 0)),
    (('conv2d', 5, 64, 32, 1024, 128, 1, 1, 'zero', 0, 0, 'none', True, True), (32, 256, 8, 1, 0)),
    (('conv1d', 5, 128, 512, 1006, 0, 3, 1, 'zero', 0, 2, 'none', True, True), (128, 64, 8, 1, 0)),
    (('conv1d', 5, 512, 512, 1006, 0, 3, 1, 'zero', 0, 2, 'none', True, True), (128, 64, 8, 1, 0)),
    (('conv1d', 5, 512, 1024, 1006, 0, 7, 1, 'reflect', 0, 5, 'none', True, True), (128, 128, 4, 1, 0)),
    # mode 2 (train-mode BatchNorm), batch 4 x 10 s
    (('conv1d', 4, 128, 256, 1001, 0, 1, 1, 'zero', 0, 1, 'none', False, True), (64, 64, 8, 1, 0)),
    (('conv1d', 4, 256, 512, 1001, 0, 1, 1, 'zero', 0, 0, 'none', False, True), (64, 64, 8, 1, 0)),
    (('conv1d', 4, 512, 1536, 1001, 0, 1, 1, 'zero', 0, 0, 'none', False, False), (128, 128, 8, 1, 0)),
    (('conv1d', 4, 512, 512, 1001, 0, 1, 1, 'zero', 0, 0, 'none', False, True), (64, 64, 8, 1, 0)),
    (('conv1d', 4, 512, 128, 1001, 0, 1, 1, 'zero', 0, 4, 'none', False, True), (64, 64, 8, 1, 1)),
    (('conv2d', 4, 8, 32, 1024, 128, 1, 1, 'zero', 0, 0, 'none', False, True), (32, 256, 8, 1, 0)),
    (('conv2d', 4, 32, 64, 512, 64, 1, 1, 'zero', 0, 0, 'none', False, True), (64, 256, 8, 1, 0)),
    (('conv2d', 4, 64, 128, 256, 32, 1, 1, 'zero', 0, 0, 'none', False, True), (128, 64, 8, 1, 0)),
    (('conv2d', 4, 128, 256, 128, 16, 1, 1, 'zero', 0, 0, 'none', False, True), (64, 64, 8, 1, 0)),
    (('conv2d', 4, 128, 256, 128, 16, 3, 1, 'zero', 0, 0, 'none', False, True), (64, 64, 4, 1, 0)),
    (('conv2d', 4, 256, 256, 128, 16, 3, 1, 'zero', 0, 0, 'in place', False, True), (64, 64, 4, 1, 0)),
    (('conv2d', 4, 256, 256, 128, 16, 3, 1, 'zero', 0, 0, 'none', False, True), (64, 64, 4, 1, 0)),
    (('conv2d', 4, 256, 256, 128, 16, 3, 1, 'zero', 0, 0, 'separate', False, True), (64, 64, 4, 1, 0)),
    (('conv2d', 4, 256, 384, 64, 8, 1, 1, 'zero', 0, 0, 'none', False, True), (64, 64, 8, 1, 1)),
    (('conv2d', 4, 256, 384, 64, 8, 3, 1, 'zero', 0, 0, 'none', False, True), (64, 64, 4, 1, 1)),
    (('conv2d', 4, 384, 384, 64, 8, 3, 1, 'zero', 0, 0, 'in place', False, True), (64, 64, 4, 1, 1)),
    (('conv2d', 4, 384, 384, 64, 8, 3, 1, 'zero', 0, 0, 'none', False, True), (64, 64, 4, 1, 1)),
    (('conv2d', 4, 384, 384, 64, 8, 3, 1, 'zero', 0, 0, 'separate', False, True), (64, 64, 4, 1, 1)),
    (('conv2d', 4, 384, 384, 32, 4, 3, 1, 'zero', 0, 0, 'none', False, True), (64, 64, 4, 1, 1)),
    (('conv2d', 4, 384, 384, 32, 4, 3, 1, 'zero', 0, 0, 'separate', False, True), (64, 64, 4, 1, 1)),
    (('conv2d', 4, 384, 384, 32, 4, 3, 1, 'zero', 0, 0, 'in place', False, True), (64, 64, 4, 1, 1)),
    (('conv2d', 4, 384, 384, 16, 2, 3, 1, 'zero', 0, 0, 'none', False, True), (64, 64, 4, 1, 1)),
    (('conv2d', 4, 384, 384, 16, 2, 3, 1, 'zero', 0, 0, 'in place', False, True), (64, 64, 4, 1, 1)),
    (('convtr2d_3x3s2', 4, 384, 384, 16, 2, 3, 2, 'zero', 0, 0, 'none', False, True), (64, 64, 8, 1, 0)),
    (('conv2d', 4, 768, 384, 32, 4, 1, 1, 'zero', 0, 0, 'none', False, True), (64, 64, 8, 1, 1)),
    (('conv2d', 4, 768, 384, 32, 4, 3, 1, 'zero', 0, 0, 'none', False, True), (64, 64, 4, 1, 1)),
    (('convtr2d_3x3s2', 4, 384, 384, 32, 4, 3, 2, 'zero', 0, 0, 'none', False, True), (64, 64, 8, 1, 0)),
    (('conv2d', 4, 768, 384, 64, 8, 1, 1, 'zero', 0, 0, 'none', False, True), (64, 64, 8, 1, 1)),
    (('conv2d', 4, 768, 384, 64, 8, 3, 1, 'zero', 0, 0, 'none', False, True), (64, 64, 4, 1, 1)),
    (('convtr2d_3x3s2', 4, 384, 256, 64, 8, 3, 2, 'zero', 0, 0, 'none', False, True), (64, 64, 8, 1, 0)),
    (('conv2d', 4, 512, 256, 128, 16, 1, 1, 'zero', 0, 0, 'none', False, True), (64, 64, 8, 1, 0)),
    (('conv2d', 4, 512, 256, 128, 16, 3, 1, 'zero', 0, 0, 'none', False, True), (64, 64, 4, 1, 0)),
    (('convtr2d_3x3s2', 4, 256, 128, 128, 16, 3, 2, 'zero', 0, 0, 'none', False, True), (128, 64, 8, 1, 0)),
    (('conv2d', 4, 256, 128, 256, 32, 1, 1, 'zero', 0, 0, 'none', False, True), (128, 64, 8, 1, 0)),
    (('convtr2d_3x3s2', 4, 128, 64, 256, 32, 3, 2, 'zero', 0, 0, 'none', False, True), (64, 256, 8, 1, 0)),
    (('conv2d', 4, 128, 64, 512, 64, 1, 1, 'zero', 0, 0, 'none', False, True), (64, 256, 8, 1, 0)),
    (('convtr2d_3x3s2', 4, 64, 32, 512, 64, 3, 2, 'zero', 0, 0, 'none', False, True), (32, 256, 8, 1, 0)),
    (('conv2d', 4, 64, 32, 1024, 128, 1, 1, 'zero', 0, 0, 'none', False, True), (32, 256, 8, 1, 0)),
    (('conv1d', 4, 128, 512, 1006, 0, 3, 1, 'zero', 0, 2, 'none', False, True), (64, 64, 8, 1, 0)),
    (('conv1d', 4, 512, 512, 1006, 0, 3, 1, 'zero', 0, 2, 'none', False, True), (64, 64, 8, 1, 0)),
    (('conv1d', 4, 512, 1024, 1006, 0, 7, 1, 'reflect', 0, 5, 'none', False, True), (128, 64, 4, 2, 0)),
]


# --------------------------------------------------------------------------------------
# one launch: inputs as the engine lays them out, canaries, float64 comparison
# --------------------------------------------------------------------------------------
RAGGED_FRACTIONS = (1.0, 0.1, 0.45, 0.76, 0.23, 0.6, 0.05, 0.9)   # row 0 fills the capacity, as the longest row of a batch does


def spec_of(key):
    op, B, cin, cout, ext, pitch, k, step, pad, pre, post, res, rows, unit = key
    return dict(op=op, B=B, cin=cin, cout=cout, ext=ext, pitch=pitch, k=k, step=step, pad=pad, pre=pre, post=post, res=res,
                rows=rows, unit=unit)


def case_id(key):
    op, B, cin, cout, ext, pitch, k, step, pad, pre, post, res, rows, unit = key
    s = "%s-B%d-%dto%d-%s%d" % (op, B, cin, cout, "H" if pitch else "L", ext)
    if pitch:
        s += "-P%d" % pitch
    s += "-k%d" % k + ("-%s%d" % ("s" if op.startswith("convtr") else "d", step) if step != 1 else "")
    s += ("-reflect" if pad == "reflect" else "") + "-pre%d-post%d" % (pre, post)
    s += {"none": "", "separate": "-res", "in place": "-resinplace"}[res] + ("-rows" if rows else "") + ("" if unit else "-framemajor")
    return s


def _rand(shape, gen, scale=1.0):
    return torch.randn(shape, generator=gen) * scale


def _up4(n):
    return (n + 3) // 4 * 4


def _row_lengths(spec):
    """Per-row extents (samples, or rows of the input map) of a ragged launch; None for a plain batch."""
    if spec.get("lengths") is not None:
        return list(spec["lengths"])
    if not spec["rows"]:
        return None
    lo = 8 if spec["pad"] == "reflect" else 1
    return [max(lo, int(round(spec["ext"] * RAGGED_FRACTIONS[b % len(RAGGED_FRACTIONS)]))) for b in range(spec["B"])]


def _inputs(spec, seed):
    """CPU fp32 operands in torch's own layouts: unit-variance activations, weights scaled by fan-in^-1/2 (`heavy`:
    times a log-normal gain per output channel, exp(1.5 z - 2.25), as trained weight-norm gains are), a bias of 0.3
    and a unit-variance residual.  Weights come from one generator, every batch row from its own: row b of a launch
    does not depend on how many rows the batch has."""
    g = torch.Generator().manual_seed(seed)
    op, B, cin, cout, ext, k, s = spec["op"], spec["B"], spec["cin"], spec["cout"], spec["ext"], spec["k"], spec["step"]
    W = spec["pitch"] - 1
    t = {}
    if op == "conv1d":
        xshape, t["w"], oshape = (cin, ext), _rand((cout, cin, k), g, (cin * k) ** -0.5), (cout, ext)
    elif op == "convtr1d":
        xshape, t["w"], oshape = (cin, ext), _rand((cin, cout, 2 * s), g, (2 * cin) ** -0.5), (cout, s * ext)
    elif op == "conv2d":
        xshape, t["w"], oshape = (cin, ext, W), _rand((cout, cin, k, k), g, (cin * k * k) ** -0.5), (cout, ext, W)
    else:
        xshape, t["w"], oshape = (cin, ext, W), _rand((cin, cout, 3, 3), g, (2.25 * cin) ** -0.5), (cout, 2 * ext, 2 * W + 1)
    if spec.get("heavy"):
        gain = torch.exp(1.5 * _rand((cout,), g) - 2.25)
        t["w"] = t["w"] * gain.reshape([-1 if d == (1 if op.startswith("convtr") else 0) else 1 for d in range(t["w"].dim())])
    nobias = op == "convtr2d_3x3s2" or (op == "conv2d" and k == 3 and spec["res"] != "none") or spec.get("bias") is False
    t["bias"] = None if nobias else _rand((cout,), g, 0.3)
    t["scale"] = 0.8 + 0.4 * torch.rand(cin, generator=g) if spec["pre"] == _lib.PRE_AFFINE_LRELU else None
    t["shift"] = _rand((cin,), g, 0.3) if spec["pre"] == _lib.PRE_AFFINE_LRELU else None
    rows = [torch.Generator().manual_seed(seed * 4099 + 1 + b) for b in range(B)]
    t["x"] = torch.stack([_rand(xshape, rg) for rg in rows])
    t["res"] = torch.stack([_rand(oshape, rg) for rg in rows]) if spec["res"] != "none" else None
    return t


def _slopes(spec):
    pre_slope = 0.0 if spec["op"] == "convtr2d_3x3s2" else 0.01
    post_slope = 0.01 if spec["op"] == "conv2d" else 0.2
    return pre_slope, post_slope


def _pre32(x, pre, slope, scale, shift):
    if pre == _lib.PRE_AFFINE_LRELU:
        shp = [1, -1] + [1] * (x.dim() - 2)
        x = x * scale.reshape(shp) + shift.reshape(shp)
    return F.leaky_relu(x, slope) if pre != _lib.PRE_NONE else x


def _post32(y, post, slope):
    if post == _lib.POST_LRELU:
        return F.leaky_relu(y, slope)
    if post == _lib.POST_ELU:
        return F.elu(y)
    if post == _lib.POST_TANH:
        return torch.tanh(y)
    if post == _lib.POST_SIGMOID:
        return torch.sigmoid(y)
    if post == _lib.POST_LRELU_SNAKE:
        u = F.leaky_relu(y, slope)
        return u + torch.sin(u)
    return y


def _cpu32(spec, t, x, res):
    """torch's fp32 CPU operator on rows `x` (all of one length)."""
    pre_slope, post_slope = _slopes(spec)
    op, k, s = spec["op"], spec["k"], spec["step"]
    xa = _pre32(x, spec["pre"], pre_slope, t["scale"], t["shift"])
    if op == "conv1d":
        p = (k - 1) // 2 * s
        y = F.conv1d(F.pad(xa, (p, p), mode="reflect") if spec["pad"] == "reflect" else F.pad(xa, (p, p)), t["w"], t["bias"], dilation=s)
    elif op == "convtr1d":
        y = F.conv_transpose1d(xa, t["w"], t["bias"], stride=s, padding=s // 2 + s % 2, output_padding=s % 2)
    elif op == "conv2d":
        y = F.conv2d(xa, t["w"], t["bias"], padding=k // 2)
    else:
        y = F.conv_transpose2d(xa, t["w"], stride=2)[:, :, :-1]
    if res is not None:
        y = y + res
    return _post32(y, spec["post"], post_slope)


def _ref64(spec, t, x, res, magnitude):
    pre_slope, post_slope = _slopes(spec)
    kw = dict(pre=spec["pre"], pre_slope=pre_slope, scale=t["scale"], shift=t["shift"], post=spec["post"], post_slope=post_slope,
              magnitude=magnitude)
    op = spec["op"]
    if op == "conv1d":
        return ref64.conv1d(x, t["w"], t["bias"], res, dilation=spec["step"], reflect=spec["pad"] == "reflect", **kw)
    if op == "convtr1d":
        return ref64.convtr1d(x, t["w"], t["bias"], spec["step"], **kw)
    if op == "conv2d":
        return ref64.conv2d(x, t["w"], t["bias"], res, **kw)
    return ref64.convtr2d_3x3s2(x, t["w"], **kw)


class _Acc:
    def __init__(self):
        self.mx, self.ss, self.n = 0.0, 0.0, 0

    def add(self, fig):
        self.mx, self.ss, self.n = max(self.mx, fig[0]), self.ss + fig[1], self.n + fig[2]

    @property
    def rms(self):
        return math.sqrt(self.ss / max(self.n, 1))


def _score(spec, t, got, lengths):
    """Device output `got` (dense fp32 CPU tensor, torch layout, full capacity) and torch's fp32 CPU operator, each against
    the float64 statement: two _Acc of |. - ref| / (lip * magnitude + |ref|).  Plain batches go in chunks of rows (one
    vectorised pass per chunk), ragged ones row by row, each row alone at its own length."""
    dev, cpu = _Acc(), _Acc()
    lip = ref64.post_lipschitz(spec["post"])
    B = spec["B"]
    omul = spec["step"] if spec["op"].startswith("convtr") else 1
    if lengths is None:
        per_row = got[0].numel()
        nb = max(1, (1 << 24) // per_row)
        chunks = [(b0, min(B, b0 + nb), None) for b0 in range(0, B, nb)]
    else:
        chunks = [(b, b + 1, n) for b, n in enumerate(lengths)]
    with torch.no_grad():
        for b0, b1, n in chunks:
            x = t["x"][b0:b1] if n is None else t["x"][b0:b1, :, :n]
            res = None if t["res"] is None else (t["res"][b0:b1] if n is None else t["res"][b0:b1, :, :n * omul])
            g = got[b0:b1] if n is None else got[b0:b1, :, :n * omul]
            ref = _ref64(spec, t, x, res, False)
            mag = _ref64(spec, t, x, res, True)
            assert ref.shape == g.shape, (ref.shape, g.shape)
            dev.add(ref64.conv_error(g, ref, mag, lip))
            cpu.add(ref64.conv_error(_cpu32(spec, t, x, res), ref, mag, lip))
    return dev, cpu


def _alloc(B, Cn, L, guard):
    """NaN-filled allocation with `guard` elements (rounded up to 4) around every row of L (rounded up to 4) elements;
    returns (base, view (B, Cn, Lp))."""
    g4, Lp = _up4(guard), _up4(L)
    base = torch.full((B, Cn, g4 + Lp + g4), NAN, device=DEV)
    return base, base[:, :, g4:g4 + Lp]


def engine_guard(spec):
    """The guard band the engine gives an input of this launch: largest tap offset + 264 (engine.G_TILE)."""
    if spec["pitch"]:
        return spec["pitch"] + 1 + 264
    return (spec["k"] - 1) // 2 * spec["step"] + 264 if spec["op"] == "conv1d" else 264


def launch_case(spec, expect, seed=0):
    """Launch `spec` once and hold it to `expect` = (BM, BL, K-chunk, grids, split-K) and the canaries.  Optional spec
    entries: guard (elements; default engine_guard), alloc_guard, lengths (explicit ragged row extents), heavy, bias (False:
    none), out_guard (guard band of the output buffer, default 8).  Returns (device output as a dense fp32 CPU tensor in
    torch's layout, the operands, the row extents)."""
    op, B, cin, cout, ext, pitch = spec["op"], spec["B"], spec["cin"], spec["cout"], spec["ext"], spec["pitch"]
    k, s = spec["k"], spec["step"]
    t = _inputs(spec, seed)
    lengths = _row_lengths(spec)
    pre_slope, post_slope = _slopes(spec)
    maps = pitch > 0
    lp = pitch.bit_length() - 1
    # ---- input: guarded, NaN in the guard bands, past every row's own end, and in the pad column when a pre-activation
    # runs over it (the kernel masks it after the activation); a map without pre-activation carries its structural zero
    Lin = ext * pitch if maps else ext
    guard = spec.get("guard", engine_guard(spec))
    xbase, xv = _alloc(B, cin, Lin, spec.get("alloc_guard", guard))     # alloc_guard: more slack than the launch is told of
    xflat = ref64.to_pitch(t["x"], lp, fill=NAN if spec["pre"] != _lib.PRE_NONE else 0.0) if maps else t["x"]
    unit_in = pitch if maps else 1
    for b in range(B):
        n = (lengths[b] if lengths is not None else ext) * unit_in
        xv[b, :, :n] = xflat[b, :, :n].to(DEV)
    xv._vfx_guard = guard
    xv._vfx_base = xbase
    if lengths is not None:
        ops.with_rows(xv, torch.tensor([n * unit_in for n in lengths], dtype=torch.int32, device=DEV))
    # ---- output: NaN everywhere; transposed 2-D into the first Cout channels of a concat buffer of 2 Cout channels
    opitch = 2 * pitch if op == "convtr2d_3x3s2" else pitch
    omul = s if op.startswith("convtr") else 1
    Lout = (omul * ext * opitch) if maps else omul * ext
    ctot = 2 * cout if op == "convtr2d_3x3s2" else cout
    if spec["unit"]:
        ybase, yfull = _alloc(B, ctot, Lout, spec.get("out_guard", 8))
        view = lambda base: base[:, :cout, _up4(spec.get("out_guard", 8)):_up4(spec.get("out_guard", 8)) + _up4(Lout)]
    else:   # the GRU projection's frame-major view: (B, T, Cout) memory, seen as (B, Cout, T)
        ybase = torch.full((B, Lout + 2, cout), NAN, device=DEV)
        view = lambda base: base[:, :Lout].transpose(1, 2)
    yv = view(ybase)
    out_ext = [(n if lengths is not None else ext) * omul * (opitch if maps else 1) for n in (lengths or [ext] * B)]
    rflat = None
    if t["res"] is not None:
        rflat = ref64.to_pitch(t["res"], lp, fill=0.0) if maps else t["res"]
        if spec["res"] == "in place":
            rv = yv
        else:
            rbase, rv = _alloc(B, cout, Lout, 8)
        for b in range(B):
            rv[b, :, :out_ext[b]] = rflat[b, :, :out_ext[b]].to(DEV)
    else:
        rv = None
    # ---- weights, activation
    pack = {"conv1d": packing.pack_conv1d, "convtr1d": packing.pack_convtr1d, "conv2d": packing.pack_conv2d,
            "convtr2d_3x3s2": packing.pack_convtr2d}[op]
    wp = pack(t["w"]).to(DEV)
    bias = t["bias"].to(DEV) if t["bias"] is not None else None
    act = ops.Act(pre=spec["pre"], pre_slope=pre_slope, scale=t["scale"].to(DEV) if t["scale"] is not None else None,
                  shift=t["shift"].to(DEV) if t["shift"] is not None else None, post=spec["post"], post_slope=post_slope)
    lib = _lib.lib()
    torch.cuda.synchronize()
    before = lib.vfx_launch_count()
    if op == "conv1d":
        ops.conv1d(xv, wp, bias, yv, ext, k, s, _lib.PAD_REFLECT if spec["pad"] == "reflect" else _lib.PAD_ZERO, act, rv,
                   cin=spec.get("cin_kw"))
    elif op == "convtr1d":
        ops.convtr1d(xv, wp, bias, yv, ext, s, act)
    elif op == "conv2d":
        ops.conv2d(xv, wp, bias, yv, ext, lp, k, act, rv, cin=cin)
    else:
        ops.convtr2d_3x3s2(xv, wp, yv, ext, lp, act)
    torch.cuda.synchronize()
    launches = int(lib.vfx_launch_count() - before)
    tile = lib.vfx_last_conv_tile()
    got_cfg = (tile // 100000, tile // 100 % 1000, tile % 100, launches)
    BM, BL, KC, grids, split = expect
    assert got_cfg == (BM, BL, KC, grids + split), "ran as (BM, BL, code, launches) = %r, the table says %r" % (got_cfg, expect)
    # ---- canaries: everything outside the valid outputs is still NaN
    allowed = torch.zeros(ybase.shape, dtype=torch.bool, device=DEV)
    av = view(allowed)
    for b in range(B):
        hi = out_ext[b]
        if split:                                   # the reduce covers the capacity (header: unspecified past a row's end)
            hi = Lout
        elif op == "convtr1d" and lengths is not None:
            hi = min(Lout, hi + s)                  # the lq_extra block of a ragged row
        av[b, :, :hi] = True
    stray = ~(torch.isnan(ybase) | allowed)
    assert not bool(stray.any()), "%d elements outside the valid output were written" % int(stray.sum())
    got_flat = yv.detach().cpu()
    if maps:
        got = ref64.from_pitch(got_flat, omul * ext, opitch.bit_length() - 1)
        for b in range(B):
            rows_b = out_ext[b] // opitch
            assert bool((got[b, :, :rows_b, opitch - 1] == 0).all()), "output pad column is not exactly 0"
        got = got[..., :opitch - 1]
    else:
        got = got_flat[:, :, :Lout]
    return got.contiguous(), t, lengths


def run_case(spec, expect, seed=0, name=""):
    """launch_case, then every valid output against the float64 statement, bounded by the fp32 CPU operator's own figure.
    Returns the device output."""
    got, t, lengths = launch_case(spec, expect, seed)
    dev, cpu = _score(spec, t, got, lengths)
    bound_mx, bound_rms = MARGIN * max(cpu.mx, ULP), MARGIN * max(cpu.rms, RMS_FLOOR)
    print("PARITY %s %.3e %.3e %.2f %.3e %.3e %.2f" % (name, cpu.mx, dev.mx, dev.mx / max(cpu.mx, ULP), cpu.rms, dev.rms,
                                                      dev.rms / max(cpu.rms, RMS_FLOOR)))
    assert dev.n > 0 and dev.mx <= bound_mx, "max error figure %.3e exceeds %.0f x the fp32 CPU operator's %.3e" % (dev.mx, MARGIN, cpu.mx)
    assert dev.rms <= bound_rms, "RMS error figure %.3e exceeds %.0f x the fp32 CPU operator's %.3e" % (dev.rms, MARGIN, cpu.rms)
    return got


# --------------------------------------------------------------------------------------
# the product's launches
# --------------------------------------------------------------------------------------
GEOMETRIES = ("b32x10", "b1x10", "b8x30", "ragged5", "train4x10")
RAGGED_SAMPLES = [441000, 44100, 200000, 333333, 100001]


@pytest.fixture(scope="module")
def pipe(seeded_states):
    from voicefixer_amd import engine
    return engine.Pipeline(seeded_states[0], seeded_states[1], DEV)


def _census(pipe, geometry):
    import bench
    n = 441000
    if geometry == "b32x10":
        wav = bench.synth_batch(32, n, 1000, DEV)
        fn = lambda: pipe.restore(wav, n)
    elif geometry == "b1x10":
        wav = bench.synth_batch(1, n, 1000, DEV)
        fn = lambda: pipe.restore(wav, n)
    elif geometry == "b8x30":
        wav = bench.synth_batch(8, 3 * n, 1001, DEV)
        fn = lambda: pipe.restore(wav, 3 * n)
    elif geometry == "ragged5":
        wav = bench.synth_batch(5, n, 1002, DEV)
        fn = lambda: pipe.restore_rows(wav, RAGGED_SAMPLES)
    else:
        wav = bench.synth_batch(4, n, 1003, DEV)
        fn = lambda: pipe.restore_train(wav, [n] * 4, [0, 1, 2, 3], 7)
    with launch_record.LaunchRecorder() as rec:
        fn()
        torch.cuda.synchronize()
    return rec


def record_key(r):
    return (r["op"], r["B"], r["cin"], r["cout"], r["L"] if "L" in r else r["H"], r.get("pitch", 0), r["k"], r["step"], r["pad"],
            r["pre"], r["post"], r["res"], r["rows"], r["unit"])


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_launch_census(pipe, geometry):
    """Every conv_taps_kernel launch of the seeded pipeline at this geometry is a row of CASES with the tile, K-chunk depth
    and launch count the row names; the census sees the launch kinds the product is known to put on this kernel."""
    table = dict(CASES)
    rec = _census(pipe, geometry)
    taps = rec.taps()
    unmatched = []
    for r in taps:
        assert r["guarded"], "the engine hands conv_taps_kernel an unguarded input: %r" % (r,)
        want = table.get(record_key(r))
        ran = (r["BM"], r["BL"], r["code"], r["launches"])
        if want is None or ran != (want[0], want[1], want[2], want[3] + want[4]):
            unmatched.append((record_key(r), ran, want))
    print("CENSUS %s: %d conv-family calls, %d on conv_taps_kernel, %d unmatched" % (geometry, len(rec.records), len(taps), len(unmatched)))
    assert not unmatched, "conv_taps_kernel launches that are not rows of CASES (key, ran as, table says):\n%s" % "\n".join(map(repr, unmatched))
    split = [r for r in taps if table[record_key(r)][4]]
    if geometry == "b32x10":
        kinds = {"k = 1 Linear": lambda r: r["op"] == "conv1d" and r["k"] == 1 and r["unit"],
                 "k = 1 with a frame-major output": lambda r: r["op"] == "conv1d" and r["k"] == 1 and not r["unit"],
                 "k = 7 reflect": lambda r: r["op"] == "conv1d" and r["k"] == 7 and r["pad"] == "reflect",
                 "1x1 on a map": lambda r: r["op"] == "conv2d" and r["k"] == 1,
                 "3x3 on a map": lambda r: r["op"] == "conv2d" and r["k"] == 3,
                 "transposed 2-D": lambda r: r["op"] == "convtr2d_3x3s2"}
        for kind, pred in kinds.items():
            assert any(pred(r) for r in taps), "no %s launch on conv_taps_kernel at batch 32" % kind
        assert len(taps) >= 40
    if geometry == "b1x10":
        assert len(split) >= 1, "no split-K launch at batch 1"
    if geometry == "ragged5":
        assert any(r["rows"] for r in taps)
    if geometry == "train4x10":
        assert any(r["op"] == "conv2d" and r["k"] == 3 and r["pre"] == _lib.PRE_NONE for r in taps)


def _heavy(i):
    return i % 4 == 0       # every fourth row of the table draws log-normal gains (each operator has several)


@pytest.mark.parametrize("i", range(len(CASES)), ids=[case_id(k) for k, _ in CASES])
def test_case_parity(i):
    """Every row of CASES at its product size (measured figures: profiles/conv_taps_parity.txt).

    Two findings of this test are fixed in the kernel and stay here as its regression cases.  The rows with a bias or
    residual and heavy-tailed gains (every fourth row) were 4 - 37 x the CPU operator's error while the accumulators
    started at bias + residual.  The 3x3 rows with K = 9 Cin = 2304 ... 6912 in one unsplit pass
    (conv2d-B32-768to384-H32-P4-k3-pre2-post1, conv2d-B5-256to256-H128-P16-k3-pre2-post1-rows,
    conv2d-B5-512to256-H128-P16-k3-pre2-post1-rows) had a device maximum of 4.8e-07 - 5.3e-07 against the floor of
    4.768e-07 while that sum was one sequential fp32 chain; it is now a two-level sum (partial sums of 64 channels)."""
    key, expect = CASES[i]
    spec = spec_of(key)
    spec["heavy"] = _heavy(i)
    run_case(spec, expect, seed=1000 + i, name=case_id(key))


def test_cases_are_distinct_and_cover_every_operator_with_heavy_tailed_weights():
    assert len(dict(CASES)) == len(CASES)
    for op in ("conv1d", "convtr1d", "conv2d", "convtr2d_3x3s2"):
        assert any(_heavy(i) and k[0] == op for i, (k, _) in enumerate(CASES)), op


# --------------------------------------------------------------------------------------
# edges the product does not reach
# --------------------------------------------------------------------------------------
# name, key (as CASES), extra spec entries, expected (BM, BL, K-chunk, grids, split-K).  What each group is for:
#  splitk-count<n>   one workgroup, Cin = 128 n: want = min(512 / nwg, 8, nchunks / 16) = n, every count from 2 to 8;
#  splitk-uneven     50 chunks in 3 splits of 17, 17, 16; channel tails (Cin = 262: 33 chunks, the last of 6 channels, general
#                    instance); bias + residual (in place / separate) + post-activation, which all move into
#                    splitk_reduce_kernel; pitch maps (out_mask in the reduce); ragged rows; the same launch at the batch
#                    sizes around nwg = 192 (B = 16: 192 workgroups, split; B = 17: 204, not split);
#  tile<BM>x<BL>     Lq = n BL - 1, n BL, n BL + 1 on each of the six tiles, k = 1 (all interior) and k = 3 d = 9 without
#                    a guard (boundary tiles on the general instance);
#  exact<BM>x<BL>    the exact-width layout (halo inside the BL columns: tile step BL - 2 for k = 3 d = 1, BL - 6 for d = 3),
#                    Lq around multiples of that step;
#  instance-*        the same launch with guard 0, a guard 4 short of (largest tap offset + 264), that guard, the smallest
#                    guard (in steps of 4) that makes every tile interior, and 4 less (the last tile goes general again);
#  convtr2d-*        every decoder level's (Cin, Cout, pitch; in_pitch_log2 1 .. 6) at h = 1, 2, 7 and with per-row heights
#                    (the 30 s heights are rows of CASES);
#  convtr1d-*        strides 2, 3, 7 on this kernel, Lin around tile multiples, ragged rows (lq_extra = 1);
#  reflect-k7-*      Lin = 8 (the minimum) upwards, around tile multiples, ragged rows (general instance on every tile);
#  framemajor-*      the GRU projection's frame-major output view at T = 1001 and 3001, B = 32, and with a residual;
#  cin*              Cin = 2 (packed to 8, general instance), the engine's 8-channel entry block, Cin = 12 and 262 tails, and
#                    tails on the 4-channel K-chunk (Cin = 6, 10, 66, 262 with 9 or 7 taps on 64- / 128-row tiles; one split-K).
EDGES = [
    ('splitk-count2', ('conv1d', 1, 256, 64, 64, 0, 1, 1, 'zero', 0, 0, 'none', False, True), {}, (64, 64, 8, 1, 1)),
    ('splitk-count3', ('conv1d', 1, 384, 64, 64, 0, 1, 1, 'zero', 0, 0, 'none', False, True), {}, (64, 64, 8, 1, 1)),
    ('splitk-count4', ('conv1d', 1, 512, 64, 64, 0, 1, 1, 'zero', 0, 0, 'none', False, True), {}, (64, 64, 8, 1, 1)),
    ('splitk-count5', ('conv1d', 1, 640, 64, 64, 0, 1, 1, 'zero', 0, 0, 'none', False, True), {}, (64, 64, 8, 1, 1)),
    ('splitk-count6', ('conv1d', 1, 768, 64, 64, 0, 1, 1, 'zero', 0, 0, 'none', False, True), {}, (64, 64, 8, 1, 1)),
    ('splitk-count7', ('conv1d', 1, 896, 64, 64, 0, 1, 1, 'zero', 0, 0, 'none', False, True), {}, (64, 64, 8, 1, 1)),
    ('splitk-count8', ('conv1d', 1, 1024, 64, 64, 0, 1, 1, 'zero', 0, 0, 'none', False, True), {}, (64, 64, 8, 1, 1)),
    ('splitk-uneven-last-partial', ('conv1d', 1, 400, 64, 64, 0, 1, 1, 'zero', 0, 0, 'none', False, True), {}, (64, 64, 8, 1, 1)),
    ('splitk-channel-tail-262', ('conv1d', 1, 262, 64, 64, 0, 1, 1, 'zero', 0, 0, 'none', False, True), {}, (64, 64, 8, 1, 1)),
    ('splitk-channel-tail-262-bias-res-tanh', ('conv1d', 2, 262, 64, 100, 0, 1, 1, 'zero', 0, 3, 'in place', False, True), {}, (64, 64, 8, 1, 1)),
    ('splitk-bias-resinplace-lrelu', ('conv1d', 3, 512, 128, 130, 0, 1, 1, 'zero', 0, 1, 'in place', False, True), {'heavy': True}, (64, 64, 8, 1, 1)),
    ('splitk-bias-res-snake-k3', ('conv1d', 1, 512, 64, 200, 0, 3, 1, 'zero', 0, 5, 'separate', False, True), {}, (64, 64, 8, 1, 1)),
    ('splitk-map-3x3-P4', ('conv2d', 2, 384, 384, 32, 4, 3, 1, 'zero', 2, 1, 'none', False, True), {}, (64, 64, 4, 1, 1)),
    ('splitk-map-3x3-P2-resinplace', ('conv2d', 3, 384, 384, 16, 2, 3, 1, 'zero', 0, 0, 'in place', False, True), {'heavy': True}, (64, 64, 4, 1, 1)),
    ('splitk-map-1x1-P8', ('conv2d', 1, 768, 384, 64, 8, 1, 1, 'zero', 0, 0, 'none', False, True), {}, (64, 64, 8, 1, 1)),
    ('splitk-map-ragged', ('conv2d', 4, 384, 384, 32, 4, 3, 1, 'zero', 2, 1, 'none', True, True), {}, (64, 64, 4, 1, 1)),
    ('splitk-ragged-1d-resinplace', ('conv1d', 3, 512, 128, 130, 0, 1, 1, 'zero', 0, 0, 'in place', False, True), {'lengths': [130, 7, 64]}, (64, 64, 8, 1, 1)),
    ('splitk-switch-B15', ('conv2d', 15, 384, 384, 32, 4, 3, 1, 'zero', 2, 1, 'none', False, True), {}, (64, 64, 4, 1, 1)),
    ('splitk-switch-B16', ('conv2d', 16, 384, 384, 32, 4, 3, 1, 'zero', 2, 1, 'none', False, True), {}, (64, 64, 4, 1, 1)),
    ('splitk-switch-B17', ('conv2d', 17, 384, 384, 32, 4, 3, 1, 'zero', 2, 1, 'none', False, True), {}, (64, 64, 4, 1, 0)),
    ('splitk-switch-B18', ('conv2d', 18, 384, 384, 32, 4, 3, 1, 'zero', 2, 1, 'none', False, True), {}, (64, 64, 4, 1, 0)),
    ('tile128x128-k1-L1535', ('conv1d', 32, 72, 128, 1535, 0, 1, 1, 'zero', 0, 1, 'none', False, True), {}, (128, 128, 8, 1, 0)),
    ('tile128x128-k1-L1536', ('conv1d', 32, 72, 128, 1536, 0, 1, 1, 'zero', 0, 1, 'none', False, True), {}, (128, 128, 8, 1, 0)),
    ('tile128x128-k1-L1537', ('conv1d', 32, 72, 128, 1537, 0, 1, 1, 'zero', 0, 1, 'none', False, True), {}, (128, 128, 8, 1, 0)),
    ('tile64x256-k1-L3071', ('conv1d', 32, 72, 64, 3071, 0, 1, 1, 'zero', 0, 1, 'none', False, True), {}, (64, 256, 8, 1, 0)),
    ('tile64x256-k1-L3072', ('conv1d', 32, 72, 64, 3072, 0, 1, 1, 'zero', 0, 1, 'none', False, True), {}, (64, 256, 8, 1, 0)),
    ('tile64x256-k1-L3073', ('conv1d', 32, 72, 64, 3073, 0, 1, 1, 'zero', 0, 1, 'none', False, True), {}, (64, 256, 8, 1, 0)),
    ('tile128x64-k1-L767', ('conv1d', 32, 72, 128, 767, 0, 1, 1, 'zero', 0, 1, 'none', False, True), {}, (128, 64, 8, 1, 0)),
    ('tile128x64-k1-L768', ('conv1d', 32, 72, 128, 768, 0, 1, 1, 'zero', 0, 1, 'none', False, True), {}, (128, 64, 8, 1, 0)),
    ('tile128x64-k1-L769', ('conv1d', 32, 72, 128, 769, 0, 1, 1, 'zero', 0, 1, 'none', False, True), {}, (128, 64, 8, 1, 0)),
    ('tile32x256-k1-L3071', ('conv1d', 32, 72, 32, 3071, 0, 1, 1, 'zero', 0, 1, 'none', False, True), {}, (32, 256, 8, 1, 0)),
    ('tile32x256-k1-L3072', ('conv1d', 32, 72, 32, 3072, 0, 1, 1, 'zero', 0, 1, 'none', False, True), {}, (32, 256, 8, 1, 0)),
    ('tile32x256-k1-L3073', ('conv1d', 32, 72, 32, 3073, 0, 1, 1, 'zero', 0, 1, 'none', False, True), {}, (32, 256, 8, 1, 0)),
    ('tile64x64-k1-L63', ('conv1d', 1, 72, 64, 63, 0, 1, 1, 'zero', 0, 1, 'none', False, True), {}, (64, 64, 8, 1, 0)),
    ('tile64x64-k1-L64', ('conv1d', 1, 72, 64, 64, 0, 1, 1, 'zero', 0, 1, 'none', False, True), {}, (64, 64, 8, 1, 0)),
    ('tile64x64-k1-L65', ('conv1d', 1, 72, 64, 65, 0, 1, 1, 'zero', 0, 1, 'none', False, True), {}, (64, 64, 8, 1, 0)),
    ('tile32x128-k1-L127', ('conv1d', 1, 72, 32, 127, 0, 1, 1, 'zero', 0, 1, 'none', False, True), {}, (32, 128, 8, 1, 0)),
    ('tile32x128-k1-L128', ('conv1d', 1, 72, 32, 128, 0, 1, 1, 'zero', 0, 1, 'none', False, True), {}, (32, 128, 8, 1, 0)),
    ('tile32x128-k1-L129', ('conv1d', 1, 72, 32, 129, 0, 1, 1, 'zero', 0, 1, 'none', False, True), {}, (32, 128, 8, 1, 0)),
    ('tile128x128-k3d9-noguard-L1535', ('conv1d', 32, 40, 128, 1535, 0, 3, 9, 'zero', 1, 0, 'none', False, True), {'guard': 0}, (128, 128, 8, 2, 0)),
    ('tile128x128-k3d9-noguard-L1536', ('conv1d', 32, 40, 128, 1536, 0, 3, 9, 'zero', 1, 0, 'none', False, True), {'guard': 0}, (128, 128, 8, 2, 0)),
    ('tile128x128-k3d9-noguard-L1537', ('conv1d', 32, 40, 128, 1537, 0, 3, 9, 'zero', 1, 0, 'none', False, True), {'guard': 0}, (128, 128, 8, 2, 0)),
    ('tile64x256-k3d9-noguard-L3071', ('conv1d', 32, 40, 64, 3071, 0, 3, 9, 'zero', 1, 0, 'none', False, True), {'guard': 0}, (64, 256, 8, 2, 0)),
    ('tile64x256-k3d9-noguard-L3072', ('conv1d', 32, 40, 64, 3072, 0, 3, 9, 'zero', 1, 0, 'none', False, True), {'guard': 0}, (64, 256, 8, 2, 0)),
    ('tile64x256-k3d9-noguard-L3073', ('conv1d', 32, 40, 64, 3073, 0, 3, 9, 'zero', 1, 0, 'none', False, True), {'guard': 0}, (64, 256, 8, 2, 0)),
    ('tile128x64-k3d9-noguard-L767', ('conv1d', 32, 40, 128, 767, 0, 3, 9, 'zero', 1, 0, 'none', False, True), {'guard': 0}, (128, 64, 8, 2, 0)),
    ('tile128x64-k3d9-noguard-L768', ('conv1d', 32, 40, 128, 768, 0, 3, 9, 'zero', 1, 0, 'none', False, True), {'guard': 0}, (128, 64, 8, 2, 0)),
    ('tile128x64-k3d9-noguard-L769', ('conv1d', 32, 40, 128, 769, 0, 3, 9, 'zero', 1, 0, 'none', False, True), {'guard': 0}, (128, 64, 8, 2, 0)),
    ('tile32x256-k3d9-noguard-L3071', ('conv1d', 32, 40, 32, 3071, 0, 3, 9, 'zero', 1, 0, 'none', False, True), {'guard': 0}, (32, 256, 8, 2, 0)),
    ('tile32x256-k3d9-noguard-L3072', ('conv1d', 32, 40, 32, 3072, 0, 3, 9, 'zero', 1, 0, 'none', False, True), {'guard': 0}, (32, 256, 8, 2, 0)),
    ('tile32x256-k3d9-noguard-L3073', ('conv1d', 32, 40, 32, 3073, 0, 3, 9, 'zero', 1, 0, 'none', False, True), {'guard': 0}, (32, 256, 8, 2, 0)),
    ('tile64x64-k3d9-noguard-L191', ('conv1d', 1, 40, 64, 191, 0, 3, 9, 'zero', 1, 0, 'none', False, True), {'guard': 0}, (64, 64, 8, 2, 0)),
    ('tile64x64-k3d9-noguard-L192', ('conv1d', 1, 40, 64, 192, 0, 3, 9, 'zero', 1, 0, 'none', False, True), {'guard': 0}, (64, 64, 8, 2, 0)),
    ('tile64x64-k3d9-noguard-L193', ('conv1d', 1, 40, 64, 193, 0, 3, 9, 'zero', 1, 0, 'none', False, True), {'guard': 0}, (64, 64, 8, 2, 0)),
    ('tile32x128-k3d9-noguard-L383', ('conv1d', 1, 40, 32, 383, 0, 3, 9, 'zero', 1, 0, 'none', False, True), {'guard': 0}, (32, 128, 8, 2, 0)),
    ('tile32x128-k3d9-noguard-L384', ('conv1d', 1, 40, 32, 384, 0, 3, 9, 'zero', 1, 0, 'none', False, True), {'guard': 0}, (32, 128, 8, 2, 0)),
    ('tile32x128-k3d9-noguard-L385', ('conv1d', 1, 40, 32, 385, 0, 3, 9, 'zero', 1, 0, 'none', False, True), {'guard': 0}, (32, 128, 8, 2, 0)),
    ('exact128x128-k3d1-L1511', ('conv1d', 32, 64, 128, 1511, 0, 3, 1, 'zero', 1, 1, 'none', False, True), {}, (128, 128, 8, 1, 0)),
    ('exact128x128-k3d1-L1512', ('conv1d', 32, 64, 128, 1512, 0, 3, 1, 'zero', 1, 1, 'none', False, True), {}, (128, 128, 8, 1, 0)),
    ('exact128x128-k3d1-L1513', ('conv1d', 32, 64, 128, 1513, 0, 3, 1, 'zero', 1, 1, 'none', False, True), {}, (128, 128, 8, 1, 0)),
    ('exact64x256-k3d1-L3047', ('conv1d', 32, 64, 64, 3047, 0, 3, 1, 'zero', 1, 1, 'none', False, True), {}, (64, 256, 8, 1, 0)),
    ('exact64x256-k3d1-L3048', ('conv1d', 32, 64, 64, 3048, 0, 3, 1, 'zero', 1, 1, 'none', False, True), {}, (64, 256, 8, 1, 0)),
    ('exact64x256-k3d1-L3049', ('conv1d', 32, 64, 64, 3049, 0, 3, 1, 'zero', 1, 1, 'none', False, True), {}, (64, 256, 8, 1, 0)),
    ('exact128x64-k3d1-L743', ('conv1d', 32, 64, 128, 743, 0, 3, 1, 'zero', 1, 1, 'none', False, True), {}, (128, 64, 8, 1, 0)),
    ('exact128x64-k3d1-L744', ('conv1d', 32, 64, 128, 744, 0, 3, 1, 'zero', 1, 1, 'none', False, True), {}, (128, 64, 8, 1, 0)),
    ('exact128x64-k3d1-L745', ('conv1d', 32, 64, 128, 745, 0, 3, 1, 'zero', 1, 1, 'none', False, True), {}, (128, 64, 8, 1, 0)),
    ('exact32x256-k3d1-L3047', ('conv1d', 32, 64, 32, 3047, 0, 3, 1, 'zero', 1, 1, 'none', False, True), {}, (32, 256, 8, 1, 0)),
    ('exact32x256-k3d1-L3048', ('conv1d', 32, 64, 32, 3048, 0, 3, 1, 'zero', 1, 1, 'none', False, True), {}, (32, 256, 8, 1, 0)),
    ('exact32x256-k3d1-L3049', ('conv1d', 32, 64, 32, 3049, 0, 3, 1, 'zero', 1, 1, 'none', False, True), {}, (32, 256, 8, 1, 0)),
    ('exact64x64-k3d1-L123', ('conv1d', 1, 64, 64, 123, 0, 3, 1, 'zero', 1, 1, 'none', False, True), {}, (64, 64, 8, 1, 0)),
    ('exact64x64-k3d1-L124', ('conv1d', 1, 64, 64, 124, 0, 3, 1, 'zero', 1, 1, 'none', False, True), {}, (64, 64, 8, 1, 0)),
    ('exact64x64-k3d1-L125', ('conv1d', 1, 64, 64, 125, 0, 3, 1, 'zero', 1, 1, 'none', False, True), {}, (64, 64, 8, 1, 0)),
    ('exact32x128-k3d1-L251', ('conv1d', 1, 64, 32, 251, 0, 3, 1, 'zero', 1, 1, 'none', False, True), {}, (32, 128, 8, 1, 0)),
    ('exact32x128-k3d1-L252', ('conv1d', 1, 64, 32, 252, 0, 3, 1, 'zero', 1, 1, 'none', False, True), {}, (32, 128, 8, 1, 0)),
    ('exact32x128-k3d1-L253', ('conv1d', 1, 64, 32, 253, 0, 3, 1, 'zero', 1, 1, 'none', False, True), {}, (32, 128, 8, 1, 0)),
    ('exact128x128-k3d3-L1463', ('conv1d', 32, 64, 128, 1463, 0, 3, 3, 'zero', 1, 1, 'none', False, True), {}, (128, 128, 8, 1, 0)),
    ('exact128x128-k3d3-L1464', ('conv1d', 32, 64, 128, 1464, 0, 3, 3, 'zero', 1, 1, 'none', False, True), {}, (128, 128, 8, 1, 0)),
    ('exact128x128-k3d3-L1465', ('conv1d', 32, 64, 128, 1465, 0, 3, 3, 'zero', 1, 1, 'none', False, True), {}, (128, 128, 8, 1, 0)),
    ('exact64x256-k3d3-L2999', ('conv1d', 32, 64, 64, 2999, 0, 3, 3, 'zero', 1, 1, 'none', False, True), {}, (64, 256, 8, 1, 0)),
    ('exact64x256-k3d3-L3000', ('conv1d', 32, 64, 64, 3000, 0, 3, 3, 'zero', 1, 1, 'none', False, True), {}, (64, 256, 8, 1, 0)),
    ('exact64x256-k3d3-L3001', ('conv1d', 32, 64, 64, 3001, 0, 3, 3, 'zero', 1, 1, 'none', False, True), {}, (64, 256, 8, 1, 0)),
    ('exact128x64-k3d3-L695', ('conv1d', 32, 64, 128, 695, 0, 3, 3, 'zero', 1, 1, 'none', False, True), {}, (128, 64, 8, 1, 0)),
    ('exact128x64-k3d3-L696', ('conv1d', 32, 64, 128, 696, 0, 3, 3, 'zero', 1, 1, 'none', False, True), {}, (128, 64, 8, 1, 0)),
    ('exact128x64-k3d3-L697', ('conv1d', 32, 64, 128, 697, 0, 3, 3, 'zero', 1, 1, 'none', False, True), {}, (128, 64, 8, 1, 0)),
    ('exact32x256-k3d3-L2999', ('conv1d', 32, 64, 32, 2999, 0, 3, 3, 'zero', 1, 1, 'none', False, True), {}, (32, 256, 8, 1, 0)),
    ('exact32x256-k3d3-L3000', ('conv1d', 32, 64, 32, 3000, 0, 3, 3, 'zero', 1, 1, 'none', False, True), {}, (32, 256, 8, 1, 0)),
    ('exact32x256-k3d3-L3001', ('conv1d', 32, 64, 32, 3001, 0, 3, 3, 'zero', 1, 1, 'none', False, True), {}, (32, 256, 8, 1, 0)),
    ('exact64x64-k3d3-L115', ('conv1d', 1, 64, 64, 115, 0, 3, 3, 'zero', 1, 1, 'none', False, True), {}, (64, 64, 8, 1, 0)),
    ('exact64x64-k3d3-L116', ('conv1d', 1, 64, 64, 116, 0, 3, 3, 'zero', 1, 1, 'none', False, True), {}, (64, 64, 8, 1, 0)),
    ('exact64x64-k3d3-L117', ('conv1d', 1, 64, 64, 117, 0, 3, 3, 'zero', 1, 1, 'none', False, True), {}, (64, 64, 8, 1, 0)),
    ('exact32x128-k3d3-L243', ('conv1d', 1, 64, 32, 243, 0, 3, 3, 'zero', 1, 1, 'none', False, True), {}, (32, 128, 8, 1, 0)),
    ('exact32x128-k3d3-L244', ('conv1d', 1, 64, 32, 244, 0, 3, 3, 'zero', 1, 1, 'none', False, True), {}, (32, 128, 8, 1, 0)),
    ('exact32x128-k3d3-L245', ('conv1d', 1, 64, 32, 245, 0, 3, 3, 'zero', 1, 1, 'none', False, True), {}, (32, 128, 8, 1, 0)),
    ('instance-k3d1-guard0', ('conv1d', 2, 64, 128, 900, 0, 3, 1, 'zero', 1, 0, 'separate', False, True), {'guard': 0, 'alloc_guard': 268}, (64, 64, 8, 2, 0)),
    ('instance-k3d1-guardshort', ('conv1d', 2, 64, 128, 900, 0, 3, 1, 'zero', 1, 0, 'separate', False, True), {'guard': 264, 'alloc_guard': 268}, (64, 64, 8, 1, 0)),
    ('instance-k3d1-guardfull', ('conv1d', 2, 64, 128, 900, 0, 3, 1, 'zero', 1, 0, 'separate', False, True), {'guard': 268, 'alloc_guard': 268}, (64, 64, 8, 1, 0)),
    ('instance-k3d1-guardmin', ('conv1d', 2, 64, 128, 900, 0, 3, 1, 'zero', 1, 0, 'separate', False, True), {'guard': 32, 'alloc_guard': 268}, (64, 64, 8, 1, 0)),
    ('instance-k3d1-guardminshort', ('conv1d', 2, 64, 128, 900, 0, 3, 1, 'zero', 1, 0, 'separate', False, True), {'guard': 28, 'alloc_guard': 268}, (64, 64, 8, 2, 0)),
    ('instance-k3d27-guard0', ('conv1d', 2, 64, 128, 900, 0, 3, 27, 'zero', 1, 0, 'separate', False, True), {'guard': 0, 'alloc_guard': 292}, (64, 64, 8, 2, 0)),
    ('instance-k3d27-guardshort', ('conv1d', 2, 64, 128, 900, 0, 3, 27, 'zero', 1, 0, 'separate', False, True), {'guard': 288, 'alloc_guard': 292}, (64, 64, 8, 1, 0)),
    ('instance-k3d27-guardfull', ('conv1d', 2, 64, 128, 900, 0, 3, 27, 'zero', 1, 0, 'separate', False, True), {'guard': 292, 'alloc_guard': 292}, (64, 64, 8, 1, 0)),
    ('instance-k3d27-guardmin', ('conv1d', 2, 64, 128, 900, 0, 3, 27, 'zero', 1, 0, 'separate', False, True), {'guard': 88, 'alloc_guard': 292}, (64, 64, 8, 1, 0)),
    ('instance-k3d27-guardminshort', ('conv1d', 2, 64, 128, 900, 0, 3, 27, 'zero', 1, 0, 'separate', False, True), {'guard': 84, 'alloc_guard': 292}, (64, 64, 8, 2, 0)),
    ('instance-k7d1-guard0', ('conv1d', 2, 64, 128, 900, 0, 7, 1, 'zero', 1, 0, 'separate', False, True), {'guard': 0, 'alloc_guard': 268}, (64, 64, 8, 2, 0)),
    ('instance-k7d1-guardshort', ('conv1d', 2, 64, 128, 900, 0, 7, 1, 'zero', 1, 0, 'separate', False, True), {'guard': 264, 'alloc_guard': 268}, (64, 64, 8, 1, 0)),
    ('instance-k7d1-guardfull', ('conv1d', 2, 64, 128, 900, 0, 7, 1, 'zero', 1, 0, 'separate', False, True), {'guard': 268, 'alloc_guard': 268}, (64, 64, 8, 1, 0)),
    ('instance-k7d1-guardmin', ('conv1d', 2, 64, 128, 900, 0, 7, 1, 'zero', 1, 0, 'separate', False, True), {'guard': 32, 'alloc_guard': 268}, (64, 64, 8, 1, 0)),
    ('instance-k7d1-guardminshort', ('conv1d', 2, 64, 128, 900, 0, 7, 1, 'zero', 1, 0, 'separate', False, True), {'guard': 28, 'alloc_guard': 268}, (64, 64, 8, 2, 0)),
    ('instance-map3x3-P16-guard0', ('conv2d', 2, 64, 64, 40, 16, 3, 1, 'zero', 2, 1, 'none', False, True), {'guard': 0, 'alloc_guard': 284}, (64, 64, 4, 2, 0)),
    ('instance-map3x3-P16-guardshort', ('conv2d', 2, 64, 64, 40, 16, 3, 1, 'zero', 2, 1, 'none', False, True), {'guard': 280, 'alloc_guard': 284}, (64, 64, 4, 1, 0)),
    ('instance-map3x3-P16-guardfull', ('conv2d', 2, 64, 64, 40, 16, 3, 1, 'zero', 2, 1, 'none', False, True), {'guard': 284, 'alloc_guard': 284}, (64, 64, 4, 1, 0)),
    ('instance-map3x3-P16-guardmin', ('conv2d', 2, 64, 64, 40, 16, 3, 1, 'zero', 2, 1, 'none', False, True), {'guard': 20, 'alloc_guard': 284}, (64, 64, 4, 1, 0)),
    ('instance-map3x3-P16-guardminshort', ('conv2d', 2, 64, 64, 40, 16, 3, 1, 'zero', 2, 1, 'none', False, True), {'guard': 16, 'alloc_guard': 284}, (64, 64, 4, 2, 0)),
    ('instance-convtr1d-s3-guard0', ('convtr1d', 2, 64, 64, 300, 0, 6, 3, 'zero', 0, 0, 'none', False, True), {'guard': 0, 'alloc_guard': 264}, (64, 64, 8, 2, 0)),
    ('instance-convtr1d-s3-guardmin', ('convtr1d', 2, 64, 64, 300, 0, 6, 3, 'zero', 0, 0, 'none', False, True), {'guard': 16, 'alloc_guard': 264}, (64, 64, 8, 1, 0)),
    ('instance-convtr1d-s3-guardminshort', ('convtr1d', 2, 64, 64, 300, 0, 6, 3, 'zero', 0, 0, 'none', False, True), {'guard': 12, 'alloc_guard': 264}, (64, 64, 8, 2, 0)),
    ('convtr2d-384to384-P2-h1', ('convtr2d_3x3s2', 2, 384, 384, 1, 2, 3, 2, 'zero', 2, 0, 'none', False, True), {'heavy': False}, (64, 64, 8, 1, 0)),
    ('convtr2d-384to384-P2-h2', ('convtr2d_3x3s2', 2, 384, 384, 2, 2, 3, 2, 'zero', 2, 0, 'none', False, True), {'heavy': False}, (64, 64, 8, 1, 0)),
    ('convtr2d-384to384-P2-h7', ('convtr2d_3x3s2', 2, 384, 384, 7, 2, 3, 2, 'zero', 2, 0, 'none', False, True), {'heavy': True}, (64, 64, 8, 1, 0)),
    ('convtr2d-384to384-P2-ragged', ('convtr2d_3x3s2', 4, 384, 384, 12, 2, 3, 2, 'zero', 2, 0, 'none', False, True), {'lengths': [12, 1, 5, 8]}, (64, 64, 8, 1, 0)),
    ('convtr2d-384to384-P4-h1', ('convtr2d_3x3s2', 2, 384, 384, 1, 4, 3, 2, 'zero', 2, 0, 'none', False, True), {'heavy': False}, (64, 64, 8, 1, 0)),
    ('convtr2d-384to384-P4-h2', ('convtr2d_3x3s2', 2, 384, 384, 2, 4, 3, 2, 'zero', 2, 0, 'none', False, True), {'heavy': False}, (64, 64, 8, 1, 0)),
    ('convtr2d-384to384-P4-h7', ('convtr2d_3x3s2', 2, 384, 384, 7, 4, 3, 2, 'zero', 2, 0, 'none', False, True), {'heavy': True}, (64, 64, 8, 1, 0)),
    ('convtr2d-384to384-P4-ragged', ('convtr2d_3x3s2', 4, 384, 384, 12, 4, 3, 2, 'zero', 2, 0, 'none', False, True), {'lengths': [12, 1, 5, 8]}, (64, 64, 8, 1, 0)),
    ('convtr2d-384to256-P8-h1', ('convtr2d_3x3s2', 2, 384, 256, 1, 8, 3, 2, 'zero', 2, 0, 'none', False, True), {'heavy': False}, (64, 64, 8, 1, 0)),
    ('convtr2d-384to256-P8-h2', ('convtr2d_3x3s2', 2, 384, 256, 2, 8, 3, 2, 'zero', 2, 0, 'none', False, True), {'heavy': False}, (64, 64, 8, 1, 0)),
    ('convtr2d-384to256-P8-h7', ('convtr2d_3x3s2', 2, 384, 256, 7, 8, 3, 2, 'zero', 2, 0, 'none', False, True), {'heavy': True}, (64, 64, 8, 1, 0)),
    ('convtr2d-384to256-P8-ragged', ('convtr2d_3x3s2', 4, 384, 256, 12, 8, 3, 2, 'zero', 2, 0, 'none', False, True), {'lengths': [12, 1, 5, 8]}, (64, 64, 8, 1, 0)),
    ('convtr2d-256to128-P16-h1', ('convtr2d_3x3s2', 2, 256, 128, 1, 16, 3, 2, 'zero', 2, 0, 'none', False, True), {'heavy': False}, (64, 64, 8, 1, 0)),
    ('convtr2d-256to128-P16-h2', ('convtr2d_3x3s2', 2, 256, 128, 2, 16, 3, 2, 'zero', 2, 0, 'none', False, True), {'heavy': False}, (64, 64, 8, 1, 0)),
    ('convtr2d-256to128-P16-h7', ('convtr2d_3x3s2', 2, 256, 128, 7, 16, 3, 2, 'zero', 2, 0, 'none', False, True), {'heavy': True}, (64, 64, 8, 1, 0)),
    ('convtr2d-256to128-P16-ragged', ('convtr2d_3x3s2', 4, 256, 128, 12, 16, 3, 2, 'zero', 2, 0, 'none', False, True), {'lengths': [12, 1, 5, 8]}, (64, 64, 8, 1, 0)),
    ('convtr2d-128to64-P32-h1', ('convtr2d_3x3s2', 2, 128, 64, 1, 32, 3, 2, 'zero', 2, 0, 'none', False, True), {'heavy': False}, (64, 64, 8, 1, 0)),
    ('convtr2d-128to64-P32-h2', ('convtr2d_3x3s2', 2, 128, 64, 2, 32, 3, 2, 'zero', 2, 0, 'none', False, True), {'heavy': False}, (64, 64, 8, 1, 0)),
    ('convtr2d-128to64-P32-h7', ('convtr2d_3x3s2', 2, 128, 64, 7, 32, 3, 2, 'zero', 2, 0, 'none', False, True), {'heavy': True}, (64, 64, 8, 1, 0)),
    ('convtr2d-128to64-P32-ragged', ('convtr2d_3x3s2', 4, 128, 64, 12, 32, 3, 2, 'zero', 2, 0, 'none', False, True), {'lengths': [12, 1, 5, 8]}, (64, 64, 8, 1, 0)),
    ('convtr2d-64to32-P64-h1', ('convtr2d_3x3s2', 2, 64, 32, 1, 64, 3, 2, 'zero', 2, 0, 'none', False, True), {'heavy': False}, (32, 128, 8, 1, 0)),
    ('convtr2d-64to32-P64-h2', ('convtr2d_3x3s2', 2, 64, 32, 2, 64, 3, 2, 'zero', 2, 0, 'none', False, True), {'heavy': False}, (32, 128, 8, 1, 0)),
    ('convtr2d-64to32-P64-h7', ('convtr2d_3x3s2', 2, 64, 32, 7, 64, 3, 2, 'zero', 2, 0, 'none', False, True), {'heavy': True}, (32, 128, 8, 1, 0)),
    ('convtr2d-64to32-P64-ragged', ('convtr2d_3x3s2', 4, 64, 32, 12, 64, 3, 2, 'zero', 2, 0, 'none', False, True), {'lengths': [12, 1, 5, 8]}, (32, 128, 8, 1, 0)),
    ('convtr1d-s2-Lin127', ('convtr1d', 2, 64, 64, 127, 0, 4, 2, 'zero', 0, 0, 'none', False, True), {'heavy': False}, (64, 64, 8, 1, 0)),
    ('convtr1d-s2-Lin128', ('convtr1d', 2, 64, 64, 128, 0, 4, 2, 'zero', 0, 0, 'none', False, True), {'heavy': False}, (64, 64, 8, 1, 0)),
    ('convtr1d-s2-Lin129', ('convtr1d', 2, 64, 64, 129, 0, 4, 2, 'zero', 0, 0, 'none', False, True), {'heavy': True}, (64, 64, 8, 1, 0)),
    ('convtr1d-s2-Lin255', ('convtr1d', 2, 64, 64, 255, 0, 4, 2, 'zero', 0, 0, 'none', False, True), {'heavy': False}, (64, 64, 8, 1, 0)),
    ('convtr1d-s2-Lin256', ('convtr1d', 2, 64, 64, 256, 0, 4, 2, 'zero', 0, 0, 'none', False, True), {'heavy': False}, (64, 64, 8, 1, 0)),
    ('convtr1d-s2-Lin257', ('convtr1d', 2, 64, 64, 257, 0, 4, 2, 'zero', 0, 0, 'none', False, True), {'heavy': False}, (64, 64, 8, 1, 0)),
    ('convtr1d-s2-ragged', ('convtr1d', 4, 64, 64, 300, 0, 4, 2, 'zero', 0, 0, 'none', False, True), {'lengths': [300, 1, 128, 255]}, (64, 64, 8, 1, 0)),
    ('convtr1d-s3-Lin127', ('convtr1d', 2, 64, 64, 127, 0, 6, 3, 'zero', 0, 0, 'none', False, True), {'heavy': False}, (64, 64, 8, 1, 0)),
    ('convtr1d-s3-Lin128', ('convtr1d', 2, 64, 64, 128, 0, 6, 3, 'zero', 0, 0, 'none', False, True), {'heavy': False}, (64, 64, 8, 1, 0)),
    ('convtr1d-s3-Lin129', ('convtr1d', 2, 64, 64, 129, 0, 6, 3, 'zero', 0, 0, 'none', False, True), {'heavy': True}, (64, 64, 8, 1, 0)),
    ('convtr1d-s3-Lin255', ('convtr1d', 2, 64, 64, 255, 0, 6, 3, 'zero', 0, 0, 'none', False, True), {'heavy': False}, (64, 64, 8, 1, 0)),
    ('convtr1d-s3-Lin256', ('convtr1d', 2, 64, 64, 256, 0, 6, 3, 'zero', 0, 0, 'none', False, True), {'heavy': False}, (64, 64, 8, 1, 0)),
    ('convtr1d-s3-Lin257', ('convtr1d', 2, 64, 64, 257, 0, 6, 3, 'zero', 0, 0, 'none', False, True), {'heavy': False}, (64, 64, 8, 1, 0)),
    ('convtr1d-s3-ragged', ('convtr1d', 4, 64, 64, 300, 0, 6, 3, 'zero', 0, 0, 'none', False, True), {'lengths': [300, 1, 128, 255]}, (64, 64, 8, 1, 0)),
    ('convtr1d-s7-Lin127', ('convtr1d', 2, 64, 64, 127, 0, 14, 7, 'zero', 0, 0, 'none', False, True), {'heavy': False}, (64, 64, 8, 1, 0)),
    ('convtr1d-s7-Lin128', ('convtr1d', 2, 64, 64, 128, 0, 14, 7, 'zero', 0, 0, 'none', False, True), {'heavy': False}, (64, 64, 8, 1, 0)),
    ('convtr1d-s7-Lin129', ('convtr1d', 2, 64, 64, 129, 0, 14, 7, 'zero', 0, 0, 'none', False, True), {'heavy': True}, (64, 64, 8, 1, 0)),
    ('convtr1d-s7-Lin255', ('convtr1d', 2, 64, 64, 255, 0, 14, 7, 'zero', 0, 0, 'none', False, True), {'heavy': False}, (64, 64, 8, 1, 0)),
    ('convtr1d-s7-Lin256', ('convtr1d', 2, 64, 64, 256, 0, 14, 7, 'zero', 0, 0, 'none', False, True), {'heavy': False}, (64, 64, 8, 1, 0)),
    ('convtr1d-s7-Lin257', ('convtr1d', 2, 64, 64, 257, 0, 14, 7, 'zero', 0, 0, 'none', False, True), {'heavy': False}, (64, 64, 8, 1, 0)),
    ('convtr1d-s7-ragged', ('convtr1d', 4, 64, 64, 300, 0, 14, 7, 'zero', 0, 0, 'none', False, True), {'lengths': [300, 1, 128, 255]}, (64, 64, 8, 1, 0)),
    ('reflect-k7-L8', ('conv1d', 2, 64, 128, 8, 0, 7, 1, 'reflect', 0, 5, 'none', False, True), {}, (64, 64, 8, 1, 0)),
    ('reflect-k7-L9', ('conv1d', 2, 64, 128, 9, 0, 7, 1, 'reflect', 0, 5, 'none', False, True), {}, (64, 64, 8, 1, 0)),
    ('reflect-k7-L127', ('conv1d', 2, 64, 128, 127, 0, 7, 1, 'reflect', 0, 5, 'none', False, True), {}, (64, 64, 8, 1, 0)),
    ('reflect-k7-L128', ('conv1d', 2, 64, 128, 128, 0, 7, 1, 'reflect', 0, 5, 'none', False, True), {}, (64, 64, 8, 1, 0)),
    ('reflect-k7-L129', ('conv1d', 2, 64, 128, 129, 0, 7, 1, 'reflect', 0, 5, 'none', False, True), {}, (64, 64, 8, 1, 0)),
    ('reflect-k7-L255', ('conv1d', 2, 64, 128, 255, 0, 7, 1, 'reflect', 0, 5, 'none', False, True), {}, (64, 64, 8, 2, 0)),
    ('reflect-k7-L256', ('conv1d', 2, 64, 128, 256, 0, 7, 1, 'reflect', 0, 5, 'none', False, True), {}, (64, 64, 8, 2, 0)),
    ('reflect-k7-L257', ('conv1d', 2, 64, 128, 257, 0, 7, 1, 'reflect', 0, 5, 'none', False, True), {}, (64, 64, 8, 2, 0)),
    ('reflect-k7-L513', ('conv1d', 2, 64, 128, 513, 0, 7, 1, 'reflect', 0, 5, 'none', False, True), {}, (64, 64, 8, 2, 0)),
    ('reflect-k7-ragged', ('conv1d', 5, 64, 128, 400, 0, 7, 1, 'reflect', 0, 5, 'none', False, True), {'lengths': [400, 8, 9, 128, 257], 'heavy': True}, (64, 64, 8, 1, 0)),
    ('reflect-k7-ragged-512to1024', ('conv1d', 3, 512, 1024, 300, 0, 7, 1, 'reflect', 0, 5, 'none', False, True), {'lengths': [300, 8, 131]}, (64, 64, 8, 1, 0)),
    ('framemajor-B32-T1001-post-sigmoid', ('conv1d', 32, 512, 1536, 1001, 0, 1, 1, 'zero', 0, 4, 'none', False, False), {}, (128, 128, 8, 1, 0)),
    ('framemajor-B32-T3001', ('conv1d', 32, 512, 1536, 3001, 0, 1, 1, 'zero', 0, 0, 'none', False, False), {}, (128, 128, 8, 1, 0)),
    ('framemajor-B3-T77-res', ('conv1d', 3, 128, 96, 77, 0, 1, 1, 'zero', 0, 0, 'separate', False, False), {}, (32, 128, 8, 1, 0)),
    ('cin2-3x3-P128', ('conv2d', 2, 2, 32, 24, 128, 3, 1, 'zero', 2, 1, 'none', False, True), {}, (32, 128, 8, 1, 0)),
    ('cin2-1x1-P128', ('conv2d', 2, 2, 32, 24, 128, 1, 1, 'zero', 0, 0, 'none', False, True), {}, (32, 128, 8, 1, 0)),
    ('cin8-entry-3x3-P128', ('conv2d', 2, 8, 32, 64, 128, 3, 1, 'zero', 2, 1, 'none', False, True), {}, (32, 128, 8, 1, 0)),
    ('cin8-entry-1x1-P128', ('conv2d', 2, 8, 32, 64, 128, 1, 1, 'zero', 0, 0, 'none', False, True), {}, (32, 128, 8, 1, 0)),
    ('cin12-k3-1d', ('conv1d', 2, 12, 64, 300, 0, 3, 1, 'zero', 1, 0, 'none', False, True), {}, (64, 64, 8, 1, 0)),
    ('cin262-k3d3-1d', ('conv1d', 2, 262, 64, 700, 0, 3, 3, 'zero', 1, 0, 'in place', False, True), {}, (64, 64, 8, 1, 1)),
    ('cin6-3x3-P16-kc4', ('conv2d', 2, 6, 64, 24, 16, 3, 1, 'zero', 2, 1, 'none', False, True), {}, (64, 64, 4, 1, 0)),
    ('cin10-3x3-P16-kc4-B8', ('conv2d', 8, 10, 128, 40, 16, 3, 1, 'zero', 0, 0, 'in place', False, True), {}, (64, 64, 4, 1, 0)),
    ('cin262-3x3-P4-kc4-splitk', ('conv2d', 2, 262, 64, 32, 4, 3, 1, 'zero', 2, 1, 'none', False, True), {}, (64, 64, 4, 1, 1)),
    ('cin66-k7-reflect-kc4', ('conv1d', 8, 66, 512, 1006, 0, 7, 1, 'reflect', 0, 5, 'none', False, True), {}, (128, 64, 4, 1, 0)),
]


def _edge_spec(key, extra):
    spec = spec_of(key)
    spec.update(extra)
    return spec


@pytest.mark.parametrize("i", range(len(EDGES)), ids=[e[0] for e in EDGES])
def test_edge_parity(i):
    name, key, extra, expect = EDGES[i]
    run_case(_edge_spec(key, extra), expect, seed=5000 + i, name=name)


def test_edges_reach_every_tile_both_chunk_depths_and_every_instance_mix():
    """The table above means to take every path: six tiles, K-chunks of 4 and 8, one and two grids, with and without split-K."""
    seen = {e[3] for e in EDGES}
    for tile in ((128, 128), (64, 256), (128, 64), (32, 256), (64, 64), (32, 128)):
        assert any(s[:2] == tile and s[3] == 1 for s in seen) and any(s[:2] == tile and s[3] == 2 for s in seen), tile
    assert {s[2] for s in seen} == {4, 8}
    assert {(s[3], s[4]) for s in seen} >= {(1, 0), (2, 0), (1, 1)}
    assert len({e[0] for e in EDGES}) == len(EDGES)


def test_splitk_counts_follow_the_rule():
    """The split counts the `splitk-count<n>` rows mean to produce, from the rule of launch_conv (vfx_conv.hip):
    want = min(512 / nwg, 8, nchunks / 16), chunks per split = ceil(nchunks / want), splits = ceil(nchunks / that)."""
    for name, key, extra, expect in EDGES:
        if not name.startswith("splitk-count"):
            continue
        cin, kc = key[2], expect[2]
        nchunks = (cin + kc - 1) // kc
        want = min(512 // 1, 8, nchunks // 16)
        cpp = (nchunks + want - 1) // want
        assert (nchunks + cpp - 1) // cpp == int(name[len("splitk-count"):]) and expect[4] == 1
    uneven = [e for e in EDGES if e[0] == "splitk-uneven-last-partial"][0]
    nchunks = uneven[1][2] // uneven[3][2]
    assert nchunks == 50 and nchunks % 3 != 0


def test_split_and_unsplit_launch_agree_around_the_workgroup_switch():
    """The same 3x3 launch at B = 16 (192 workgroups: split-K) and B = 17 (204: one pass): rows 0 .. 15 see the same
    operands (_inputs draws every row from its own generator), so the two results differ only by the order of the sum --
    each is held to float64, and here to each other."""
    rows = {e[0]: e for e in EDGES if e[0].startswith("splitk-switch-B")}
    lo, hi = rows["splitk-switch-B16"], rows["splitk-switch-B17"]
    assert lo[3][4] == 1 and hi[3][4] == 0
    a = run_case(_edge_spec(lo[1], lo[2]), lo[3], seed=77, name="switch-B16")
    b = run_case(_edge_spec(hi[1], hi[2]), hi[3], seed=77, name="switch-B17")
    assert a.shape[0] == 16 and b.shape[0] == 17
    # a handful of ulps of the output peak: twice what either is allowed against float64 (K = 3456 products of order
    # K^-1/2: the figure's magnitude is of the order of the peak)
    assert (a - b[:16]).abs().max() <= 2 * MARGIN * 4 * ULP * b.abs().max()


def test_ragged_reflect_rows_equal_the_rows_alone():
    """Reflect padding mirrors at every row's OWN end (general instance on every tile): row b of the ragged launch is
    bit-equal to the same row launched alone at its own length whenever the two launches use the same K-chunk depth
    (the order of the sum depends on nothing else), and within a few ulps otherwise."""
    name, key, extra, expect = [e for e in EDGES if e[0] == "reflect-k7-ragged"][0]
    spec = _edge_spec(key, extra)
    t = _inputs(spec, 91)
    B, cin, cout, cap = spec["B"], spec["cin"], spec["cout"], spec["ext"]
    lengths = spec["lengths"]
    wp = packing.pack_conv1d(t["w"]).to(DEV)
    bias = t["bias"].to(DEV)
    act = ops.Act(post=_lib.POST_LRELU_SNAKE, post_slope=0.2)
    lib = _lib.lib()

    def launch(x, lens):
        xb, xv = _alloc(x.shape[0], cin, x.shape[2], 264)
        for b, n in enumerate(lens):
            xv[b, :, :n] = x[b, :, :n].to(DEV)
        xv._vfx_guard = 264
        if len(set(lens)) > 1 or lens[0] != x.shape[2]:
            ops.with_rows(xv, torch.tensor(lens, dtype=torch.int32, device=DEV))
        yb, yv = _alloc(x.shape[0], cout, x.shape[2], 8)
        ops.conv1d(xv, wp, bias, yv, x.shape[2], 7, 1, _lib.PAD_REFLECT, act)
        torch.cuda.synchronize()
        return yv.cpu(), lib.vfx_last_conv_tile() % 100

    batch, kc_batch = launch(t["x"], lengths)
    for b, n in enumerate(lengths):
        alone, kc = launch(t["x"][b:b + 1, :, :n].contiguous(), [n])
        assert torch.isfinite(alone[0, :, :n]).all()
        if kc == kc_batch:
            assert torch.equal(batch[b, :, :n], alone[0, :, :n]), "row %d (%d samples) differs from the row alone" % (b, n)
        else:
            assert (batch[b, :, :n] - alone[0, :, :n]).abs().max() <= 16 * ULP * alone[0, :, :n].abs().max()
        assert torch.isnan(batch[b, :, n:]).all()


def test_argument_checks_return_codes():
    """Refusals are return codes on valid buffers, before anything is launched: reflect padding needs 8 samples
    (VFX_EINVAL at Lin = 7, fine at 8), Cout must be a multiple of 32, k odd, a map kernel 1 or 3, rows 16-byte aligned."""
    lib = _lib.lib()
    x = torch.zeros((1, 64, 64), device=DEV)
    y = torch.full((1, 64, 512), NAN, device=DEV)
    w = torch.zeros((7, 64, 64), device=DEV)
    before = lib.vfx_launch_count()
    with pytest.raises(_lib.VfxError, match="code -1"):
        ops.conv1d(x, w, None, y, 7, 7, 1, _lib.PAD_REFLECT)
    with pytest.raises(_lib.VfxError, match="code -1"):
        ops.conv1d(x, w[:, :, :48].contiguous(), None, y, 64, 7)              # Cout = 48
    with pytest.raises(_lib.VfxError, match="code -1"):
        ops.conv1d(x, w, None, y, 64, 4)                                      # even k
    with pytest.raises(_lib.VfxError, match="code -1"):
        ops.conv2d(x, w, None, y, 4, 4, 2)                                    # 2x2
    with pytest.raises(_lib.VfxError, match="code -2"):
        ops.conv1d(x[:, :, 1:33], w, None, y, 32, 7)                          # misaligned rows: VFX_EALIGN
    torch.cuda.synchronize()
    assert lib.vfx_launch_count() == before and torch.isnan(y).all()
    ops.conv1d(x, w, None, y, 8, 7, 1, _lib.PAD_REFLECT)
    torch.cuda.synchronize()
    assert lib.vfx_launch_count() > before and (y[:, :, :8] == 0).all() and torch.isnan(y[:, :, 8:]).all()
