"""packing.pack_wino32_tr: the channel-major row order of convtw_kernel's weight blob, [4 planes][Cin/8][s Cout][8] with row
c s + r = (channel c, output phase r).  Every element is checked against the F(3,2) weight transform of that phase and channel,
computed here in float64 and rounded once."""
import numpy as np
import pytest
import torch

from voicefixer_amd import packing

LANE_CI = (0, 2, 4, 6, 1, 3, 5, 7)   # pack_direct: position within a group of 8 input channels -> channel


@pytest.mark.parametrize("s", [2, 3, 7])
def test_wino32_tr_rows_are_channel_major(s):
    Cin, Cout = 24, 10
    g = torch.Generator().manual_seed(900 + s)
    w = torch.randn((Cin, Cout, 2 * s), generator=g)
    wp = packing.pack_convtr1d(w)                         # [2 s][Cin][Cout] tap slabs
    blob = packing.pack_wino32_tr(wp, s)
    assert blob.dtype == torch.float32 and blob.is_contiguous()
    assert tuple(blob.shape) == (4, Cin // 8, s * Cout, 8)
    got = blob.numpy()
    w64 = wp.double().numpy()
    for r in range(s):
        g0, g1 = w64[r + s], w64[r]                       # out[q s + r - pad] = g0 x[q - 1] + g1 x[q]
        U = [g0, (g0 + g1) * 0.5, (g0 - g1) * 0.5, g1]
        for k in range(4):
            want = U[k].astype(np.float32)                # [Cin][Cout], rounded once
            for grp in range(Cin // 8):
                for lane, ci in enumerate(LANE_CI):
                    np.testing.assert_array_equal(got[k, grp, r::s, lane], want[grp * 8 + ci],
                                                  err_msg="plane %d group %d phase %d lane %d" % (k, grp, r, lane))


def test_wino32_tr_taps_are_the_transposed_convolution():
    """The slabs pack_wino32_tr starts from: g1 = w[:, :, r], g0 = w[:, :, r + s] of the torch ConvTranspose1d weight."""
    s, Cin, Cout = 3, 8, 4
    w = torch.randn((Cin, Cout, 2 * s), generator=torch.Generator().manual_seed(5))
    blob = packing.pack_wino32_tr(packing.pack_convtr1d(w), s).numpy()
    for r in range(s):
        for c in range(Cout):
            for lane, ci in enumerate(LANE_CI):
                assert blob[0, 0, c * s + r, lane] == w[ci, c, r + s].item()
                assert blob[3, 0, c * s + r, lane] == w[ci, c, r].item()
