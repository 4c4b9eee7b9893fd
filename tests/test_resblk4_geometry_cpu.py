"""The tile geometry of resblk4_kernel and resblk4s_kernel (voicefixer_amd/csrc/vfx_resblk4.inc, vfx_resblk4s.inc) as a plain
Python model, written from the kernels' own comments and host code.

Both kernels address x, y and the weights through buffer resources with num_records = 0x7fffffff: an index error is not
clipped, it reads or writes outside the allocation.  So the index arithmetic is stated once here -- the host's choice of
kernel and strip pitch (``takes``, ``block_geometry``, ``strip_geometry``, ``grid_x``), a tile's first-half quads, where
their outputs go in the LDS tile Y, and which output quads the second half owns (``tile``) -- and ``check(d, L)`` walks every
workgroup of a launch and asserts:

* every output position in [0, L) is stored by exactly one (tile, quad lane, element), and no store (or residual load: the
  same offsets) lies outside [0, L);
* every Y column written or read, by any lane, is below the row pitch yp = 260;
* every quad that stores anything reads six Y columns that the first half of the SAME tile wrote, and they hold the
  positions qq - 1 .. qq + 4 (a stale column would enter all four outputs of the quad through B^T d);
* the XCD-aware tile order visits every tile exactly once, and fast_div is exact wherever the kernels use it.

tests/test_resblk4_gpu.py launches a (d, L) only after ``check`` has passed it.
"""
import numpy as np
import pytest

YP = 260                       # resblk4_fill_args: a.yp


# --------------------------------------------------------------------------------------
# the host side
# --------------------------------------------------------------------------------------
def takes(d):
    """resblk4_takes: the block tile takes a dilation whose blocks of 4d positions fill a 256-column tile."""
    nb = 256 // (4 * d)
    return d <= 32 and nb >= 1 and nb * d >= 48


def block_geometry(d):
    nb = 256 // (4 * d)
    W = 4 * d * nb
    nq2 = (W - 2) // 4
    return dict(strip=False, d=d, nb=nb, W=W, nq1=nb * d, nq2=nq2, bl_step=4 * nq2)


def strip_geometry(d):
    nseg_of = lambda P: (d + P - 5) // (P - 4)
    pshift = 5 if 32 * nseg_of(32) < 64 * nseg_of(64) else 6
    P = 1 << pshift
    return dict(strip=True, d=d, pshift=pshift, P=P, W=P - 4, nseg=nseg_of(P), G=64 >> pshift)


def geometry(d):
    """What vfx_resblock_wino4_f32 launches at this dilation."""
    return block_geometry(d) if takes(d) else strip_geometry(d)


def ntiles_of(g, L):
    if not g["strip"]:
        return (L + g["bl_step"] - 1) // g["bl_step"]
    nblk = (L + 4 * g["d"] - 1) // (4 * g["d"])
    return (nblk * g["nseg"] + g["G"] - 1) // g["G"]


def grid_x(ntiles):
    """convw_grid_x: (grid.x, xcd_chunk); fewer than 64 tiles run in linear order."""
    if ntiles < 64:
        return ntiles, 0
    chunk = (ntiles + 7) // 8
    return 8 * chunk, chunk


def code_of(d):
    return 97 if geometry(d)["strip"] else 96


# --------------------------------------------------------------------------------------
# the device side
# --------------------------------------------------------------------------------------
def fast_div(i, d):
    """fast_div of vfx_conv.hip in fp32, asserted exact (the kernels rely on it for 0 <= i < 2^20, 0 < d < 2^12)."""
    i = np.asarray(i, dtype=np.int64)
    assert (i >= 0).all() and (i < 1 << 20).all() and 0 < d < 1 << 12
    inv = np.float32(1.0) / np.float32(d)
    q = (i.astype(np.float32) * inv).astype(np.int64)
    q = np.where(q * d > i, q - 1, q)
    q = np.where((q + 1) * d <= i, q + 1, q)
    assert (q == i // d).all()
    return q


def tile(g, Lrow, bx):
    """One workgroup.  None when it returns at once; else a dict of per-lane arrays (64 quad lanes):
    first half: p0 (position of output 0 of the quad), qok, col0 (its Y column), ystep; second half: qq, nown, yc2."""
    d, Q = g["d"], np.arange(64)
    if g["strip"]:
        pshift, P, W, nseg = g["pshift"], g["P"], g["W"], g["nseg"]
        n = (bx << (6 - pshift)) + np.arange(2)
        blk = fast_div(n, nseg)
        sr0 = (n - blk * nseg) * W
        sstart = 4 * d * blk + sr0
        if sstart[0] >= Lrow:
            return None
        seg, j = Q >> pshift, Q & (P - 1)
        p0, qok, col0, ystep = sstart[seg] - 1 + j, j < P - 2, (seg << (pshift + 2)) + j, P
        nq2s = W >> 2
        t = fast_div(Q, nq2s)
        jq = Q - t * nq2s
        sok = t < (4 << (6 - pshift))
        t = np.where(sok, t, 0)
        rr = sr0[t >> 2] + 4 * jq
        qq = sstart[t >> 2] + (t & 3) * d + 4 * jq
        nown = np.where(sok, np.minimum(Lrow - qq, d - rr), 0)
        yc2 = (t << pshift) + 4 * jq
    else:
        q0 = bx * g["bl_step"]
        if q0 >= Lrow:
            return None
        blk = fast_div(Q, d)
        u0 = 4 * d * blk + (Q - blk * d)
        p0, qok, col0, ystep = q0 - 1 + u0, Q < g["nq1"], u0, d
        qend = min(Lrow, q0 + g["bl_step"])
        qq, nown, yc2 = q0 + 4 * Q, qend - (q0 + 4 * Q), 4 * Q
    return dict(p0=p0, qok=qok, col0=col0, ystep=ystep, qq=qq, nown=nown, yc2=yc2)


def check(d, L, Lrow=None):
    """Walk every workgroup of a launch of capacity L on a row of Lrow <= L positions and assert the invariants of the
    module docstring.  Returns (tiles, tiles that did work, tiles with a partly owned quad)."""
    Lrow = L if Lrow is None else Lrow
    assert 1 <= Lrow <= L and d >= 1
    g = geometry(d)
    if g["strip"]:
        assert g["P"] in (32, 64) and g["G"] * g["P"] == 64 and (g["nseg"] - 1) * g["W"] < d <= g["nseg"] * g["W"]
        other = 96 - g["P"]
        assert g["nseg"] * g["P"] <= ((d + other - 5) // (other - 4)) * other, "the pitch with fewer quad columns per block"
        assert 4 * g["G"] * g["P"] <= 256 < YP and g["nseg"] < 1 << 12
        assert ntiles_of(g, L) * g["G"] < 1 << 20, "the host declines (fast_div's range)"
    else:
        assert 48 <= g["nq1"] <= 64 and g["W"] <= 256 < YP and g["bl_step"] % 4 == 0 and 0 < g["bl_step"] <= g["W"] - 2
    ntiles = ntiles_of(g, L)
    gx, chunk = grid_x(ntiles)
    raw = np.arange(gx)
    order = (raw & 7) * chunk + (raw >> 3) if chunk else raw
    order = order[order < ntiles]                       # the early return bx >= ntiles_l
    assert np.array_equal(np.sort(order), np.arange(ntiles)), "every tile exactly once"
    owners = np.zeros(Lrow, dtype=np.int64)
    worked = tails = 0
    for bx in range(ntiles):
        t = tile(g, Lrow, bx)
        if t is None:
            continue
        worked += 1
        # ---- first half: taps, Y writes
        qok = t["qok"]
        # (tap loads are masked to [0, Lrow) position by position in the kernel itself: nothing to model)
        ycols = (t["col0"][qok, None] + t["ystep"] * np.arange(4)).ravel()
        ypos = (t["p0"][qok, None] + d * np.arange(4)).ravel()
        assert ycols.min() >= 0 and ycols.max() < YP, "a Y column written at or past the row pitch"
        assert np.unique(ycols).size == ycols.size, "two first-half outputs share a Y column"
        holds = np.full(YP, np.iinfo(np.int64).min)
        holds[ycols] = ypos
        # ---- second half: Y reads of every lane, ownership, stores
        assert t["yc2"].min() >= 0 and t["yc2"].max() + 5 < YP, "a Y column read at or past the row pitch"
        nown, qq = t["nown"], t["qq"]
        own = nown > 0
        reads = t["yc2"][own, None] + np.arange(6)
        assert np.array_equal(holds[reads], qq[own, None] - 1 + np.arange(6)), \
            "an owned quad reads Y columns its own tile's first half did not write for those positions"
        cnt = np.minimum(nown[own], 4)
        tails += bool((cnt < 4).any())
        pos = np.concatenate([q + np.arange(c) for q, c in zip(qq[own], cnt)]) if own.any() else np.zeros(0, dtype=np.int64)
        assert pos.size == 0 or (pos.min() >= 0 and pos.max() < Lrow), "a store outside [0, L)"
        np.add.at(owners, pos, 1)
    assert (owners == 1).all(), "positions stored %s times: %r" % ("0 or 2+", np.nonzero(owners != 1)[0][:8])
    return ntiles, worked, tails


# --------------------------------------------------------------------------------------
# the lengths tests/test_resblk4_gpu.py launches, stated once
# --------------------------------------------------------------------------------------
def case_length(d):
    """test_case_parity.  Block tile: two whole tiles and a third that ends inside a quad.  Strip tile: one whole block of
    4d positions, then a second cut inside strip 1, part-way through a segment."""
    g = geometry(d)
    return 5 * d + g["W"] + 3 if g["strip"] else 2 * g["bl_step"] + 23


def ragged_lengths(d, L):
    return [L, 1, max(2, d - 1), d + 13, 4 * d, 4 * d + 1]


def edge_lengths(d):
    g = geometry(d)
    ls = {1, 2, 3, 4, 5, d - 1, d, d + 1, 4 * d - 1, 4 * d, 4 * d + 1}
    if g["strip"]:
        ls |= {4 * d + g["W"] - 1, 4 * d + g["W"], 4 * d + g["W"] + 1}
    else:
        ls |= {g["bl_step"] - 1, g["bl_step"], g["bl_step"] + 1}
    return sorted(n for n in ls if n >= 1)


DILATIONS = list(range(1, 257)) + [243, 729, 2187, 4096]


@pytest.mark.parametrize("d", sorted(set(DILATIONS)))
def test_every_tile_of_every_length(d):
    L = case_length(d)
    lengths = sorted(set(edge_lengths(d) + [L] + ragged_lengths(d, L)))
    for n in lengths:
        nt, worked, _ = check(d, n)
        assert 1 <= worked <= nt        # (strip tile: the last block's segments past the end return at once)
    cap = max(lengths)
    for n in lengths:                                   # the same rows inside a ragged launch of the largest capacity
        check(d, cap, n)


XCD_LENGTHS = {1: (252 * 63, 252 * 70 + 5, 252 * 72), 81: (4 * 81 * 40, 4 * 81 * 44, 4 * 81 * 48)}     # tests/test_resblk4_gpu.py launches these


@pytest.mark.parametrize("d", sorted(XCD_LENGTHS))
def test_xcd_tile_order(d):
    """Fewer than 64 tiles run in linear order; 64 and more are spread over the XCDs, with the early return when the
    count is no multiple of 8 (d = 81: P = 32, two segments per tile, three per block: 60, 66 and 72 tiles)."""
    g = geometry(d)
    nts = [ntiles_of(g, L) for L in XCD_LENGTHS[d]]
    assert nts[0] < 64 <= nts[1] and nts[1] % 8 != 0 and nts[2] >= 64 and nts[2] % 8 == 0, nts
    assert [grid_x(n)[1] > 0 for n in nts] == [False, True, True] and grid_x(nts[1])[0] > nts[1]
    for L in XCD_LENGTHS[d]:
        check(d, L)
        check(d, L, L // 2 + 1)


def test_the_host_rule():
    """resblk4_takes and the strip-pitch choice, restated: the stage's dilations, the dilations on either side of every change
    the GPU edges name, and both pitches."""
    assert [d for d in range(1, 40) if not takes(d)] == [22, 23] + list(range(33, 40))
    assert [code_of(3 ** i) for i in range(8)] == [96] * 4 + [97] * 4
    assert [block_geometry(d)["bl_step"] for d in (1, 3, 9, 27)] == [252, 248, 248, 212]
    assert sorted({block_geometry(d)["nb"] for d in (1, 2, 5, 7, 12, 13, 16, 17, 21, 24, 32)}) == [2, 3, 4, 5, 9, 12, 32, 64]
    assert [(strip_geometry(d)["P"], strip_geometry(d)["nseg"]) for d in (81, 243, 729, 2187)] == [(32, 3), (32, 9), (64, 13), (64, 37)]
    for a, b in ((28, 29), (60, 61), (84, 85), (120, 121)):
        ga, gb = strip_geometry(a), strip_geometry(b)
        assert ga["P"] != gb["P"], (a, b)
    # (at 56 | 57 the 28-wide segments go from two to three per block; P = 64 is chosen on both sides)
    assert [(strip_geometry(d)["P"], strip_geometry(d)["nseg"]) for d in (56, 57)] == [(64, 1), (64, 1)]
    assert {strip_geometry(d)["P"] for d in (22, 23, 33, 64, 100, 4096)} == {32, 64}


def test_the_model_notices_a_broken_tile():
    """The model is not vacuous: a tile step one quad too long, a strip segment one quad too wide and a pitch of Y one
    column too small each break an invariant."""
    g = block_geometry(3)
    bad = dict(g, bl_step=g["bl_step"] + 4)
    t = tile(bad, 1000, 0)
    own = t["nown"] > 0
    assert (t["yc2"][own] + 5).max() >= g["W"]          # the last owned quad reads past the columns the first half wrote
    global YP
    keep = YP
    try:
        YP = 253
        with pytest.raises(AssertionError):
            check(81, 1000)
    finally:
        YP = keep
    check(81, 1000)
