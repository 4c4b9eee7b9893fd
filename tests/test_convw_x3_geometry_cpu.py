"""The host rules of convw_kernel and conv_x3_kernel restated (voicefixer_amd/csrc/vfx_convw.inc: try_launch_convw,
try_launch_convw_2d, convw_setup; vfx_conv.hip: try_launch_x3, fill_phase, halo_fits), as tests/test_wg4_geometry_cpu.py restates
those of the Winograd family: what each takes and declines, the tile, the chunk depth kcx (codes 51 / 52 / 54), bl_step, the staging
mode, ROWS / NT, the 384-workgroup floor, the "<= 96 workgroups and K >= 1024" rule, the guard-interior checks and nph_fold.

``plan_convw`` / ``plan_x3`` return None for a launch the host declines and otherwise a record that names the template instance.
tests/test_convw_gpu.py and tests/test_conv_x3_gpu.py walk every case through them first and assert vfx_last_conv_tile() against
the record afterwards.  The CPU tests here pin the rules on hand-worked launches and establish which template instances no C-ABI
call can reach."""
import pytest

PRE_NONE, PRE_LRELU, PRE_AFFINE_LRELU = 0, 1, 2
MAXNXV, LDS_BUDGET, MAXNT = 6, 52 * 1024, 3
G_TILE = 264                 # engine.G_TILE: the guard band the engine adds to the largest tap offset


def up4(n):
    return (n + 3) // 4 * 4


def floor4(v):
    return v & ~3 if v >= 0 else -(((-v) + 3) & ~3)


def phases(op, k, step, pitch=0):
    """The tap tables of the entry points (vfx_conv1d_f32, vfx_convtr1d_f32, vfx_conv2d_f32): a list of phases, each
    ([(offset, slab), ...], output offset)."""
    if op == "conv1d":
        return [([((t - (k - 1) // 2) * step, t) for t in range(k)], 0)]
    if op == "convtr1d":
        pad = step // 2 + step % 2
        return [([(0, r), (-1, r + step)], r - pad) for r in range(step)]
    assert op == "conv2d"
    return [([((ky - k // 2) * pitch + (kx - k // 2), ky * k + kx) for ky in range(k) for kx in range(k)], 0)]


def extents(op, ext, step, pitch=0):
    """(Lin, Lq, Lout) of a launch: `ext` is L, Lin or the map's H."""
    if op == "convtr1d":
        return ext, ext + 1, step * ext
    n = ext * pitch if op == "conv2d" else ext
    return n, n, n


def span_of(taps):
    offs = [o for o, _ in taps]
    return min(offs), max(offs), max(offs) - min(offs)


def halo_fits(taps, BL):
    return BL + span_of(taps)[2] + 3 <= len(taps) * (BL + 3)


def fill_phase(taps, halo, exact, pitch):
    """fill_phase: (segment origins, LDS column of every tap, weight slab of every tap)."""
    mn = span_of(taps)[0]
    seg, lds = {}, []
    for t, (off, _) in enumerate(taps):
        frm = mn if halo else off
        org = frm if exact else floor4(frm)
        seg[0 if halo else t] = org
        lds.append((0 if halo else t * pitch) + off - org)
    return [seg[i] for i in sorted(seg)], lds, [s for _, s in taps]


def _affine(v):
    return all(v[i] - v[0] == i * (v[1] - v[0]) for i in range(2, len(v)))


# --------------------------------------------------------------------------------------
# convw_kernel
# --------------------------------------------------------------------------------------
def convw_setup(phs, cin, Lin, Lq, guard, BL, pre=PRE_NONE, pre_slope=0.0):
    """convw_setup for an unfused launch (halo_extra = 0, no fixed tile step): None = declined."""
    if cin % 8 or guard <= 0:
        return None
    if pre in (PRE_LRELU, PRE_AFFINE_LRELU) and not 0.0 <= pre_slope <= 1.0:
        return None
    nt = len(phs[0][0])
    if any(len(t) != nt for t, _ in phs):
        return None
    maxspan = max(span_of(t)[2] for t, _ in phs)
    all_segments = all(not halo_fits(t, BL) for t, _ in phs)
    shrink = 0 < maxspan <= 8
    exact = shrink or all_segments
    kcx = 32
    while True:
        if kcx < 8:
            return None
        if cin % kcx == 0:
            segw = 0
            for t, _ in phs:
                mn, _, sp = span_of(t)
                need = BL if exact else ((mn - floor4(mn)) + BL + sp if halo_fits(t, BL) else BL + 3)
                segw = max(segw, up4(need))
            tabs = [fill_phase(t, halo_fits(t, BL), exact, kcx * segw) for t, _ in phs]
            if not exact:
                segw = up4(BL + maxspan)
                if any(len(tb[0]) != 1 for tb in tabs):
                    segw = max(segw, up4(BL))
                tabs = [fill_phase(t, len(tb[0]) == 1, True, kcx * segw) for (t, _), tb in zip(phs, tabs)]
            maxseg = max(len(tb[0]) for tb in tabs)
            xs_floats = maxseg * kcx * segw
            nxv = (maxseg * kcx * (segw // 4) + 255) // 256
            if nxv <= MAXNXV and 2 * xs_floats * 4 <= LDS_BUDGET:
                break
        kcx >>= 1
    bl_step = BL - maxspan if shrink else BL
    ntiles = (Lq + bl_step - 1) // bl_step
    seg_mn = min(min(tb[0]) for tb in tabs)
    seg_mx = max(max(tb[0]) for tb in tabs)
    if -seg_mn > guard or (ntiles - 1) * bl_step + seg_mx + segw > Lin + guard:
        return None
    for tb in tabs[1:]:
        if tb[0] != tabs[0][0] or tb[1] != tabs[0][1]:
            return None
    if not all(_affine(tb[1]) and _affine(tb[2]) for tb in tabs) or not _affine(tabs[0][0]):
        return None
    if not _affine([tb[2][0] for tb in tabs]) or not _affine([o for _, o in phs]):
        return None
    if nt > 1 and any(tb[2][1] - tb[2][0] != tabs[0][2][1] - tabs[0][2][0] for tb in tabs):
        return None
    staging = "shrink" if shrink else ("segments" if maxseg > 1 else "halo")
    return dict(kcx=kcx, segw=segw, nxv=nxv, bl_step=bl_step, ntiles=ntiles, staging=staging, nseg=maxseg,
                lds=2 * xs_floats * 4 + 64)


def grid_x(ntiles):
    """convw_grid_x: (xcd_chunk, grid.x): linear below 64 tiles, else the XCD order on a grid rounded up to a multiple of 8."""
    if ntiles < 64:
        return 0, ntiles
    chunk = (ntiles + 7) // 8
    return chunk, 8 * chunk


def plan_convw(op, B, cin, cout, ext, k, step, guard, pitch=0, pre=PRE_NONE, pre_slope=0.0, offered=True):
    """try_launch_convw / try_launch_convw_2d: None = declined (the launch runs on conv_taps_kernel); else the instance."""
    if not offered:
        return None
    phs = phases(op, k, step, pitch)
    Lin, Lq, _ = extents(op, ext, step, pitch)
    nt = len(phs[0][0])
    if op == "conv2d":
        if k != 3 or cin % 8 or guard <= 0 or pre not in (PRE_NONE, PRE_AFFINE_LRELU):
            return None
        if cout % 128 == 0:
            BM, BL = 128, (64 if ((Lq + 127) // 128) * (cout // 128) * B < 768 else 128)
        elif cout % 64 == 0:
            BM, BL = 64, 128
        elif cout % 32 == 0:
            BM, BL = 32, 256
        else:
            return None
        ntiles, gy = (Lq + BL - 1) // BL, cout // BM
        if ntiles * gy * B < 384:
            return None
        segw = up4(BL + 2)
        nxv = (3 * 8 * (segw // 4) + 255) // 256
        if pitch + 1 > guard or (ntiles - 1) * BL + (pitch - 1) + segw > Lin + guard:
            return None
        chunk, gx = grid_x(ntiles)
        NXV = 4 if (BM, BL) == (128, 64) or nxv <= 4 else 7
        two_level = cin >= (256 if (BM, BL) == (128, 128) else 64)     # the instance with a second accumulator set (K = 9 Cin)
        return dict(code=59, BM=BM, BL=BL, NT=9, NXV=NXV, kcx=8, bl_step=BL, ntiles=ntiles, xcd_chunk=chunk, grid=(gx, gy, B),
                    nph_fold=0, staging="rows", two_level=two_level,
                    name="convw<%d,%d,NT9,NXV%d%s>" % (BM, BL, NXV, ",TWO_LEVEL" if two_level else ""))
    if pre == PRE_AFFINE_LRELU or nt < 2 or nt > MAXNT:
        return None
    if cout % 128 == 0:
        BM, BL = 128, 128
    elif cout % 64 == 0:
        BM, BL = 64, 256
    else:
        return None
    s = convw_setup(phs, cin, Lin, Lq, guard, BL, pre, pre_slope)
    if s is None:
        return None
    nph = len(phs)
    gy = nph * cout // BM
    if s["ntiles"] * gy * B < 384:
        return None
    chunk, gx = grid_x(s["ntiles"])
    fold = nph if nph > 1 and chunk > 0 else 0
    if fold:
        gx, gy = gx * nph, cout // BM
    NXV = 4 if s["nxv"] <= 4 else s["nxv"]
    return dict(s, code=50 + s["kcx"] // 8, BM=BM, BL=BL, NT=nt, NXV=NXV, xcd_chunk=chunk, grid=(gx, gy, B), nph_fold=fold,
                name="convw<%d,%d,NT%d,NXV%d>" % (BM, BL, nt, NXV))


# --------------------------------------------------------------------------------------
# conv_x3_kernel
# --------------------------------------------------------------------------------------
X3_INSTANCES = sorted(
    [(BM, BL, nt, mode, 1) for BM, BL in ((128, 128), (64, 256), (64, 128)) for nt in (1, 2, 3) for mode in (0, 1, 2)] +
    [(BM, BL, nt, 0, 3) for BM, BL in ((128, 128), (64, 256), (64, 128)) for nt in (1, 3)] +
    [(32, 256, 3, 0, 3), (32, 256, 1, 0, 1)])          # every conv_x3_kernel<BM, BL, .., NT, MODE, ROWS> try_launch_x3 names


def plan_x3(op, B, cin, cout, ext, k, step, guard, pitch=0, pre=PRE_NONE, reflect=False, rows=False, offered=True):
    """try_launch_x3: None = declined (the launch runs on the fp32 chain); else the instance."""
    if not offered or cin % 32 or cout % 32 or reflect or rows:
        return None
    phs = phases(op, k, step, pitch)
    Lin, Lq, _ = extents(op, ext, step, pitch)
    nph = len(phs)
    rws, P = 1, 0
    if nph == 1 and len(phs[0][0]) == 9:
        if pitch < 4:
            return None
        rws, P = 3, pitch
        phs = [([(t - 1, t) for t in range(3)], phs[0][1])]
    if rws == 1 and nph == 1 and len(phs[0][0]) == 3 and phs[0][0][2][0] > 60:       # (the entry point's k = 3 is always symmetric)
        rws, P = 3, phs[0][0][2][0]
        phs = [([(0, 0)], phs[0][1])]
    nt = len(phs[0][0])
    if nt < 1 or nt > 3 or any(len(t) != nt for t, _ in phs):
        return None
    span = max(span_of(t)[2] for t, _ in phs)
    seg_lo = min(span_of(t)[0] for t, _ in phs)
    seg_hi = max(span_of(t)[1] for t, _ in phs)
    mode = 0 if span <= 8 else (1 if span <= 120 else 2)
    if cout % 128 == 0:
        BM, BL = 128, 128
    elif cout % 64 == 0:
        BM, BL = (64, 256) if mode != 2 and Lq >= 4096 else (64, 128)
    else:
        if mode == 2:
            return None
        BM, BL = 32, 256
    segw = BL + span if mode == 1 else BL
    bl_eff = BL - span if mode == 0 else BL
    ntiles = (Lq + bl_eff - 1) // bl_eff
    rowspan = P if rws == 3 else 0
    if -seg_lo + rowspan > guard or (ntiles - 1) * bl_eff + seg_hi + BL + rowspan > Lin + guard:
        return None
    xplane = (nt if mode == 2 else 1) * segw * 32
    lds = 2 * (2 * xplane + nt * 2 * BM * 32) + (cin * 8 if pre == PRE_AFFINE_LRELU else 0)
    if lds > 160 * 1024:
        return None
    gy = nph * cout // BM
    if ntiles * gy * B <= 96 and cin * (9 if rws == 3 and nt == 3 else nt) >= 1024:
        return None
    if BM == 32 and not ((rws == 3 and nt == 3) or (rws == 1 and nt == 1 and mode == 0)):
        return None
    inst = (BM, BL, nt, mode, rws)
    assert inst in X3_INSTANCES, inst
    return dict(code=16, BM=BM, BL=BL, NT=nt, MODE=mode, ROWS=rws, bl_eff=bl_eff, ntiles=ntiles, grid=(ntiles, gy, B), lds=lds,
                instance=inst, name="x3<%d,%d,NT%d,MODE%d,ROWS%d>" % inst)


# --------------------------------------------------------------------------------------
# the rules on hand-worked launches
# --------------------------------------------------------------------------------------
def test_convw_tiles_chunk_depths_and_the_384_floor():
    g = G_TILE + 1
    p = plan_convw("conv1d", 4, 128, 128, 96 * 126, 3, 1, g)                     # 96 tiles x 4 rows = 384 workgroups
    assert (p["BM"], p["BL"], p["code"], p["bl_step"], p["staging"], p["ntiles"], p["xcd_chunk"]) == (128, 128, 54, 126, "shrink", 96, 12)
    assert plan_convw("conv1d", 4, 128, 128, 96 * 126 - 126, 3, 1, g) is None       # 95 x 4 = 380
    assert plan_convw("conv1d", 8, 64, 64, 48 * 254, 3, 1, g)["BL"] == 256 and plan_convw("conv1d", 8, 64, 96, 48 * 254, 3, 1, g) is None
    # chunk depths: the deepest of 32 / 16 / 8 that divides Cin and fits 6 staging slots and the 52 KB double buffer
    depth = {cin: plan_convw("conv1d", 8, cin, 128, 8192, 3, 1, g)["kcx"] for cin in (8, 24, 40, 64, 96)}
    assert depth == {8: 8, 24: 8, 40: 8, 64: 32, 96: 32}
    assert plan_convw("conv1d", 8, 48, 128, 8192, 3, 1, g)["code"] == 52 and plan_convw("conv1d", 8, 12, 128, 8192, 3, 1, g) is None
    # the shrink boundary: span 8 stages BL columns for BL - 8 outputs, span 10 a halo tile of BL + 10
    assert plan_convw("conv1d", 8, 64, 128, 8192, 3, 4, 4 + G_TILE)["bl_step"] == 120
    q = plan_convw("conv1d", 8, 64, 128, 8192, 3, 5, 5 + G_TILE)
    assert (q["bl_step"], q["staging"], q["segw"]) == (128, "halo", 140)
    # a wide halo costs chunk depth; past d = BL + 3 every tap stages its own segment
    assert plan_convw("conv1d", 8, 64, 128, 8192, 3, 81, 81 + G_TILE)["kcx"] == 16
    r = plan_convw("conv1d", 8, 64, 128, 8192, 3, 2187, 2187 + G_TILE)
    assert (r["staging"], r["nseg"], r["kcx"]) == ("segments", 3, 16)
    assert plan_convw("conv1d", 8, 64, 128, 8192, 5, 1, g) is None and plan_convw("conv1d", 8, 64, 128, 8192, 1, 1, g) is None
    assert plan_convw("conv1d", 8, 64, 128, 8192, 3, 1, g, pre=PRE_LRELU, pre_slope=1.5) is None
    assert plan_convw("conv1d", 8, 64, 128, 8192, 3, 1, g, pre=PRE_LRELU, pre_slope=-0.1) is None
    assert plan_convw("conv1d", 8, 64, 128, 8192, 3, 1, g, pre=PRE_AFFINE_LRELU, pre_slope=0.1) is None
    assert plan_convw("conv1d", 8, 64, 128, 8192, 3, 1, 0) is None


def test_convw_guard_one_short_of_interior_is_declined():
    L = 8192
    # d = 1: 66 tiles of 126 outputs; the last starts at 8190 and stages the 128 columns from 8189: 125 past the row's end
    assert plan_convw("conv1d", 8, 64, 128, L, 3, 1, 125) is not None and plan_convw("conv1d", 8, 64, 128, L, 3, 1, 124) is None
    # d = 27: 64 tiles of 128; the last stages up4(128 + 54) = 184 columns from 63 * 128 - 27: 29 past the end (the left side needs 27)
    need = 63 * 128 + (-27) + up4(128 + 54) - L                            # (ntiles - 1) bl_step + seg + segw - Lin
    assert need == 29
    assert plan_convw("conv1d", 8, 64, 128, L, 3, 27, need) is not None and plan_convw("conv1d", 8, 64, 128, L, 3, 27, need - 1) is None


def test_convw_transposed_phases_fold_from_64_tiles():
    for s in (2, 3, 7, 8):
        big = plan_convw("convtr1d", 8, 64, 128, 64 * 127 - 1, 2 * s, s, G_TILE)          # Lq = Lin + 1 = 64 tiles of 127
        assert (big["ntiles"], big["nph_fold"], big["grid"]) == (64, s, (64 * s, 1, 8)) and big["bl_step"] == 127 and big["NT"] == 2
        small = plan_convw("convtr1d", 64, 64, 128, 63 * 127 - 1, 2 * s, s, G_TILE)
        assert (small["ntiles"], small["nph_fold"], small["xcd_chunk"], small["grid"]) == (63, 0, 0, (63, s, 64))
    assert plan_convw("convtr1d", 64, 64, 128, 65 * 127 - 1, 4, 2, G_TILE)["grid"][0] == 72 * 2      # 65 tiles: a grid of 72, seven idle


def test_convw_2d_tiles():
    g = 64 + 1 + G_TILE
    assert plan_convw("conv2d", 32, 64, 128, 512, 3, 1, g, pitch=64)["name"] == "convw<128,128,NT9,NXV4>"
    assert plan_convw("conv2d", 32, 256, 128, 512, 3, 1, g, pitch=64)["name"] == "convw<128,128,NT9,NXV4,TWO_LEVEL>"
    assert plan_convw("conv2d", 2, 64, 128, 512, 3, 1, g, pitch=64)["name"] == "convw<128,64,NT9,NXV4,TWO_LEVEL>"    # 512 < 768 at 128 wide
    assert plan_convw("conv2d", 2, 56, 128, 512, 3, 1, g, pitch=64)["name"] == "convw<128,64,NT9,NXV4>"
    assert plan_convw("conv2d", 3, 64, 128, 512, 3, 1, g, pitch=64)["BL"] == 128                               # 768
    assert plan_convw("conv2d", 4, 32, 64, 512, 3, 1, g, pitch=64)["name"] == "convw<64,128,NT9,NXV4>"
    assert plan_convw("conv2d", 4, 64, 64, 512, 3, 1, g, pitch=64)["name"] == "convw<64,128,NT9,NXV4,TWO_LEVEL>"
    assert plan_convw("conv2d", 4, 8, 32, 512, 3, 1, g, pitch=64)["name"] == "convw<32,256,NT9,NXV7>"
    assert plan_convw("conv2d", 1, 64, 128, 128, 3, 1, g, pitch=64) is None                                    # 128 workgroups of 128 x 64
    assert plan_convw("conv2d", 32, 64, 128, 512, 3, 1, 64, pitch=64) is None                                  # guard < P + 1
    assert plan_convw("conv2d", 32, 64, 128, 512, 3, 1, g, pitch=64, pre=PRE_LRELU, pre_slope=0.01) is None
    assert plan_convw("conv2d", 32, 64, 128, 512, 1, 1, g, pitch=64) is None


def test_x3_tiles_modes_and_the_small_launch_rule():
    g = G_TILE
    assert plan_x3("conv1d", 2, 64, 128, 1000, 3, 4, 4 + g)["name"] == "x3<128,128,NT3,MODE0,ROWS1>"
    assert plan_x3("conv1d", 2, 64, 128, 1000, 3, 5, 5 + g)["name"] == "x3<128,128,NT3,MODE1,ROWS1>"
    assert plan_x3("conv1d", 2, 64, 128, 1000, 3, 60, 60 + g)["MODE"] == 1
    assert plan_x3("conv1d", 2, 64, 128, 1000, 3, 61, 61 + g)["name"] == "x3<128,128,NT1,MODE0,ROWS3>"        # one tap per K-step
    assert plan_x3("conv1d", 1, 64, 64, 4096, 3, 1, 1 + g)["BL"] == 256 and plan_x3("conv1d", 1, 64, 64, 4095, 3, 1, 1 + g)["BL"] == 128
    assert plan_x3("conv1d", 2, 64, 32, 1000, 1, 1, g)["name"] == "x3<32,256,NT1,MODE0,ROWS1>"
    assert plan_x3("conv1d", 2, 64, 32, 1000, 3, 1, 1 + g) is None and plan_x3("convtr1d", 2, 64, 32, 1000, 4, 2, g) is None
    assert plan_x3("conv2d", 2, 64, 32, 8, 3, 1, 5 + g, pitch=4)["name"] == "x3<32,256,NT3,MODE0,ROWS3>"
    assert plan_x3("conv2d", 2, 64, 64, 8, 3, 1, 3 + g, pitch=2) is None
    assert plan_x3("conv1d", 2, 48, 64, 1000, 3, 1, 1 + g) is None and plan_x3("conv1d", 2, 64, 64, 1000, 3, 1, 1 + g, rows=True) is None
    assert plan_x3("conv1d", 2, 64, 64, 1000, 7, 1, 3 + g) is None and plan_x3("conv1d", 2, 64, 64, 1000, 3, 1, 0) is None
    # <= 96 workgroups and K >= 1024: declined; either side of each
    assert plan_x3("conv1d", 1, 352, 128, 96 * 126, 3, 1, 1 + g) is None and plan_x3("conv1d", 1, 352, 128, 96 * 126 + 1, 3, 1, 1 + g) is not None
    assert plan_x3("conv1d", 1, 320, 128, 96 * 126, 3, 1, 1 + g) is not None                                   # K = 960
    # the affine pre-activation's table counts against the 160 KB of LDS
    assert plan_x3("conv2d", 32, 2048, 128, 64, 3, 1, 9 + g, pitch=8, pre=PRE_AFFINE_LRELU)["lds"] == 65536 + 2048 * 8
    assert plan_x3("conv2d", 32, 12288, 128, 64, 3, 1, 9 + g, pitch=8, pre=PRE_AFFINE_LRELU)["lds"] == 160 * 1024
    assert plan_x3("conv2d", 32, 12320, 128, 64, 3, 1, 9 + g, pitch=8, pre=PRE_AFFINE_LRELU) is None
    assert plan_x3("conv2d", 32, 12320, 128, 64, 3, 1, 9 + g, pitch=8) is not None


def test_x3_guard_one_short_is_declined():
    assert plan_x3("conv1d", 2, 64, 128, 1000, 3, 9, 9) is None            # the last tile's BL + span columns pass Lin + guard
    need = 7 * 128 + 9 + 128 - 1000
    assert plan_x3("conv1d", 2, 64, 128, 1000, 3, 9, need) is not None and plan_x3("conv1d", 2, 64, 128, 1000, 3, 9, need - 1) is None


def test_x3_instances_no_call_can_reach():
    """Sweep every geometry the three entry points can hand try_launch_x3 (k = 1 .. 7 odd at dilations to 3000, transposed strides
    1 .. 16, 1x1 and 3x3 at every pitch, the three Cout classes, Lq on both sides of 4096) with a guard that makes every tile
    interior: the template instances that are never named are unreachable through the C ABI.  They are all of MODE 2 (a symmetric
    k = 3 with d > 60 takes the one-tap-per-step path first, and nothing else with nt <= 3 has a span above 120), the NT = 2 halo
    mode 1 (a transposed phase's two taps are one position apart) and NT = 1 with a halo."""
    seen = set()
    big = 1 << 20
    for cout in (32, 64, 128):
        for L in (1000, 5000):
            for k in (1, 3, 5, 7):
                for d in list(range(1, 140)) + [243, 729, 2187, 3000]:
                    p = plan_x3("conv1d", 4, 64, cout, L, k, d, big)
                    seen |= {p["instance"]} if p else set()
            for s in range(1, 17):
                p = plan_x3("convtr1d", 4, 64, cout, L, 2 * s, s, big)
                seen |= {p["instance"]} if p else set()
            for lp in range(1, 8):
                for k in (1, 3):
                    p = plan_x3("conv2d", 4, 64, cout, max(1, L >> lp), k, 1, big, pitch=1 << lp)
                    seen |= {p["instance"]} if p else set()
    unreached = [i for i in X3_INSTANCES if i not in seen]
    assert all(i[3] == 2 or (i[2] == 2 and i[3] == 1) or (i[2] == 1 and i[3] == 1 and i[4] == 1) for i in unreached), unreached
    assert {i for i in X3_INSTANCES if i[3] == 2} <= set(unreached), "a MODE 2 instance is reachable: test it"
    assert len(unreached) == 15 and len(seen) == len(X3_INSTANCES) - 15, (sorted(seen), unreached)
