"""The host side and the index arithmetic of the stand-alone Winograd F(4,3) convolutions -- convwg4_kernel, convwg4p_kernel
and convwg4x_kernel (voicefixer_amd/csrc/vfx_convwg.inc, vfx_convwg4p.inc, vfx_convwg4x.inc; vfx_last_conv_tile() % 100 == 80,
81, 82) -- as a plain Python model, written from the host code (try_launch_convwg4 / 4p / 4x) and the kernels' own comments.

All three kernels address x, y, the residual and the weights through buffer resources with num_records = 0x7fffffff (the
trickle of convwg4x_kernel's D1 instances: one row): an index error is not clipped, it reads or writes outside the
allocation.  So what tests/test_wg4_gpu.py relies on is stated once here:

* ``dispatch`` -- which kernel a launch runs on (the quad count, the tile counts of both tile shapes, the 512-workgroup
  minimum, the two persistent thresholds N >= 4 nwg, ``xcd_chunk``) and which instance (SPEC 0 / 1 / 2, D1);
* ``work_items`` -- the work list of the persistent kernels, n = xcd * chunk + jw + k * per, and the XCD-folded grid of
  convwg4_kernel;
* ``check`` -- walks a launch and asserts that every (batch item, tile, channel block) is visited exactly once, that a
  workgroup's channel block never changes, that every output position in [0, len_b) of every row is stored by exactly one
  (tile, quad lane, output index) and none outside it, that every element a valid lane loads or stores lies inside
  [0, up4(L)) of its row -- the view the test allocates, guards not counted -- that every byte offset fits 31 bits, and that
  fast_div is exact wherever the kernels use it.

The tables of tests/test_wg4_gpu.py (``CASES``, ``EDGES``, the exact-property launches) live here, so that this module proves
every one of them without a GPU; the GPU module launches a spec only after ``check`` has passed it and asserts the kernel
code ``dispatch`` gives.
"""
import functools

import numpy as np
import pytest

PRE_NONE, PRE_LRELU = 0, 1
POST_NONE, POST_LRELU, POST_ELU, POST_SNAKE = 0, 1, 2, 5
POST_NAMES = {POST_NONE: "none", POST_LRELU: "lrelu", POST_ELU: "elu", POST_SNAKE: "snake"}
CUS = 256                      # compute units of an MI355X; the GPU module reads the device's own count and passes it in
G_TILE, G_DIL4 = 264, 2452     # engine.G_TILE; engine.G_DIL rounded up to 4: the guards of a stage's ys / xs


def up4(n):
    return (n + 3) // 4 * 4


def cdiv(a, b):
    return (a + b - 1) // b


# --------------------------------------------------------------------------------------
# the host side
# --------------------------------------------------------------------------------------
def grid_x(ntiles):
    """convw_grid_x: (grid.x, xcd_chunk); fewer than 64 tiles run in linear order."""
    if ntiles < 64:
        return ntiles, 0
    chunk = cdiv(ntiles, 8)
    return 8 * chunk, chunk


def persistent(N, gy, nwg_all):
    """The common tail of try_launch_convwg4p / 4x: (nwg, xcd_chunk), or None when the launch is too short."""
    nwg = nwg_all - nwg_all % (8 * gy)
    if N >= 1 << 30 or nwg < 8 * gy or N < 4 * nwg:
        return None
    chunk = cdiv(cdiv(N, 8), gy) * gy
    return nwg, chunk


def dispatch(B, cin, cout, L, d, pre=PRE_NONE, post=POST_NONE, res=False, pre_slope=0.01, post_slope=0.0, vec_ok=True, cus=CUS):
    """try_launch_convwg4 and what it tries first: None when the family declines the launch (it then runs on another kernel),
    else the launch: code 82 / 81 / 80, tile (BM channels x BQ quads), tiles per row, channel blocks gy, instance."""
    if cin % 32 or cout % 64 or d < 1:
        return None
    if pre not in (PRE_NONE, PRE_LRELU) or (pre == PRE_LRELU and not 0.0 <= pre_slope <= 1.0):
        return None
    if post == POST_LRELU and not 0.0 <= post_slope <= 1.0:
        return None
    nquads = cdiv(L, 4 * d) * d
    wide = cout % 128 == 0
    BQ = 32 if wide else 64
    ntiles = cdiv(nquads, BQ)
    gy = cout // (128 if wide else 64)
    if ntiles * gy * B < 512:
        return None
    d1vec = d == 1 and vec_ok
    first = not res and pre == PRE_LRELU and post == POST_LRELU
    second = d1vec and res and pre == PRE_NONE and post == POST_NONE
    common = dict(B=B, cin=cin, cout=cout, L=L, d=d, d1=d1vec, gy=gy, res=res, spec=1 if first else (2 if second else 0))
    if wide and (first or second) and cin // 8 >= 8 and (cin // 8) % 2 == 0:
        nt = cdiv(nquads, 64)
        p = persistent(B * nt * gy, gy, cus)
        if p:
            return dict(common, code=82, BM=128, BQ=64, KC=8, ntiles=nt, N=B * nt * gy, nwg=p[0], chunk=p[1])
    if (first or second) and cin // 16 >= 4 and (cin // 16) % 2 == 0:
        p = persistent(B * ntiles * gy, gy, 2 * cus)
        if p:
            return dict(common, code=81, BM=128 if wide else 64, BQ=BQ, KC=16, ntiles=ntiles, N=B * ntiles * gy, nwg=p[0], chunk=p[1])
    gx, chunk = grid_x(ntiles)
    return dict(common, code=80, BM=128 if wide else 64, BQ=BQ, KC=16, ntiles=ntiles, N=B * ntiles * gy, gx=gx, chunk=chunk)


# --------------------------------------------------------------------------------------
# the device side
# --------------------------------------------------------------------------------------
def fast_div(i, d, inv=None):
    """fast_div of vfx_conv.hip in fp32, asserted exact for the arguments it is given here (the kernels call it with quad
    indices and with Lrow + 4d - 1 over 4d, whose reciprocal they form as 0.25f * (1.0f / d))."""
    i = np.asarray(i, dtype=np.int64)
    inv = np.float32(1.0) / np.float32(d) if inv is None else inv
    q = (i.astype(np.float32) * np.float32(inv)).astype(np.int64)
    q = np.where(q * d > i, q - 1, q)
    q = np.where((q + 1) * d <= i, q + 1, q)
    assert (q == i // d).all(), "fast_div is off"
    return q


def work_items(g):
    """Every (work item n, channel block) the launch's workgroups visit, as two arrays (any order)."""
    gy = g["gy"]
    if g["code"] == 80:
        nt, B = g["ntiles"], g["B"]
        if g["chunk"] and gy > 1:                 # convwg_fold_blocks: grid (gx * gy, 1, B)
            bx = np.arange(g["gx"] * gy)
            k = bx >> 3
            t = k // gy
            mblk, tile = k - t * gy, (bx & 7) * g["chunk"] + t
        else:                                     # grid (gx, gy, B)
            bx, mblk = (a.ravel() for a in np.meshgrid(np.arange(g["gx"]), np.arange(gy), indexing="ij"))
            tile = (bx & 7) * g["chunk"] + (bx >> 3) if g["chunk"] else bx
        ok = tile < nt                            # the early return bx >= ntiles_l
        tile, mblk = tile[ok], mblk[ok]
        b = np.repeat(np.arange(B), tile.size)
        return (np.tile(tile, B) + b * nt) * gy + np.tile(mblk, B), np.tile(mblk, B)
    nwg, chunk, N = g["nwg"], g["chunk"], g["N"]
    assert nwg % (8 * gy) == 0 and chunk % gy == 0 and 8 * chunk >= N
    per = nwg >> 3
    ns, ms = [], []
    for wg in range(nwg):
        xcd, jw = wg & 7, wg >> 3
        nend = min(N, (xcd + 1) * chunk)
        n = np.arange(xcd * chunk + jw, max(nend, xcd * chunk + jw), per)
        assert ((n % gy) == jw % gy).all(), "a workgroup's channel block changes along its list"
        ns.append(n)
        ms.append(np.full(n.size, jw % gy))
    return np.concatenate(ns), np.concatenate(ms)


def row_walk(g, L, Lrow):
    """One row of `Lrow` positions in a launch of capacity L: the positions every valid tile stores (with multiplicity) and the
    largest x element any of its lanes loads.  Tiles at or past nblk * d quads are skipped (`valid_` / the early return)."""
    d, BQ, nt = g["d"], g["BQ"], g["ntiles"]
    inv4 = np.float32(0.25) * (np.float32(1.0) / np.float32(d))
    nblk = int(fast_div([Lrow + 4 * d - 1], 4 * d, inv4)[0])
    Q = np.arange(nt * BQ)
    valid = (Q // BQ) * BQ < nblk * d
    Q = Q[valid]
    if g["d1"] or d == 1:
        q = 4 * Q
    else:
        blk = fast_div(Q, d)
        q = 4 * d * blk + (Q - blk * d)
    pos = q[:, None] + d * np.arange(4)
    stored = pos[pos < Lrow]
    taps = q[:, None] + d * np.arange(-1, 5)
    loaded = taps[(taps >= 0) & (taps < Lrow)]
    xmax = int(loaded.max()) if loaded.size else -1
    if g["d1"]:                                   # the aligned 16-byte vector x[4Q .. 4Q + 3], loaded when its first element is in the row
        first = q[q < Lrow]
        xmax = max(xmax, int(first.max()) + 3 if first.size else -1)
    return stored, xmax, int(valid.sum()) // BQ


def check(spec, cus=CUS):
    """Walk the launch of `spec` (a dict as ``make_spec`` returns) and assert the invariants of the module docstring.  Returns
    the dispatch record."""
    B, L, d = spec["B"], spec["L"], spec["d"]
    lens = spec["lengths"] if spec["lengths"] is not None else [L] * B
    assert len(lens) == B and max(lens) <= L and min(lens) >= 1
    g = dispatch(B, spec["cin"], spec["cout"], L, d, spec["pre"], spec["post"], spec["res"] != "none", spec["pre_slope"],
                 spec["post_slope"], spec["vec_ok"], cus)
    assert g is not None, "the Winograd F(4,3) family declines this launch"
    n, mblk = work_items(g)
    assert n.size == g["N"] and np.array_equal(np.sort(n), np.arange(g["N"])), "every (batch item, tile, channel block) exactly once"
    assert np.array_equal(n % g["gy"], mblk) and mblk.max() * g["BM"] + g["BM"] <= spec["cout"]
    u = n // g["gy"]
    assert (u // g["ntiles"]).max() < B           # (the batch item x_rows[] is read for)
    assert g["ntiles"] * g["BQ"] + 64 < 1 << 20
    Lp = up4(L)
    for Lrow in sorted(set(lens)):
        stored, xmax, worked = row_walk(g, L, Lrow)
        assert worked >= 1
        assert stored.size == Lrow and np.array_equal(np.sort(stored), np.arange(Lrow)), "every position of the row stored exactly once"
        assert xmax < Lp, "a tap load past the row's allocation"
    # byte offsets: one batch item through 32-bit offsets (offsets_fit31 on the host), rows inside their views
    for cn, guard, wpad in ((spec["cin"], spec["x_guard"], 0), (spec["cout"], spec["y_guard"], spec["y_wpad"]),
                            (spec["cout"], spec["r_guard"], spec["r_wpad"])):
        cs = up4(guard) + Lp + up4(guard) + wpad
        assert (cn * cs + L) * 4 < (1 << 31) - (1 << 21)
    assert 6 * (spec["cin"] // 8) * spec["cout"] * 32 < (1 << 31) - (1 << 21)
    assert spec["cin"] % g["KC"] == 0 and (spec["cin"] // g["KC"]) % 2 == 0      # whole chunks, in pairs
    return g


# --------------------------------------------------------------------------------------
# the launches of tests/test_wg4_gpu.py, stated once
# --------------------------------------------------------------------------------------
def make_spec(cin, cout, d, L, B, pre=PRE_NONE, post=POST_NONE, post_slope=0.0, pre_slope=0.01, bias=True, res="none", lengths=None,
              heavy=False, x_guard=None, y_guard=None, r_guard=G_TILE, y_wpad=0, r_wpad=0, y_cpad=0, r_cpad=0, vec_ok=True, w_scale=1.0):
    """One launch.  res: "none", "in place" (res is y) or "separate".  Guards default to the engine's: the first convolution of
    a layer reads xs (guard G_DIL) and writes ys (G_TILE), the second reads ys and updates xs in place."""
    assert res in ("none", "in place", "separate")
    if x_guard is None:
        x_guard = G_TILE if res != "none" else G_DIL4
    if y_guard is None:
        y_guard = G_DIL4 if res == "in place" else G_TILE
    if lengths is not None:
        assert len(lengths) == B and lengths[0] == L and max(lengths) == L, "row 0 fills the capacity"
    if res == "in place":
        r_guard, r_wpad, r_cpad = y_guard, y_wpad, y_cpad
    return dict(cin=cin, cout=cout, d=d, L=L, B=B, pre=pre, pre_slope=pre_slope if pre == PRE_LRELU else 0.0, post=post,
                post_slope=post_slope, bias=bias, res=res, lengths=lengths, heavy=heavy, x_guard=x_guard, y_guard=y_guard,
                r_guard=r_guard, y_wpad=y_wpad, r_wpad=r_wpad, y_cpad=y_cpad, r_cpad=r_cpad, vec_ok=vec_ok, w_scale=w_scale)


def length_for(nquads_min, d, cut=True):
    """The shortest capacity with at least `nquads_min` quads -- whole blocks of 4d positions -- whose last block is cut: the
    run of fourth outputs is absent and the run of third outputs one short (d = 1: L = 3 mod 4, the straddling quad)."""
    nblk = cdiv(nquads_min, d)
    return 4 * d * nblk - (d + 1 if cut else 0)


def threshold_shape(code, cout, d, B, cus=CUS, extra=0, cut=True):
    """(L, tiles per row) of the smallest launch of B rows that the host still gives to the kernel `code`: 82: B nt gy >= 4 nwg
    with 64-quad tiles; 81: the same with the tile of convwg4_kernel and two workgroups per CU; 80: 512 workgroups."""
    wide = cout % 128 == 0
    gy = cout // (128 if wide else 64)
    if code == 82:
        assert wide
        BQ, need = 64, 4 * (cus - cus % (8 * gy))
    elif code == 81:
        BQ, need = (32 if wide else 64), 4 * (2 * cus - 2 * cus % (8 * gy))
    else:
        BQ, need = (32 if wide else 64), 512
    nt = cdiv(need + extra, B * gy)
    return length_for((nt - 1) * BQ + 1, d, cut), nt


def just_met(g, need):
    """The launch has at least `need` work items, and one block of 4d positions less per row would not."""
    nquads = cdiv(g["L"], 4 * g["d"]) * g["d"]
    return g["N"] >= need > g["B"] * cdiv(nquads - g["d"], g["BQ"]) * g["gy"]


def ragged_lengths(L, d):
    """Row 0 fills the capacity; a long row that ends inside a quad (a workgroup's list leaves it and enters the next row: invalid
    tiles in the middle of the list), one of a single position, a row shorter than one tile, rows that end on a block of 4d and
    one past it."""
    return [L, (3 * L // 4) | 1, 1, max(2, min(L, d + 13)), min(L, 4 * d), min(L, 4 * d + 1)]


# code, Cin, Cout, d, pre, post, post slope, bias, residual, row tags: every distinct launch of the three kernels in the five
# census geometries of tests/test_conv_taps_gpu.py (test_launch_census of tests/test_wg4_gpu.py keeps the table complete)
def _stage_rows(code, c, rows):
    """A stage's launches but its closing one: the eight first convolutions and the second one (seven launches per step)."""
    first = [(code, c, c, 3 ** i, PRE_LRELU, POST_LRELU, 0.01, True, "none", rows) for i in range(8)]
    return first + [(code, c, c, 1, PRE_NONE, POST_NONE, 0.0, True, "in place", rows)]


# batch 32 and 8 x 30 s: every stage on convwg4x_kernel; batch 1: C = 128 and 256 on convwg4_kernel (C = 512 has fewer than 512
# workgroups there and leaves the family); four rows of 10 s (train mode, and the ragged batch of five): C = 512 on convwg4_kernel,
# the others on convwg4x_kernel.  The stage-closing layers and the condnet (batch 8 and more) always run on convwg4_kernel.
CASES = [row for c in (512, 256, 128) for row in _stage_rows(82, c, False)]
CASES += [row for c in (512, 256, 128) for row in _stage_rows(80, c, False)]
CASES += [row for c in (256, 128) for row in _stage_rows(82, c, True)] + _stage_rows(80, 512, True)
CASES += [(80, c, c, 1, PRE_NONE, POST_SNAKE, 0.2, True, "in place", rows) for rows in (False, True) for c in (512, 256, 128)]
CASES += [(80, cin, 512, 1, PRE_NONE, POST_ELU, 0.0, True, "none", False) for cin in (128, 512)]


def case_id(key):
    code, cin, cout, d, pre, post, ps, bias, res, rows = key
    return "k%d-c%d%s-d%d-%s-%s%s%s%s%s" % (code, cin, "" if cin == cout else "x%d" % cout, d, "pre" if pre else "nopre", POST_NAMES[post],
                                          ("%g" % ps) if post in (POST_LRELU, POST_SNAKE) else "", "-bias" if bias else "",
                                          {"none": "", "in place": "-inplace", "separate": "-res"}[res], "-rows" if rows else "")


def case_spec(key, heavy=False, cus=CUS):
    """The reduced launch of a CASES row: Cin and Cout are the product's (the fp32 chain and gy), B = 4 rows whose length just
    meets the threshold of the row's kernel and ends inside a block of 4d (d = 1: inside a quad); with row tags B = 6, rows
    1 .. 5 shorter: the capacity alone carries the threshold, as on the host."""
    code, cin, cout, d, pre, post, ps, bias, res, rows = key
    B = 6 if rows else 4
    L, _ = threshold_shape(code, cout, d, B, cus)
    lengths = ragged_lengths(L, d) if rows else None
    return make_spec(cin, cout, d, L, B, pre, post, ps, bias=bias, res=res, lengths=lengths, heavy=heavy)


# name, expected code, spec: the code paths the product does not reach
def _edges(cus=CUS):
    e = []
    first = dict(pre=PRE_LRELU, post=POST_LRELU, post_slope=0.01)
    second = dict(res="in place")

    def add(name, code, cin, cout, d, B=4, want=None, extra=0, L=None, lengths=None, cut=True, **kw):
        B = 6 if lengths == "ragged" else B
        if L is None:
            L, _ = threshold_shape(want or code, cout, d, B, cus, extra, cut)
        if lengths == "ragged":
            lengths = ragged_lengths(L, d)
        e.append((name, code, make_spec(cin, cout, d, L, B, lengths=lengths, **kw)))

    # ---- convwg4x_kernel: K-loop lengths (S = Cin / 8 = 8: the trickle cannot finish inside the K loop; 10 = NIT + 2 exactly;
    # 12; 24), Cin != Cout on the first instance, gy = 2
    for cin in (64, 96, 192):
        add("x-first-cin%d" % cin, 82, cin, 128, 3, **first)
        add("x-second-cin%d" % cin, 82, cin, 128, 1, **second)
    add("x-first-cin64-d1-rows", 82, 64, 128, 1, lengths="ragged", **first)
    add("x-first-cin192-cout256-d9", 82, 192, 256, 9, **first)
    add("x-second-cin64-cout256-separate", 82, 64, 256, 1, res="separate", r_guard=8, r_wpad=4, r_cpad=1)
    # ---- row ends on the D1 instances: L = 256 n - 1 .. 256 n + 3 (the quad that straddles a row's end)
    L0, _ = threshold_shape(82, 128, 1, 4, cus)
    L0 = cdiv(L0, 256) * 256
    for k in (-1, 0, 1, 2, 3):
        add("x-second-L256n%+d" % k, 82, 64, 128, 1, L=L0 + 256 + k, **second)
        add("x-first-d1-L256n%+d" % k, 82, 64, 128, 1, L=L0 + 256 + k, **first)
    # ---- the dilated instance: L off a multiple of 4d; a single block shorter than 4d needs B large
    for d in (3, 9, 27):
        add("x-first-d%d-whole" % d, 82, 64, 128, d, cut=False, **first)
        add("x-first-d%d-rows" % d, 82, 64, 128, d, lengths="ragged", **first)
    # ---- the work list: N = 4 nwg exactly, + 1, a short last XCD chunk, and one below (declined: convwg4_kernel)
    nwg = cus - cus % 8
    Lt = length_for((nwg // 8 - 1) * 64 + 1, 1)               # nwg / 8 tiles per row
    add("x-N4nwg", 82, 64, 128, 1, B=32, L=Lt, **second)
    add("x-N4nwg-first-d3", 82, 64, 128, 3, B=32, L=length_for((nwg // 8 - 1) * 64 + 1, 3), **first)
    Lt1 = length_for((4 * nwg) * 64 + 1, 1)                   # one row of 4 nwg + 1 tiles
    add("x-N4nwg+1", 82, 64, 128, 1, B=1, L=Lt1, **second)
    add("x-N4nwg+5-short-last-chunk", 82, 64, 128, 1, B=1, L=length_for((4 * nwg + 4) * 64 + 1, 1), **second)
    add("x-N4nwg-1-declined", 80, 64, 128, 1, B=1, L=length_for((4 * nwg - 2) * 64 + 1, 1), **second)
    # ---- operands: no bias; residual separate with strides of its own; y with strides of its own
    add("x-first-nobias", 82, 64, 128, 3, bias=False, **first)
    add("x-second-nobias-rows", 82, 64, 128, 1, bias=False, lengths="ragged", **second)
    add("x-first-ylayout", 82, 64, 128, 9, y_guard=8, y_wpad=4, y_cpad=3, lengths="ragged", **first)
    add("x-second-ylayout", 82, 64, 128, 1, y_guard=8, y_wpad=12, y_cpad=2, **second)
    # ---- declines: no vector path at d = 1 (the second convolution leaves the persistent kernels), a snake post-activation
    add("x-second-unaligned-declined", 80, 64, 128, 1, want=82, vec_ok=False, **second)
    add("x-first-unaligned-d1", 82, 64, 128, 1, vec_ok=False, **first)
    add("x-snake-declined", 80, 64, 128, 1, want=82, res="in place", post=POST_SNAKE, post_slope=0.2)
    # ---- convwg4_kernel, the run-time instance: the stage-closing call, vector and dword paths; bias without residual; both tiles
    for cout in (128, 64, 192):
        add("g-close-snake-c%d" % cout, 80, 64, cout, 1, res="in place", post=POST_SNAKE, post_slope=0.2, lengths="ragged")
        add("g-close-lrelu-c%d-dword" % cout, 80, 64, cout, 1, res="in place", post=POST_LRELU, post_slope=0.2, vec_ok=False)
        add("g-bias-elu-c%d" % cout, 80, 64, cout, 1, post=POST_ELU)
        add("g-res-separate-d3-c%d" % cout, 80, 64, cout, 3, res="separate", pre=PRE_LRELU, r_guard=8, r_wpad=4)
    add("g-spec1-c128", 80, 64, 128, 9, **first)
    add("g-spec2-c128-rows", 80, 64, 128, 1, lengths="ragged", **second)
    add("g-nobias-nores-c128", 80, 64, 128, 3, bias=False)
    # ---- convwg4p_kernel: Cout = 64 and 192 at its threshold, first and second instance
    for cout in (64, 192):
        add("p-first-c%d-d3" % cout, 81, 64, cout, 3, **first)
        add("p-first-c%d-d1-rows" % cout, 81, 64, cout, 1, lengths="ragged", **first)
        add("p-second-c%d" % cout, 81, 64, cout, 1, **second)
    add("p-second-c64-separate-nobias", 81, 64, 64, 1, res="separate", bias=False, r_guard=8, r_wpad=4, r_cpad=1)
    return e


EDGES = _edges()
DECLINED = [("cin72", dict(B=4, cin=72, cout=128, L=70000, d=1)), ("cout96", dict(B=4, cin=64, cout=96, L=70000, d=1)),
            ("short", dict(B=1, cin=64, cout=128, L=4096, d=1))]


# --------------------------------------------------------------------------------------
# the tests
# --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _checked(i, heavy):
    return check(case_spec(CASES[i], heavy))


@pytest.mark.parametrize("i", range(len(CASES)), ids=[case_id(k) for k in CASES])
def test_every_case_of_the_table(i):
    """Each CASES row at its reduced size: walked, on the kernel the row names, and no larger than the threshold asks."""
    key = CASES[i]
    g = _checked(i, False)
    assert g["code"] == key[0]
    spec = case_spec(key)
    assert spec["L"] % (4 * key[3]) != 0
    assert just_met(g, 4 * g["nwg"] if key[0] == 82 else 512), "the threshold is just met"


def test_cases_are_distinct():
    assert len(set(CASES)) == len(CASES)


@pytest.mark.parametrize("i", range(len(EDGES)), ids=[e[0] for e in EDGES])
def test_every_edge_of_the_table(i):
    name, code, spec = EDGES[i]
    assert check(spec)["code"] == code, name


def test_edges_reach_what_they_are_meant_to():
    assert len({e[0] for e in EDGES}) == len(EDGES) and len(EDGES) <= 64
    gs = {name: check(spec) for name, _, spec in EDGES}
    x = {n: g for n, g in gs.items() if g["code"] == 82}
    # K-loop lengths of convwg4x_kernel: S = 8 (trickle_drain), 12, 24; NIT + 2 = 10 chunks would be Cin = 80, which the family
    # declines (Cin % 32 != 0): the nearest the host accepts on either side are 8 and 12
    assert {g["cin"] // 8 for g in x.values()} >= {8, 12, 24} and dispatch(4, 80, 128, 70000, 1, res=True) is None
    assert any(g["cin"] != g["cout"] and g["spec"] == 1 for g in x.values()) and any(g["gy"] == 2 for g in x.values())
    assert {s["L"] % 256 for n, _, s in EDGES if "L256n" in n} == {255, 0, 1, 2, 3}
    nwg = CUS - CUS % 8
    assert gs["x-N4nwg"]["N"] == 4 * nwg and gs["x-N4nwg+1"]["N"] == 4 * nwg + 1 and gs["x-N4nwg-first-d3"]["N"] == 4 * nwg
    g = gs["x-N4nwg+5-short-last-chunk"]
    assert g["N"] == 4 * nwg + 5 and 0 < g["N"] - 7 * g["chunk"] < g["chunk"] - 1       # the last XCD's chunk is short
    g = gs["x-N4nwg-1-declined"]               # (32-quad tiles there: 64 N' quads in N = 2 N' - 1 tiles, below 4 x 2 nwg too)
    assert g["code"] == 80 and cdiv(g["N"], 2) == 4 * nwg - 1
    # ragged rows: tiles that are invalid in the middle of a workgroup's list and at its end
    for name in ("x-first-cin64-d1-rows", "x-first-d9-rows", "x-second-nobias-rows"):
        spec = [s for n, _, s in EDGES if n == name][0]
        g = gs[name]
        n, _ = work_items(g)
        per = g["nwg"] >> 3
        valid = np.zeros(g["N"], dtype=bool)
        for b, Lrow in enumerate(spec["lengths"]):
            worked = row_walk(g, spec["L"], Lrow)[2]
            valid[b * g["ntiles"]:b * g["ntiles"] + worked] = True
        lists = [valid[np.arange(x * g["chunk"] + j, min(g["N"], (x + 1) * g["chunk"]), per)] for x in range(8) for j in range(per)]
        mid = lambda l: any(not l[i] and l[:i].any() and l[i + 1:].any() for i in range(l.size))
        assert any(mid(l) for l in lists), "no list with an invalid tile between two valid ones"
        assert any(l.size > 1 and l.any() and not l[-1] for l in lists), "no list that ends on an invalid tile"
        assert any(l.size > 1 and not l[0] and l.any() for l in lists), "no list that starts on an invalid tile"
    # the three codes, the three instances of convwg4_kernel, both of its tiles, both persistent tiles of convwg4p_kernel
    assert {g["code"] for g in gs.values()} == {80, 81, 82}
    g80 = [g for g in gs.values() if g["code"] == 80]
    assert {g["spec"] for g in g80} == {0, 1, 2} and {g["BQ"] for g in g80} == {32, 64} and {g["d1"] for g in g80} == {False, True}
    assert {(g["cout"], g["spec"]) for g in gs.values() if g["code"] == 81} >= {(64, 1), (64, 2), (192, 1), (192, 2)}
    for g in gs.values():
        if g["code"] == 81:
            assert just_met(g, 4 * g["nwg"])


def test_the_host_rule():
    """try_launch_convwg4 restated: what the family declines, the 512-workgroup minimum, the two persistent thresholds."""
    for name, kw in DECLINED:
        assert dispatch(**kw) is None, name
    kw = dict(pre=PRE_LRELU, post=POST_LRELU, post_slope=0.01)
    assert dispatch(4, 128, 128, 65536, 1, **kw)["code"] == 82 and dispatch(4, 128, 128, 65536 - 256, 1, **kw)["code"] == 80
    assert dispatch(4, 128, 128, 65536, 1, post=POST_SNAKE, post_slope=0.2, res=True)["code"] == 80
    assert dispatch(4, 128, 128, 65536, 1, res=True)["spec"] == 2 and dispatch(4, 128, 128, 65536, 3, res=True)["spec"] == 0
    assert dispatch(8, 64, 64, 66001, 81, **kw)["code"] == 81 and dispatch(8, 64, 64, 66002, 1, res=True)["code"] == 81
    assert dispatch(4, 32, 128, 65536, 1, **kw)["code"] == 80          # two 16-channel chunks: neither persistent kernel
    assert dispatch(4, 512, 512, 4 * 4096, 1, **kw)["nwg"] == 256 and dispatch(4, 128, 384, 65536, 3, **kw)["nwg"] == 240
    assert dispatch(4, 128, 128, 65536, 1, cus=304, **kw)["code"] == 80 and dispatch(5, 128, 128, 65536, 1, cus=304, **kw)["nwg"] == 304
    # the product's dilations: fast_div's reciprocal of 4d is formed as 0.25f / d
    for d in (1, 3, 9, 27, 81, 243, 729, 2187):
        for n in (1, 4 * d - 1, 4 * d, 4 * d + 1, 70000, 441000 * 2):
            fast_div([n + 4 * d - 1], 4 * d, np.float32(0.25) * (np.float32(1.0) / np.float32(d)))


@pytest.mark.parametrize("cus", [208, 240, 304])
def test_tables_hold_for_other_cu_counts(cus):
    """The GPU module sizes every launch by the device's own CU count: the tables pass the model at others than 256 too."""
    for key in CASES[::7]:
        assert check(case_spec(key, cus=cus), cus)["code"] == key[0]
    for name, code, spec in _edges(cus)[::3]:
        assert check(spec, cus)["code"] == code, name


def test_the_model_notices_a_broken_launch():
    """The model is not vacuous: a work list cut with a chunk that is no multiple of gy, a tile count one short and a capacity
    whose last vector load leaves the view each break an invariant."""
    spec = case_spec(CASES[0])
    g = check(spec)
    with pytest.raises(AssertionError):
        work_items(dict(g, chunk=g["chunk"] + 1))
    stored, _, _ = row_walk(dict(g, ntiles=g["ntiles"] - 1), spec["L"], spec["L"])
    assert stored.size < spec["L"]
    g1 = dispatch(4, 64, 128, 65535, 1, res=True)
    assert row_walk(g1, 65535, 65533)[1] == 65535 and row_walk(g1, 65535, 65533)[1] < up4(65535)
