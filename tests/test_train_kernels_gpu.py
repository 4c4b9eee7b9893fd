"""The mode-2 kernels of voicefixer_amd/csrc/vfx_train.hip -- bn_partial_kernel + bn_finalize_kernel (ops.bn_stats),
bn_apply_kernel<VEC> (ops.bn_apply) and dropout_kernel (ops.dropout) -- at every launch the product makes, against float64 /
the numpy specification, one launch at a time.

* ``region_stats`` is the float64 statement of the region the file's header defines (``test_region_stats_is_train_mode_
  batch_norm`` pins it against torch's own train-mode batch_norm, on the CPU).
* ``GEOMS`` is the table of launch geometries, both forms.  It holds the smallest shapes that reach each path of the two
  statistics kernels (``test_tables_reach_the_paths_they_name`` does the chunk arithmetic on the CPU: more than 64 partials,
  empty partials behind a non-empty one in one lane, lanes with nothing at all, chunks that straddle segments) and one row
  per geometry the product launches.  ``test_bn_stats`` runs every row with three inputs (iid; a drift whose variance lies
  BETWEEN the 4096-element chunks; channels of mean 1e3 / std 1e-2, of a constant and of zeros), ``test_bn_apply`` every row
  with scale and shift of the test's own choice for slopes None / 0.0 / 0.01, out of place and in place, on the float4 and on
  the scalar instance, ``test_dropout`` the rows of ``DROPOUT``.
* ``test_census_*`` wrap the three launchers, run the train-mode restorer once at T = 65 and once on a ragged batch, and
  assert that every call is a row of those tables; the number of calls per key is pinned at T = 65.

Buffers are guarded views as the engine lays them out; the guard bands, a map's spare column and everything past a row's
extent hold a NaN with a payload, and every test compares the whole allocation as int32 afterwards: nothing outside
[0, extent) of a row may change by a bit.  The module is not marked as a whole because its CPU tests must run where no
device is visible: every device test carries ``@gpu``.

Bounds.  Statistics: those of tests/test_train_mode_gpu.py (scale rtol 2e-5; shift rtol 2e-4 + atol 2e-4).  Apply: 1 float32
ulp of float32(float64(x) * float64(a) + float64(s)) (fmaf is correctly rounded; the ulp covers the double rounding of this
reference and the slope product).  Dropout: equality.  Every case prints ``PARITY <id> ...`` (the worst error as a multiple of
its bound) before it asserts; profiles/train_kernels_parity.txt is that output.

Finding, fixed in the kernel; the extent assertions of ``test_bn_apply`` are its regression cases.  bn_apply_kernel<true>
returned only when the first of its four positions was past the extent and then stored a whole float4, so with
extent % 4 != 0 it wrote up to three positions past the extent (1-D form with T % 4 != 0, tagged or not; lp = 1 maps with an
odd number of map rows): on the parent's library 24 of this file's 114 float4 launches did -- all six of each geometry with
such an extent (1d-C128-L2077-rows, 1d-C512-L65-rows, 1d-C512-L65, map-lp1-C5-H7-rows), out of place and in place, none
elsewhere.  The last vector of a row now stores its positions one by one under ``l0 + i < valid``.
"""
import math
import zlib

import numpy as np
import pytest
import torch

from voicefixer_amd import _lib, dropout, engine, ops

gpu = pytest.mark.gpu

DEV = "cuda"
EPS = 1e-5
CHUNK = 4096                  # elements per bn_partial_kernel workgroup (BN_CHUNK)
B = 3
X_NAN = 0x7FC0BEEF            # what x holds wherever the region does not count
Y_NAN = 0x7FC0F00D            # what an out-of-place y holds before the launch (another payload: a copied x NaN shows)
SENTINEL = 1.5                # in place: finite values past the extent, so that a stray x * a + s there changes bits
SLOPES = (None, 0.0, 0.01)
KINDS = ("iid", "drift", "special")


def up4(n):
    return (n + 3) // 4 * 4


# --------------------------------------------------------------------------------------
# 0. the reference
# --------------------------------------------------------------------------------------
def region_stats(x, form, valid, P):
    """(count, mean, biased variance) in float64, each (B, G), of the regions vfx_train.hip's header defines, for x (B, C, L)
    and the extents ``valid`` (B ints).  form "map": G = C, per (b, c) over the positions < valid[b] whose column (position
    mod P) is not P - 1; form "1d": G = 1, per b over all C channels x the positions < valid[b]."""
    x = np.asarray(x, np.float64)
    nb, C, L = x.shape
    pos = np.arange(L)
    cnt, mean, var = [], [], []
    for b in range(nb):
        keep = pos < valid[b]
        if form == "map":
            r = x[b][:, keep & (pos % P != P - 1)]
        else:
            r = x[b][:, keep].reshape(1, -1)
        n = r.shape[1]
        m = r.sum(axis=1) / n
        cnt.append(np.full(r.shape[0], float(n)))
        mean.append(m)
        var.append(((r - m[:, None]) ** 2).sum(axis=1) / n)
    return np.stack(cnt), np.stack(mean), np.stack(var)


def test_region_stats_is_train_mode_batch_norm():
    """Mean and biased variance of both forms against torch.nn.functional.batch_norm(training=True) in float64 on the same
    valid regions (momentum 1: the running statistics ARE the batch's; torch's running variance is the unbiased one)."""
    import torch.nn.functional as F
    rng = np.random.default_rng(0)

    def torch_stats(region):                       # region (1, G, ...) float64
        G = region.shape[1]
        rm, rv = torch.zeros(G, dtype=torch.float64), torch.ones(G, dtype=torch.float64)
        out = F.batch_norm(region, rm, rv, None, None, True, 1.0, EPS)
        n = region.numel() // G
        return rm.numpy(), rv.numpy() * (n - 1) / n, out.numpy()

    C, H, P, rows_h = 4, 5, 4, [5, 3, 2]
    x = rng.standard_normal((B, C, H * P)) * 3 + 5
    cnt, mean, var = region_stats(x, "map", [h * P for h in rows_h], P)
    for b, h in enumerate(rows_h):
        reg = x[b].reshape(C, H, P)[:, :h, :P - 1]
        m, v, out = torch_stats(torch.from_numpy(reg.copy())[None])
        assert np.all(cnt[b] == h * (P - 1))
        np.testing.assert_allclose(mean[b], m, rtol=1e-12)
        np.testing.assert_allclose(var[b], v, rtol=1e-12)
        np.testing.assert_allclose((reg - mean[b][:, None, None]) / np.sqrt(var[b] + EPS)[:, None, None], out[0], rtol=1e-12, atol=1e-12)
    C, L, T = 6, 11, [11, 6, 3]
    x = rng.standard_normal((B, C, L)) * 3 + 5
    cnt, mean, var = region_stats(x, "1d", T, 1)
    for b, t in enumerate(T):
        reg = x[b, :, :t]
        m, v, out = torch_stats(torch.from_numpy(reg.copy())[None, None])
        assert cnt.shape == (B, 1) and cnt[b, 0] == C * t
        np.testing.assert_allclose(mean[b], m, rtol=1e-12)
        np.testing.assert_allclose(var[b], v, rtol=1e-12)
        np.testing.assert_allclose((reg - mean[b, 0]) / np.sqrt(var[b, 0] + EPS), out[0, 0], rtol=1e-12, atol=1e-12)


# --------------------------------------------------------------------------------------
# the tables
# --------------------------------------------------------------------------------------
class Geom:
    """One launch geometry.  form "1d": x (B, C, L = ext), one BN channel per row; "map": x (B, C, L = ext * P) with
    P = 1 << lp, one BN channel per map channel.  rows: None (no row tag) or the extent of every row, in positions (1d) or in
    map rows (map)."""

    def __init__(self, form, C, ext, lp=0, rows=None):
        self.form, self.C, self.ext, self.lp, self.rows = form, C, ext, lp, rows
        self.P = 1 << lp if form == "map" else 1
        self.L = ext * self.P
        self.G = C if form == "map" else 1
        self.valid = [self.L] * B if rows is None else [r * self.P for r in rows]
        self.guard = up4(self.P + 8) if form == "map" else 16
        self.nblk = nblk(form, C, self.L)
        tag = "" if rows is None else "-rows" + ".".join(map(str, rows))
        self.id = ("1d-C%d-L%d%s" % (C, ext, tag)) if form == "1d" else ("map-lp%d-C%d-H%d%s" % (lp, C, ext, tag))

    def parts(self):
        """The geometry's part of a census key: form, lp, row tag, more than 64 partials, an extent that is no multiple of 4."""
        return (self.form, self.lp, self.rows is not None, self.nblk > 64, any(v % 4 for v in self.valid))


def nblk(form, C, L):
    """Partials per (row, BN channel): ceil(nseg * span / 4096), span = L rounded up to 4 (bn_geom / bn_nblk)."""
    return ((C if form == "1d" else 1) * up4(L) + CHUNK - 1) // CHUNK


# -- the paths of the statistics kernels (arithmetic: test_tables_reach_the_paths_they_name) and of bn_apply_kernel's tails
PATHS = [
    Geom("1d", 128, 2077, rows=[2077, 1038, 65]),        # span 2080, 65 partials: lane 0 folds two; extents % 4 = 1, 2, 1
    Geom("1d", 256, 2066, rows=[2066, 1035, 65]),        # span 2068, 130 partials: lanes 0, 1 fold three (the last one empty in
                                                         # the short rows); chunks straddle segments; % 4 = 2, 3, 1
    Geom("1d", 512, 65, rows=[65, 35, 65]),              # span 68, 9 partials: lanes 9 .. 63 hold nothing; % 4 = 1, 3, 1
    Geom("map", 2, 2112, lp=7, rows=[2112, 1057, 2]),    # 66 partials; the 2-row map: partials 1 .. 65 empty, lane 0 skips its second one
    Geom("map", 5, 7, lp=1, rows=[7, 3, 1]),             # extents 14 / 6 / 2: odd map-row counts, % 4 = 2; the last row counts ONE element
    Geom("map", 3, 300, lp=4, rows=[300, 151, 2]),       # 2 partials
]
# -- what the product launches (test_census_*): untagged at T = 65 (1-D extent 65, maps of 128 >> k rows), tagged on ragged batches
PRODUCT = [Geom("1d", 512, 65)]
PRODUCT += [Geom("map", 3, 8, lp=1, rows=[8, 4, 2]), Geom("map", 3, 6, lp=1)]      # extents 16 / 8 / 4 and 12: multiples of 4, as the product's
for _lp in range(2, 8):
    PRODUCT += [Geom("map", 3, 12, lp=_lp, rows=[12, 7, 2]), Geom("map", 3, 12, lp=_lp)]
GEOMS = PATHS + PRODUCT
APPLY_GEOMS = [g for g in GEOMS if g.C * g.L < 500000]   # (all but 1d-C256-L2066 and map-lp7-C2-H2112, whose size only the
                                                         # statistics need: bn_apply has no path that only they reach)
IDS = lambda gs: [g.id for g in gs]

# T, row tags, segments: three blockIdx.x with extents on both sides of a block's end / one block, untagged (the product at T = 65)
DROPOUT = [(600, [600, 257, 256], [0, 5, 4294967295]), (65, None, [2, 0, 7])]
SEEDS = (0, 2 ** 64 - 1, 123456789012345)


def stats_key(parts):
    return ("bn_stats",) + parts


def apply_key(parts, groups_c, slope, inplace):
    return ("bn_apply",) + parts + (groups_c, slope, inplace)


def dropout_key(C, layer, relu, rows, T):
    return ("dropout", C, layer, relu, rows, T > 256)


def table_keys():
    keys = {stats_key(g.parts()) for g in GEOMS}
    keys |= {apply_key(g.parts(), g.form == "map", s, ip) for g in APPLY_GEOMS for s in SLOPES for ip in (False, True)}
    keys |= {dropout_key(512, layer, layer == 0, rows is not None, T) for T, rows, _ in DROPOUT for layer in (0, 1)}
    return keys


def chunk_counts(g, valid):
    """How many elements each bn_partial_kernel workgroup of one (row, BN channel) pair counts (the kernel's own indexing)."""
    span = up4(g.L)
    j = np.arange((g.C if g.form == "1d" else 1) * span)
    off = j % span
    c = off < valid
    if g.P > 1:
        c &= (off & (g.P - 1)) != g.P - 1
    full = np.zeros(g.nblk * CHUNK, bool)
    full[:j.size] = c
    return full.reshape(g.nblk, CHUNK).sum(axis=1)


def test_tables_reach_the_paths_they_name():
    """The chunk arithmetic behind PATHS, on the CPU.  Lane l of bn_finalize_kernel folds partials l, l + 64, ...

    1-D form: a chunk of 4096 elements is longer than a segment (span 2080 / 2068 / 68), so every FULL chunk holds the start
    of a segment and with it at least one counted element, however short the row; only the last, partial chunk can be empty.
    C = 256, L = 2066: 256 * 2068 = 129 chunks + 1024 elements, the offsets 1044 .. 2067 of the last segment: partial 129 is
    empty for the extents 1035 and 65, and lane 1 (partials 1, 65, 129) skips it (`nb == 0.0`).  With 65 / 130 partials no lane
    of the 1-D form is empty; empty lanes there come from nblk < 64 (C = 512, L = 65: 512 * 68 = 34816 = 8.5 chunks, lanes
    9 .. 63).  Map form, lp = 7, H = 2112: 2112 * 128 = 270336 = 66 chunks; the row of 2 map rows counts 2 * 127 = 254
    elements, all in chunk 0, so lane 0 folds chunk 0 and then skips the empty chunk 64 (`nb == 0.0`), lane 1 folds the empty
    chunks 1 and 65 and lanes 2 .. 63 one empty chunk each: 63 lanes enter the tree with a count of 0 (`nb > 0.0`)."""
    assert [g.nblk for g in PATHS] == [65, 130, 9, 66, 1, 2]
    assert 128 * 2080 == 65 * CHUNK and 256 * 2068 == 129 * CHUNK + 1024 and 2068 % 4 == 0 and CHUNK % 2068 != 0
    for g in PATHS[:3]:
        for v in g.valid:
            c = chunk_counts(g, v)
            assert np.all(c[:-1] > 0) and (c[-1] > 0) == (g.C != 256 or v > 1044), (g.id, v)
    c = chunk_counts(PATHS[3], 2 * 128)
    assert c[0] == 254 and not c[1:].any() and c.size == 66
    lanes = [c[l::64] for l in range(64)]
    assert list(lanes[0]) == [254, 0] and all(not lane.any() for lane in lanes[1:])
    c = chunk_counts(PATHS[3], 1057 * 128)                 # the middle row: chunks 0 .. 33 hold something, lanes 34 .. 63 nothing
    assert c[:34].all() and not c[34:].any()
    assert chunk_counts(PATHS[4], 2).tolist() == [1]
    assert {v % 4 for g in PATHS[:3] for v in g.valid} == {1, 2, 3} and {v % 4 for v in PATHS[4].valid} == {2}
    assert len({g.id for g in GEOMS}) == len(GEOMS)
    assert all(not any(v % 4 for v in g.valid) and g.nblk <= 64 for g in PRODUCT if g.form == "map")


# --------------------------------------------------------------------------------------
# buffers
# --------------------------------------------------------------------------------------
def _keep(g, b):
    """Positions of row b that the region counts: below the extent and, in a map, not in the spare column."""
    pos = np.arange(g.L)
    k = pos < g.valid[b]
    if g.P > 1:
        k &= (pos & (g.P - 1)) != g.P - 1
    return k


def upload(g, dense, nan_bits, off=0, past=None):
    """A guarded (B, C, up4(L)) device view of geometry g, `off` floats off its 16-byte alignment, inside an allocation that
    holds the NaN `nan_bits` everywhere except: `dense` (B, C, L) where the region counts (None: nowhere) and, if `past` is
    given, that value from every row's extent to the end of its padded span.  Tagged with g's rows.  Returns (view, base
    tensor, the allocation's int32 image on the host)."""
    Lp, gd = up4(g.L), g.guard
    img = np.full((B, g.C, gd + Lp + gd + 4), nan_bits, np.int32).view(np.float32)
    lo = gd + off
    for b in range(B):
        if dense is not None:
            k = _keep(g, b)
            img[b][:, lo:lo + g.L][:, k] = dense[b][:, k]
        if past is not None:
            img[b, :, lo + g.valid[b]:lo + Lp] = past
    base = torch.from_numpy(img).to(DEV)
    v = base[:, :, lo:lo + Lp]
    v._vfx_guard, v._vfx_base = (gd if off == 0 else 0), base
    if g.rows is not None:
        ops.with_rows(v, torch.tensor(g.valid, dtype=torch.int32, device=DEV))
    return v, base, img.view(np.int32).copy()


def bits(t):
    return t.cpu().numpy().view(np.int32)


def _rng(*what):
    return np.random.default_rng(zlib.crc32(repr(what).encode()))


def make_input(g, kind, rng):
    """dense (B, C, L) fp32 and the kind of every (row, BN channel) pair ((B, G) of "", "big", "const", "zero")."""
    x = rng.standard_normal((B, g.C, g.L))
    kinds = np.full((B, g.G), "", dtype=object)
    if g.form == "1d":
        x = 3 * x + 5
    if kind == "drift":                                   # -50 .. +50 across the flattened region of the pair, + unit noise
        x = rng.standard_normal((B, g.C, g.L))
        for b, v in enumerate(g.valid):
            if g.form == "map":
                x[b, :, :v] += -50 + 100 * np.arange(v) / max(v - 1, 1)
            else:
                x[b, :, :v] += -50 + 100 * (np.arange(g.C)[:, None] * v + np.arange(v)) / (g.C * v - 1)
    elif kind == "special":
        for b in range(B):
            for c in range(g.G):
                k = ("big", "const", "zero", "")[(b * g.G + c) % 4]
                sl = (b, c) if g.form == "map" else (b,)
                if k == "big":
                    x[sl] = 1e3 + 1e-2 * rng.standard_normal(x[sl].shape)
                elif k:
                    x[sl] = 0.25 if k == "const" else 0.0
                kinds[b, c] = k
    return x.astype(np.float32), kinds


# --------------------------------------------------------------------------------------
# 1. statistics
# --------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("g", GEOMS, ids=IDS(GEOMS))
def test_bn_stats(g, kind):
    """ops.bn_stats on x with NaN wherever the region does not count, against region_stats: the bounds of
    tests/test_train_mode_gpu.py, the same bits on a second call, finite results, x untouched.  Measured: at most 0.004 x the
    scale bound for iid and drift inputs at every nblk; the mean-1e3 / std-1e-2 pairs reach 0.88 x at map-lp1-C5-H7 (7 counted
    elements: a thread's fp32 sum of two values near 1e3 rounds at 6e-5, which is not small against a deviation of 1e-2 once
    divided by so few elements) and 0.05 x or less where a pair counts thousands."""
    rng = _rng(g.id, kind)
    dense, kinds = make_input(g, kind, rng)
    x, base, img = upload(g, dense, X_NAN)
    gamma = rng.uniform(0.5, 2, g.G).astype(np.float32)
    beta = rng.standard_normal(g.G).astype(np.float32)
    gd, bd = torch.from_numpy(gamma).to(DEV), torch.from_numpy(beta).to(DEV)
    out = [torch.full((B * g.G,), float("nan"), device=DEV) for _ in range(4)]
    lib = _lib.lib()
    assert lib.vfx_bn_stats_workspace_bytes(B, g.C, g.L, g.lp) == B * g.G * g.nblk * 24
    ops.bn_stats(x, g.L, g.lp, gd, bd, out[0], out[1])
    ops.bn_stats(x, g.L, g.lp, gd, bd, out[2], out[3])
    torch.cuda.synchronize()
    assert torch.equal(out[0], out[2]) and torch.equal(out[1], out[3])            # no atomics: the same bits
    assert np.array_equal(bits(base), img)                                        # x is read only
    sc, sh = out[0].cpu().numpy().reshape(B, g.G), out[1].cpu().numpy().reshape(B, g.G)
    assert np.isfinite(sc).all() and np.isfinite(sh).all()                        # nothing of the NaN fill was counted
    cnt, mean, var = region_stats(dense, g.form, g.valid, g.P)
    a = gamma.astype(np.float64) / np.sqrt(var + EPS)
    s = beta.astype(np.float64) - mean * a
    e_sc = np.abs(sc - a) / (2e-5 * np.abs(a))
    e_sh = np.abs(sh - s) / (2e-4 + 2e-4 * np.abs(s))
    print("PARITY stats %s %s nblk %d scale %.3f shift %.3f" % (g.id, kind, g.nblk, e_sc.max(), e_sh.max()))
    assert e_sc.max() <= 1.0, "scale: %.3f x (rtol 2e-5) at %r" % (e_sc.max(), np.unravel_index(e_sc.argmax(), e_sc.shape))
    assert e_sh.max() <= 1.0, "shift: %.3f x (rtol 2e-4 + atol 2e-4) at %r" % (e_sh.max(), np.unravel_index(e_sh.argmax(), e_sh.shape))
    # variance exactly 0 (a constant, zeros, a region of one element): scale = gamma / sqrt(eps) to an ulp; zeros: shift = beta
    if kind == "special":
        assert np.all(var[kinds == "const"] == 0) and np.all(var[kinds == "zero"] == 0)
        assert (kinds == "const").any() and (kinds == "zero").any() and (kinds == "big").any()
        assert np.array_equal(sh[kinds == "zero"], np.broadcast_to(beta, (B, g.G))[kinds == "zero"])
    flat = np.broadcast_to(gamma, (B, g.G))[var == 0]
    want = (flat.astype(np.float64) / math.sqrt(1e-5)).astype(np.float32)
    assert np.all(np.abs(sc[var == 0].astype(np.float64) - want) <= np.spacing(want))


# --------------------------------------------------------------------------------------
# 2. apply
# --------------------------------------------------------------------------------------
def apply_expected(g, dense, a, s, slope):
    """float32(float64(x) * float64(a) + float64(s)) (the product is exact in float64), then the leaky ReLU as one product."""
    shp = (B, g.G, 1) if g.form == "map" else (B, 1, 1)
    r = (dense.astype(np.float64) * a.astype(np.float64).reshape(shp) + s.astype(np.float64).reshape(shp)).astype(np.float32)
    if slope is not None:
        r = np.where(r > 0, r, (r.astype(np.float64) * float(np.float32(slope))).astype(np.float32))
    return r


@gpu
@pytest.mark.parametrize("g", APPLY_GEOMS, ids=IDS(APPLY_GEOMS))
def test_bn_apply(g):
    """bn_apply alone with the test's own scale and shift (groups = C for maps, 1 for the 1-D form): slopes None / 0.0 / 0.01,
    out of place and in place, the float4 instance (aligned views) and the scalar one (x one float, y three floats off their
    alignment).  Pair (0, 0) cancels: x near 1e3, s = -1e3 a, so an unfused multiply and add is thousands of ulps off."""
    rng = _rng(g.id, "apply")
    dense = rng.standard_normal((B, g.C, g.L))
    dense[(0, 0) if g.form == "map" else (0,)] = 1e3 + 1e-2 * rng.standard_normal(dense[(0, 0) if g.form == "map" else (0,)].shape)
    dense = dense.astype(np.float32)
    a = (rng.uniform(0.5, 2, B * g.G) * rng.choice([-1.0, 1.0], B * g.G)).astype(np.float32)
    s = rng.standard_normal(B * g.G).astype(np.float32)
    a[0] = np.float32(95.3)
    s[0] = np.float32(-1e3 * float(a[0]))
    ad, sd = torch.from_numpy(a).to(DEV), torch.from_numpy(s).to(DEV)
    worst, failures = 0.0, []
    for slope in SLOPES:
        want = apply_expected(g, dense, a, s, slope)
        for inplace in (False, True):
            for off in (0, 1):
                x, xbase, ximg = upload(g, dense, X_NAN, off, past=SENTINEL if inplace else None)
                if inplace:
                    y, ybase, before, yoff = x, xbase, ximg, off
                else:
                    yoff = 3 * off
                    y, ybase, before = upload(g, None, Y_NAN, yoff)
                ops.bn_apply(x, y, g.L, g.lp, ad, sd, slope=slope, groups=g.G)
                torch.cuda.synchronize()
                after = bits(ybase)
                name = "%s slope %r %s %s" % (g.id, slope, "in place" if inplace else "out of place", "scalar" if off else "float4")
                lo = g.guard + yoff
                written = np.zeros(after.shape, bool)
                for b, v in enumerate(g.valid):
                    written[b, :, lo:lo + v] = True
                    k = _keep(g, b)
                    got = after[b, :, lo:lo + g.L].view(np.float32)[:, k].astype(np.float64)
                    w = want[b][:, k]
                    assert np.isfinite(got).all(), name
                    worst = max(worst, float((np.abs(got - w) / np.spacing(np.abs(w))).max()))
                    below = np.arange(g.L) < v
                    assert not after[b, :, lo:lo + g.L][:, below & ~k].any(), name + ": the spare column below the extent is not +0"
                if not inplace:
                    assert np.array_equal(bits(xbase), ximg), name + ": x was written"
                # the extent contract: at or past rows[b], in the pad of the span and in the guard nothing changes by a bit
                stray = (after != before) & ~written
                if stray.any():
                    bb, cc, pp = np.nonzero(stray)
                    failures.append("%s: %d positions outside [0, extent) written, e.g. row %d channel %d position %d (extent %d)" % (
                        name, stray.sum(), bb[0], cc[0], pp[0] - lo, g.valid[bb[0]]))
    print("PARITY apply %s worst %.3f ulp, %d of 12 launches wrote outside a row's extent" % (g.id, worst, len(failures)))
    assert worst <= 1.0
    assert not failures, "\n".join(failures)


# --------------------------------------------------------------------------------------
# 3. dropout
# --------------------------------------------------------------------------------------
_MASKS = {}


def _mask(seed, seg, layer, T):
    if (seed, seg, layer, T) not in _MASKS:
        _MASKS[(seed, seg, layer, T)] = dropout.mask(seed, seg, layer, T).T.copy()       # (C, T)
    return _MASKS[(seed, seg, layer, T)]


@gpu
@pytest.mark.parametrize("layer", [0, 1])
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("case", range(len(DROPOUT)), ids=["T%d-%s" % (c[0], "rows" if c[1] else "norows") for c in DROPOUT])
def test_dropout(case, seed, layer):
    """ops.dropout against dropout.mask bit for bit (layer 0 fused with ReLU, layer 1 plain), nothing written at or past a
    row's extent or in the guard band, and a row's mask independent of where in the batch the row stands."""
    T, rows, segs = DROPOUT[case]
    C, relu = 512, layer == 0
    g = Geom("1d", C, T, rows=rows)
    rng = _rng("dropout", T)
    x = rng.standard_normal((B, C, T)).astype(np.float32)
    x[:, 0:64, 3] = -0.0
    x[:, 64:128, 3] = 1e-40                               # subnormal: x 2 must not flush
    x[:, 128:192, 3] = -1e-40
    k0, k1 = dropout.key_of(seed)
    results = []
    for perm in ([0, 1, 2], [2, 0, 1]):
        gp = Geom("1d", C, T, rows=None if rows is None else [rows[p] for p in perm])
        v, base, img = upload(gp, x[perm], X_NAN)
        rk = torch.from_numpy(np.array([[segs[p], k0, k1] for p in perm], np.uint32).view(np.int32)).to(DEV)
        ops.dropout(v, T, rk, layer, relu=relu)
        torch.cuda.synchronize()
        after = bits(base)
        written = np.zeros(after.shape, bool)
        for i, p in enumerate(perm):
            t = gp.valid[i]
            written[i, :, g.guard:g.guard + t] = True
            got = after[i, :, g.guard:g.guard + t].view(np.float32)
            want = x[p][:, :t] * _mask(seed, segs[p], layer, T)[:, :t]
            if relu:
                want = np.maximum(want, 0)
            assert np.array_equal(got, want), (perm, i)
        assert np.array_equal(after[~written], img[~written]), "written at or past a row's extent or in the guard band"
        results.append(after)
    for i, p in enumerate([2, 0, 1]):
        t = g.valid[p]
        assert np.array_equal(results[1][i, :, g.guard:g.guard + t], results[0][p, :, g.guard:g.guard + t])
    assert 0.45 < float((results[0][0, :, g.guard:g.guard + g.valid[0]].view(np.float32) == 0).mean()) < (0.8 if relu else 0.55)


# --------------------------------------------------------------------------------------
# 4. the product's launches are rows of the tables
# --------------------------------------------------------------------------------------
def _parts_of(x, L, lp):
    rows = getattr(x, "_vfx_rows", None)
    form, C = ("map" if lp > 0 else "1d"), x.shape[1]
    ext = [L] if rows is None else [min(int(r), L) for r in rows.cpu().tolist()]
    return (form, lp, rows is not None, nblk(form, C, L) > 64, any(e % 4 for e in ext))


class _Census:
    """Records every ops.bn_stats / ops.bn_apply / ops.dropout call as its key; the wrappers call the real launchers."""

    def __init__(self):
        self.keys = []

    def __enter__(self):
        self.orig = (ops.bn_stats, ops.bn_apply, ops.dropout)
        st, ap, dr = self.orig

        def bn_stats(x, L, pitch_log2, *a, **kw):
            self.keys.append(stats_key(_parts_of(x, L, pitch_log2)))
            return st(x, L, pitch_log2, *a, **kw)

        def bn_apply(x, y, L, pitch_log2, scale, shift, slope=None, groups=None):
            gc = (pitch_log2 > 0) if groups is None else groups == x.shape[1]
            self.keys.append(apply_key(_parts_of(x, L, pitch_log2), gc, slope, x.data_ptr() == y.data_ptr()))
            return ap(x, y, L, pitch_log2, scale, shift, slope=slope, groups=groups)

        def dropout_(x, T, rowkey, layer, relu=False):
            self.keys.append(dropout_key(x.shape[1], layer, bool(relu), getattr(x, "_vfx_rows", None) is not None, T))
            return dr(x, T, rowkey, layer, relu=relu)

        ops.bn_stats, ops.bn_apply, ops.dropout = bn_stats, bn_apply, dropout_
        return self

    def __exit__(self, *exc):
        ops.bn_stats, ops.bn_apply, ops.dropout = self.orig
        return False


@pytest.fixture(scope="module")
def pipe(seeded_states):
    return engine.Pipeline(seeded_states[0], seeded_states[1], "cuda:0")


def counts_t65():
    """Calls per key of one forward_train at T = 65 (B = 1, no row tags; Tp = 128, level k a map of 128 >> k rows of pitch
    128 >> k).  Denoiser: six BatchNorm2d(1) -- four plain, two with ReLU -- in place, two dropouts.  UNet: a ConvBlockRes is two
    statistics, one apply into scratch and one in place, slope 0.01; four per encoder block (lp 7 .. 2), one centre (lp 1),
    four per decoder block (lp 2 .. 7), one after (lp 7): 9 / 8 / 1 at lp 7 / 6 .. 2 / 1; each decoder block opens with one
    statistics + ReLU apply into scratch at its input level (lp 1 .. 6)."""
    one_d = ("1d", 0, False, False, True)
    c = {stats_key(one_d): 6, apply_key(one_d, False, None, True): 4, apply_key(one_d, False, 0.0, True): 2,
         dropout_key(512, 0, True, False, 65): 1, dropout_key(512, 1, False, False, 65): 1}
    for lp in range(1, 8):
        blocks = {7: 9, 1: 1}.get(lp, 8)
        m = ("map", lp, False, False, False)
        c[stats_key(m)] = 2 * blocks + (1 if lp <= 6 else 0)
        c[apply_key(m, True, 0.01, False)] = c[apply_key(m, True, 0.01, True)] = blocks
        if lp <= 6:
            c[apply_key(m, True, 0.0, False)] = 1
    return c


def _report(name, keys):
    for k in sorted(set(keys), key=repr):
        print("CENSUS-KEY %s %r x%d" % (name, k, keys.count(k)))


@gpu
def test_census_forward_train_t65(pipe):
    g = torch.Generator().manual_seed(1)
    T = 65
    mel = (torch.rand((1, T, 128), generator=g) ** 2) * 3
    k0, k1 = dropout.key_of(5)
    rk = torch.from_numpy(np.array([[0, k0, k1]], np.uint32).view(np.int32)).to(DEV)
    with _Census() as rec:
        pipe.restorer.forward_train(mel.to(DEV), T, rk)
        torch.cuda.synchronize()
    assert ops.bn_stats is rec.orig[0] and ops.bn_apply is rec.orig[1] and ops.dropout is rec.orig[2]
    _report("T65", rec.keys)
    table = table_keys()
    unmatched = sorted({k for k in rec.keys if k not in table}, key=repr)
    assert not unmatched, "train-mode launches that are not rows of the tables:\n%s" % "\n".join(map(repr, unmatched))
    assert {k: rec.keys.count(k) for k in set(rec.keys)} == counts_t65()


@gpu
def test_census_restore_train_ragged(pipe):
    """The ragged batch T = 65 / 230 / 1001 of tests/test_train_mode_gpu.py: every call is a row of the tables (the 1-D form now
    tagged, extents 65 / 230 / 1001, 126 partials at C = 512), and -- with bn_apply_kernel<true> storing the last vector of a
    row element by element -- the restored batch is the same bits on a second run."""
    rng = np.random.default_rng(8)
    lens = [441 * (t - 1) + 100 for t in (65, 230, 1001)]
    wav = np.zeros((3, max(lens)), np.float32)
    for b, n in enumerate(lens):
        wav[b, :n] = 0.2 * rng.standard_normal(n)
    wd = torch.from_numpy(wav).to(DEV)
    with _Census() as rec:
        out = pipe.restore_train(wd, lens, [0, 3, 1], 77).cpu().numpy()
    _report("ragged", rec.keys)
    again = pipe.restore_train(wd, lens, [0, 3, 1], 77).cpu().numpy()
    assert np.isfinite(out).all() and np.array_equal(out, again)
    table = table_keys()
    unmatched = sorted({k for k in rec.keys if k not in table}, key=repr)
    assert not unmatched, "train-mode launches that are not rows of the tables:\n%s" % "\n".join(map(repr, unmatched))
    assert stats_key(("1d", 0, True, True, True)) in rec.keys and stats_key(("1d", 0, True, False, True)) in rec.keys
    assert any(k[0] == "dropout" and k[4] and k[5] for k in rec.keys)


# --------------------------------------------------------------------------------------
# 5. host checks
# --------------------------------------------------------------------------------------
@gpu
def test_argument_checks():
    """Refusals are return codes on valid buffers, before anything is launched (VFX_EINVAL -1, VFX_EALIGN -2)."""
    lib = _lib.lib()
    z = lambda *shape: torch.zeros(shape, device=DEV)
    g1, sc, sh = torch.ones(8, device=DEV), z(64), z(64)
    buf = z(4096)
    rk = torch.zeros((2, 3), dtype=torch.int32, device=DEV)
    einval, ealign = r"vfx_\w+ failed with code -1$", r"vfx_\w+ failed with code -2$"
    torch.cuda.synchronize()
    before = lib.vfx_launch_count()
    ok = buf.as_strided((2, 4, 8), (512, 8, 1))
    refusals = [
        ("cstride < span (1-D, C > 1)", einval, lambda: ops.bn_stats(buf.as_strided((2, 4, 8), (512, 4, 1)), 8, 0, g1, g1, sc, sh)),
        ("pitch_log2 = 8", einval, lambda: ops.bn_stats(buf.as_strided((2, 2, 512), (1024, 512, 1)), 512, 8, g1, g1, sc, sh)),
        ("L no multiple of P", einval, lambda: ops.bn_stats(buf.as_strided((2, 4, 20), (512, 32, 1)), 20, 3, g1, g1, sc, sh)),
        ("unaligned pointer", ealign, lambda: ops.bn_stats(buf[1:].as_strided((2, 4, 8), (512, 8, 1)), 8, 0, g1, g1, sc, sh)),
        ("eps = 0", einval, lambda: ops.bn_stats(ok, 8, 0, g1, g1, sc, sh, eps=0.0)),
        ("groups neither 1 nor C", einval, lambda: ops.bn_apply(ok, ok, 8, 0, sc, sh, groups=2)),
        ("dropout C = 6", einval, lambda: ops.dropout(buf.as_strided((2, 6, 8), (512, 8, 1)), 8, rk, 0)),
        ("dropout layer = -1", einval, lambda: ops.dropout(ok, 8, rk, -1)),
    ]
    for name, code, call in refusals:
        with pytest.raises(_lib.VfxError, match=code):
            call()
            pytest.fail("accepted: " + name)
    torch.cuda.synchronize()
    assert lib.vfx_launch_count() == before, "a refused call launched something"
    ops.bn_stats(ok, 8, 0, g1, g1, sc, sh)                 # the same buffers, valid arguments: accepted
    ops.bn_apply(ok, ok, 8, 0, sc, sh, groups=4)
    ops.dropout(ok, 8, rk, 1)
    torch.cuda.synchronize()
    assert lib.vfx_launch_count() == before + 4
    for g in GEOMS:
        assert lib.vfx_bn_stats_workspace_bytes(B, g.C, g.L, g.lp) == B * g.G * g.nblk * 24, g.id
    assert lib.vfx_bn_stats_workspace_bytes(B, 4, 20, 3) == 0 and lib.vfx_bn_stats_workspace_bytes(0, 4, 8, 0) == 0
