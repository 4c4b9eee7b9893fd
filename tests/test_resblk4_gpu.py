"""resblk4_kernel and resblk4s_kernel (voicefixer_amd/csrc/vfx_resblk4.inc, vfx_resblk4s.inc; vfx_last_conv_tile() % 100 == 96 / 97:
one whole C = 64 ResStack layer, both convolutions as Winograd F(4,3), on the block tile for d = 1, 3, 9, 27 and on the strip
tile for d = 81 .. 2187) at every launch the product makes, against float64.

* ``test_launch_census`` runs the seeded pipeline at the five geometries of tests/test_conv_taps_gpu.py under
  voicefixer_amd.launch_record and asserts that every code-96 / 97 launch is a row of ``CASES``; the key is (code, d, post,
  post slope, bias pair present, row tags).  The eight ``resblock_wino4`` launches of a run are pinned in order.
* ``test_case_parity`` launches every row of ``CASES`` at a reduced size (C = 64 is the product's whole fp32 chain; only B and L
  shrink), once with unit gains and once with heavy-tailed weight-norm gains and unit-scale biases.
* ``test_edge_parity`` does the same for the index arithmetic and the options the product does not reach (``EDGES``).
* ``test_ragged_rows_equal_the_rows_alone``, ``test_batch_items_are_independent``, ``test_resblock_entry_runs_the_same_kernel``:
  exact properties.

Every (d, L) is first walked by the CPU model of the tile geometry (tests/test_resblk4_geometry_cpu.py: ``check``); only what
it passes is launched.  Buffers are laid out as engine.forward_cond lays out xs / ys: guarded views with guard G_DIL rounded
up to 4, NaN in the guard bands and past every row's own end of x, y NaN-filled.  Every launch asserts the tile code and one
launch, no NaN in [0, len_b) of any row, nothing but NaN everywhere else in the y allocation, and x unchanged bit for bit.

The figure is ``conv_error`` against ``f64_reference.resblock`` and its ``magnitude=True`` twin, per output:
|got - ref| / (lip * M + |ref|).  The bound is measured on the reference side, on ``f64_reference.resblock_f43_f32`` -- a plain
fp32 statement of the same algorithm with bias and residual added after the output transforms: the device may be at most
MARGIN = 4 times worse, maximum and RMS, with the floors of tests/test_conv_taps_gpu.py.  The device forms the same products in
another order, which moves a rounding error by a small factor, not by its order.  Every case prints
``PARITY <id> <stmt max> <dev max> <ratio> <stmt rms> <dev rms> <ratio> direct <max> <rms>`` (the last two: torch's direct fp32
operators) before it asserts; profiles/resblk4_parity.txt is that output.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from voicefixer_amd import ops, packing, _lib  # noqa: E402
from oracle import f64_reference as ref64  # noqa: E402
from test_conv_taps_gpu import GEOMETRIES, MARGIN, RMS_FLOOR, ULP, _Acc, _census, pipe  # noqa: E402,F401
import test_resblk4_geometry_cpu as geo  # noqa: E402

DEV = "cuda"
NAN = float("nan")
C64 = 64
G_DIL4 = 2452            # engine.G_DIL = 3^7 + 264, rounded up to 4: the guard of the stage's xs / ys
NONE, LRELU, SNAKE = _lib.POST_NONE, _lib.POST_LRELU, _lib.POST_LRELU_SNAKE
POST_NAMES = {NONE: "none", LRELU: "lrelu", SNAKE: "snake"}

# code, d, post, post slope, bias pair present, row tags: every distinct launch of the two kernels in the five census
# geometries (test_launch_census keeps the table complete)
CASES = ([(geo.code_of(3 ** i), 3 ** i, LRELU if i == 7 else NONE, 0.2 if i == 7 else 0.0, True, False) for i in range(8)] +
         [(geo.code_of(3 ** i), 3 ** i, LRELU if i == 7 else NONE, 0.2 if i == 7 else 0.0, True, True) for i in range(8)])


def case_key_id(key):
    code, d, post, ps, bias, rows = key
    return "k%d-d%d-%s%s%s%s" % (code, d, POST_NAMES[post], ("%g" % ps) if post != NONE else "", "-bias" if bias else "",
                                 "-rows" if rows else "")


# --------------------------------------------------------------------------------------
# one launch
# --------------------------------------------------------------------------------------
def make_spec(d, L, B=2, rows=False, lengths=None, post=NONE, post_slope=0.0, slope=0.01, heavy=False, b1=True, b2=True,
              w2_scale=1.0, y_guard=G_DIL4, y_wpad=0, y_cpad=0):
    if rows and lengths is None:
        lengths = geo.ragged_lengths(d, L)
        B = len(lengths)
    if lengths is not None:
        assert len(lengths) == B and lengths[0] == L and max(lengths) == L, "row 0 fills the capacity"
    return dict(d=d, L=L, B=B, lengths=lengths, post=post, post_slope=post_slope, slope=slope, heavy=heavy, b1=b1, b2=b2,
                w2_scale=w2_scale, y_guard=y_guard, y_wpad=y_wpad, y_cpad=y_cpad)


def _rand(shape, gen, scale=1.0):
    return torch.randn(shape, generator=gen) * scale


def _up4(n):
    return (n + 3) // 4 * 4


def _inputs(spec, seed):
    """CPU fp32 operands in torch's layouts, as tests/test_convtw_gpu.py draws them: unit-variance activations, weights scaled
    by fan-in^-1/2 and biases of 0.3; `heavy`: both convolutions' weights times a log-normal gain per output channel,
    exp(1.5 z - 2.25) (trained weight-norm gains), and unit-scale biases, so that some channels are all bias (first
    convolution) or all residual (second).  Biases are drawn per channel: a gather by the wrong index shows."""
    g = torch.Generator().manual_seed(seed)
    t = {}
    for k in ("w1", "w2"):
        t[k] = _rand((C64, C64, 3), g, (3 * C64) ** -0.5)
        if spec["heavy"]:
            t[k] = t[k] * torch.exp(1.5 * _rand((C64,), g) - 2.25).reshape(-1, 1, 1)
    t["w2"] = t["w2"] * spec["w2_scale"]
    for k in ("b1", "b2"):
        b = _rand((C64,), g, 1.0 if spec["heavy"] else 0.3)
        t[k] = b if spec[k] else None
    t["x"] = _rand((spec["B"], C64, spec["L"]), g)
    return t


@functools.lru_cache(maxsize=None)
def _model_passes(d, L, n):
    geo.check(d, L, n)
    return True


def launch(spec, seed, t=None, entry="wino4"):
    """Launch `spec` once and hold it to the tile code, the launch count and the canaries.  Returns (device output as a dense
    (B, 64, L) fp32 CPU tensor with NaN past every row's own end, the operands)."""
    d, L, B = spec["d"], spec["L"], spec["B"]
    lens = spec["lengths"] if spec["lengths"] is not None else [L] * B
    for n in set(lens):
        assert _model_passes(d, L, n)                     # the CPU model of the tile geometry first: never launch what it fails
    t = _inputs(spec, seed) if t is None else t
    xbase = torch.full((B, C64, G_DIL4 + _up4(L) + G_DIL4), NAN, device=DEV)
    xv = xbase[:, :, G_DIL4:G_DIL4 + _up4(L)]
    xd = t["x"].to(DEV)
    for n in sorted(set(lens)):
        idx = torch.tensor([b for b in range(B) if lens[b] == n], device=DEV)
        xv[idx, :, :n] = xd[idx, :, :n]
    xv._vfx_guard, xv._vfx_base = G_DIL4, xbase
    gy, cpad = spec["y_guard"], spec["y_cpad"]
    assert gy % 4 == 0 and spec["y_wpad"] % 4 == 0, "rows of y stay 16-byte aligned"
    ybase = torch.full((B, C64 + 2 * cpad, gy + _up4(L) + gy + spec["y_wpad"]), NAN, device=DEV)
    yv = ybase[:, cpad:cpad + C64, gy:gy + _up4(L)]
    yv._vfx_guard, yv._vfx_base = gy, ybase
    if spec["lengths"] is not None:
        rows = torch.tensor(lens, dtype=torch.int32, device=DEV)
        ops.with_rows(xv, rows)
        ops.with_rows(yv, rows)
    p1, p2 = packing.pack_conv1d(t["w1"]), packing.pack_conv1d(t["w2"])
    w1g4, w2g4 = packing.pack_wino4(p1).to(DEV), packing.pack_wino4(p2).to(DEV)
    b1 = t["b1"].to(DEV) if t["b1"] is not None else None
    b2 = t["b2"].to(DEV) if t["b2"] is not None else None
    xkeep = xbase.clone()
    lib = _lib.lib()
    torch.cuda.synchronize()
    before = lib.vfx_launch_count()
    if entry == "wino4":
        ops.resblock_wino4(xv, yv, w1g4, b1, w2g4, b2, L, d, spec["slope"], spec["post"], spec["post_slope"])
    else:
        ops.resblock(xv, yv, packing.pack_direct(p1).to(DEV), b1, packing.pack_direct(p2).to(DEV), b2, L, d, spec["slope"],
                     spec["post"], spec["post_slope"], w2g=packing.pack_wino(p2).to(DEV), w2g4=w2g4, w1g4=w1g4)
    torch.cuda.synchronize()
    tile, launches = lib.vfx_last_conv_tile(), int(lib.vfx_launch_count() - before)
    assert tile % 100 == geo.code_of(d), "ran as %d, expected code %d" % (tile, geo.code_of(d))
    assert launches == 1
    # ---- canaries: NaN past each row's own end, past the capacity, in the guard bands and the neighbouring channels
    allowed = torch.zeros(ybase.shape, dtype=torch.bool, device=DEV)
    av = allowed[:, cpad:cpad + C64, gy:gy + _up4(L)]
    for n in sorted(set(lens)):
        idx = torch.tensor([b for b in range(B) if lens[b] == n], device=DEV)
        av[idx, :, :n] = True
    stray = ~(torch.isnan(ybase) | allowed)
    assert not bool(stray.any()), "%d elements outside the valid output were written" % int(stray.sum())
    assert not bool((torch.isnan(ybase) & allowed).any()), "NaN inside [0, len) of a row"
    assert torch.equal(xbase.view(torch.int32), xkeep.view(torch.int32)), "x was written"
    return yv[:, :, :L].detach().cpu().contiguous(), t


def _kw(spec):
    return dict(slope=spec["slope"], post=spec["post"], post_slope=spec["post_slope"], lengths=spec["lengths"])


def direct32(spec, t):
    """The layer as torch's direct fp32 CPU operators, every row of a ragged batch alone."""
    d, L, B, s = spec["d"], spec["L"], spec["B"], spec["slope"]
    lens = spec["lengths"] if spec["lengths"] is not None else [L] * B
    full = torch.full((B, C64, L), NAN)
    for n in sorted(set(lens)):
        idx = [b for b in range(B) if lens[b] == n]
        x = t["x"][idx][:, :, :n]
        mid = F.conv1d(F.leaky_relu(x, s), t["w1"], t["b1"], dilation=d, padding=d)
        y = x + F.conv1d(F.leaky_relu(mid, s), t["w2"], t["b2"], padding=1)
        if spec["post"] != NONE:
            y = F.leaky_relu(y, spec["post_slope"])
            y = y + torch.sin(y) if spec["post"] == SNAKE else y
        full[idx, :, :n] = y
    return full


def score(spec, t, got):
    """`got`, the fp32 F(4,3) statement and torch's direct fp32 operators, each against the float64 statement -- every row of
    a ragged batch against the layer applied to that row alone.  Returns three _Acc (device, statement, direct)."""
    a = (t["x"], t["w1"], t["b1"], t["w2"], t["b2"], spec["d"])
    with torch.no_grad():
        ref = ref64.resblock(*a, **_kw(spec))
        mag = ref64.resblock(*a, slope=spec["slope"], lengths=spec["lengths"], magnitude=True)
        stmt = ref64.resblock_f43_f32(*a, **_kw(spec))
        dire = direct32(spec, t)
    assert got.shape == ref.shape
    lip = ref64.post_lipschitz(spec["post"])
    accs = []
    for y in (got, stmt, dire):
        acc = _Acc()
        acc.add(ref64.conv_error(y, ref, mag, lip))
        accs.append(acc)
    return accs


def check(name, dev, cpu, dire):
    """Print the figures, then assert: the device at most MARGIN x the yardstick `cpu`, maximum and RMS, with the floors."""
    print("PARITY %s %.3e %.3e %.2f %.3e %.3e %.2f direct %.3e %.3e" % (
        name, cpu.mx, dev.mx, dev.mx / max(cpu.mx, ULP), cpu.rms, dev.rms, dev.rms / max(cpu.rms, RMS_FLOOR), dire.mx, dire.rms))
    assert dev.n > 0 and dev.n == cpu.n
    assert dev.mx <= MARGIN * max(cpu.mx, ULP), "%s: max figure %.3e exceeds %.0f x the yardstick's %.3e" % (name, dev.mx, MARGIN, cpu.mx)
    assert dev.rms <= MARGIN * max(cpu.rms, RMS_FLOOR), "%s: RMS figure %.3e exceeds %.0f x the yardstick's %.3e" % (name, dev.rms, MARGIN, cpu.rms)


def run_case(spec, seed, name):
    got, t = launch(spec, seed)
    dev, stmt, dire = score(spec, t, got)
    check(name, dev, stmt, dire)
    return got, t


# --------------------------------------------------------------------------------------
# the product's launches
# --------------------------------------------------------------------------------------
def record_key(r):
    return (r["code"], r["step"], r["post"], r["post_slope"] if r["post"] != NONE else 0.0, all(r["bias_pair"]), r["rows"])


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_launch_census(pipe, geometry):  # noqa: F811
    """Every resblk4_kernel / resblk4s_kernel launch of the seeded pipeline at this geometry is a row of CASES, and the C = 64
    stage is exactly eight resblock_wino4 launches, d = 3^0 .. 3^7 in order, four on each kernel: adding, removing or
    re-routing a product launch on these kernels fails here.  The other stages' layers do not come through ops.resblock in
    the default product (they run as two Winograd launches per layer)."""
    table = set(CASES)
    rec = _census(pipe, geometry)
    rb = rec.rb4()
    unmatched = [record_key(r) for r in rb if record_key(r) not in table]
    wino = [r for r in rec.records if r["op"] == "resblock_wino4"]
    other = [r for r in rec.records if r["op"] == "resblock"]
    print("CENSUS %s: %d conv-family calls, %d resblock_wino4 (codes %r), %d resblock (%r), %d on codes 96 / 97, %d unmatched" % (
        geometry, len(rec.records), len(wino), [r["code"] for r in wino], len(other),
        sorted({(r["cin"], r["step"], r["code"]) for r in other}), len(rb), len(unmatched)))
    assert not unmatched, "launches on codes 96 / 97 that are not rows of CASES:\n%s" % "\n".join(map(repr, sorted(set(unmatched))))
    assert [r["step"] for r in wino] == [3 ** i for i in range(8)]
    assert tuple(r["code"] for r in wino) == (96, 96, 96, 96, 97, 97, 97, 97)
    for i, r in enumerate(wino):
        assert r["cin"] == C64 and r["launches"] == 1 and r["guarded"] and r["unit"] and r["slope"] == 0.01, r
        assert (r["post"], r["post_slope"]) == ((LRELU, 0.2) if i == 7 else (NONE, 0.0)), r
        assert r["bias_pair"] == (True, True) and r["rows"] == (geometry == "ragged5"), r
    assert not other, "ops.resblock launches in the default product"
    assert len(rb) == len(wino) == 8 and all(a is b for a, b in zip(rb, wino))


def _case_spec(key, heavy):
    """The reduced launch of a CASES row.  Block tile: B = 2, L = 2 bl_step + 23 (two whole tiles and a third that ends inside a
    quad).  Strip tile: B = 2, L = 5d + W + 3 (one whole block of 4d positions, then a second cut inside strip 1, part-way
    through a segment; every strip boundary with r >= d is crossed).  Ragged rows: B = 6 with lengths (L, 1, max(2, d - 1),
    d + 13, 4d, 4d + 1)."""
    code, d, post, ps, bias, rows = key
    g = geo.geometry(d)
    L = geo.case_length(d)
    assert geo.code_of(d) == code
    if g["strip"]:
        assert L == 5 * d + g["W"] + 3 and g["W"] + 3 < d and g["nseg"] >= 2     # strip 1 of block 1 ends at r = W + 3: inside segment 1
    else:
        assert geo.ntiles_of(g, L) == 3 and L % 4 != 0
    return make_spec(d, L, rows=rows, post=post, post_slope=ps, heavy=heavy, b1=bias, b2=bias)


@pytest.mark.parametrize("gains", ["unit", "heavy"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=[case_key_id(k) for k in CASES])
def test_case_parity(i, gains):
    """Every row of CASES at its reduced size, with unit gains and with heavy-tailed ones (profiles/resblk4_parity.txt).

    Finding, fixed in the kernel; these are its regression cases.  While the second half started planes 0, 1, 3 and 5 at the
    solution of A^T m = x + b2, every later partial sum was rounded at several times the residual, and the output transform
    multiplied that by up to 8: all 16 rows with heavy-tailed gains measured 30 - 253 x the fp32 statement's maximum and
    10 - 20 x its RMS (k97-d729-none-bias-heavy: 2.38e-05 against 6.36e-08), the rows with unit gains 2.0 - 5.5 x / 0.9 - 1.5 x
    (four of 16 above the bound), and 70 of the 121 edges failed.  With all six planes started at zero and b2 and the
    residual added after the output transform every row is at 0.34 - 1.29 x / 0.25 - 0.69 x and the worst edge at 1.5 x / 0.9 x.
    b1 as the start value of the FIRST half's plane 1 -- the construction convtw_kernel had to give up -- was measured both
    ways and left as it is: 0.34 - 1.21 x / 0.25 - 0.65 x with b1 added after the transform between the halves instead."""
    run_case(_case_spec(CASES[i], gains == "heavy"), 3000 + 2 * i + (gains == "heavy"), case_key_id(CASES[i]) + "-" + gains)


def test_cases_are_distinct():
    assert len(set(CASES)) == len(CASES) == 16
    for code, d, post, ps, bias, rows in CASES:
        assert code == geo.code_of(d)


# --------------------------------------------------------------------------------------
# edges the product does not reach
# --------------------------------------------------------------------------------------
BLOCK_DILATIONS = (1, 2, 4, 5, 6, 7, 8, 10, 12, 13, 16, 17, 21, 24, 32)      # every block count nb the block tile takes (3, 9: CASES) ...
STRIP_DILATIONS = (22, 23, 33, 28, 29, 56, 57, 60, 61, 84, 85, 120, 121, 64, 100, 4096)   # ... what it declines, pitch changes, even d
PROBES = (3, 81, 729)                                                         # block tile, strip P = 32, strip P = 64
XCD_LENGTHS = geo.XCD_LENGTHS


def _e(name, d, L, **extra):
    return (name, dict(d=d, L=L, **extra))


def _edges():
    e = []
    for d in BLOCK_DILATIONS + STRIP_DILATIONS:
        e.append(_e("d%d" % d, d, geo.case_length(d), rows=(d % 3 == 1)))
    for d in PROBES:
        for L in geo.edge_lengths(d):
            e.append(_e("d%d-L%d" % (d, L), d, L))
    # XCD tile order: fewer than 64 tiles (linear), 64 and more with a count that is no multiple of 8 (the early return;
    # ragged with a row that ends half-way: tiles past it return as well), and a multiple of 8
    for d in sorted(XCD_LENGTHS):
        for j, L in enumerate(XCD_LENGTHS[d]):
            e.append(_e("d%d-xcd%d" % (d, geo.ntiles_of(geo.geometry(d), L)), d, L, B=2 if j == 1 else 1,
                        lengths=[L, L // 2 + 1] if j == 1 else None))
    for d in PROBES:
        L = geo.case_length(d)
        e.append(_e("d%d-post-none" % d, d, L, post=NONE))
        for post in (LRELU, SNAKE):
            for ps in (0.0, 0.2, 1.0):
                e.append(_e("d%d-post-%s%g" % (d, POST_NAMES[post], ps), d, L, post=post, post_slope=ps, rows=(ps == 0.2)))
        for s in (0.0, 1.0):
            e.append(_e("d%d-slope%g" % (d, s), d, L, slope=s))
        # biases absent (the kernel then points its bias resource at x, with an out-of-range offset)
        e.append(_e("d%d-nob1" % d, d, L, b1=False))
        e.append(_e("d%d-nob2" % d, d, L, b2=False, rows=True))
        e.append(_e("d%d-nobias" % d, d, L, b1=False, b2=False))
        # second convolution with zero weights: the output is post(x + b2), the figure's denominator the residual alone
        e.append(_e("d%d-w2zero" % d, d, L, w2_scale=0.0, heavy=True))
        e.append(_e("d%d-w2zero-rows-snake" % d, d, L, w2_scale=0.0, heavy=True, rows=True, post=SNAKE, post_slope=0.2))
        # output layout: another guard than x, a channel stride that is a multiple of 4 and not of 16 floats, padding channels
        e.append(_e("d%d-ylayout" % d, d, L, y_guard=8, y_wpad=4 + (_up4(L) % 16 == 12) * 4, y_cpad=3, rows=True))
    return e


EDGES = _edges()


def _edge_spec(i):
    kw = dict(EDGES[i][1])
    kw.setdefault("heavy", i % 2 == 1)
    return make_spec(kw.pop("d"), kw.pop("L"), **kw)


@pytest.mark.parametrize("i", range(len(EDGES)), ids=[e[0] for e in EDGES])
def test_edge_parity(i):
    run_case(_edge_spec(i), 7000 + i, EDGES[i][0])


def test_edges_reach_what_they_are_meant_to():
    assert len({e[0] for e in EDGES}) == len(EDGES)
    specs = [_edge_spec(i) for i in range(len(EDGES))]
    for s in specs:
        assert s["B"] <= 6 and s["L"] <= 21000
    geos = [geo.geometry(s["d"]) for s in specs]
    blocks = [(s, g) for s, g in zip(specs, geos) if not g["strip"]]
    strips = [(s, g) for s, g in zip(specs, geos) if g["strip"]]
    # dilations: every block count the block tile takes, what it declines below 33, both pitches, even and odd d, d = 4096
    assert {g["nb"] for _, g in blocks} | {7} == {geo.block_geometry(d)["nb"] for d in range(1, 33) if geo.takes(d)}     # (nb = 7: d = 9 of CASES)
    assert {s["d"] for s, _ in blocks} >= {1, 2, 5, 7, 12, 13, 16, 17, 21, 24, 32}
    assert {s["d"] for s, _ in strips} >= {22, 23, 33, 56, 57, 60, 61, 84, 85, 120, 121, 64, 100, 4096}
    assert {s["d"] for s, _ in blocks} >= {28, 29}     # (the strip rule changes pitch there, but the block tile takes both)
    assert {g["P"] for _, g in strips} == {32, 64} and {g["P"] for s, g in strips if s["d"] % 2 == 0} == {32, 64}
    for a, b in ((60, 61), (84, 85), (120, 121)):
        assert geo.strip_geometry(a)["P"] != geo.strip_geometry(b)["P"]
    assert [geo.geometry(d)["strip"] and geo.geometry(d)["P"] for d in PROBES] == [False, 32, 64]
    for d in PROBES:
        mine = [s for s in specs if s["d"] == d]
        g = geo.geometry(d)
        want = {1, 2, 3, 4, 5, d - 1, d, d + 1, 4 * d - 1, 4 * d, 4 * d + 1}
        want |= {4 * d + g["W"] - 1, 4 * d + g["W"], 4 * d + g["W"] + 1} if g["strip"] else {g["bl_step"] - 1, g["bl_step"], g["bl_step"] + 1}
        assert {s["L"] for s in mine if s["lengths"] is None} >= want
        assert {(s["post"], s["post_slope"]) for s in mine} >= {(NONE, 0.0)} | {(p, v) for p in (LRELU, SNAKE) for v in (0.0, 0.2, 1.0)}
        assert {s["slope"] for s in mine} == {0.0, 0.01, 1.0}
        assert {(s["b1"], s["b2"]) for s in mine} == {(True, True), (False, True), (True, False), (False, False)}
        assert any(s["w2_scale"] == 0.0 and s["heavy"] for s in mine)
        lay = [s for s in mine if s["y_cpad"]]
        assert lay and all(s["y_guard"] != G_DIL4 and (2 * s["y_guard"] + _up4(s["L"]) + s["y_wpad"]) % 16 in (4, 8, 12) for s in lay)
        assert any(s["lengths"] is not None for s in mine) and any(s["heavy"] for s in mine) and any(not s["heavy"] for s in mine)
    # tails: block tiles that end inside a quad and on a quad's end; XCD order: linear, remapped with and without the early return
    assert any(s["L"] % 4 for s, _ in blocks) and any(s["L"] % 4 == 0 for s, _ in blocks)
    for kind in (False, True):
        nts = [geo.ntiles_of(g, s["L"]) for s, g in zip(specs, geos) if g["strip"] == kind]
        assert any(n < 64 for n in nts) and any(n >= 64 and n % 8 for n in nts) and any(n >= 64 and n % 8 == 0 for n in nts)


# --------------------------------------------------------------------------------------
# exact properties
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [9, 81, 729])
def test_ragged_rows_equal_the_rows_alone(d):
    """Row b of a ragged launch is bit-equal to that row in a plain launch of its own length: the tile grids of both kernels
    depend on d only, so the order of every sum depends on nothing but the row."""
    L = geo.case_length(d)
    spec = make_spec(d, L, rows=True, heavy=True, post=SNAKE, post_slope=0.2)
    got, t = launch(spec, 8200 + d)
    for b, n in enumerate(spec["lengths"]):
        alone = make_spec(d, n, B=1, heavy=True, post=SNAKE, post_slope=0.2)
        ya, _ = launch(alone, 0, t=dict(t, x=t["x"][b:b + 1, :, :n].contiguous()))
        assert torch.equal(got[b, :, :n], ya[0]), "row %d of length %d" % (b, n)


@pytest.mark.parametrize("d", [9, 81, 729])
def test_batch_items_are_independent(d):
    """The same row at batch index 0 and 3 of a B = 4 launch, with different neighbours, is bit-equal."""
    spec = make_spec(d, geo.case_length(d), B=4, heavy=True)
    t = _inputs(spec, 8300 + d)
    t["x"][3] = t["x"][0]
    got, _ = launch(spec, 0, t=t)
    assert torch.equal(got[0], got[3]) and not torch.equal(got[0], got[1])


@pytest.mark.parametrize("d", [1, 3, 9, 27])
def test_resblock_entry_runs_the_same_kernel(d):
    """ops.resblock with both F(4,3) weight sets at d <= 27 is vfx_resblock_f32 -> resblk4_kernel: the same bits as
    ops.resblock_wino4 (launch() asserts code 96 and one launch for both)."""
    spec = make_spec(d, geo.case_length(d), rows=(d == 9), post=LRELU, post_slope=0.2)
    a, t = launch(spec, 8400 + d)
    b, _ = launch(spec, 0, t=t, entry="resblock")
    assert torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0))
