"""convtw_kernel (voicefixer_amd/csrc/vfx_convtw.inc, vfx_last_conv_tile() % 100 == 83: the transposed convolutions of the
UpsampleNet as Winograd F(3,2) along the input axis) at every launch the product makes, against float64.

* ``test_launch_census`` runs the seeded pipeline at the five geometries of tests/test_conv_taps_gpu.py under
  voicefixer_amd.launch_record and asserts that every code-83 launch is a row of ``CASES``.  The key is (BM, Cin, Cout, s,
  bias, row tags, work order); the work order is derived here from the host's rule (16 s Cin Cout bytes of transformed
  weights <= 3 MB: row block fastest, else tile fastest).  ``CENSUS`` pins which kernel each of the four UpsampleNet
  launches of a geometry runs on.
* ``test_case_parity`` launches every row of ``CASES`` once at the product's Cin (the length of the fp32 chain), with Cout
  cut to one or two row blocks, two tiles of input with the last triple incomplete, and the least batch that reaches the
  kernel's 512 workgroups; once with unit gains and once with heavy-tailed weight-norm gains and a unit-scale bias.
* ``test_edge_parity`` does the same for the index arithmetic the product does not reach (``EDGES``).
* ``test_zero_weights_return_the_bias`` and ``test_ragged_rows_equal_the_rows_alone``: two exact properties.
* ``test_declined_*``: what the kernel's host side refuses runs elsewhere (or nowhere) and stays right.

Buffers are laid out as engine.forward_cond lays them out: x is a guarded view with NaN in its guard bands and past every
row's own length; y is a NaN-filled guarded buffer.  Every launch asserts the tile code and one launch, no NaN in
[0, s len_b) of any row and nothing but NaN everywhere else in the allocation.

The figure is ``conv_error`` against ``f64_reference.convtr1d`` and its ``magnitude=True`` twin, per output:
|got - ref| / (magnitude + |ref|).  The bound is measured on the reference side, on ``f64_reference.convtr1d_f32_f32`` -- a
plain fp32 statement of the same algorithm: the device may be at most MARGIN = 4 times worse, maximum and RMS, with the
floors of tests/test_conv_taps_gpu.py (4 x 2^-23, 4 x 2^-24 / sqrt(3) / 2).  The device forms the same products in another
order (pairs of channels per MFMA, one chain over all of Cin), which moves a rounding error by a small factor, not by its
order.  Every case prints ``PARITY <id> <stmt max> <dev max> <ratio> <stmt rms> <dev rms> <ratio> direct <max> <rms>``
(the last two: torch's direct fp32 operator) before it asserts; profiles/convtw_parity.txt is that output.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from voicefixer_amd import ops, packing, _lib  # noqa: E402
from oracle import f64_reference as ref64  # noqa: E402
from test_conv_taps_gpu import GEOMETRIES, MARGIN, RMS_FLOOR, ULP, _Acc, _census, pipe  # noqa: E402,F401

DEV = "cuda"
NAN = float("nan")
MIN_WGS = 512            # try_launch_convtw: smaller launches stay on the direct kernels
G_IN, G_OUT = 264, 2452  # engine.G_TILE; engine.G_DIL rounded up to 4: the guards of an UpsampleNet stage's input and output

# BM, Cin, Cout, s, bias, row tags, work order: every distinct convtw_kernel launch of the five census geometries
# (test_launch_census keeps the table complete)
CASES = [
    # batch 32 x 10 s, batch 8 x 30 s, mode 2 at batch 4 x 10 s: up1 .. up4
    (128, 1024, 512, 7, True, False, "tile"),
    (128, 512, 256, 7, True, False, "tile"),
    (128, 256, 128, 3, True, False, "rowblock"),
    (64, 128, 64, 3, True, False, "rowblock"),
    # ragged mode-0 batch of five rows
    (128, 1024, 512, 7, True, True, "tile"),
    (128, 512, 256, 7, True, True, "tile"),
    (128, 256, 128, 3, True, True, "rowblock"),
    (64, 128, 64, 3, True, True, "rowblock"),
]

# geometry -> vfx_last_conv_tile() % 100 of the four convtr1d launches, up1 .. up4.  Batch 1 x 10 s: up1 has 11 tiles x 7
# phases x 4 row blocks = 308 workgroups, below the 512 this kernel asks for, and runs on conv_taps_kernel (K-chunk 8: a
# row of tests/test_conv_taps_gpu.py's CASES); up2 .. up4 reach 512 on their own length.  The fallback kernels are not
# held to the bound of this file.
CENSUS = {"b32x10": (83, 83, 83, 83), "b1x10": (8, 83, 83, 83), "b8x30": (83, 83, 83, 83), "ragged5": (83, 83, 83, 83),
          "train4x10": (83, 83, 83, 83)}


# --------------------------------------------------------------------------------------
# geometry of a launch
# --------------------------------------------------------------------------------------
def tile_of(cout):
    """(BM, BT) of the instance the host picks: <4,1> (128 rows x 32 triples) when Cout % 128 == 0, else <2,2> (64 x 64)."""
    return (128, 32) if cout % 128 == 0 else (64, 64)


def ntiles_of(Lin, cout):
    return -(-((Lin + 1 + 2) // 3) // tile_of(cout)[1])


def nwg_of(s, cout, Lin):
    """Workgroups per batch item: tiles x the row blocks of the s Cout rows."""
    return ntiles_of(Lin, cout) * s * (cout // tile_of(cout)[0])


def order_of(s, cin, cout):
    """The host's rule: row block fastest while the transformed weights of all rows fit an XCD's L2 together."""
    return "rowblock" if 16 * s * cin * cout <= (3 << 20) else "tile"


def batch_for(s, cout, Lin):
    return -(-MIN_WGS // nwg_of(s, cout, Lin))


def expected_tile(cout):
    BM, BT = tile_of(cout)
    return BM * 100000 + 3 * BT * 100 + 83


def ragged_lengths(B, Lin, BT):
    """Per-row input lengths of a ragged launch, cycled over the batch; row 0 fills the capacity."""
    ls = [Lin, 1, 2, 3, 3 * BT - 1, 3 * BT, max(1, Lin - 1), max(1, Lin // 2)]
    return [min(Lin, ls[b % len(ls)]) for b in range(B)]


def make_spec(cin, cout, s, Lin, bias=True, rows=False, heavy=False, **extra):
    spec = dict(cin=cin, cout=cout, s=s, Lin=Lin, bias=bias, rows=rows, heavy=heavy, w_scale=1.0, y_guard=8, y_cpad=4, y_off=0,
                y_wpad=0, lengths=None)
    spec.update(extra)
    spec.setdefault("B", batch_for(s, cout, Lin))
    if rows and spec["lengths"] is None:
        spec["lengths"] = ragged_lengths(spec["B"], Lin, tile_of(cout)[1])
    return spec


def case_key_id(key):
    BM, cin, cout, s, bias, rows, order = key
    return "BM%d-%dto%d-s%d%s%s-%s" % (BM, cin, cout, s, "-bias" if bias else "", "-rows" if rows else "", order)


# --------------------------------------------------------------------------------------
# one launch
# --------------------------------------------------------------------------------------
def _rand(shape, gen, scale=1.0):
    return torch.randn(shape, generator=gen) * scale


def _up4(n):
    return (n + 3) // 4 * 4


def _inputs(spec, seed):
    """CPU fp32 operands in torch's layouts: unit-variance activations, weights scaled by fan-in^-1/2 and a bias of 0.3;
    `heavy`: the weights times a log-normal gain per output channel, exp(1.5 z - 2.25), as tests/test_conv_taps_gpu.py
    draws them (trained weight-norm gains), and a unit-scale bias, so that some channels are dominated by it.  The bias is
    drawn per channel: a gather by the wrong index shows."""
    g = torch.Generator().manual_seed(seed)
    B, cin, cout, s, Lin = spec["B"], spec["cin"], spec["cout"], spec["s"], spec["Lin"]
    t = {"w": _rand((cin, cout, 2 * s), g, (2 * cin) ** -0.5) * spec["w_scale"]}
    if spec["heavy"]:
        t["w"] = t["w"] * torch.exp(1.5 * _rand((cout,), g) - 2.25).reshape(1, -1, 1)
    t["bias"] = _rand((cout,), g, 1.0 if spec["heavy"] else 0.3) if spec["bias"] else None
    t["x"] = _rand((B, cin, Lin), g)
    return t


def launch(spec, seed, expect83=True, act=None, t=None):
    """Launch `spec` once and hold it to the tile code, the launch count and the canaries.  Returns (device output as a
    dense (B, Cout, s Lin) fp32 CPU tensor with NaN past every row's own end, the operands)."""
    B, cin, cout, s, Lin = spec["B"], spec["cin"], spec["cout"], spec["s"], spec["Lin"]
    lens = spec["lengths"] if spec["lengths"] is not None else [Lin] * B
    t = _inputs(spec, seed) if t is None else t
    xbase = torch.full((B, cin, G_IN + _up4(Lin) + G_IN), NAN, device=DEV)
    xv = xbase[:, :, G_IN:G_IN + _up4(Lin)]
    xd = t["x"].to(DEV)
    for n in sorted(set(lens)):
        idx = torch.tensor([b for b in range(B) if lens[b] == n], device=DEV)
        xv[idx, :, :n] = xd[idx, :, :n]
    xv._vfx_guard = G_IN
    xv._vfx_base = xbase
    if spec["lengths"] is not None:
        ops.with_rows(xv, torch.tensor(lens, dtype=torch.int32, device=DEV))
    Lo, g, cpad, off = s * Lin, spec["y_guard"], spec["y_cpad"], spec["y_off"]
    ybase = torch.full((B, cout + 2 * cpad, g + _up4(Lo) + g + spec["y_wpad"]), NAN, device=DEV)
    yv = ybase[:, cpad:cpad + cout, g + off:g + off + _up4(Lo)]
    assert off <= g and yv.shape[2] == _up4(Lo)
    wp = packing.pack_convtr1d(t["w"])
    wt = packing.pack_wino32_tr(wp, s).to(DEV)
    wd = packing.pack_direct(wp).to(DEV)
    wp = wp.to(DEV)
    bias = t["bias"].to(DEV) if t["bias"] is not None else None
    lib = _lib.lib()
    torch.cuda.synchronize()
    before = lib.vfx_launch_count()
    ops.convtr1d(xv, wp, bias, yv, Lin, s, act, wd=wd, wg4=wt)
    torch.cuda.synchronize()
    tile, launches = lib.vfx_last_conv_tile(), int(lib.vfx_launch_count() - before)
    if expect83:
        assert tile == expected_tile(cout), "ran as %d, expected %d" % (tile, expected_tile(cout))
        assert launches == 1
    else:
        assert tile % 100 != 83 and launches >= 1, "ran as %d" % tile
    # ---- canaries: NaN past each row's own end, past the capacity, in the guard bands and the neighbouring channels
    allowed = torch.zeros(ybase.shape, dtype=torch.bool, device=DEV)
    av = allowed[:, cpad:cpad + cout, g + off:g + off + _up4(Lo)]
    for n in sorted(set(lens)):
        idx = torch.tensor([b for b in range(B) if lens[b] == n], device=DEV)
        av[idx, :, :n * s] = True
    stray = ~(torch.isnan(ybase) | allowed)
    assert not bool(stray.any()), "%d elements outside the valid output were written" % int(stray.sum())
    assert not bool((torch.isnan(ybase) & allowed).any()), "NaN inside [0, s len) of a row"
    return yv[:, :, :Lo].detach().cpu().contiguous(), t


def direct32(spec, t):
    """torch's direct fp32 CPU operator, every row of a ragged batch alone (the full transposed convolution, cut: torch
    takes no output_padding of 1 at stride 1)."""
    s, Lin = spec["s"], spec["Lin"]
    pad = s // 2 + s % 2
    if spec["lengths"] is None:
        return F.conv_transpose1d(t["x"], t["w"], t["bias"], stride=s)[:, :, pad:pad + s * Lin]
    full = torch.full((spec["B"], spec["cout"], s * Lin), NAN)
    for n in sorted(set(spec["lengths"])):
        idx = [b for b in range(spec["B"]) if spec["lengths"][b] == n]
        full[idx, :, :n * s] = F.conv_transpose1d(t["x"][idx][:, :, :n], t["w"], t["bias"], stride=s)[:, :, pad:pad + s * n]
    return full


def score(spec, t, got, yardstick="f32"):
    """`got`, the fp32 F(3,2) statement and torch's direct fp32 operator, each against the float64 statement -- every row
    of a ragged batch against the convolution of that row alone.  Returns three _Acc (device, statement, direct)."""
    s, lengths = spec["s"], spec["lengths"]
    with torch.no_grad():
        ref = ref64.convtr1d(t["x"], t["w"], t["bias"], s, lengths=lengths)
        mag = ref64.convtr1d(t["x"], t["w"], t["bias"], s, lengths=lengths, magnitude=True)
        stmt = ref64.convtr1d_f32_f32(t["x"], t["w"], t["bias"], s, lengths=lengths)
        dire = direct32(spec, t)
    assert got.shape == ref.shape
    accs = []
    for y in (got, stmt, dire):
        a = _Acc()
        a.add(ref64.conv_error(y, ref, mag))
        accs.append(a)
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
    return (r["BM"], r["cin"], r["cout"], r["step"], r["bias"], r["rows"], order_of(r["step"], r["cin"], r["cout"]))


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_launch_census(pipe, geometry):  # noqa: F811
    """Every convtw_kernel launch of the seeded pipeline at this geometry is a row of CASES, and the four UpsampleNet
    launches run on the kernels CENSUS names: adding or removing a product launch on this kernel fails here."""
    table = set(CASES)
    rec = _census(pipe, geometry)
    tw = rec.tw()
    unmatched = []
    for r in tw:
        assert r["op"] == "convtr1d" and r["guarded"] and r["unit"] and r["launches"] == 1, r
        assert r["pre"] == _lib.PRE_NONE and r["post"] == _lib.POST_NONE and r["res"] == "none", r
        assert (r["BM"], r["BL"]) == (tile_of(r["cout"])[0], 3 * tile_of(r["cout"])[1]), r
        if record_key(r) not in table:
            unmatched.append(record_key(r))
    ups = [r for r in rec.records if r["op"] == "convtr1d"]
    print("CENSUS %s: %d conv-family calls, %d convtr1d, %d on convtw_kernel, codes %r, %d unmatched" % (
        geometry, len(rec.records), len(ups), len(tw), [r["code"] for r in ups], len(unmatched)))
    assert not unmatched, "convtw_kernel launches that are not rows of CASES:\n%s" % "\n".join(map(repr, sorted(set(unmatched))))
    assert [(r["cin"], r["cout"], r["step"]) for r in ups] == [(1024, 512, 7), (512, 256, 7), (256, 128, 3), (128, 64, 3)]
    assert tuple(r["code"] for r in ups) == CENSUS[geometry]
    assert len(tw) == sum(c == 83 for c in CENSUS[geometry])
    keys = {record_key(r) for r in tw}
    if geometry != "b1x10":
        assert len(tw) == 4, "four launches on convtw_kernel"
        assert {k[0] for k in keys} == {128, 64} and {k[6] for k in keys} == {"tile", "rowblock"}, "both instances, both work orders"
    assert all(k[5] == (geometry == "ragged5") for k in keys), "row tags on every launch of a ragged batch, and only there"


def _case_spec(key, heavy):
    """The reduced launch of a CASES row: the product's Cin and stride; Cout cut to 128 (<4,1>, one row block per phase)
    or kept at 64 (<2,2>); two tiles of input with the last triple incomplete; the least batch that reaches 512
    workgroups; the output buffer with the stage's guard."""
    BM, cin, cout, s, bias, rows, order = key
    rc = 128 if BM == 128 else 64
    BT = tile_of(rc)[1]
    Lin = 3 * 2 * BT - 2                      # triples cover q = 0 .. Lin: 2 BT of them, the last holds two of its three q
    spec = make_spec(cin, rc, s, Lin, bias=bias, rows=rows, heavy=heavy, y_guard=G_OUT, y_cpad=0)
    assert tile_of(rc)[0] == BM and order_of(s, cin, rc) == order == order_of(s, cin, cout)
    assert ntiles_of(Lin, rc) == 2 and (Lin + 1) % 3 == 2
    assert nwg_of(s, rc, Lin) * spec["B"] >= MIN_WGS > nwg_of(s, rc, Lin) * (spec["B"] - 1)
    return spec


@pytest.mark.parametrize("gains", ["unit", "heavy"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=[case_key_id(k) for k in CASES])
def test_case_parity(i, gains):
    """Every row of CASES at its reduced size, with unit gains and with heavy-tailed ones (profiles/convtw_parity.txt).

    Finding, fixed in the kernel; these are its regression cases.  While the bias entered as the C operand of plane 1's
    first MFMA, every later partial sum of that plane was rounded at the size of the bias: all eight rows with heavy-tailed
    gains measured 3.3 - 14.9 x the fp32 statement's maximum and 5.2 - 11.6 x its RMS (BM128-1024to512-s7-bias-tile-heavy:
    1.78e-06 against 7.91e-08), the rows with unit gains 0.9 - 2.6 x / 1.0 - 1.5 x.  With all four planes started at zero
    and the bias added after the output transform every row is at 0.9 - 2.5 x / 1.0 - 1.5 x; the one fp32 chain over
    Cin = 1024 alone measures 2.5 x / 1.4 x and was left as it is."""
    run_case(_case_spec(CASES[i], gains == "heavy"), 3000 + 2 * i + (gains == "heavy"), case_key_id(CASES[i]) + "-" + gains)


def test_cases_are_distinct():
    assert len(set(CASES)) == len(CASES)
    for key in CASES:
        assert key[0] == tile_of(key[2])[0] and key[6] == order_of(key[3], key[1], key[2])


# --------------------------------------------------------------------------------------
# edges the product does not reach
# --------------------------------------------------------------------------------------
WIDE, NARROW = 128, 64       # Cout of <4,1> / <2,2>


def _e(name, cin, cout, s, Lin, **extra):
    return (name, dict(cin=cin, cout=cout, s=s, Lin=Lin, **extra))


def _edges():
    e = []
    inst = (("wide", WIDE, 32), ("narrow", NARROW, 64))
    # K loop: Cin = 32 runs only the peeled pair of chunks, 64 one trip of the loop, 96 and 160 reach the prefetch and
    # A-group clamps at odd places
    for cin in (32, 64, 96, 160):
        e.append(_e("wide-cin%d" % cin, cin, WIDE, 7, 97))
        e.append(_e("narrow-cin%d" % cin, cin, NARROW, 3, 193))
    # strides: s = 1 (the s1mask path), divisors of 32 (no shared rows), 5, 6, 31 (nearly every row shared)
    for s in (1, 2, 4, 8, 16, 32, 5, 6, 31):
        for tag, cout, BT in inst:
            e.append(_e("%s-s%d" % (tag, s), 32, cout, s, 3 * BT + 1, rows=(s in (1, 6, 16, 31))))
    # row blocks: Cout = 192 (<2,2>, three blocks), 256 (<4,1>, two); both work orders on either side of 3 MB; fewer than
    # 64 workgroups per batch item (linear order: every wide-/narrow- edge above); 64 and more with a count that is no
    # multiple of 8 (the XCD remap's early return) and one that is
    e.append(_e("cout192-rowblock", 32, 192, 3, 193))
    e.append(_e("cout192-tile", 352, 192, 3, 193))
    e.append(_e("cout256-rowblock", 32, 256, 7, 97))
    e.append(_e("cout128-tile", 224, 128, 7, 97))
    e.append(_e("cout256-xcd84-rowblock", 32, 256, 7, 481, rows=True))
    e.append(_e("cout256-xcd84-tile", 224, 256, 7, 481))
    e.append(_e("cout256-xcd64", 32, 256, 8, 289))
    e.append(_e("cout192-xcd90", 32, 192, 5, 3 * 64 * 5 + 1, rows=True))
    # lengths: Lin = 1, 2, 3, 3 BT - 2 .. 3 BT + 1, 6 BT + 1 on both instances, then the ragged rows
    for tag, cout, BT in inst:
        s = 7 if cout == WIDE else 3
        for Lin in (1, 2, 3, 3 * BT - 2, 3 * BT - 1, 3 * BT, 3 * BT + 1, 6 * BT + 1):
            e.append(_e("%s-Lin%d" % (tag, Lin), 32, cout, s, Lin))
        Lin = 6 * BT + 1
        for bias in (True, False):
            e.append(_e("%s-ragged%s" % (tag, "" if bias else "-nobias"), 32, cout, s, Lin, bias=bias,
                        lengths_cycle=[1, 2, 3, 3 * BT - 1, 3 * BT, Lin]))
    # no bias (the dummy resource then points at x)
    e.append(_e("wide-nobias", 64, WIDE, 7, 97, bias=False))
    e.append(_e("narrow-nobias", 64, NARROW, 3, 193, bias=False))
    e.append(_e("wide-s1-nobias", 32, WIDE, 1, 97, bias=False))
    # output address: rows that start 1, 2, 3 floats off a 16-byte boundary, a channel stride that is no multiple of 4
    for off in (1, 2, 3):
        e.append(_e("wide-yoff%d" % off, 32, WIDE, 7, 97, y_off=off, y_wpad=off))
        e.append(_e("narrow-yoff%d" % off, 32, NARROW, 3, 193, y_off=off, y_wpad=4 - off, rows=True))
    return e


EDGES = _edges()


def _edge_spec(i):
    d = dict(EDGES[i][1])
    cyc = d.pop("lengths_cycle", None)
    spec = make_spec(d.pop("cin"), d.pop("cout"), d.pop("s"), d.pop("Lin"), heavy=(i % 4 == 0), **d)
    if cyc is not None:
        spec["rows"], spec["lengths"] = True, [cyc[(b + 5) % len(cyc)] for b in range(spec["B"])]     # row 0 fills the capacity
    return spec


@pytest.mark.parametrize("i", range(len(EDGES)), ids=[e[0] for e in EDGES])
def test_edge_parity(i):
    """The output-address edges (yoff): the kernel's 16-byte stores are unaligned by construction (a channel's span starts
    `pad` floats before a multiple of s), so a y view off a 16-byte boundary or with an odd channel stride is taken by
    this kernel and the result must be right -- the same assertions as every other edge."""
    run_case(_edge_spec(i), 7000 + i, EDGES[i][0])


def test_edges_reach_what_they_are_meant_to():
    assert len({e[0] for e in EDGES}) == len(EDGES)
    specs = [_edge_spec(i) for i in range(len(EDGES))]
    for s in specs:
        assert s["cin"] % 32 == 0 and s["cout"] % 64 == 0 and 1 <= s["s"] <= 32
        assert nwg_of(s["s"], s["cout"], s["Lin"]) * s["B"] >= MIN_WGS > nwg_of(s["s"], s["cout"], s["Lin"]) * (s["B"] - 1)
        if s["lengths"] is not None:
            assert len(s["lengths"]) == s["B"] and s["lengths"][0] == s["Lin"]
    for cout in (WIDE, NARROW):
        mine = [s for s in specs if s["cout"] == cout]
        BT = tile_of(cout)[1]
        assert {s["cin"] for s in mine} >= {32, 64, 96, 160}
        assert {s["s"] for s in mine} >= {1, 2, 3, 4, 5, 6, 7, 8, 16, 31, 32} - ({3} if cout == WIDE else {7})
        assert {s["Lin"] for s in mine} >= {1, 2, 3, 3 * BT - 2, 3 * BT - 1, 3 * BT, 3 * BT + 1, 6 * BT + 1}
        assert any(s["lengths"] is not None and {1, 2, 3, 3 * BT - 1, 3 * BT} <= set(s["lengths"]) for s in mine)
        assert any(not s["bias"] for s in mine) and {s["y_off"] for s in mine} == {0, 1, 2, 3}
    assert {s["cout"] for s in specs} == {64, 128, 192, 256}
    nwgs = [(nwg_of(s["s"], s["cout"], s["Lin"]), order_of(s["s"], s["cin"], s["cout"])) for s in specs]
    assert any(n < 64 for n, _ in nwgs) and any(n >= 64 and n % 8 for n, _ in nwgs) and any(n >= 64 and n % 8 == 0 for n, _ in nwgs)
    assert {o for n, o in nwgs if n >= 64} == {"tile", "rowblock"} == {o for n, o in nwgs if n < 64}
    for a, b in (("cout192-rowblock", "cout192-tile"), ("cout256-xcd84-rowblock", "cout256-xcd84-tile")):
        sa, sb = (specs[[e[0] for e in EDGES].index(n)] for n in (a, b))
        assert (order_of(sa["s"], sa["cin"], sa["cout"]), order_of(sb["s"], sb["cin"], sb["cout"])) == ("rowblock", "tile")
        assert (sa["s"], sa["cout"], sa["Lin"]) == (sb["s"], sb["cout"], sb["Lin"])
    assert any(s["y_wpad"] % 4 for s in specs)


# --------------------------------------------------------------------------------------
# exact properties
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("cout,s", [(WIDE, 7), (NARROW, 3), (WIDE, 1)], ids=["wide-s7", "narrow-s3", "wide-s1"])
def test_zero_weights_return_the_bias(cout, s):
    """Zero weights: every valid output is its channel's bias, bit for bit (all four planes start at zero and the bias is
    added after the output transform), on ragged rows."""
    spec = make_spec(64, cout, s, 6 * tile_of(cout)[1] + 1, rows=True, w_scale=0.0)
    got, t = launch(spec, 8100 + s)
    for b, n in enumerate(spec["lengths"]):
        assert torch.equal(got[b, :, :n * s], t["bias"].reshape(-1, 1).expand(cout, n * s)), "row %d" % b


@pytest.mark.parametrize("cout,s", [(WIDE, 7), (NARROW, 3)], ids=["wide-s7", "narrow-s3"])
def test_ragged_rows_equal_the_rows_alone(cout, s):
    """Row b of a ragged launch is bit-equal to that row in a plain launch of its own length: the order of the sum depends
    on nothing but the row."""
    BT = tile_of(cout)[1]
    Lin = 6 * BT + 1
    spec = make_spec(96, cout, s, Lin, heavy=True)
    cyc = [Lin, 1, 2, 3, 3 * BT - 1, 3 * BT]
    spec["rows"], spec["lengths"] = True, [cyc[b % len(cyc)] for b in range(spec["B"])]
    got, t = launch(spec, 8200 + s)
    for n in cyc:
        alone = make_spec(96, cout, s, n, heavy=True, B=max(spec["B"], batch_for(s, cout, n)))
        reps = -(-alone["B"] // spec["B"])
        ta = dict(t, x=t["x"][:, :, :n].repeat(reps, 1, 1)[:alone["B"]].contiguous())
        ya, _ = launch(alone, 0, t=ta)
        for b in range(spec["B"]):
            if spec["lengths"][b] == n:
                assert torch.equal(got[b, :, :n * s], ya[b]), "row %d of length %d" % (b, n)


# --------------------------------------------------------------------------------------
# what the host side declines
# --------------------------------------------------------------------------------------
TOL = 2e-5               # the direct kernels' bound of tests/test_convtw_rows_gpu.py, against torch's fp32 operator

DECLINED = [
    ("cin48", dict(cin=48, cout=128, s=7, Lin=97), None),                     # Cin % 32 != 0
    ("cout96", dict(cin=32, cout=96, s=3, Lin=193), None),                    # Cout % 64 != 0
    ("one-batch-item-short", dict(cin=32, cout=128, s=7, Lin=97, B=36), None),   # 14 x 36 = 504 workgroups
    ("pre-lrelu", dict(cin=32, cout=128, s=7, Lin=97), dict(pre=_lib.PRE_LRELU, pre_slope=0.2)),
    ("post-lrelu", dict(cin=32, cout=128, s=7, Lin=97), dict(post=_lib.POST_LRELU, post_slope=0.2)),
]


@pytest.mark.parametrize("i", range(len(DECLINED)), ids=[d[0] for d in DECLINED])
def test_declined_shapes_fall_back_and_stay_right(i):
    """Launches that offer the Winograd planes and that try_launch_convtw refuses do not report code 83, write nothing
    outside their output and meet torch's fp32 operator at 2e-5 of the output's peak."""
    name, shape, actkw = DECLINED[i]
    spec = make_spec(**shape)
    got, t = launch(spec, 9600 + i, expect83=False, act=ops.Act(**actkw) if actkw else None)
    x = F.leaky_relu(t["x"], 0.2) if actkw and "pre" in actkw else t["x"]
    want = direct32(spec, dict(t, x=x))
    want = F.leaky_relu(want, 0.2) if actkw and "post" in actkw else want
    err = (got - want).abs().max().item()
    assert err <= TOL * max(1.0, want.abs().max().item()), "%s: max err %g" % (name, err)


@pytest.mark.parametrize("s", [33, 35])
def test_declined_strides_above_32_are_refused(s):
    """Strides above 32 never reach this kernel (a wave's 32 rows would lie inside one channel: the epilogue's split into
    whole and shared channels assumes s <= 32), and no other kernel of the entry point takes more than 8 phases: the call
    returns VFX_EINVAL, launches nothing and writes nothing -- there is no result to hold to a bound."""
    spec = make_spec(32, WIDE, s, 97)
    t = _inputs(spec, 9700 + s)
    x = ops.guarded(spec["B"], 32, 97, G_IN, DEV)
    x.copy_(torch.zeros_like(x))
    y = torch.full((spec["B"], WIDE, _up4(s * 97)), NAN, device=DEV)
    wp = packing.pack_convtr1d(t["w"])
    lib = _lib.lib()
    before = lib.vfx_launch_count()
    with pytest.raises(_lib.VfxError, match="code -1"):
        ops.convtr1d(x, wp.to(DEV), t["bias"].to(DEV), y, 97, s, None, wd=packing.pack_direct(wp).to(DEV),
                     wg4=packing.pack_wino32_tr(wp, s).to(DEV))
    torch.cuda.synchronize()
    assert lib.vfx_launch_count() == before and torch.isnan(y).all()
