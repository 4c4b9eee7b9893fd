"""convwg4_kernel, convwg4p_kernel and convwg4x_kernel (voicefixer_amd/csrc/vfx_convwg.inc, vfx_convwg4p.inc, vfx_convwg4x.inc;
vfx_last_conv_tile() % 100 == 80 / 81 / 82: the stand-alone Winograd F(4,3) k = 3 convolutions of the ResStacks with C >= 128, of
the condnet and of the stage-closing layers) at every launch the product makes, against float64.

* ``test_launch_census`` runs the seeded pipeline at the five geometries of tests/test_conv_taps_gpu.py under
  voicefixer_amd.launch_record and asserts that every code-80 / 81 / 82 launch is a row of ``CASES``; the key is (code, Cin, Cout,
  d, pre, post, post slope, bias, residual none / in place / separate, row tags).  How many launches each code takes is pinned
  per geometry.  convwg4p_kernel has NO product launch: the C = 64 layers it was written for run on resblk4_kernel, and a wide
  launch long enough for it is long enough for convwg4x_kernel.  It gets edges only.
* ``test_case_parity`` launches every row of ``CASES`` at a reduced size -- Cin = Cout = the product's (the fp32 chain and the
  gy = Cout / 128 of the work list), B and L cut down until the host's own threshold for the row's kernel is just met (about
  33.5 M outputs for convwg4x_kernel whatever C is, 8.4 M for convwg4_kernel) -- once with unit gains and once with heavy-tailed
  weight-norm gains and unit-scale biases.
* ``test_edge_parity`` does the same for the code paths the product does not reach (``EDGES``), ``test_declines`` asserts what
  must run on another kernel.
* ``test_zero_weights_return_bias_plus_residual``, ``test_ragged_rows_equal_the_rows_alone``, ``test_batch_items_are_independent``,
  ``test_rows_agree_across_the_persistent_threshold``: exact properties.

Every spec is first walked by the CPU model of the host rule and the work list (tests/test_wg4_geometry_cpu.py: ``check``, at
this device's own CU count); only what it passes is launched, through ops.conv1d, and the kernel code it names is asserted
afterwards.  Buffers are laid out as engine.forward_cond lays out xs / ys: guarded views, NaN in the guard bands and past every
row's own end, y a NaN-filled allocation (the in-place residual: the residual inside [0, len_b), NaN elsewhere).  Every launch
asserts the tile code and one launch, no NaN in [0, len_b) of any row, nothing but NaN everywhere else in the y allocation, x
(and a separate residual) unchanged bit for bit; the in-place residual is read before it is overwritten or the parity fails.

The figure is ``conv_error`` against ``f64_reference.conv1d`` and its ``magnitude=True`` twin, per output:
|got - ref| / (lip * M + |ref|).  The bound is measured on the reference side, on ``f64_reference.conv1d_f43_f32`` -- a plain fp32
statement of the same algorithm with bias and residual added after the output transform: the device may be at most MARGIN = 4
times worse, maximum and RMS, with the floors of tests/test_conv_taps_gpu.py.  Float64 over 33 M outputs x Cin = 512 is minutes
on a CPU, so both are scored on a SUBSET of the output channels, over all positions and batch items: the first and the last row
of every 32-row wave block of every 128-channel block, seeded others up to one channel in eight, and -- under heavy-tailed
gains -- the four channels with the largest |bias| / rms(convolution), taken from torch's direct fp32 result.  Every other
channel is still compared with torch's direct fp32 operator at 2e-5 of the launch's peak.  Every case prints
``PARITY <id> <stmt max> <dev max> <ratio> <stmt rms> <dev rms> <ratio> direct <max> <rms>`` before it asserts;
profiles/wg4_parity.txt is that output.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from voicefixer_amd import ops, packing, _lib  # noqa: E402
from oracle import f64_reference as ref64  # noqa: E402
from test_conv_taps_gpu import GEOMETRIES, MARGIN, RMS_FLOOR, ULP, _Acc, _census, pipe  # noqa: E402,F401
import test_wg4_geometry_cpu as geo  # noqa: E402
from test_wg4_geometry_cpu import CASES, EDGES, case_id  # noqa: E402

DEV = "cuda"
NAN = float("nan")
NONE, LRELU, ELU, SNAKE = _lib.POST_NONE, _lib.POST_LRELU, _lib.POST_ELU, _lib.POST_LRELU_SNAKE
assert (NONE, LRELU, ELU, SNAKE) == (geo.POST_NONE, geo.POST_LRELU, geo.POST_ELU, geo.POST_SNAKE)
assert (_lib.PRE_NONE, _lib.PRE_LRELU) == (geo.PRE_NONE, geo.PRE_LRELU)
DIRECT_TOL = 2e-5            # the channels outside the float64 subset: torch's direct fp32 operator, of the launch's peak

_CUS = []


def cus():
    """Compute units of this device: what try_launch_convwg4p / 4x size their grids and thresholds by."""
    if not _CUS:
        _CUS.append(torch.cuda.get_device_properties(0).multi_processor_count)
    return _CUS[0]


# --------------------------------------------------------------------------------------
# one launch
# --------------------------------------------------------------------------------------
def _rand(shape, gen, scale=1.0):
    return torch.randn(shape, generator=gen) * scale


def _lens(spec):
    return spec["lengths"] if spec["lengths"] is not None else [spec["L"]] * spec["B"]


def _inputs(spec, seed):
    """CPU fp32 operands in torch's layouts, as tests/test_convtw_gpu.py and tests/test_resblk4_gpu.py draw them: unit-variance
    activations and residual, weights scaled by fan-in^-1/2 and biases of 0.3; `heavy`: the weights times a log-normal gain per
    output channel, exp(1.5 z - 2.25) (trained weight-norm gains), and unit-scale biases, so that some channels are all bias
    or all residual.  Biases are drawn per channel: a gather by the wrong index shows."""
    g = torch.Generator().manual_seed(seed)
    cin, cout, B, L = spec["cin"], spec["cout"], spec["B"], spec["L"]
    t = {"w": _rand((cout, cin, 3), g, (3 * cin) ** -0.5)}
    if spec["heavy"]:
        t["w"] = t["w"] * torch.exp(1.5 * _rand((cout,), g) - 2.25).reshape(-1, 1, 1)
    t["w"] = t["w"] * spec["w_scale"]
    b = _rand((cout,), g, 1.0 if spec["heavy"] else 0.3)
    t["bias"] = b if spec["bias"] else None
    t["x"] = _rand((B, cin, L), g)
    t["res"] = _rand((B, cout, L), g) if spec["res"] != "none" else None
    return t


def _alloc(B, Cn, Lp, guard, wpad=0, cpad=0, off=0):
    """NaN-filled allocation and the (B, Cn, Lp) view inside it: `guard` elements on both sides of every row, `wpad` more behind
    it, `cpad` channels on both sides, the view `off` elements off its 16-byte alignment."""
    g4 = geo.up4(guard)
    base = torch.full((B, Cn + 2 * cpad, g4 + Lp + g4 + wpad + (4 if off else 0)), NAN, device=DEV)
    v = base[:, cpad:cpad + Cn, g4 + off:g4 + off + Lp]
    v._vfx_guard, v._vfx_base = g4, base
    return base, v


def _fill(view, data, lens):
    """data (B, C, L) into [0, len_b) of every row of the view."""
    for n in sorted(set(lens)):
        idx = torch.tensor([b for b in range(len(lens)) if lens[b] == n], device=DEV)
        view[idx, :, :n] = data[idx, :, :n]


def launch(spec, seed=0, t=None, code=None):
    """Launch `spec` once and hold it to the kernel code the CPU model gives (`code`: what the table says, asserted against
    the model first), one launch and the canaries.  Returns (device output as a dense (B, Cout, L) fp32 CPU tensor with NaN
    past every row's own end, the operands, the model's dispatch record)."""
    g = geo.check(spec, cus())                     # the CPU model first: never launch what it fails
    assert code is None or g["code"] == code, "the model gives code %d, the table %d" % (g["code"], code)
    B, L, cin, cout = spec["B"], spec["L"], spec["cin"], spec["cout"]
    lens, Lp = _lens(spec), geo.up4(spec["L"])
    t = _inputs(spec, seed) if t is None else t
    xbase, xv = _alloc(B, cin, Lp, spec["x_guard"])
    _fill(xv, t["x"].to(DEV), lens)
    # vec_ok = False: the y view (and with it the in-place residual) 4 bytes off a 16-byte boundary -- no vector path at d = 1.
    # (An x view off its alignment is refused by the entry point itself: test_unaligned_x_is_refused.)
    off = 0 if spec["vec_ok"] else 1
    ybase, yv = _alloc(B, cout, Lp, spec["y_guard"], spec["y_wpad"], spec["y_cpad"], off=off)
    rv = rbase = None
    if spec["res"] == "in place":
        _fill(yv, t["res"].to(DEV), lens)
        rv = yv
    elif spec["res"] == "separate":
        rbase, rv = _alloc(B, cout, Lp, spec["r_guard"], spec["r_wpad"], spec["r_cpad"])
        _fill(rv, t["res"].to(DEV), lens)
    if spec["lengths"] is not None:
        rows = torch.tensor(lens, dtype=torch.int32, device=DEV)
        ops.with_rows(xv, rows)
        ops.with_rows(yv, rows)
        if spec["res"] == "separate":
            ops.with_rows(rv, rows)
    wp = packing.pack_conv1d(t["w"])
    wg4 = packing.pack_wino4(wp).to(DEV)
    bias = t["bias"].to(DEV) if t["bias"] is not None else None
    act = ops.Act(pre=spec["pre"], pre_slope=spec["pre_slope"], post=spec["post"], post_slope=spec["post_slope"])
    xkeep = xbase.clone()
    rkeep = rbase.clone() if rbase is not None else None
    lib = _lib.lib()
    torch.cuda.synchronize()
    before = lib.vfx_launch_count()
    ops.conv1d(xv, wp.to(DEV), bias, yv, L, 3, spec["d"], _lib.PAD_ZERO, act, rv, wg4=wg4)
    torch.cuda.synchronize()
    tile, launches = lib.vfx_last_conv_tile(), int(lib.vfx_launch_count() - before)
    assert tile % 100 == g["code"], "ran as %d, expected code %d" % (tile, g["code"])
    assert launches == 1
    # ---- canaries: NaN past each row's own end, past the capacity, in the guard bands and the neighbouring channels
    allowed = torch.zeros(ybase.shape, dtype=torch.bool, device=DEV)
    g4, cp = geo.up4(spec["y_guard"]), spec["y_cpad"]
    av = allowed[:, cp:cp + cout, g4 + off:g4 + off + Lp]
    for n in sorted(set(lens)):
        idx = torch.tensor([b for b in range(B) if lens[b] == n], device=DEV)
        av[idx, :, :n] = True
    stray = ~(torch.isnan(ybase) | allowed)
    assert not bool(stray.any()), "%d elements outside the valid output were written" % int(stray.sum())
    assert not bool((torch.isnan(ybase) & allowed).any()), "NaN inside [0, len) of a row"
    assert torch.equal(xbase.view(torch.int32), xkeep.view(torch.int32)), "x was written"
    if rbase is not None:
        assert torch.equal(rbase.view(torch.int32), rkeep.view(torch.int32)), "the residual was written"
    return yv[:, :, :L].detach().cpu().contiguous(), t, g


def _groups(spec):
    lens = _lens(spec)
    return [(n, [b for b in range(spec["B"]) if lens[b] == n]) for n in sorted(set(lens))]


def direct32(spec, t):
    """torch's direct fp32 CPU operator, every row of a ragged batch alone: (the bare convolution, the launch's result), both
    (B, Cout, L) with NaN past a row's own end."""
    B, L, d = spec["B"], spec["L"], spec["d"]
    conv = torch.full((B, spec["cout"], L), NAN)
    for n, idx in _groups(spec):
        x = t["x"][idx][:, :, :n]
        if spec["pre"] == _lib.PRE_LRELU:
            x = F.leaky_relu(x, spec["pre_slope"])
        conv[idx, :, :n] = F.conv1d(x, t["w"], None, dilation=d, padding=d)
    y = conv
    if t["bias"] is not None:
        y = y + t["bias"].reshape(1, -1, 1)
    if t["res"] is not None:
        y = y + t["res"]
    post, ps = spec["post"], spec["post_slope"]
    if post in (LRELU, SNAKE):
        y = F.leaky_relu(y, ps)
        y = y + torch.sin(y) if post == SNAKE else y
    elif post == ELU:
        y = F.elu(y)
    return conv, y


def subset(spec, t, conv, seed):
    """The output channels scored in float64 (module docstring), sorted."""
    cout = spec["cout"]
    sub = {c for c in range(cout) if c % 32 in (0, 31)}
    g = torch.Generator().manual_seed(seed)
    for c in torch.randperm(cout, generator=g).tolist():
        if len(sub) >= max(cout // 8, 8):
            break
        sub.add(c)
    if spec["heavy"] and t["bias"] is not None:
        rms = torch.nan_to_num(conv, nan=0.0).double().pow(2).sum(dim=(0, 2)).sqrt()       # (the same count for every channel)
        ratio = t["bias"].double().abs() / rms.clamp(min=1e-300)
        sub |= set(torch.topk(ratio, 4).indices.tolist())
    return sorted(sub)


def score(spec, t, got, seed):
    """`got`, the fp32 F(4,3) statement and torch's direct fp32 operator, each against the float64 statement on the channel
    subset -- every row of a ragged batch against the convolution of that row alone; the other channels against torch's
    direct fp32 operator.  Returns three _Acc (device, statement, direct)."""
    with torch.no_grad():
        conv, dire = direct32(spec, t)
        sub = subset(spec, t, conv, seed)
        del conv
        w, bias = t["w"][sub], (t["bias"][sub] if t["bias"] is not None else None)
        res = t["res"][:, sub] if t["res"] is not None else None
        kw = dict(pre=spec["pre"], pre_slope=spec["pre_slope"], lengths=spec["lengths"])
        ref = ref64.conv1d(t["x"], w, bias, res, spec["d"], post=spec["post"], post_slope=spec["post_slope"], **kw)
        mag = ref64.conv1d(t["x"], w, bias, res, spec["d"], magnitude=True, **kw)
        stmt = ref64.conv1d_f43_f32(t["x"], w, bias, res, spec["d"], spec["pre"], spec["pre_slope"], spec["post"], spec["post_slope"],
                                    lengths=spec["lengths"])
    assert got.shape == dire.shape and ref.shape == got[:, sub].shape
    lip = ref64.post_lipschitz(spec["post"])
    accs = []
    for y in (got[:, sub], stmt, dire[:, sub]):
        acc = _Acc()
        acc.add(ref64.conv_error(y, ref, mag, lip))
        accs.append(acc)
    # ---- every other channel: torch's direct fp32 operator at DIRECT_TOL of the launch's peak
    ok = ~torch.isnan(dire)
    assert torch.equal(torch.isnan(got), ~ok), "NaN pattern of the output"
    peak = float(dire[ok].abs().max())
    worst = float((got - dire)[ok].abs().max())
    assert worst <= DIRECT_TOL * peak, "direct fp32 comparison: %.3e of the peak" % (worst / peak)
    return accs


def check(name, dev, cpu, dire):
    """Print the figures, then assert: the device at most MARGIN x the yardstick `cpu`, maximum and RMS, with the floors."""
    print("PARITY %s %.3e %.3e %.2f %.3e %.3e %.2f direct %.3e %.3e" % (
        name, cpu.mx, dev.mx, dev.mx / max(cpu.mx, ULP), cpu.rms, dev.rms, dev.rms / max(cpu.rms, RMS_FLOOR), dire.mx, dire.rms))
    assert dev.n > 0 and dev.n == cpu.n
    assert dev.mx <= MARGIN * max(cpu.mx, ULP), "%s: max figure %.3e exceeds %.0f x the yardstick's %.3e" % (name, dev.mx, MARGIN, cpu.mx)
    assert dev.rms <= MARGIN * max(cpu.rms, RMS_FLOOR), "%s: RMS figure %.3e exceeds %.0f x the yardstick's %.3e" % (name, dev.rms, MARGIN, cpu.rms)


def run_case(spec, seed, name, code):
    got, t, _ = launch(spec, seed, code=code)
    dev, stmt, dire = score(spec, t, got, seed)
    check(name, dev, stmt, dire)


# --------------------------------------------------------------------------------------
# the product's launches
# --------------------------------------------------------------------------------------
def record_key(r):
    return (r["code"], r["cin"], r["cout"], r["step"], r["pre"], r["post"], round(r["post_slope"], 6) if r["post"] in (LRELU, SNAKE) else 0.0,
            r["bias"], r["res"], r["rows"])


# launches per step on codes (80, 81, 82).  A stage with C >= 128 is eight layers: eight first convolutions and seven second
# ones on convwg4x_kernel where B x L reaches its threshold and on convwg4_kernel below it (batch 1; C = 512 at four and five
# rows; batch 1 at C = 512 leaves the family), the stage-closing second one (snake behind the residual) on convwg4_kernel; the
# five condnet convolutions run on convwg4_kernel where the batch gives them 512 workgroups (batch 32, 8 x 30 s).
COUNTS = {"b32x10": (8, 0, 45), "b1x10": (32, 0, 0), "b8x30": (8, 0, 45), "ragged5": (18, 0, 30), "train4x10": (18, 0, 30)}


_RECS = {}


def _cached_census(pipe, geometry):  # noqa: F811
    if geometry not in _RECS:
        _RECS[geometry] = _census(pipe, geometry)
    return _RECS[geometry]


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_launch_census(pipe, geometry):  # noqa: F811
    """Every convwg4_kernel / convwg4p_kernel / convwg4x_kernel launch of the seeded pipeline at this geometry is a row of
    CASES -- the table is complete: adding, removing or re-routing a product launch on these kernels fails here -- and the
    number of launches on each code is the pinned one.  convwg4p_kernel has no product launch at any geometry."""
    table = set(CASES)
    rec = _cached_census(pipe, geometry)
    wg = rec.wg4()
    keys = [record_key(r) for r in wg]
    unmatched = sorted({k for k in keys if k not in table})
    counts = tuple(sum(1 for r in wg if r["code"] == c) for c in (80, 81, 82))
    print("CENSUS %s: %d conv-family calls, %d on codes 80 / 81 / 82 = %r, %d distinct keys, %d unmatched" % (
        geometry, len(rec.records), len(wg), counts, len(set(keys)), len(unmatched)))
    for k in sorted(set(keys)):
        print("CENSUS-KEY %s %s x%d" % (geometry, case_id(k) if k[5] in geo.POST_NAMES else repr(k), keys.count(k)))
    assert not unmatched, "launches on codes 80 / 81 / 82 that are not rows of CASES:\n%s" % "\n".join(map(repr, unmatched))
    for r in wg:
        assert r["op"] == "conv1d" and r["k"] == 3 and r["launches"] == 1 and r["guarded"] and r["unit"] and r["pad"] == "zero", r
    assert counts == COUNTS[geometry]
    assert counts[1] == 0, "convwg4p_kernel has a product launch: it needs rows in CASES"


def test_every_case_is_a_product_launch(pipe):  # noqa: F811
    """The other direction: no row of CASES that none of the five geometries launches."""
    seen = {record_key(r) for geometry in GEOMETRIES for r in _cached_census(pipe, geometry).wg4()}
    missing = [case_id(k) for k in CASES if k not in seen]
    assert not missing, "rows of CASES that no census geometry launches: %r" % missing


@pytest.mark.parametrize("gains", ["unit", "heavy"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=[case_id(k) for k in CASES])
def test_case_parity(i, gains):
    """Every row of CASES at its reduced size, with unit gains and with heavy-tailed ones (profiles/wg4_parity.txt).

    Finding, fixed in the kernels; these are its regression cases.  While convwg4x_kernel, convwg4p_kernel and the SPEC 1 / 2
    instances of convwg4_kernel opened plane 1 with the bias, and convwg4_kernel's run-time instance started planes 0, 1, 3
    and 5 at the solution of A^T m = residual + bias, every partial sum of the K loop rounded at the size of bias (+ residual):
    69 of these 178 rows were above the bound -- with heavy-tailed gains 55 of 74 first-convolution and condnet rows (up to
    4.2 x the statement's maximum / 7.3 x its RMS on convwg4x_kernel, 8.9 x / 8.7 x on convwg4_kernel), 6 of 9 second
    convolutions (up to 4.6 x / 5.7 x) and all six stage-closing launches at 17 - 171 x / 17 - 33 x (k80-c512-d1-nopre-snake0.2-
    bias-inplace-heavy: 4.84e-05 against 2.83e-07), two of those six with unit gains as well (up to 4.4 x).  With every plane
    started at zero, the bias product  acc[1] += bias (x) 1  behind the last k-step, and bias and residual added to the
    transformed outputs in the run-time instance, all rows are at 0.75 - 3.33 x / 0.84 - 1.71 x."""
    key = CASES[i]
    run_case(geo.case_spec(key, gains == "heavy", cus()), 4000 + 2 * i + (gains == "heavy"), case_id(key) + "-" + gains, key[0])


# --------------------------------------------------------------------------------------
# edges the product does not reach
# --------------------------------------------------------------------------------------
def _edge(i):
    """The edge table at this device's CU count (the module-level one, at 256, names the tests)."""
    e = geo._edges(cus())
    assert [x[0] for x in e] == [x[0] for x in EDGES]
    return e[i]


@pytest.mark.parametrize("i", range(len(EDGES)), ids=[e[0] for e in EDGES])
def test_edge_parity(i):
    """The code paths the product does not reach; every second edge draws heavy-tailed gains.  An edge named `declined` is a
    launch one of the persistent kernels must NOT take: it runs on convwg4_kernel (code 80), and is held to the same bound."""
    name, code, spec = _edge(i)
    run_case(dict(spec, heavy=i % 2 == 1), 7000 + i, name, code)


@pytest.mark.parametrize("i", range(len(geo.DECLINED)), ids=[d[0] for d in geo.DECLINED])
def test_declines(i):
    """What the family declines runs on another kernel (Cin = 72: Cin % 32 != 0, as is Cin = 80; Cout = 96; fewer than 512
    workgroups), with the same result at the direct kernels' tolerance."""
    name, kw = geo.DECLINED[i]
    assert geo.dispatch(cus=cus(), **kw) is None
    B, cin, cout, L, d = kw["B"], kw["cin"], kw["cout"], kw["L"], kw["d"]
    g = torch.Generator().manual_seed(7500 + i)
    x, w, bias = _rand((B, cin, L), g), _rand((cout, cin, 3), g, (3 * cin) ** -0.5), _rand((cout,), g, 0.3)
    _, xv = _alloc(B, cin, geo.up4(L), geo.G_TILE)
    xv[:, :, :L] = x.to(DEV)
    ybase, yv = _alloc(B, cout, geo.up4(L), geo.G_TILE)
    wp = packing.pack_conv1d(w)
    wg4 = packing.pack_wino4(wp).to(DEV) if cin % 8 == 0 else None
    ops.conv1d(xv, wp.to(DEV), bias.to(DEV), yv, L, 3, d, _lib.PAD_ZERO, ops.Act(), None, wg4=wg4)
    torch.cuda.synchronize()
    assert _lib.lib().vfx_last_conv_tile() % 100 not in (80, 81, 82)
    ref = F.conv1d(x, w, bias, dilation=d, padding=d)
    got = yv[:, :, :L].cpu()
    assert float((got - ref).abs().max()) <= DIRECT_TOL * float(ref.abs().max())


def test_unaligned_x_is_refused():
    """An input view that does not start on a 16-byte boundary never reaches a kernel: vfx_conv1d_f32 returns VFX_EALIGN."""
    base, xv = _alloc(2, 64, 1024, 8)
    base.zero_()
    x1 = base[:, :, 9:9 + 1020]
    x1._vfx_guard = 8
    _, yv = _alloc(2, 128, 1024, 8)
    w = packing.pack_conv1d(torch.zeros((128, 64, 3)))
    lib = _lib.lib()
    before = lib.vfx_launch_count()
    with pytest.raises(_lib.VfxError):
        ops.conv1d(x1, w.to(DEV), None, yv, 1020, 3, 1, _lib.PAD_ZERO, ops.Act(), None, wg4=packing.pack_wino4(w).to(DEV))
    torch.cuda.synchronize()
    assert lib.vfx_launch_count() == before


# --------------------------------------------------------------------------------------
# exact properties
# --------------------------------------------------------------------------------------
FIRST = dict(pre=geo.PRE_LRELU, post=geo.POST_LRELU, post_slope=0.01)
SECOND = dict(res="in place")
CLOSE = dict(res="in place", post=geo.POST_LRELU, post_slope=0.2)
# name, code, Cout, d, options: the instances of the three kernels (convwg4x / 4p SPEC 1 dilated and D1, SPEC 2; convwg4 SPEC 0 with
# the residual, vector and dword path, and both of its tiles)
EXACT = [("x-first-d9", 82, 128, 9, FIRST), ("x-first-d1", 82, 128, 1, FIRST), ("x-second", 82, 128, 1, SECOND),
         ("p-first-d3", 81, 64, 3, FIRST), ("p-second", 81, 192, 1, SECOND),
         ("g-close", 80, 128, 1, CLOSE), ("g-close-c64-dword", 80, 64, 1, dict(CLOSE, vec_ok=False)), ("g-first-d3", 80, 128, 3, FIRST),
         ("g-res-separate-d3", 80, 128, 3, dict(res="separate", post=geo.POST_LRELU, post_slope=0.2))]
EXACT_IDS = [e[0] for e in EXACT]


def _exact_spec(e, rows=False, **kw):
    name, code, cout, d, opts = e
    B = 6 if rows else 4
    L, _ = geo.threshold_shape(code, cout, d, B, cus())
    return geo.make_spec(64, cout, d, L, B, lengths=geo.ragged_lengths(L, d) if rows else None, **dict(opts, **kw))


@pytest.mark.parametrize("e", EXACT, ids=EXACT_IDS)
def test_zero_weights_return_bias_plus_residual(e):
    """With zero weights every output is post(bias + residual) bit for bit: bias and residual are added to the transformed
    outputs, once, in torch's order, and nothing of them passes through the transform's constants."""
    spec = _exact_spec(e, rows=True, w_scale=0.0, heavy=True)
    got, t, _ = launch(spec, 8100, code=e[1])
    want = t["bias"].reshape(1, -1, 1).expand(spec["B"], -1, spec["L"])
    if t["res"] is not None:
        want = want + t["res"]
    if spec["post"] == LRELU:
        want = torch.maximum(want, want * torch.tensor(spec["post_slope"], dtype=torch.float32))
    ok = ~torch.isnan(got)
    assert bool(ok.any()) and torch.equal(got[ok], want[ok])


def _alone(spec, t, b, n):
    """Row b of `spec` as a launch of its own: capacity n, no row tags, as many copies of the row as the family needs to take
    the launch (512 workgroups).  Returns (row 0 of the result, the kernel code it ran on)."""
    copies = 1
    while geo.dispatch(copies, spec["cin"], spec["cout"], n, spec["d"], spec["pre"], spec["post"], spec["res"] != "none", spec["pre_slope"],
                       spec["post_slope"], spec["vec_ok"], cus()) is None:
        copies *= 2
    alone = dict(spec, B=copies, L=n, lengths=None, x_guard=8, y_guard=8, r_guard=8)
    rep = lambda a: None if a is None else a[b:b + 1, :, :n].expand(copies, -1, -1).contiguous()
    got, _, g = launch(alone, 0, t=dict(t, x=rep(t["x"]), res=rep(t["res"])))
    assert torch.equal(got, got[:1].expand_as(got)), "copies of one row differ"
    return got[0], g["code"]


@pytest.mark.parametrize("e", EXACT, ids=EXACT_IDS)
def test_ragged_rows_equal_the_rows_alone(e):
    """Row b of a ragged launch is bit-equal to that row launched alone at its own length -- on whichever of the three kernels
    the host gives the shorter launch: every output is one chain over the input channels in ascending order, on all of them
    (the claim of vfx_convwg4p.inc and vfx_convwg4x.inc that their results equal convwg4_kernel's)."""
    spec = _exact_spec(e, rows=True, heavy=True)
    got, t, _ = launch(spec, 8200, code=e[1])
    codes = set()
    for b, n in enumerate(spec["lengths"]):
        ya, code = _alone(spec, t, b, n)
        codes.add(code)
        assert torch.equal(got[b, :, :n], ya), "row %d of length %d (alone: code %d)" % (b, n, code)
    print("ALONE %s: the rows alone ran on codes %r" % (e[0], sorted(codes)))


@pytest.mark.parametrize("e", EXACT, ids=EXACT_IDS)
def test_batch_items_are_independent(e):
    """The same row at batch index 0 and 3 of a launch, with different neighbours, is bit-equal."""
    spec = _exact_spec(e, heavy=True)
    t = _inputs(spec, 8300)
    t["x"][3] = t["x"][0]
    if t["res"] is not None:
        t["res"][3] = t["res"][0]
    got, _, _ = launch(spec, 0, t=t, code=e[1])
    assert torch.equal(got[0], got[3]) and not torch.equal(got[0], got[1])


@pytest.mark.parametrize("e", [x for x in EXACT if x[1] != 80], ids=[x[0] for x in EXACT if x[1] != 80])
def test_rows_agree_across_the_persistent_threshold(e):
    """The same operands just above the persistent threshold (convwg4x_kernel / convwg4p_kernel) and, one batch item fewer, just
    below it (convwg4_kernel): the rows they share are bit-equal."""
    spec = _exact_spec(e, heavy=True)
    above, t, _ = launch(spec, 8400, code=e[1])
    fewer = dict(spec, B=spec["B"] - 1)
    cut = lambda a: None if a is None else a[:spec["B"] - 1].contiguous()
    below, _, g = launch(fewer, 0, t=dict(t, x=cut(t["x"]), res=cut(t["res"])), code=80)
    assert torch.equal(above[:spec["B"] - 1], below)
