"""Recorder of the conv-family launches of a run (development and test infrastructure; shared by tools/launch_table.py and
tests/test_conv_taps_gpu.py).  Inside ``with LaunchRecorder() as rec:`` every call of ops.conv1d / convtr1d / conv2d /
convtr2d_3x3s2 / resblock / resblock_wino4 appends one record to ``rec.records``: what the caller asked for (shape, activations, bias, residual,
row tags, guard, output strides) and what the library did with it (vfx_last_conv_tile(), the vfx_launch_count() delta).
Nothing on the launch path changes: the wrappers call the real launchers."""
import inspect

from . import ops, _lib

NAMES = ("conv1d", "resblock", "resblock_wino4", "convtr1d", "conv2d", "convtr2d_3x3s2")
PAD_NAMES = {_lib.PAD_ZERO: "zero", _lib.PAD_REFLECT: "reflect"}
FAMILIES = {51: "convw", 52: "convw", 54: "convw", 59: "convw 3x3", 61: "fused", 62: "fused", 64: "fused", 71: "fused+F23",
            72: "fused+F23", 74: "fused+F23", 91: "fused+F43", 92: "fused+F43", 94: "fused+F43", 96: "fused F43+F43", 97: "fused F43+F43 strip",
            80: "convwg4", 81: "convwg4p", 82: "convwg4x", 83: "convtw", 88: "convwg4s", 16: "x3", 32: "convh"}


def family(code):
    """Kernel family of a vfx_last_conv_tile() code (include/vfx_hip.h); 4 / 8 are conv_taps_kernel's K-chunk depths."""
    return FAMILIES.get(code, "conv_taps KC=%d" % code)


def _describe(name, a):
    """The caller's side of one launch, from the bound arguments of the ops launcher."""
    x, w = a["x"], a["w"] if "w" in a else None
    y, res, act = a.get("y"), a.get("res"), a.get("act")
    d = {"op": name, "B": x.shape[0]}
    if name in ("resblock", "resblock_wino4"):
        d.update(cin=x.shape[1], cout=x.shape[1], L=a["L"], k=3, step=a["dilation"], pad="zero", slope=a["slope"],
                 post_slope=a["post_slope"], bias_pair=(a["b1"] is not None, a["b2"] is not None))
    else:
        d.update(cin=x.shape[1] if a.get("cin") is None else a["cin"], cout=w.shape[2])
    if name == "conv1d":
        d.update(L=a["L"], k=a["k"], step=a["dilation"], pad=PAD_NAMES[a["pad_mode"]])
    elif name == "convtr1d":
        d.update(L=a["Lin"], k=2 * a["stride"], step=a["stride"], pad="zero")
    elif name == "conv2d":
        d.update(H=a["H"], pitch=1 << a["pitch_log2"], k=a["ksize"], step=1, pad="zero")
    elif name == "convtr2d_3x3s2":
        d.update(H=a["h"], pitch=1 << a["in_pitch_log2"], k=3, step=2, pad="zero")
    d["pre"] = act.c.pre_act if isinstance(act, ops.Act) else _lib.PRE_NONE
    d["post"] = act.c.post_act if isinstance(act, ops.Act) else (a.get("post", _lib.POST_NONE) if name.startswith("resblock") else _lib.POST_NONE)
    if isinstance(act, ops.Act):
        d["post_slope"] = float(act.c.post_slope)
    elif not name.startswith("resblock"):
        d["post_slope"] = 0.0
    d["bias"] = a.get("bias") is not None
    d["res"] = "none" if res is None else ("in place" if res.data_ptr() == y.data_ptr() else "separate")
    d["rows"] = getattr(x, "_vfx_rows", None) is not None
    d["guarded"] = getattr(x, "_vfx_guard", 0) > 0
    d["unit"] = y.stride(2) == 1
    return d


class LaunchRecorder:
    def __init__(self):
        self.records = []
        self._orig = {}

    def _wrap(self, name, fn):
        sig = inspect.signature(fn)
        lib = _lib.lib()

        def inner(*args, **kw):
            bound = sig.bind(*args, **kw)
            bound.apply_defaults()
            nprof = len(ops.PROFILE) if ops.PROFILE is not None else 0
            before = lib.vfx_launch_count()
            out = fn(*args, **kw)
            rec = _describe(name, bound.arguments)
            tile = lib.vfx_last_conv_tile()
            rec.update(BM=tile // 100000, BL=tile // 100 % 1000, code=tile % 100, launches=int(lib.vfx_launch_count() - before),
                       prof=ops.PROFILE[nprof:] if ops.PROFILE is not None else [])
            self.records.append(rec)
            return out
        return inner

    def __enter__(self):
        for k in NAMES:
            self._orig[k] = getattr(ops, k)
            setattr(ops, k, self._wrap(k, self._orig[k]))
        return self

    def __exit__(self, *exc):
        for k, fn in self._orig.items():
            setattr(ops, k, fn)
        self._orig = {}
        return False

    def taps(self):
        """The records that ran on the first-generation conv_taps_kernel (codes 4 / 8)."""
        return [r for r in self.records if r["code"] in (4, 8)]

    def wg4s(self):
        """The records that ran on convwg4s_kernel (code 88: the 3x3 Winograd F(4,3) kernel of the ResUNet)."""
        return [r for r in self.records if r["code"] == 88]

    def tw(self):
        """The records that ran on convtw_kernel (code 83: the Winograd F(3,2) transposed convolution of the UpsampleNet)."""
        return [r for r in self.records if r["code"] == 83]

    def rb4(self):
        """The records that ran on resblk4_kernel / resblk4s_kernel (codes 96 / 97: one whole C = 64 ResStack layer, both
        halves Winograd F(4,3), on the block tile / the strip tile)."""
        return [r for r in self.records if r["code"] in (96, 97)]

    def wg4(self):
        """The records that ran on the stand-alone Winograd F(4,3) convolutions (codes 80 / 81 / 82: convwg4_kernel, its
        persistent form convwg4p_kernel and the re-blocked persistent convwg4x_kernel)."""
        return [r for r in self.records if r["code"] in (80, 81, 82)]


def split_k(rec):
    """Did split-K run?  A conv_taps launch of the product is one grid when every tile takes the same instance (guarded
    zero-padded inputs: interior; channel tails and ragged reflect padding: general) and two when a reflect-padded launch has
    interior tiles between its mirroring boundary tiles; one launch more than that is splitk_reduce_kernel."""
    two_grids = rec["pad"] == "reflect" and not rec["rows"]
    return rec["launches"] == (3 if two_grids else 2)


def shape_text(r):
    if r["op"].startswith("resblock"):
        return "C %d L %d d %d" % (r["cin"], r["L"], r["step"])
    if r["op"] == "conv1d":
        return "Cin %d Cout %d L %d k %d d %d%s" % (r["cin"], r["cout"], r["L"], r["k"], r["step"], " res" if r["res"] != "none" else "")
    if r["op"] == "convtr1d":
        return "Cin %d Cout %d Lin %d s %d" % (r["cin"], r["cout"], r["L"], r["step"])
    if r["op"] == "conv2d":
        return "Cin %d Cout %d H %d P %d k %d%s" % (r["cin"], r["cout"], r["H"], r["pitch"], r["k"], " res" if r["res"] != "none" else "")
    return "Cin %d Cout %d h %d P %d" % (r["cin"], r["cout"], r["H"], r["pitch"])
