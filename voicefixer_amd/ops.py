"""Thin Python launchers for the libvfx_hip C ABI.

torch is used here only as the owner of device memory and of the current HIP stream:
every function takes CUDA(=HIP) tensors, fills ``vfx_tensor`` descriptors from their
strides and calls the C entry point on ``torch.cuda.current_stream()``.  No torch
arithmetic happens on this path.
"""
import ctypes as C
import math

import torch

from . import _lib
from ._lib import (vfx_tensor, vfx_act, check, PRE_NONE, PRE_LRELU, PRE_AFFINE_LRELU, POST_NONE,
                   POST_LRELU, POST_ELU, POST_TANH, POST_SIGMOID, POST_LRELU_SNAKE, PAD_ZERO,
                   PAD_REFLECT, MATH_F32, MATH_BF16X3)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.VfxError("libvfx_hip operates on device tensors only (got a CPU tensor)")


def tdesc(t):
    """vfx_tensor for a (B, C, L) tensor view (any strides; element units).  Views created by
    ``guarded()`` carry a ``_vfx_guard`` attribute: readable slack on both sides of every row."""
    assert t.dim() == 3 and t.dtype == torch.float32
    rows = getattr(t, "_vfx_rows", None)   # ragged batches: device int32 (B,) valid length per batch item
    return vfx_tensor(t.data_ptr(), t.stride(0), t.stride(1), t.stride(2), getattr(t, "_vfx_guard", 0),
                      rows.data_ptr() if rows is not None else None)


def with_rows(t, rows):
    """Tag a (B, C, L) view with per-batch-item valid lengths (device int32 (B,)); None removes the tag."""
    if rows is not None:
        assert rows.dtype == torch.int32 and rows.is_cuda and rows.numel() == t.shape[0]
    t._vfx_rows = rows
    return t


def guarded(B, Cn, L, guard, device):
    """(B, C, Lp) view (Lp = L rounded up to 4) with ``guard`` readable elements before and after every
    row; the conv kernels mask whatever they read there, so the slack is never initialised."""
    guard = (guard + 3) // 4 * 4
    Lp = (L + 3) // 4 * 4
    buf = torch.empty((B, Cn, guard + Lp + guard), device=device)
    v = buf[:, :, guard:guard + Lp]
    v._vfx_guard = guard
    v._vfx_base = buf  # keep the allocation alive
    return v


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


# Optional per-launch profiling of the MFMA conv family (bench.py roofline bookkeeping):
# when PROFILE is a list, every conv-family launch is bracketed by HIP events on the launch
# stream and (tile id, algorithmic MACs, start event, end event) is appended.  EVENT_POOL, if set,
# is a list of pre-created timing events that are consumed instead of creating new ones (creating
# an event costs ~10 us of host time, which a launch-bound batch-1 run would otherwise show).
PROFILE = None
EVENT_POOL = None


def _event():
    if EVENT_POOL:
        return EVENT_POOL.pop()
    return torch.cuda.Event(enable_timing=True)


def _prof_begin():
    if PROFILE is None:
        return None
    e = _event()
    e.record()
    return e


def _prof_end(e0, macs):
    if e0 is None:
        return
    e1 = _event()
    e1.record()
    PROFILE.append((_lib.lib().vfx_last_conv_tile(), macs, e0, e1))


class Act:
    """Bundles the fused pre/post activation of a conv launch (keeps tensors alive)."""

    def __init__(self, pre=PRE_NONE, pre_slope=0.0, scale=None, shift=None, post=POST_NONE,
                 post_slope=0.0):
        self.scale, self.shift = scale, shift
        self.c = vfx_act(pre, float(pre_slope), scale.data_ptr() if scale is not None else None,
                         shift.data_ptr() if shift is not None else None, post, float(post_slope))


_NOACT = None
_ACTVARIANTS = {}


def _act(a, w3=None, wd=None, wg4=None):
    """vfx_act* for a launch.  ``w3`` (packing.pack_x3 planes on the device) opts the launch into VFX_MATH_BF16X3 (the
    library falls back to fp32 for geometries its bf16x3 kernel does not cover); ``wd`` (packing.pack_direct on the
    device) offers the fp32 launch the convw_kernel weight layout (vfx_act.w_direct; the library decides); ``wg4``
    (packing.pack_wino4 / pack_wino4_2d on the device) offers a k = 3 / 3x3 launch the Winograd F(4,3) kernels
    (vfx_act.w_wino4)."""
    global _NOACT
    if a is None:
        if _NOACT is None:
            _NOACT = Act()
        a = _NOACT
    if w3 is None and wd is None and wg4 is None:
        return C.byref(a.c)
    key = (id(a), w3.data_ptr() if w3 is not None else 0, wd.data_ptr() if wd is not None else 0,
           wg4.data_ptr() if wg4 is not None else 0)
    ent = _ACTVARIANTS.get(key)
    if ent is None:
        c = vfx_act(a.c.pre_act, a.c.pre_slope, a.c.pre_scale, a.c.pre_shift, a.c.post_act, a.c.post_slope,
                    MATH_BF16X3 if w3 is not None else MATH_F32, w3.data_ptr() if w3 is not None else None,
                    wd.data_ptr() if wd is not None else None, wg4.data_ptr() if wg4 is not None else None)
        ent = _ACTVARIANTS[key] = (c, a, w3, wd, wg4)  # keep the owners alive with the struct
    return C.byref(ent[0])


def conv1d(x, w, bias, y, L, k, dilation=1, pad_mode=PAD_ZERO, act=None, res=None, cin=None, w3=None, wd=None, wg4=None):
    """x (B,Cin,>=L) -> y (B,Cout,>=L) views; w packed [k][CinPad][Cout].  Optional weight layouts the library may use
    instead (it decides per launch, see include/vfx_hip.h: vfx_act): w3 = bf16x3 planes (opts the launch into that
    arithmetic), wd = packing.pack_direct, wg4 = the Winograd F(4,3) transform (k = 3 only)."""
    _need_cuda(x, w, y, res, bias)
    B = x.shape[0]
    cin = x.shape[1] if cin is None else cin
    cout = w.shape[2]
    xd, yd = tdesc(x), tdesc(y)
    rd = tdesc(res) if res is not None else None
    e0 = _prof_begin()
    rc = _lib.lib().vfx_conv1d_f32(C.byref(xd), _ptr(w), _ptr(bias), C.byref(rd) if rd is not None else None,
                                   C.byref(yd), B, cin, cout, L, k, dilation, pad_mode, _act(act, w3, wd, wg4), _stream())
    check(rc, "vfx_conv1d_f32")
    _prof_end(e0, B * L * cin * cout * k)


def conv1d_f16(x, w16, bias, y, L, dilation, act=None, res=None, flag=None):
    """The opt-in f16 arithmetic of a wide ResStack convolution (vfx_conv1d_f16): x (B,C,>=L) -> y (B,C,>=L), k = 3, zero
    padding, w16 = packing.pack_f16 on the device; ``flag`` (device int32 (1,)) is raised when an activation operand leaves
    the fp16 range.  Returns False, launching nothing, when the library does not take the launch (VFX_ENOTSUP): the caller
    then runs it on ``conv1d``."""
    _need_cuda(x, w16, y, res, bias, flag)
    assert w16.dtype == torch.float16
    B, cn = x.shape[0], x.shape[1]
    xd, yd = tdesc(x), tdesc(y)
    rd = tdesc(res) if res is not None else None
    e0 = _prof_begin()
    rc = _lib.lib().vfx_conv1d_f16(C.byref(xd), _ptr(w16), _ptr(bias), C.byref(rd) if rd is not None else None,
                                   C.byref(yd), B, cn, L, dilation, _act(act), _ptr(flag), _stream())
    if rc == _lib.ENOTSUP:
        return False
    check(rc, "vfx_conv1d_f16")
    _prof_end(e0, B * L * cn * cn * 3)
    return True


def resblock(x, y, w1d, b1, w2d, b2, L, dilation, slope=0.01, post=POST_NONE, post_slope=0.0, w2g=None, w2g4=None, w1g4=None):
    """One fused ResStack layer (vfx_resblock_f32): x (B,C,>=L) guarded view -> y (B,C,>=L), y must not alias x.
    ``w2g`` (packing.pack_wino of the second convolution, optional): its dilation-1 half runs as Winograd F(2,3);
    ``w2g4`` (packing.pack_wino4, optional, C = 64): as F(4,3) when the rows of x and y are 16-byte aligned;
    ``w1g4`` (packing.pack_wino4 of the FIRST convolution, optional, C = 64): with w2g4 and a dilation <= 27 BOTH halves run as
    F(4,3) (resblk4_kernel)."""
    _need_cuda(x, y, w1d, b1, w2d, b2, w2g, w2g4, w1g4)
    B, Cn = x.shape[0], x.shape[1]
    xd, yd = tdesc(x), tdesc(y)
    e0 = _prof_begin()
    wts = _lib.vfx_resblock_w(_ptr(w1d), _ptr(b1), _ptr(w2d), _ptr(b2), _ptr(w2g), _ptr(w2g4), _ptr(w1g4))
    rc = _lib.lib().vfx_resblock_f32(C.byref(xd), C.byref(yd), C.byref(wts), B, Cn, L, dilation, float(slope), post,
                                     float(post_slope), _stream())
    check(rc, "vfx_resblock_f32")
    _prof_end(e0, 2 * B * L * Cn * Cn * 3)


def resblock_wino4(x, y, w1g4, b1, w2g4, b2, L, dilation, slope=0.01, post=POST_NONE, post_slope=0.0):
    """One C = 64 ResStack layer with both convolutions as Winograd F(4,3) at any dilation, one launch (vfx_resblock_wino4_f32):
    x (B,64,>=L) -> y (B,64,>=L), y must not alias x.  ``w1g4`` / ``w2g4``: packing.pack_wino4 of the two convolutions.
    Raises where the kernel does not take the layer (alignment, 32-bit offsets, y aliasing x)."""
    _need_cuda(x, y, w1g4, b1, w2g4, b2)
    B, Cn = x.shape[0], x.shape[1]
    xd, yd = tdesc(x), tdesc(y)
    e0 = _prof_begin()
    wts = _lib.vfx_resblock_w(None, _ptr(b1), None, _ptr(b2), None, _ptr(w2g4), _ptr(w1g4))
    rc = _lib.lib().vfx_resblock_wino4_f32(C.byref(xd), C.byref(yd), C.byref(wts), B, Cn, L, dilation, float(slope), post,
                                           float(post_slope), _stream())
    check(rc, "vfx_resblock_wino4_f32")
    _prof_end(e0, 2 * B * L * Cn * Cn * 3)


def convtr1d(x, w, bias, y, Lin, stride, act=None, w3=None, wd=None, wg4=None):
    """``wg4`` (packing.pack_wino32_tr on the device) offers the launch the Winograd F(3,2) kernel (convtw_kernel)."""
    _need_cuda(x, w, y, bias)
    B, cin = x.shape[0], x.shape[1]
    cout = w.shape[2]
    xd, yd = tdesc(x), tdesc(y)
    e0 = _prof_begin()
    rc = _lib.lib().vfx_convtr1d_f32(C.byref(xd), _ptr(w), _ptr(bias), C.byref(yd), B, cin, cout, Lin, stride,
                                     _act(act, w3, wd, wg4), _stream())
    check(rc, "vfx_convtr1d_f32")
    _prof_end(e0, B * Lin * cin * cout * 2 * stride)


def conv2d(x, w, bias, y, H, pitch_log2, ksize, act=None, res=None, cin=None, w3=None, wd=None, wg4=None):
    """x (B,Cin,H*P) pitch map -> y (B,Cout,H*P)."""
    _need_cuda(x, w, y, res, bias)
    B = x.shape[0]
    cin = x.shape[1] if cin is None else cin
    cout = w.shape[2]
    xd, yd = tdesc(x), tdesc(y)
    rd = tdesc(res) if res is not None else None
    e0 = _prof_begin()
    rc = _lib.lib().vfx_conv2d_f32(C.byref(xd), _ptr(w), _ptr(bias), C.byref(rd) if rd is not None else None,
                                   C.byref(yd), B, cin, cout, H, pitch_log2, ksize, _act(act, w3, wd, wg4), _stream())
    check(rc, "vfx_conv2d_f32")
    _prof_end(e0, B * H * ((1 << pitch_log2) - 1) * cin * cout * ksize * ksize)


def convtr2d_3x3s2(x, w, y, h, in_pitch_log2, act=None, w3=None):
    _need_cuda(x, w, y)
    B, cin = x.shape[0], x.shape[1]
    cout = w.shape[2]
    xd, yd = tdesc(x), tdesc(y)
    e0 = _prof_begin()
    rc = _lib.lib().vfx_convtr2d_3x3s2_f32(C.byref(xd), _ptr(w), C.byref(yd), B, cin, cout, h, in_pitch_log2,
                                           _act(act, w3), _stream())
    check(rc, "vfx_convtr2d_3x3s2_f32")
    _prof_end(e0, B * h * ((1 << in_pitch_log2) - 1) * cin * cout * 9)


def conv1d_cout1(x, w, bias, y, L, k, pad_mode=PAD_ZERO, post=POST_NONE, out_mask_log2=0):
    _need_cuda(x, w, y, bias)
    B, cin = x.shape[0], x.shape[1]
    xd, yd = tdesc(x), tdesc(y)
    rc = _lib.lib().vfx_conv1d_cout1_f32(C.byref(xd), _ptr(w), _ptr(bias), C.byref(yd), B, cin, L, k, pad_mode,
                                         post, out_mask_log2, _stream())
    check(rc, "vfx_conv1d_cout1_f32")


def avgpool2x2(x, y, H, pitch_log2):
    _need_cuda(x, y)
    B, Cn = x.shape[0], x.shape[1]
    xd, yd = tdesc(x), tdesc(y)
    check(_lib.lib().vfx_avgpool2x2_f32(C.byref(xd), C.byref(yd), B, Cn, H, pitch_log2, _stream()),
          "vfx_avgpool2x2_f32")


_frontend_ready = set()   # device indices whose tables are uploaded (the library keeps one copy per device)


def frontend_init():
    """Upload window / twiddles / banded HTK filterbank (voicefixer/tools/mel_scale.py:147-238
    restated in float32 torch with the same op order, so the support set is bit-identical)."""
    dev = torch.cuda.current_device()
    if dev in _frontend_ready:
        return
    from .frontend_tables import tables
    win, tw, lo, hi, off, coef = tables()
    check(_lib.lib().vfx_frontend_init(win.ctypes.data, tw.ctypes.data, lo.ctypes.data, hi.ctypes.data,
                                       off.ctypes.data, coef.ctypes.data, int(coef.shape[0])),
          "vfx_frontend_init")
    _frontend_ready.add(dev)


def frontend_readback(which=0):
    """Test hook: the banded filterbank as it sits in device memory (0: HTK / restorer, 1: slaney / Vocoder.oracle)."""
    import numpy as np
    lo, hi, off = (np.zeros(128, np.int32) for _ in range(3))
    coef = np.zeros(8192, np.float32)
    nnz = C.c_int(0)
    check(_lib.lib().vfx_frontend_readback(which, lo.ctypes.data, hi.ctypes.data, off.ctypes.data, coef.ctypes.data,
                                           int(coef.shape[0]), C.byref(nnz)), "vfx_frontend_readback")
    return lo, hi, off, coef[:nnz.value].copy()


def stft_mel(wav, mel, N):
    """wav (B, >=N) device float32 -> mel (B, T, 128)."""
    _need_cuda(wav, mel)
    frontend_init()
    assert wav.stride(1) == 1 and mel.is_contiguous()
    e0 = _prof_begin()
    check(_lib.lib().vfx_stft_mel_f32(_ptr(wav), wav.stride(0), wav.shape[0], N, _ptr(mel), _stream()),
          "vfx_stft_mel_f32")
    if e0 is not None:  # bench.py: HBM roofline of the front-end, algorithmic bytes 4*N + 512*T per utterance
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        PROFILE.append((-1, wav.shape[0] * (4 * N + 512 * (1 + N // 441)), e0, e1))


def stft_mel_rows(wav, mel, n_rows, T):
    """wav (B, >= max n) device float32, n_rows device int32 (B,) (every n >= 1025) -> mel (B, T, 128): row b gets its own
    1 + n_rows[b] // 441 frames; T is the row pitch of mel and must be >= every row's frame count (frames past a row's
    own count are not written)."""
    _need_cuda(wav, mel, n_rows)
    frontend_init()
    assert wav.stride(1) == 1 and mel.is_contiguous() and n_rows.dtype == torch.int32
    check(_lib.lib().vfx_stft_mel_rows_f32(_ptr(wav), wav.stride(0), wav.shape[0], _ptr(n_rows), T, _ptr(mel), _stream()),
          "vfx_stft_mel_rows_f32")


_oracle_ready = set()


def oracle_mel(wav, N):
    """Vocoder.oracle front-end on the device: wav (B, >=N) -> slaney mel (B, T, 128) of wav/max|wav|."""
    _need_cuda(wav)
    frontend_init()
    if torch.cuda.current_device() not in _oracle_ready:
        from .frontend_tables import oracle_tables
        lo, hi, off, coef = oracle_tables()
        check(_lib.lib().vfx_frontend_init_oracle(lo.ctypes.data, hi.ctypes.data, off.ctypes.data, coef.ctypes.data,
                                                  int(coef.shape[0])), "vfx_frontend_init_oracle")
        _oracle_ready.add(torch.cuda.current_device())
    B = wav.shape[0]
    T = 1 + N // 441
    peak = torch.empty((B,), dtype=torch.int32, device=wav.device)
    check(_lib.lib().vfx_peak_f32(_ptr(wav), wav.stride(0), N, B, _ptr(peak), _stream()), "vfx_peak_f32")
    mel = torch.empty((B, T, 128), device=wav.device)
    check(_lib.lib().vfx_stft_mel_oracle_f32(_ptr(wav), wav.stride(0), B, N, _ptr(peak), _ptr(mel), _stream()),
          "vfx_stft_mel_oracle_f32")
    return mel, T


def mel_to_cond_plain(mel, cond, T):
    """dB / normalise / clip / tail-pad WITHOUT the mel-weight division (Vocoder.oracle path)."""
    _need_cuda(mel, cond)
    cd = tdesc(cond)
    check(_lib.lib().vfx_mel_to_cond_ex_f32(_ptr(mel), C.byref(cd), mel.shape[0], T, 0, _stream()),
          "vfx_mel_to_cond_ex_f32")


def hf_cut(wav, N, ratio=0.95):
    """mode-1 pre-filter (remove_higher_frequency): wav (B, >=N) device -> ((B, 512*(N//512)), cut-off bins)."""
    _need_cuda(wav)
    frontend_init()
    B = wav.shape[0]
    nbytes = _lib.lib().vfx_hf_workspace_bytes(B, N)
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=wav.device)
    out = torch.empty((B, 512 * (N // 512)), device=wav.device)
    cut = torch.empty((B,), dtype=torch.int32, device=wav.device)
    check(_lib.lib().vfx_hf_cut_f32(_ptr(wav), wav.stride(0), B, N, _ptr(out), out.stride(0), float(ratio), _ptr(ws),
                                    nbytes, _ptr(cut), _stream()), "vfx_hf_cut_f32")
    return out, cut


def tm_to_cm(src, dst, T, Cn):
    """src (B,T,C) contiguous -> dst (B,C,>=T) view."""
    _need_cuda(src, dst)
    assert src.is_contiguous() and dst.stride(2) == 1
    check(_lib.lib().vfx_tm_to_cm_f32(_ptr(src), _ptr(dst), src.shape[0], T, Cn, dst.stride(0), dst.stride(1),
                                      _stream()), "vfx_tm_to_cm_f32")


def unet_input(mel, mask, unet_in, T, Tp):
    """unet_in: (B, nch >= 2, >= Tp*128) view; channels >= 2 are written as zero."""
    _need_cuda(mel, mask, unet_in)
    md, ud = tdesc(mask), tdesc(unet_in)
    check(_lib.lib().vfx_unet_input_f32(_ptr(mel), C.byref(md), C.byref(ud), unet_in.shape[1], mel.shape[0], T, Tp,
                                        _stream()), "vfx_unet_input_f32")


def unet_output(unet_out, unet_in, mel, mask, logmel, denoised, T, Tp):
    _need_cuda(unet_out, unet_in, mel, mask, logmel, denoised)
    md, od, ud = tdesc(mask), tdesc(unet_out), tdesc(unet_in)
    check(_lib.lib().vfx_unet_output_f32(C.byref(od), C.byref(ud), _ptr(mel), C.byref(md), _ptr(logmel),
                                         _ptr(denoised), mel.shape[0], T, Tp, _stream()), "vfx_unet_output_f32")


def gru_layout():
    a, b, c = C.c_int(), C.c_int(), C.c_int()
    _lib.lib().vfx_gru_layout(C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def gru_bidir(gi, whh_t, bhh, out, T):
    """whh_t: packed by packing.pack_gru_whh(..., *gru_layout())."""
    _need_cuda(gi, whh_t, bhh, out)
    od = tdesc(out)
    check(_lib.lib().vfx_gru_bidir_f32(_ptr(gi), _ptr(whh_t), _ptr(bhh), C.byref(od), gi.shape[0], T, _stream()),
          "vfx_gru_bidir_f32")


GRU2_MAX_B = 60  # C ABI limit: 4 workgroups per utterance, one per CU, all resident (engine.Pipeline.set_streams sizes launches per stream count)


def gru_bidir2(gi, whh_t, bhh, out, T, err_flag):
    """Two-CU-per-sequence GRU (vfx_gru_bidir2_f32).  whh_t: plain (2,256,768); err_flag: device int32[1]."""
    _need_cuda(gi, whh_t, bhh, out, err_flag)
    B = gi.shape[0]
    assert B <= GRU2_MAX_B
    nbytes = B * 2 * 2 * 2 * 384 * 8
    mbox = torch.empty((nbytes // 4,), dtype=torch.int32, device=gi.device)
    od = tdesc(out)
    check(_lib.lib().vfx_gru_bidir2_f32(_ptr(gi), _ptr(whh_t), _ptr(bhh), C.byref(od), B, T, _ptr(mbox), nbytes,
                                        _ptr(err_flag), _stream()), "vfx_gru_bidir2_f32")
    return mbox  # keep alive until the stream has consumed it (caller holds the reference)


def mel_to_cond(mel, cond, T, t_rows=None):
    """mel (B, T, 128) -> cond (B, 128, >= T'); t_rows (device int32 or None): frames of every row (ragged batches)."""
    _need_cuda(mel, cond, t_rows)
    assert mel.is_contiguous()
    cd = tdesc(cond)
    check(_lib.lib().vfx_mel_to_cond_rows_f32(_ptr(mel), C.byref(cd), mel.shape[0], T, _ptr(t_rows), 1, _stream()),
          "vfx_mel_to_cond_rows_f32")


def post_rows(y, Ly, out, n_rows, n_max, peak_ws, ly_rows=None):
    """y (B, >=Ly) -> out (B, >= n_max): per-utterance peak rule + centre trim to n_rows[b] samples (device int32);
    ly_rows (device int32 or None): vocoder samples of every row."""
    _need_cuda(y, out, peak_ws, n_rows, ly_rows)
    check(_lib.lib().vfx_post_rows_f32(_ptr(y), y.stride(0), Ly, _ptr(ly_rows), _ptr(out), out.stride(0), _ptr(n_rows),
                                       n_max, y.shape[0], _ptr(peak_ws), _stream()), "vfx_post_rows_f32")


def post(y, Ly, out, N, peak_ws):
    """y (B, >=Ly) -> out (B, N): per-utterance peak rule + centre trim."""
    _need_cuda(y, out, peak_ws)
    check(_lib.lib().vfx_post_f32(_ptr(y), y.stride(0), Ly, _ptr(out), out.stride(0), N, y.shape[0],
                                  _ptr(peak_ws), _stream()), "vfx_post_f32")


# ---- train-mode restorer (mode 2) --------------------------------------------------------------------------------
def bn_stats(x, L, pitch_log2, gamma, beta, scale, shift, eps=1e-5):
    """Batch statistics of train-mode BatchNorm -> scale / shift (device float32 (B*G,)).  ``pitch_log2`` > 0: x is a
    (B,C,L = H*P) pitch map, one BN channel per map channel, over each row's x._vfx_rows extent and the first P-1
    columns; 0: x is a (B,C,L) activation and one BN channel spans all C channels (BatchNorm2d(1) on (B,1,T,C)).
    The workspace comes from torch's caching allocator (stream-ordered: it is not reused before the launches ran)."""
    _need_cuda(x, gamma, beta, scale, shift)
    B, Cn = x.shape[0], x.shape[1]
    h = _lib.lib()
    nb = h.vfx_bn_stats_workspace_bytes(B, Cn, L, pitch_log2)
    ws = torch.empty(((nb + 7) // 8,), dtype=torch.float64, device=x.device)
    xd = tdesc(x)
    check(h.vfx_bn_stats_f32(C.byref(xd), B, Cn, L, pitch_log2, _ptr(gamma), _ptr(beta), float(eps), _ptr(scale),
                             _ptr(shift), _ptr(ws), nb, _stream()), "vfx_bn_stats_f32")


def bn_apply(x, y, L, pitch_log2, scale, shift, slope=None, groups=None):
    """y = act(x * scale + shift) over x's valid region (x._vfx_rows); ``slope`` None: identity, else leaky ReLU with
    that slope (0.0: ReLU).  ``groups`` defaults to the channel count for maps (pitch_log2 > 0) and to 1 otherwise."""
    _need_cuda(x, y, scale, shift)
    B, Cn = x.shape[0], x.shape[1]
    if groups is None:
        groups = Cn if pitch_log2 > 0 else 1
    xd, yd = tdesc(x), tdesc(y)
    act, s = (POST_NONE, 0.0) if slope is None else (POST_LRELU, float(slope))
    check(_lib.lib().vfx_bn_apply_f32(C.byref(xd), C.byref(yd), B, Cn, L, pitch_log2, groups, _ptr(scale), _ptr(shift),
                                      act, s, _stream()), "vfx_bn_apply_f32")


def dropout(x, T, rowkey, layer, relu=False):
    """Seeded dropout (voicefixer_amd/dropout.py) in place on x (B,C,>=T), rows from x._vfx_rows; ``rowkey`` device
    int32 (B,3) = (segment, key lo, key hi) per row."""
    _need_cuda(x, rowkey)
    assert rowkey.dtype == torch.int32 and rowkey.is_contiguous() and rowkey.numel() == 3 * x.shape[0]
    xd = tdesc(x)
    check(_lib.lib().vfx_dropout_f32(C.byref(xd), x.shape[0], x.shape[1], T, _ptr(rowkey), int(layer), int(bool(relu)),
                                     _stream()), "vfx_dropout_f32")


_RESAMPLE_BANKS = {}


def resample_bank(device, up, down):
    """(bank, J, c) of the (up, down) conversion on ``device``: audio_io.hq_bank uploaded once per device and cached."""
    key = (str(torch.device(device)), up, down)
    hit = _RESAMPLE_BANKS.get(key)
    if hit is None:
        from . import audio_io
        bank, J, c = audio_io.hq_bank(up, down)
        hit = (torch.from_numpy(bank).to(device), J, c)
        _RESAMPLE_BANKS[key] = hit
    return hit


def resample_rows(x, n_rows, y, up, down, ny_max=None, row_index=None):
    """Polyphase rate conversion on the device (vfx_resample_rows_f32): x (B, >= max n) -> y (B, >= ny_max); row r holds
    n_rows[r] samples (device int32 (B,)) and receives ceil(n_rows[r] * up / down) of them (at most ny_max, default y's
    width).  row_index (device int32 or None): only the listed rows are converted, the others are left untouched."""
    _need_cuda(x, n_rows, y, row_index)
    assert x.dtype == torch.float32 and y.dtype == torch.float32 and x.dim() == 2 and y.dim() == 2
    assert x.stride(1) == 1 and y.stride(1) == 1 and x.shape[0] == y.shape[0] == n_rows.numel()
    assert n_rows.dtype == torch.int32 and (row_index is None or row_index.dtype == torch.int32)
    ny_max = y.shape[1] if ny_max is None else int(ny_max)
    if ny_max > y.shape[1]:
        raise _lib.VfxError("resample_rows: ny_max %d exceeds the output width %d" % (ny_max, y.shape[1]))
    bank, J, c = resample_bank(x.device, int(up), int(down))
    n_index = x.shape[0] if row_index is None else row_index.numel()
    check(_lib.lib().vfx_resample_rows_f32(_ptr(x), x.stride(0) if x.shape[0] > 1 else x.shape[1], _ptr(n_rows),
                                           x.shape[0], _ptr(row_index), n_index, _ptr(bank), J, int(up), int(down), c,
                                           _ptr(y), y.stride(0) if y.shape[0] > 1 else y.shape[1], ny_max, _stream()),
          "vfx_resample_rows_f32")


INT64_MAX = 2 ** 63 - 1


def _check_span(name, xw, out, m0, m1):
    """What the ``*_span`` wrappers ask of their window and their output: float32, 1-D, contiguous, on the device, and room for
    the m1 - m0 outputs (VfxError otherwise).  Returns (m0, m1) as ints."""
    _need_cuda(xw, out)
    assert xw.dtype == torch.float32 and out.dtype == torch.float32 and xw.dim() == 1 and out.dim() == 1
    assert (xw.numel() == 0 or xw.stride(0) == 1) and (out.numel() == 0 or out.stride(0) == 1)
    m0, m1 = int(m0), int(m1)
    if m1 - m0 > out.numel():
        raise _lib.VfxError("%s: %d outputs into a buffer of %d" % (name, m1 - m0, out.numel()))
    return m0, m1


def resample_span(xw, g0, n_total, up, down, m0, m1, y):
    """Outputs [m0, m1) of ONE row's rate conversion from a window of it (vfx_resample_span_f32): xw (wlen,) device holds
    samples [g0, g0 + wlen) of a row of ``n_total`` samples (None: its end is not known yet), y (>= m1 - m0,) receives
    output m at y[m - m0] -- the bits ops.resample_rows writes for output m of the whole row.  The window must cover what
    the span reads (audio_io.span_window clipped to [0, n_total)), or VfxError.  The bank is resample_bank's."""
    m0, m1 = _check_span("resample_span", xw, y, m0, m1)
    bank, J, c = resample_bank(xw.device, int(up), int(down))
    check(_lib.lib().vfx_resample_span_f32(_ptr(xw), int(g0), xw.numel(), INT64_MAX if n_total is None else int(n_total),
                                           _ptr(bank), J, int(up), int(down), c, m0, m1, _ptr(y), _stream()),
          "vfx_resample_span_f32")


def xfade(tail, head, fade, out):
    """out = tail * (1 - fade) + head * fade over the n = fade.numel() samples of an overlap (vfx_xfade_f32): the bits of the
    float32 numpy expression of restore_stream.  out may be tail or head."""
    _need_cuda(tail, head, fade, out)
    n = fade.numel()
    for t in (tail, head, fade, out):
        assert t.dtype == torch.float32 and t.dim() == 1 and t.numel() == n and (n == 0 or t.stride(0) == 1)
    check(_lib.lib().vfx_xfade_f32(_ptr(tail), _ptr(head), _ptr(fade), n, _ptr(out), _stream()), "vfx_xfade_f32")


def quantize_rows(x, n_rows, bit_depth, dither, seed, n0=None, chan=None, out=None):
    """Word-length reduction on the device (vfx_quantize_rows_f32; wordlength.py is the specification): row r of x (B, >= max
    n) holds n_rows[r] float samples (device int32 (B,)) and becomes ``bit_depth``-bit PCM -- int16 rows at 16, int32 rows at 24
    -- with the dither ``dither`` ("none", "tpdf", "hp") of ``seed``.  ``n0`` (device int64 (B,), default 0): the absolute index
    of every row's first sample in its file; ``chan`` (device int32 (B,), default 0): its channel (0..7).  Returns (out, result):
    ``out`` (default: a new (B, width of x) tensor) is written up to every row's own length and nowhere else, ``result`` is a device
    int32 (B, 2) of {clipped samples, max |q|}.  One kernel behind one clear of ``result``, no synchronisation."""
    from . import dropout, wordlength
    _need_cuda(x, n_rows, n0, chan, out)
    bits, kind, seed = wordlength.check_bit_depth(bit_depth), wordlength.check_dither(dither), dropout.check_seed(seed)
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and x.shape[0] == n_rows.numel()
    assert n_rows.dtype == torch.int32 and n_rows.is_contiguous()
    B, n_max = x.shape
    assert n0 is None or (n0.dtype == torch.int64 and n0.is_contiguous() and n0.numel() == B)
    assert chan is None or (chan.dtype == torch.int32 and chan.is_contiguous() and chan.numel() == B)
    dtype = torch.int16 if bits == 16 else torch.int32
    if out is None:
        out = torch.empty((B, n_max), dtype=dtype, device=x.device)
    assert out.dtype == dtype and out.dim() == 2 and out.stride(1) == 1 and out.shape[0] == B and out.shape[1] >= n_max
    res = torch.empty((B, 2), dtype=torch.int32, device=x.device)
    check(_lib.lib().vfx_quantize_rows_f32(_ptr(x), x.stride(0) if B > 1 else n_max, _ptr(n_rows), B, n_max, _ptr(n0), _ptr(chan),
                                           bits, wordlength.DITHERS.index(kind), seed, _ptr(out),
                                           out.stride(0) if B > 1 else out.shape[1], _ptr(res), _stream()),
          "vfx_quantize_rows_f32")
    return out, res


_LOUDNESS_MPOW = {}


def true_peak_bank(device, R):
    """(bank, J, c) of the R-times interpolator of the true-peak measurement on ``device``: audio_io.hq_bank(R, 1) uploaded
    once per device and cached (the cache of resample_bank: there is one filter design)."""
    if R not in (2, 4):
        raise _lib.VfxError("true_peak_bank: R must be 2 or 4 (got %r)" % (R,))
    return resample_bank(device, int(R), 1)


def _loudness_plan(x, rate):
    from . import loudness
    p = loudness.plan(rate)
    key = (str(x.device), int(rate))
    mpow = _LOUDNESS_MPOW.get(key)
    if mpow is None:
        mpow = torch.from_numpy(p["mpow"]).to(x.device)
        _LOUDNESS_MPOW[key] = mpow
    R = loudness.oversampling(rate)
    bank, J, c = true_peak_bank(x.device, R) if R > 1 else (mpow, 1, 0)      # (R = 1: never read, must not be null)
    return p, mpow, (C.c_double * 10)(*[float(v) for v in p["coef"]]), (bank, J, R, c)


def loudness_rows(x, n_rows, rate, target=None, ceiling_db=-1.0, out=None, true_peak=False):
    """Integrated loudness (BS.1770-4, one channel) of the rows of x (B, >= max n) on the device (vfx_loudness_rows_f32):
    row r holds n_rows[r] samples (device int32 (B,)) at ``rate`` Hz.  Returns a device float64 (B, 3) of {L in LUFS (-inf:
    nothing above the gates), gain, sample peak}.  ``target`` (LUFS): rows are scaled by float32(gain) into ``out`` (default:
    in place, into x) up to their own lengths; None measures only.  At most 4 launches, no synchronisation.
    ``true_peak=True`` (vfx_loudness_tp_rows_f32): the ceiling is a TRUE-peak one (dBTP; loudness.py), the result is
    (B, 4) = {L, gain, sample peak, true peak}, one launch more (none more at rates from 192 kHz)."""
    from . import loudness
    if loudness.check_true_peak(true_peak):
        return _loudness_tp_rows(x, n_rows, rate, target, ceiling_db, out)
    _need_cuda(x, n_rows, out)
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and x.shape[0] == n_rows.numel()
    assert n_rows.dtype == torch.int32
    target = loudness.check_target(target)
    ceiling_db = loudness.check_ceiling(ceiling_db)
    p = loudness.plan(rate)
    key = (str(x.device), int(rate))
    mpow = _LOUDNESS_MPOW.get(key)
    if mpow is None:
        mpow = torch.from_numpy(p["mpow"]).to(x.device)
        _LOUDNESS_MPOW[key] = mpow
    if target is not None and out is None:
        out = x
    if out is not None:
        assert out.dtype == torch.float32 and out.dim() == 2 and out.stride(1) == 1 and out.shape[0] == x.shape[0]
        assert out.shape[1] >= x.shape[1]
    B, n_max = x.shape
    h = _lib.lib()
    nb = h.vfx_loudness_workspace_bytes(B, n_max, p["hop"], p["S"])
    ws = torch.empty(((nb + 7) // 8,), dtype=torch.float64, device=x.device)
    res = torch.empty((B, 3), dtype=torch.float64, device=x.device)
    coef = (C.c_double * 10)(*[float(v) for v in p["coef"]])
    check(h.vfx_loudness_rows_f32(_ptr(x), x.stride(0) if B > 1 else n_max, _ptr(n_rows), B, n_max, coef, _ptr(mpow),
                                  p["S"], p["hop"], p["lookback"], float("nan") if target is None else target, ceiling_db,
                                  _ptr(out), (out.stride(0) if B > 1 else out.shape[1]) if out is not None else 0, _ptr(res),
                                  _ptr(ws), nb, _stream()), "vfx_loudness_rows_f32")
    return res


def _loudness_tp_rows(x, n_rows, rate, target, ceiling_db, out):
    from . import loudness
    _need_cuda(x, n_rows, out)
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and x.shape[0] == n_rows.numel()
    assert n_rows.dtype == torch.int32
    target = loudness.check_target(target)
    ceiling_db = loudness.check_ceiling(ceiling_db)
    p, mpow, coef, (bank, J, R, c) = _loudness_plan(x, rate)
    if target is not None and out is None:
        out = x
    if out is not None:
        assert out.dtype == torch.float32 and out.dim() == 2 and out.stride(1) == 1 and out.shape[0] == x.shape[0]
        assert out.shape[1] >= x.shape[1]
    B, n_max = x.shape
    h = _lib.lib()
    nb = h.vfx_loudness_workspace_bytes(B, n_max, p["hop"], p["S"]) + h.vfx_true_peak_workspace_bytes(B, n_max, R, J)
    ws = torch.empty(((nb + 7) // 8,), dtype=torch.float64, device=x.device)
    res = torch.empty((B, 4), dtype=torch.float64, device=x.device)
    check(h.vfx_loudness_tp_rows_f32(_ptr(x), x.stride(0) if B > 1 else n_max, _ptr(n_rows), B, n_max, coef, _ptr(mpow),
                                     p["S"], p["hop"], p["lookback"], float("nan") if target is None else target,
                                     ceiling_db, _ptr(bank), J, R, c, _ptr(out),
                                     (out.stride(0) if B > 1 else out.shape[1]) if out is not None else 0, _ptr(res),
                                     _ptr(ws), nb, _stream()), "vfx_loudness_tp_rows_f32")
    return res


def loudness_report_rows(x, n_rows, rate):
    """Loudness report of the rows of x (B, >= max n) on the device (vfx_loudness_report_rows_f32; definitions:
    loudness.py): a device float64 (B, 6) of {integrated loudness, loudness range, maximum momentary, maximum short-term
    loudness, sample peak, true peak} (peaks linear).  Measures only; one launch more than loudness_rows(true_peak=True)."""
    _need_cuda(x, n_rows)
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and x.shape[0] == n_rows.numel()
    assert n_rows.dtype == torch.int32
    p, mpow, coef, (bank, J, R, c) = _loudness_plan(x, rate)
    B, n_max = x.shape
    h = _lib.lib()
    nb = h.vfx_loudness_report_workspace_bytes(B, n_max, p["hop"], p["S"], R, J)
    ws = torch.empty(((nb + 7) // 8,), dtype=torch.float64, device=x.device)
    rep = torch.empty((B, 6), dtype=torch.float64, device=x.device)
    check(h.vfx_loudness_report_rows_f32(_ptr(x), x.stride(0) if B > 1 else n_max, _ptr(n_rows), B, n_max, coef, _ptr(mpow),
                                         p["S"], p["hop"], p["lookback"], _ptr(bank), J, R, c, _ptr(rep), _ptr(ws), nb,
                                         _stream()), "vfx_loudness_report_rows_f32")
    return rep


_LOUDNESS_GROUPS = {}


def _loudness_groups_plan(x, n_rows, groups, weights):
    """Host checks of a grouped call and its cached uploads: (device n_rows, group_start, weight, G).  The uploads are keyed
    by (device, groups, weights, lengths): a repeated call with the lengths as a LIST uploads nothing and never waits for
    the device; a device ``n_rows`` is read back for the checks (one synchronising copy per call)."""
    from . import loudness
    B = x.shape[0]
    groups = [loudness.check_channel_count(g) for g in groups]
    if sum(groups) != B:
        raise ValueError("loudness_groups: the channel counts sum to %d, the batch has %d rows" % (sum(groups), B))
    lens = [int(v) for v in (n_rows.tolist() if torch.is_tensor(n_rows) else n_rows)]
    if len(lens) != B:
        raise ValueError("loudness_groups: %d lengths for %d rows" % (len(lens), B))
    if weights is None:
        weights = [w for g in groups for w in loudness.channel_weights(g)]
    else:
        weights = [float(w) for w in weights]
        if len(weights) != B or not all(math.isfinite(w) and w >= 0.0 for w in weights):
            raise ValueError("loudness_groups: weights must be %d finite numbers >= 0" % B)
    start = [0]
    for g in groups:
        if len(set(lens[start[-1]:start[-1] + g])) != 1:
            raise ValueError("loudness_groups: the rows of a programme must have one length (rows %d..%d have %r)"
                             % (start[-1], start[-1] + g - 1, lens[start[-1]:start[-1] + g]))
        start.append(start[-1] + g)
    if min(lens) < 0 or max(lens) > x.shape[1]:
        raise ValueError("loudness_groups: row lengths must be in [0, %d]" % x.shape[1])
    key = (str(x.device), tuple(groups), tuple(weights), tuple(lens))
    hit = _LOUDNESS_GROUPS.get(key)
    if hit is None:
        if len(_LOUDNESS_GROUPS) >= 64:
            _LOUDNESS_GROUPS.clear()
        hit = (torch.tensor(start, dtype=torch.int32).to(x.device), torch.tensor(weights, dtype=torch.float64).to(x.device),
               torch.tensor(lens, dtype=torch.int32).to(x.device))
        _LOUDNESS_GROUPS[key] = hit
    return (n_rows if torch.is_tensor(n_rows) else hit[2]), hit[0], hit[1], len(groups)


def loudness_groups(x, n_rows, groups, fs, target=None, peak_ceiling=-1.0, out=None, weights=None, true_peak=True):
    """Integrated loudness of PROGRAMMES of several channels (vfx_loudness_groups_f32; loudness.py): the
    rows of x (B, >= max n) are ``groups`` = [C_0, C_1, ...] adjacent channels per programme (each 1..8, summing to B), row
    r holding n_rows[r] samples -- one length per programme.  ``n_rows`` as a LIST of ints is the non-blocking form: the
    checks run on the list and the uploaded lengths, group starts and weights are cached, so a repeated call neither copies
    nor waits.  A device int32 (B,) is accepted too, but it is read back to the host for the equal-length check on every
    call, which synchronises with the device.  ``weights``: B channel weights (default: loudness.channel_weights of every programme).
    Returns a device float64 (G, 4) of {L, gain, sample peak, true peak} per programme; with ``target`` every row is
    scaled by its programme's float32(gain) into ``out`` (default: in place).  The launches of
    loudness_rows(true_peak=True); ValueError before anything is launched on groups or lengths that do not fit.
    ``true_peak=False``: nothing is oversampled (the entry point's R = 1 form, one launch fewer), the fourth value repeats
    the sample peak and ``peak_ceiling`` is a sample-peak ceiling."""
    from . import loudness
    _need_cuda(x, out)
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
    target = loudness.check_target(target)
    peak_ceiling = loudness.check_ceiling(peak_ceiling)
    n_rows, start, wt, G = _loudness_groups_plan(x, n_rows, groups, weights)
    _need_cuda(n_rows)
    assert n_rows.dtype == torch.int32 and n_rows.numel() == x.shape[0]
    p, mpow, coef, (bank, J, R, c) = _loudness_plan(x, fs)
    if not loudness.check_true_peak(true_peak):
        bank, J, R, c = mpow, 1, 1, 0                      # (R = 1: the bank is never read, must not be null)
    if target is not None and out is None:
        out = x
    if out is not None:
        assert out.dtype == torch.float32 and out.dim() == 2 and out.stride(1) == 1 and out.shape[0] == x.shape[0]
        assert out.shape[1] >= x.shape[1]
    B, n_max = x.shape
    h = _lib.lib()
    nb = h.vfx_loudness_groups_workspace_bytes(B, n_max, p["hop"], p["S"], R, J)
    ws = torch.empty(((nb + 7) // 8,), dtype=torch.float64, device=x.device)
    res = torch.empty((G, 4), dtype=torch.float64, device=x.device)
    check(h.vfx_loudness_groups_f32(_ptr(x), x.stride(0) if B > 1 else n_max, _ptr(n_rows), B, n_max, _ptr(start), _ptr(wt),
                                    G, coef, _ptr(mpow), p["S"], p["hop"], p["lookback"],
                                    float("nan") if target is None else target, peak_ceiling, _ptr(bank), J, R, c, _ptr(out),
                                    (out.stride(0) if B > 1 else out.shape[1]) if out is not None else 0, _ptr(res),
                                    _ptr(ws), nb, _stream()), "vfx_loudness_groups_f32")
    return res


def loudness_limit(x, n_rows, rate, target, ceiling_db=-1.0, true_peak=True, lookahead_ms=3.0, out=None, groups=None,
                   weights=None):
    """Loudness normalisation with the look-ahead peak limiter in place of the static ceiling (vfx_loudness_limit_f32;
    loudness.py): the rows of x (B, >= max n) at ``rate`` Hz are brought to ``target`` LUFS, and where that
    would pass the ceiling (dBTP with ``true_peak``, else dBFS) a gain curve that looks ``lookahead_ms`` ahead holds the peaks
    under it.  ``groups`` = [C_0, C_1, ...]: programmes of adjacent channels as in loudness_groups (``n_rows`` then a list or
    a device tensor as there, one gain curve per programme); None: one programme per row, ``n_rows`` a device int32 (B,).
    Writes ``out`` (default: in place) up to every row's own length and returns a device float64 (G or B, 8) of {L, gL, P,
    TP, bound, min g, t, peak after}.  No synchronisation; the launch count depends on neither B nor the lengths."""
    from . import loudness
    _need_cuda(x, out)
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
    target = loudness.check_target(target)
    if target is None:
        raise ValueError("loudness_limit: the limiter needs a loudness target")
    ceiling_db = loudness.check_ceiling(ceiling_db)
    true_peak = loudness.check_true_peak(true_peak)
    H = loudness.limiter_window(rate, lookahead_ms)[0]
    start = wt = None
    G = 0
    if groups is not None:
        n_rows, start, wt, G = _loudness_groups_plan(x, n_rows, groups, weights)
    _need_cuda(n_rows)
    assert n_rows.dtype == torch.int32 and n_rows.numel() == x.shape[0]
    p, mpow, coef, (bank, J, R, c) = _loudness_plan(x, rate)
    if not true_peak:
        bank, J, R, c = mpow, 1, 1, 0                      # (R = 1: the bank is never read, must not be null)
    if out is None:
        out = x
    assert out.dtype == torch.float32 and out.dim() == 2 and out.stride(1) == 1 and out.shape[0] == x.shape[0]
    assert out.shape[1] >= x.shape[1]
    B, n_max = x.shape
    h = _lib.lib()
    nb = h.vfx_loudness_limit_workspace_bytes(B, n_max, p["hop"], p["S"], R, J)
    ws = torch.empty(((nb + 7) // 8,), dtype=torch.float64, device=x.device)
    res = torch.empty((G if G else B, 8), dtype=torch.float64, device=x.device)
    check(h.vfx_loudness_limit_f32(_ptr(x), x.stride(0) if B > 1 else n_max, _ptr(n_rows), B, n_max, _ptr(start), _ptr(wt), G,
                                   coef, _ptr(mpow), p["S"], p["hop"], p["lookback"], target, ceiling_db, _ptr(bank), J, R, c,
                                   _ptr(out), out.stride(0) if B > 1 else out.shape[1], H, 1 if true_peak else 0, _ptr(res),
                                   _ptr(ws), nb, _stream()), "vfx_loudness_limit_f32")
    return res


def _limit_span_impl(name, rows, xw, g0, n_total, rate, gain_db, m0, m1, out, ceiling_db, true_peak, lookahead_ms):
    """``limit_span`` and ``limit_span_rows`` (``name``) behind their checks of the window and the output: rows = (C, w_stride,
    out_stride) of xw (C, wlen) and out (C, >= m1 - m0) -- a row is (1, wlen, m1 - m0), its 1-D tensors taken as they are (only
    their pointers and the last dimension are used, so no 2-D view is made); m0 and m1 are ints.  Only the entry point depends on
    ``name``: a row keeps the mono entry point, its order of refusals and its name in an error."""
    from . import loudness
    gain_db = loudness.check_gain(gain_db)
    if gain_db is None:
        raise ValueError("%s: the limiter needs a gain (gain_db=...)" % name)
    ceiling_db = loudness.check_ceiling(ceiling_db)
    true_peak = loudness.check_true_peak(true_peak)
    H = loudness.limiter_window(rate, lookahead_ms)[0]
    if m1 == m0:
        return torch.tensor([1.0, 0.0], dtype=torch.float64).to(xw.device)
    R = loudness.oversampling(rate) if true_peak else 1
    bank, J, c = true_peak_bank(xw.device, R) if R > 1 else (None, 1, 0)
    h = _lib.lib()
    nb = h.vfx_limit_span_rows_workspace_bytes(m1 - m0, H, rows[0])
    ws = torch.empty(((nb + 7) // 8,), dtype=torch.float64, device=xw.device)
    rec = torch.empty((2,), dtype=torch.float64, device=xw.device)
    span = (int(g0), xw.shape[-1], INT64_MAX if n_total is None else int(n_total), m0, m1, 10.0 ** (gain_db / 20.0), ceiling_db, H,
            _ptr(bank), J, R, c, _ptr(out))
    tail = (_ptr(rec), _ptr(ws), nb, _stream())
    check(h.vfx_limit_span_f32(_ptr(xw), *span, *tail) if name == "limit_span" else
          h.vfx_limit_span_rows_f32(_ptr(xw), rows[1], rows[0], *span, rows[2], *tail), "vfx_%s_f32" % name)
    return rec


def limit_span(xw, g0, n_total, rate, gain_db, m0, m1, out, ceiling_db=-1.0, true_peak=False, lookahead_ms=3.0):
    """Outputs [m0, m1) of the fixed-gain look-ahead limiter over ONE row from a window of it (vfx_limit_span_f32; loudness.py,
    DESIGN.md 3.16): xw (wlen,) device holds samples [g0, g0 + wlen) of a row of ``n_total`` samples at ``rate`` Hz (None: its
    end is not known yet), out (>= m1 - m0,) receives output n at out[n - m0] -- the bits the single span [0, n_total) over the
    whole row writes for it.  The window must cover [m0 - 2 H - Bk, m1 - 1 + 2 H + Fw] clipped to the row
    (loudness.limiter_reach), or VfxError.  Returns the record, a device float64 (2,) of {min g, max |out|} over the span
    ({1, 0} for an empty one).  Three launches, no synchronisation."""
    m0, m1 = _check_span("limit_span", xw, out, m0, m1)
    return _limit_span_impl("limit_span", (1, xw.numel(), m1 - m0), xw, g0, n_total, rate, gain_db, m0, m1, out, ceiling_db, true_peak, lookahead_ms)


def _check_span_rows(name, xw, out, m0, m1):
    """What the ``*_span_rows`` wrappers ask of their windows and their outputs: float32, 2-D with the same 1..8 rows, unit
    stride along a row (any row stride), on the device, and room for the m1 - m0 outputs per row (VfxError otherwise).  Returns
    (C, m0, m1, w_stride, out_stride) as ints."""
    from . import loudness
    _need_cuda(xw, out)
    assert xw.dtype == torch.float32 and out.dtype == torch.float32 and xw.dim() == 2 and out.dim() == 2
    C = loudness.check_channel_count(int(xw.shape[0]))
    assert out.shape[0] == C
    assert (xw.shape[1] <= 1 or xw.stride(1) == 1) and (out.shape[1] <= 1 or out.stride(1) == 1)
    m0, m1 = int(m0), int(m1)
    if m1 - m0 > out.shape[1]:
        raise _lib.VfxError("%s: %d outputs per channel into a buffer of %d" % (name, m1 - m0, out.shape[1]))
    # (one row: any stride that holds the row will do)
    return (C, m0, m1, int(xw.stride(0)) if C > 1 else max(int(xw.stride(0)), int(xw.shape[1])),
            int(out.stride(0)) if C > 1 else max(int(out.stride(0)), int(out.shape[1])))


def limit_span_rows(xw, g0, n_total, rate, gain_db, m0, m1, out, ceiling_db=-1.0, true_peak=False, lookahead_ms=3.0):
    """Outputs [m0, m1) of the LINKED fixed-gain limiter over a programme of C channels from a window of it
    (vfx_limit_span_rows_f32): ``limit_span`` with xw (C, wlen) and out (C, >= m1 - m0), rows of unit stride and
    any row stride.  One envelope, the maximum over the channels, hence one gain for all of them; the record is {min g, max |out|
    over all channels}.  C = 1: the bits and the record of ``limit_span``.  Three launches, no synchronisation."""
    C_, m0, m1, ws_, os_ = _check_span_rows("limit_span_rows", xw, out, m0, m1)
    return _limit_span_impl("limit_span_rows", (C_, ws_, os_), xw, g0, n_total, rate, gain_db, m0, m1, out, ceiling_db, true_peak,
                            lookahead_ms)


_LEVELLER_MPOW = {}


def level_state(device):
    """A fresh state of the leveller for one row: device float64 (loudness.LEVELLER_STATE,); the first call (m0 = 0) fills it."""
    from . import loudness
    return torch.zeros((loudness.LEVELLER_STATE,), dtype=torch.float64, device=device)


def _level_span_impl(name, rows, xw, g0, n_total, rate, target, m0, m1, out, state, max_gain_db, gate, weights):
    """``level_span`` and ``level_span_rows`` (``name``) behind their checks of the window and the output: rows, xw, out, m0, m1
    as in ``_limit_span_impl``.  Only the entry point, which for a row takes no weights, depends on ``name``."""
    from . import loudness
    _need_cuda(state)
    assert state.dtype == torch.float64 and state.dim() == 1 and state.numel() >= loudness.LEVELLER_STATE and state.stride(0) == 1
    target, max_gain_db, gate = loudness.check_leveller(target, max_gain_db, gate, rate)
    wt = None if name == "level_span" else (C.c_double * rows[0])(*loudness.channel_weights(rows[0], weights))
    p = loudness.leveller_plan(rate)
    key = (str(xw.device), int(rate))
    mpow = _LEVELLER_MPOW.get(key)
    if mpow is None:
        mpow = torch.from_numpy(p["mpow"]).to(xw.device)
        _LEVELLER_MPOW[key] = mpow
    coef = (C.c_double * 10)(*[float(v) for v in p["coef"]])
    h = _lib.lib()
    nb = h.vfx_level_span_rows_workspace_bytes(max(m1 - m0, 0), p["hop"], rows[0])
    ws = torch.empty(((nb + 7) // 8,), dtype=torch.float64, device=xw.device)
    span = (int(g0), xw.shape[-1], INT64_MAX if n_total is None else int(n_total), m0, m1, int(rate), coef, _ptr(mpow), p["S"], target,
            max_gain_db, gate, _ptr(state), _ptr(out))
    tail = (_ptr(ws), nb, _stream())
    check(h.vfx_level_span_f32(_ptr(xw), *span, *tail) if name == "level_span" else
          h.vfx_level_span_rows_f32(_ptr(xw), rows[1], rows[0], wt, *span, rows[2], *tail), "vfx_%s_f32" % name)


def level_span(xw, g0, n_total, rate, target, m0, m1, out, state, max_gain_db=12.0, gate=-50.0):
    """Outputs [m0, m1) of the streaming loudness leveller over ONE row from a window of it (vfx_level_span_f32; loudness.py,
    DESIGN.md 3.17): xw (wlen,) device holds samples [g0, g0 + wlen) of a row of ``n_total`` samples at ``rate`` Hz (None: its
    end is not known yet, and m1 may not pass loudness.leveller_ready(g0 + wlen, hop)), out (>= m1 - m0,) receives output t at
    out[t - m0] -- the bits one call over the whole row writes for it.  Calls come in order (m0 = 0 first, then the m1 of the call
    before) on one ``state`` (``level_state``), which carries the last quarters' energies, the held gain and the record
    state[:4] = {min G, max G, anchors, gated}.  The window must cover [m0, m1) and the regions of the quarters that become
    measurable (loudness.leveller_counts), or VfxError.  At most three launches, no synchronisation."""
    m0, m1 = _check_span("level_span", xw, out, m0, m1)
    _level_span_impl("level_span", (1, xw.numel(), m1 - m0), xw, g0, n_total, rate, target, m0, m1, out, state, max_gain_db, gate, None)


def level_span_rows(xw, g0, n_total, rate, target, m0, m1, out, state, max_gain_db=12.0, gate=-50.0, weights=None):
    """Outputs [m0, m1) of the LINKED loudness leveller over a programme of C channels from a window of it
    (vfx_level_span_rows_f32): ``level_span`` with xw (C, wlen) and out (C, >= m1 - m0), rows of unit stride and
    any row stride, and ONE ``state``.  The quarter energies are summed over the channels with ``weights``
    (loudness.channel_weights(C, weights): BS.1770-4 Table 4 by default), so one ramp multiplies every channel.  C = 1 with the
    weight 1: the bits and the state of ``level_span``.  At most three launches, no synchronisation."""
    C_, m0, m1, ws_, os_ = _check_span_rows("level_span_rows", xw, out, m0, m1)
    _level_span_impl("level_span_rows", (C_, ws_, os_), xw, g0, n_total, rate, target, m0, m1, out, state, max_gain_db, gate, weights)


def meter_state(device):
    """A fresh state of the streaming loudness meter for one programme: device float64 (loudness.METER_STATE,) of zeros -- the
    state of a programme nothing of which has been metered; the first call (m0 = 0) fills it."""
    from . import loudness
    return torch.zeros((loudness.METER_STATE,), dtype=torch.float64, device=device)


def meter_span_rows(xw, g0, n_total, rate, m0, m1, state, qlog, weights=None, true_peak=True):
    """Folds the samples [m0, m1) of a programme of C channels into a streaming loudness meter (vfx_meter_span_rows_f32;
    loudness.py): xw (C, wlen) device -- or (wlen,), one channel -- holds samples [g0, g0 + wlen) of rows of
    ``n_total`` samples at ``rate`` Hz (None: the end is not known yet, and m1 may not pass loudness.meter_ready(g0 + wlen, Fw)).
    Calls come in order (m0 = 0 first, then the m1 of the call before) on one ``state`` (``meter_state``) and one ``qlog``, a
    device float64 tensor of at least m1 // hop values that the caller owns and grows (by doubling) BETWEEN calls: 8 bytes per
    100 ms of the programme.  Afterwards qlog[:m1 // hop] are the linked quarter energies (``weights``:
    loudness.channel_weights(C, weights)) and state[:5] = {sample peak, true peak, quarters logged, samples metered, flag}: the
    bits of one call over the whole row.  The window must cover [m0 - Bk, m1 - 1 + Fw] clipped to the row (loudness.meter_reach)
    and the regions of the quarters that become complete, or VfxError.  ``true_peak=False``: the sample-peak form (the entry
    point's R = 1: nothing is interpolated, the samples count for both peaks, Bk = Fw = 0) -- how a report in the middle of a
    session accounts for the samples whose interpolated values are not known yet.  At most three launches, no synchronisation."""
    from . import loudness
    _need_cuda(xw, state, qlog)
    assert xw.dtype == torch.float32 and xw.dim() in (1, 2) and (xw.shape[-1] <= 1 or xw.stride(-1) == 1)
    assert state.dtype == torch.float64 and state.dim() == 1 and state.numel() >= loudness.METER_STATE and state.stride(0) == 1
    assert qlog.dtype == torch.float64 and qlog.dim() == 1 and (qlog.numel() <= 1 or qlog.stride(0) == 1)
    loudness.check_meter(True, rate)
    Cn = loudness.check_channel_count(int(xw.shape[0])) if xw.dim() == 2 else 1
    wlen = int(xw.shape[-1])
    w_stride = int(xw.stride(0)) if Cn > 1 else wlen      # (one row: any stride that holds the row will do)
    wt = (C.c_double * Cn)(*loudness.channel_weights(Cn, weights))
    m0, m1 = int(m0), int(m1)
    p = loudness.leveller_plan(rate)
    key = (str(xw.device), int(rate))
    mpow = _LEVELLER_MPOW.get(key)
    if mpow is None:
        mpow = torch.from_numpy(p["mpow"]).to(xw.device)
        _LEVELLER_MPOW[key] = mpow
    coef = (C.c_double * 10)(*[float(v) for v in p["coef"]])
    R = loudness.oversampling(rate) if loudness.check_true_peak(true_peak) else 1
    bank, J, c = true_peak_bank(xw.device, R) if R > 1 else (None, 1, 0)
    h = _lib.lib()
    nb = h.vfx_meter_span_workspace_bytes(max(m1 - m0, 0), p["hop"], Cn)
    ws = torch.empty(((nb + 7) // 8,), dtype=torch.float64, device=xw.device)
    check(h.vfx_meter_span_rows_f32(_ptr(xw), w_stride, Cn, wt, int(g0), wlen, INT64_MAX if n_total is None else int(n_total), m0, m1,
                                    int(rate), coef, _ptr(mpow), p["S"], _ptr(bank), J, R, c, _ptr(state), _ptr(qlog),
                                    int(qlog.numel()), _ptr(ws), nb, _stream()), "vfx_meter_span_rows_f32")


def meter_report(state, qlog, rate):
    """The EBU R 128 figures of a streaming loudness meter (vfx_meter_report_f32): a device float64 (10,) of
    {integrated loudness, loudness range, maximum momentary, maximum short-term loudness, sample peak, true peak (both linear),
    momentary and short-term loudness of the last 4 / 30 quarters, quarters, flag} from ``state`` and ``qlog`` as
    ``meter_span_rows`` left them.  Writes neither: a report in the middle of a session changes nothing that follows.  One
    launch, no synchronisation (the caller's read of the result is the one)."""
    from . import loudness
    _need_cuda(state, qlog)
    assert state.dtype == torch.float64 and state.dim() == 1 and state.numel() >= loudness.METER_STATE and state.stride(0) == 1
    assert qlog.dtype == torch.float64 and qlog.dim() == 1 and (qlog.numel() <= 1 or qlog.stride(0) == 1)
    loudness.check_meter(True, rate)
    h = _lib.lib()
    nb = h.vfx_meter_report_workspace_bytes(int(qlog.numel()))
    ws = torch.empty(((nb + 7) // 8,), dtype=torch.float64, device=state.device)
    rep = torch.empty((10,), dtype=torch.float64, device=state.device)
    check(h.vfx_meter_report_f32(_ptr(state), _ptr(qlog), loudness.hop_length(rate), _ptr(rep), _ptr(ws), nb, _stream()),
          "vfx_meter_report_f32")
    return rep


def loudness_report_groups(x, n_rows, groups, fs, weights=None):
    """Loudness report of programmes of several channels (vfx_loudness_report_groups_f32; arguments as loudness_groups): a
    device float64 (G, 6) of {integrated loudness, loudness range, maximum momentary, maximum short-term loudness, sample
    peak, true peak} per programme.  Measures only; the launches of loudness_report_rows."""
    _need_cuda(x)
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
    n_rows, start, wt, G = _loudness_groups_plan(x, n_rows, groups, weights)
    _need_cuda(n_rows)
    assert n_rows.dtype == torch.int32 and n_rows.numel() == x.shape[0]
    p, mpow, coef, (bank, J, R, c) = _loudness_plan(x, fs)
    B, n_max = x.shape
    h = _lib.lib()
    nb = h.vfx_loudness_report_groups_workspace_bytes(B, n_max, p["hop"], p["S"], R, J)
    ws = torch.empty(((nb + 7) // 8,), dtype=torch.float64, device=x.device)
    rep = torch.empty((G, 6), dtype=torch.float64, device=x.device)
    check(h.vfx_loudness_report_groups_f32(_ptr(x), x.stride(0) if B > 1 else n_max, _ptr(n_rows), B, n_max, _ptr(start),
                                           _ptr(wt), G, coef, _ptr(mpow), p["S"], p["hop"], p["lookback"], _ptr(bank), J, R,
                                           c, _ptr(rep), _ptr(ws), nb, _stream()), "vfx_loudness_report_groups_f32")
    return rep
