"""The opt-in f16 arithmetic on the MI355X: vfx_conv1d_f16 against a CPU reference of the stated arithmetic (operands
rounded to fp16 with round-to-nearest-even, products summed in fp64), its range guard, and the engine's f16 arithmetic
(Pipeline / VocoderEngine.set_math("f16"); not offered by the public classes until it is faster) end to end."""
import contextlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import voicefixer_amd  # noqa: E402
from voicefixer_amd import _lib, engine, ops, packing  # noqa: E402
from voicefixer_amd._lib import PRE_NONE, PRE_LRELU, POST_NONE, POST_LRELU, POST_LRELU_SNAKE  # noqa: E402
from conftest import GOLDEN  # noqa: E402
from oracle import oracle  # noqa: E402  (checker only)

CONVH_TILE = 128 * 100000 + 128 * 100 + 32   # vfx_last_conv_tile() of convh_kernel (include/vfx_hip.h)
# the parity sweep below measured at most 5.7e-7 of the output peak on MI355X
PARITY_BOUND = 2e-6   # (values as printed: profiles/f16_kernel_parity.txt)
# End to end, f16 results cannot match any other evaluation to fp32 rounding: a perturbation of the operands at fp32-rounding
# level (2e-7 relative) flips fp16 roundings that then propagate through the vocoder's 32 residual layers, and moves the CPU
# emulation's OWN waveform by ~5e-5 RMS (profiles/f16_error.txt; the f16 - f32 difference itself is ~6e-5).  The end-to-end checks therefore hold the
# device to that noise floor (twice it) and to the size of the emulated f16 error, which the bf16 emulation exceeds 8x.
E2E_FLOOR = 1.2e-4


def _rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


def _f16(t):
    return t.to(torch.float16).to(torch.float64)


def _reference(x, w, bias, res, d, pre_slope, post, post_slope, rows=None):
    """CPU: y = post(bias + res + sum f16(w) * f16(pre(x))), zero padding at each row's own end, products in fp64."""
    x = x.double()
    if pre_slope is not None:
        x = F.leaky_relu(x, pre_slope)
    if rows is not None:
        x = x.clone()
        for b, n in enumerate(rows):
            x[b, :, n:] = 0
    y = F.conv1d(_f16(x), _f16(w), None, padding=d, dilation=d)
    if bias is not None:
        y = y + bias.double()[None, :, None]
    if res is not None:
        y = y + res.double()
    if post == POST_LRELU:
        y = F.leaky_relu(y, post_slope)
    elif post == POST_LRELU_SNAKE:
        y = F.leaky_relu(y, post_slope)
        y = y + torch.sin(y)
    return y


def _setup(C, L, B=1, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, L, generator=g) * scale
    w = torch.randn(C, C, 3, generator=g) / np.sqrt(3 * C)
    bias = 0.1 * torch.randn(C, generator=g)
    res = torch.randn(B, C, L, generator=g)
    return x, w, bias, res


def _dev_in(x, guard):
    """x (B, C, L) on the device: a guarded view (guard > 0, slack filled with garbage) or a plain contiguous tensor."""
    B, C, L = x.shape
    if guard == 0:
        return x.cuda().contiguous()
    v = ops.guarded(B, C, L, guard, "cuda")
    v._vfx_base.fill_(1e30)                 # whatever lies in the guard band must never be read
    v[:, :, :L] = x.cuda()
    return v


def _run(x, w, bias, res, d, act, guard=0, rows=None, flag=None):
    B, C, L = x.shape
    xd = _dev_in(x, guard)
    if rows is not None:
        ops.with_rows(xd, torch.tensor(rows, dtype=torch.int32, device="cuda"))
    y = res.cuda().contiguous() if res is not None else torch.zeros(B, C, L, device="cuda")
    w16 = packing.pack_f16(packing.pack_conv1d(w)).cuda()
    ok = ops.conv1d_f16(xd, w16, bias.cuda() if bias is not None else None, y, L, d, act,
                        res=y if res is not None else None, flag=flag)
    assert ok
    assert _lib.lib().vfx_last_conv_tile() == CONVH_TILE
    torch.cuda.synchronize()
    return y.cpu()


def _err(got, ref):
    return float((got.double() - ref).abs().max()) / float(ref.abs().max())


@pytest.mark.parametrize("C,d,L,B", [(128, 1, 301, 2), (256, 3, 257, 1), (512, 27, 300, 2), (128, 243, 777, 1),
                                     (256, 2187, 1001, 2), (512, 2187, 130, 1), (128, 81, 50, 3), (512, 9, 1, 1)])
def test_conv1d_f16_matches_rounded_operand_reference(C, d, L, B):
    x, w, bias, _ = _setup(C, L, B, seed=C + d + L)
    act = ops.Act(pre=PRE_LRELU, pre_slope=0.01, post=POST_NONE)
    got = _run(x, w, bias, None, d, act)
    ref = _reference(x, w, bias, None, d, 0.01, POST_NONE, 0.0)
    e = _err(got, ref)
    print("C=%d d=%d L=%d B=%d  max err / peak = %.3e" % (C, d, L, B, e))
    assert e < PARITY_BOUND


@pytest.mark.parametrize("C,d", [(128, 1), (512, 729)])
def test_conv1d_f16_residual_and_snake_in_place(C, d):
    L, B = 389, 2
    x, w, bias, res = _setup(C, L, B, seed=11 + d)
    act = ops.Act(pre=PRE_LRELU, pre_slope=0.01, post=POST_LRELU_SNAKE, post_slope=0.2)
    got = _run(x, w, bias, res, d, act)
    ref = _reference(x, w, bias, res, d, 0.01, POST_LRELU_SNAKE, 0.2)
    e = _err(got, ref)
    print("residual + snake C=%d d=%d  max err / peak = %.3e" % (C, d, e))
    assert e < PARITY_BOUND


def test_conv1d_f16_guard_band_is_never_read():
    x, w, bias, _ = _setup(256, 700, 2, seed=5)
    act = ops.Act(pre=PRE_LRELU, pre_slope=0.01, post=POST_LRELU, post_slope=0.2)
    for d in (1, 27, 2187):
        a = _run(x, w, bias, None, d, act, guard=0)
        b = _run(x, w, bias, None, d, act, guard=engine.G_DIL)
        assert torch.equal(a, b), d


def test_conv1d_f16_ragged_rows_equal_separate_launches():
    C, L = 128, 600
    rows = [600, 333, 129]
    x, w, bias, res = _setup(C, L, len(rows), seed=9)
    act = ops.Act(pre=PRE_LRELU, pre_slope=0.01, post=POST_LRELU_SNAKE, post_slope=0.2)
    for d in (3, 243):
        got = _run(x, w, bias, res, d, act, rows=rows)
        for b, n in enumerate(rows):
            one = _run(x[b:b + 1, :, :n].contiguous(), w, bias, res[b:b + 1, :, :n].contiguous(), d, act)
            assert torch.equal(got[b:b + 1, :, :n], one), (d, b)


def test_conv1d_f16_rounds_to_nearest_even():
    """Operands exactly halfway between two fp16 values: round-to-nearest-even and round-toward-zero differ."""
    C, L = 128, 64
    x = torch.zeros(1, C, L)
    w = torch.zeros(C, C, 3)
    w[0, 5, 1] = 1.0            # y[0, l] = x[5, l] through the centre tap
    up = 1 + 3 * 2.0 ** -11     # halfway between 1 + 2^-10 and 1 + 2^-9: RNE -> 1 + 2^-9, RTZ -> 1 + 2^-10
    x[0, 5, 10] = up
    x[0, 5, 11] = -up
    x[0, 5, 12] = 1 + 2.0 ** -11   # halfway between 1 and 1 + 2^-10: RNE -> 1 (even)
    got = _run(x, w, None, None, 1, ops.Act())
    assert float(got[0, 0, 10]) == 1 + 2.0 ** -9
    assert float(got[0, 0, 11]) == -(1 + 2.0 ** -9)
    assert float(got[0, 0, 12]) == 1.0


def test_conv1d_f16_range_flag():
    x, w, bias, _ = _setup(128, 300, 1, seed=2)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    act = ops.Act(pre=PRE_LRELU, pre_slope=0.01)
    _run(x, w, bias, None, 9, act, flag=flag)
    assert int(flag.item()) == 0
    x[0, 17, 123] = 7e4
    _run(x, w, bias, None, 9, act, flag=flag)
    assert int(flag.item()) != 0


def test_conv1d_f16_declines_other_shapes():
    x = torch.zeros(1, 64, 100, device="cuda")
    w16 = torch.zeros(3, 8, 64, 8, dtype=torch.float16, device="cuda")
    assert ops.conv1d_f16(x, w16, None, x.clone(), 100, 1) is False


# ---- public API -------------------------------------------------------------------------------------------------------
F16_LAYERS = 5 + 16 * 3   # condnet's five k = 3 convolutions come first, then 16 per ResStack stage; the first three stages run f16


@contextlib.contextmanager
def _emulated_f16():
    """The oracle's vocoder with the operands of the 48 wide ResStack convolutions rounded to fp16 (RNE), computed in fp32."""
    real = F.conv1d
    count = [0]

    def conv1d(x, w, *args, **kw):
        if w.dim() == 3 and w.shape[-1] == 3:
            k = count[0] % (5 + 16 * 4)
            count[0] += 1
            if 5 <= k < F16_LAYERS:
                return real(x.half().float(), w.half().float(), *args, **kw)
        return real(x, w, *args, **kw)

    F.conv1d = conv1d
    try:
        yield
    finally:
        F.conv1d = real


@pytest.fixture(scope="module")
def vf(seeded_states):
    return voicefixer_amd.VoiceFixer.from_state(*seeded_states)


def test_restore_inmem_f16(vf, seeded_states):
    g = np.load(os.path.join(GOLDEN, "restore_speech_T51.npz"))
    ref32 = vf.restore_inmem(g["wav"], cuda=True)
    vf._get_pipe().set_math("f16")
    try:
        out = vf.restore_inmem(g["wav"], cuda=True)
    finally:
        vf._get_pipe().set_math("f32")
    with torch.no_grad(), _emulated_f16():
        emu = oracle.restore_inmem(g["wav"], *seeded_states)
    print("restore_inmem f16: rms vs golden %.3e, vs emulation %.3e" % (_rms(out, g["restored"]), _rms(out, emu)))
    assert _rms(out, g["restored"]) < 1e-3
    assert not np.array_equal(out, ref32)
    assert _rms(out, emu) < E2E_FLOOR
    assert 0.5 < _rms(out, g["restored"]) / _rms(emu, g["restored"]) < 2.0


def test_vocoder_forward_f16(seeded_states):
    gv = np.load(os.path.join(GOLDEN, "vocoder_T101.npz"))
    voc = voicefixer_amd.Vocoder.from_state(seeded_states[0])
    ref32 = voc.forward(torch.from_numpy(gv["mel"])).numpy()
    voc._get_engine().set_math("f16")
    out = voc.forward(torch.from_numpy(gv["mel"])).numpy()
    with torch.no_grad(), _emulated_f16():
        emu = oracle.vocoder_forward(torch.from_numpy(gv["mel"]), seeded_states[0]).numpy()
    print("Vocoder.forward f16: rms vs golden %.3e, vs emulation %.3e" % (_rms(out, gv["wav"]), _rms(out, emu)))
    assert _rms(out, gv["wav"]) < 1e-3
    assert not np.array_equal(out, ref32)
    assert _rms(out, emu) < E2E_FLOOR
    assert 0.5 < _rms(out, gv["wav"]) / _rms(emu, gv["wav"]) < 2.0


def test_restore_batch_f16_rows_match_single_files(vf):
    """Every row of a 32-row ragged f16 batch against its single-file f16 result: within the f16 noise floor (E2E_FLOOR: the
    two runs differ upstream at fp32 rounding, by tile shapes); the f16 kernel itself gives ragged rows bit-identical to
    separate launches (test_conv1d_f16_ragged_rows_equal_separate_launches)."""
    g = torch.Generator().manual_seed(21)
    lens = [int(v) for v in torch.randint(12000, 40000, (32,), generator=g)]
    wavs = [(0.1 * torch.randn(n, generator=g)).numpy() for n in lens]
    vf._get_pipe().set_math("f16")
    try:
        outs = vf.restore_batch(wavs, batch_size=32)
        for w, o in zip(wavs, outs):
            assert o.shape == (1, len(w))
            assert _rms(o, vf.restore_inmem(w, cuda=True)) < E2E_FLOOR
    finally:
        vf._get_pipe().set_math("f32")


def test_switching_back_to_f32_is_bit_identical(seeded_states):
    g = np.load(os.path.join(GOLDEN, "restore_speech_T51.npz"))
    a = voicefixer_amd.VoiceFixer.from_state(*seeded_states).restore_inmem(g["wav"], cuda=True)
    vf = voicefixer_amd.VoiceFixer.from_state(*seeded_states)
    vf._get_pipe().set_math("f16")
    vf.restore_inmem(g["wav"], cuda=True)
    vf._get_pipe().set_math("f32")
    b = vf.restore_inmem(g["wav"], cuda=True)
    assert np.array_equal(a, b)


def _hot_vocoder_state(state):
    """The first ResStack layer's gain scaled so that its output leaves the fp16 range."""
    sd = dict(state)
    key = [k for k in sd if k.startswith("generator.4.layers.0.1.") and ("original0" in k or k.endswith("weight_g"))][0]
    sd[key] = sd[key] * 1e6
    return sd


def test_range_overflow_falls_back_to_f32(seeded_states):
    gv = np.load(os.path.join(GOLDEN, "vocoder_T101.npz"))
    vsd = _hot_vocoder_state(seeded_states[0])
    mel = torch.from_numpy(gv["mel"])
    want = voicefixer_amd.Vocoder.from_state(vsd).forward(mel).numpy()
    voc = voicefixer_amd.Vocoder.from_state(vsd)
    voc._get_engine().set_math("f16")
    got = voc.forward(mel).numpy()
    assert voc._get_engine().f16_fallbacks == 1
    np.testing.assert_array_equal(got, want)

    g = np.load(os.path.join(GOLDEN, "restore_speech_T51.npz"))
    want = voicefixer_amd.VoiceFixer.from_state(vsd, seeded_states[1]).restore_inmem(g["wav"], cuda=True)
    vf = voicefixer_amd.VoiceFixer.from_state(vsd, seeded_states[1])
    vf._get_pipe().set_math("f16")
    got = vf.restore_inmem(g["wav"], cuda=True)
    assert vf._get_pipe().f16_fallbacks == 1
    np.testing.assert_array_equal(got, want)


def test_pipeline_set_math_drops_captured_graphs(seeded_states):
    """A captured graph has the arithmetic baked in: after a change of arithmetic the replay path recaptures, and switching
    back to f32 gives what an f32 pipeline that never switched gives."""
    g = np.load(os.path.join(GOLDEN, "restore_speech_T51.npz"))
    wav = torch.from_numpy(g["wav"])[None].cuda()
    n = wav.shape[1]
    want = voicefixer_amd.VoiceFixer.from_state(*seeded_states)._get_pipe().restore(wav, n).cpu()
    pipe = voicefixer_amd.VoiceFixer.from_state(*seeded_states)._get_pipe()
    pipe.enable_graphs(max_shapes=2, max_batch=1)
    a = pipe.restore(wav, n).cpu()
    pipe.set_math("f16")
    f = pipe.restore(wav, n).cpu()
    pipe.set_math("f32")
    b = pipe.restore(wav, n).cpu()
    assert torch.equal(a, want) and torch.equal(b, want)
    assert not torch.equal(f, want)


def test_vocoder_oracle_f16_reads_the_range_flag(seeded_states, tmp_path):
    from voicefixer_amd import audio_io
    voc = voicefixer_amd.Vocoder.from_state(_hot_vocoder_state(seeded_states[0]))
    fin = str(tmp_path / "in.wav")
    g = torch.Generator().manual_seed(9)
    audio_io.save_wave((0.1 * torch.randn(1, 20000, generator=g)).numpy(), fin)
    voc.oracle(fin, str(tmp_path / "want.wav"))
    voc._get_engine().set_math("f16")
    voc.oracle(fin, str(tmp_path / "got.wav"))
    assert voc._get_engine().f16_fallbacks == 1
    np.testing.assert_array_equal(audio_io.load_wav(str(tmp_path / "got.wav")), audio_io.load_wav(str(tmp_path / "want.wav")))
    assert int(voc._get_engine().f16_flag.item()) == 0      # nothing left over for the next call
