"""The look-ahead peak limiter on the MI355X (vfx_loudness_limit_f32; ops.loudness_limit) against the float64 reference of
tests/test_limiter_cpu.py: every row length, peak position and peak distance at which a tile seam, the clamped extension or a
merged dip can go wrong, every oversampling factor, the sample-peak form, programmes, reproducibility, launch counts, bad
arguments, and the public surface.

Per sample |out - ref| <= Cl (TP_BOUND max(1, gL / Cl) + (2 H + 9) 2^-24): the oversampling sum is held to TP_BOUND = 2e-6
max(1, ref) (tests/test_true_peak_gpu.py); an output sample at a bound position is Cl x / e with e >= Cl / gL, so the envelope
contributes at most Cl TP_BOUND max(1, gL / Cl); the fp32 smoothing sum of terms <= 1 adds at most (2 H + 1) 2^-24, the other
fp32 roundings (threshold, quotient, weights, gain products, trim) less than 8 2^-24.  The same bound, relative, holds for
t and min g.  Observed on the MI355X: see DESIGN.md 3.14."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import voicefixer_amd  # noqa: E402
from voicefixer_amd import _lib, loudness, ops  # noqa: E402
from test_loudness_cpu import ref_loudness  # noqa: E402
from test_true_peak_cpu import ref_true_peak  # noqa: E402
from test_limiter_cpu import ref_limit  # noqa: E402

TP_BOUND = 2e-6
PAD = 40


def _quarter_sine(n, amp, fade=False):
    x = amp * np.sin(2 * np.pi * np.arange(n) / 4 + math.pi / 4)
    if fade:
        k = n // 8
        ramp = 0.5 - 0.5 * np.cos(np.pi * np.arange(k) / k)
        x[:k] *= ramp
        x[n - k:] *= ramp[::-1]
    return x.astype(np.float32)


def _bound(H, gL, Cl):
    return Cl * (TP_BOUND * max(1.0, gL / Cl) + (2 * H + 9) * 2.0 ** -24)


def _stage(rows):
    lens = [len(r) for r in rows]
    x = np.full((len(rows), max(lens) + PAD), np.nan, np.float32)      # NaN canaries past every row end
    for r, v in enumerate(rows):
        x[r, :lens[r]] = v
    return x, lens


def _limit_c_abi(x, n_rows, fs, target, ceiling_db, ms, out):
    """ops.loudness_limit(true_peak=True) without its range check of the target: the C entry point takes any finite one (a
    sine at fs / 4 of amplitude 0.9 is louder than -6 LUFS, so doubling it needs a target above 0)."""
    import ctypes as C
    p = loudness.plan(fs)
    R = loudness.oversampling(fs)
    bank, J, c = ops.true_peak_bank("cuda", R)
    B, W = x.shape
    lib = _lib.lib()
    nb = lib.vfx_loudness_limit_workspace_bytes(B, W, p["hop"], p["S"], R, J)
    ws = torch.empty((nb // 8 + 1,), dtype=torch.float64, device="cuda")
    mp = torch.from_numpy(p["mpow"]).cuda()
    res = torch.empty((B, 8), dtype=torch.float64, device="cuda")
    P = ops._ptr
    assert lib.vfx_loudness_limit_f32(P(x), W, P(n_rows), B, W, None, None, 0, (C.c_double * 10)(*p["coef"]), P(mp), p["S"], p["hop"],
                                      p["lookback"], target, ceiling_db, P(bank), J, R, c, P(out), W,
                                      loudness.limiter_window(fs, ms)[0], 1, P(res), P(ws), nb, None) == 0
    torch.cuda.synchronize()
    return res


def _run(rows, fs, target, ceiling_db=-1.0, true_peak=True, ms=3.0, groups=None, in_place=False):
    """One ragged call: (out, record) as numpy; checks the canaries, the untouched input and the launch count."""
    x, lens = _stage(rows)
    xd = torch.from_numpy(x).cuda()
    out = xd.clone() if in_place else torch.full(x.shape, float("nan"), device="cuda")
    src = out if in_place else xd
    n_rows = lens if groups is not None else torch.tensor(lens, dtype=torch.int32, device="cuda")
    lib = _lib.lib()
    c0 = lib.vfx_launch_count()
    if target >= 0.0:
        res = _limit_c_abi(src, n_rows, fs, target, ceiling_db, ms, out)
    else:
        res = ops.loudness_limit(src, n_rows, fs, target, ceiling_db, true_peak, ms, out=out, groups=groups)
    launches = lib.vfx_launch_count() - c0
    R = loudness.oversampling(fs) if true_peak else 1
    assert launches == (10 if R > 1 else 8), launches      # whatever B and the lengths
    got, rec = out.cpu().numpy(), res.cpu().numpy()
    assert np.array_equal(xd.cpu().numpy(), x, equal_nan=True)
    for r, n in enumerate(lens):
        assert np.all(np.isnan(got[r, n:])), r
        assert not np.any(np.isnan(got[r, :n])), r
    return x, lens, got, rec


def _check_rows(what, x, lens, got, rec, fs, ceiling_db=-1.0, true_peak=True, ms=3.0, expect_bound=None):
    """Every row against ref_limit with the recorded gL; returns the worst error / bound."""
    Cl = 10.0 ** (ceiling_db / 20.0)
    worst, worst_abs = 0.0, 0.0
    for r, n in enumerate(lens):
        L, gL, P, TP, bound, gmin, t, after = rec[r]
        xr = x[r, :n]
        ref = ref_limit(xr, fs, gL, ceiling_db, ms, true_peak)
        ratio = gL * ref["TP"] / Cl
        assert not 1 - 1e-3 <= ratio <= 1 + 1e-3, (what, r, ratio)      # the test's own rows stay clear of the border
        assert bool(bound) == ref["bound"], (what, r, ratio)
        if expect_bound is not None:
            assert bool(bound) == expect_bound[r], (what, r)
        assert abs(TP - ref["TP"]) <= TP_BOUND * max(1.0, ref["TP"]), (what, r)
        if not ref["bound"]:
            assert gmin == 1.0 and t == 1.0, (what, r)
            assert np.array_equal(got[r, :n], np.float32(gL) * xr), (what, r)
            continue
        H = ref["H"]
        tol = _bound(H, gL, Cl)
        assert ref["t"] > 0.9999, (what, r, ref["t"])                   # the reference's own trim: next to nothing
        err = float(np.abs(got[r, :n].astype(np.float64) - ref["out"]).max()) if n else 0.0
        worst = max(worst, err / tol)
        worst_abs = max(worst_abs, err)
        assert err <= tol, (what, r, n, err, tol, int(np.abs(got[r, :n] - ref["out"]).argmax()))
        assert abs(t - ref["t"]) <= tol / Cl and abs(gmin - ref["g"].min()) <= tol / Cl, (what, r, t, ref["t"], gmin, ref["g"].min())
        assert t >= 0.99 and t <= 1.0, (what, r, t)
        tp_out = ref_true_peak(got[r, :n], fs) if true_peak else float(np.abs(got[r, :n]).max())
        assert tp_out <= Cl * (1.0 + TP_BOUND), (what, r, tp_out / Cl)
        assert abs(after - tp_out) <= TP_BOUND * max(1.0, tp_out) + 2.0 ** -23, (what, r, after, tp_out)
    print("limiter %s: worst |out - ref| = %.2e, worst |out - ref| / bound = %.3f over %d rows" % (what, worst_abs, worst, len(lens)))
    return worst


def _noise(rng, n, amp=0.1):
    return (amp * rng.uniform(-1, 1, n)).astype(np.float32)


def test_row_lengths_peak_positions_and_peak_distances():
    """fs = 44100: R = 4, H = 132, true-peak tiles and output tiles of 1024 samples (the former start 2 samples early).  All rows are
    under 400 ms, so L = -inf and gL = 1: they are limited because their peaks pass the ceiling."""
    fs, H, T = 44100, 132, 1024
    rng = np.random.default_rng(5)
    rows = []
    for n in (1, 2, H, H + 1, 2 * H + 1, 2 * H + 2, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1):
        v = _noise(rng, n)
        v[n // 2] = 0.97
        rows.append(v)
    N = 3000
    singles = [0, N - 1] + list(range(1019, 1029)) + [2 * T - 1, 2 * T, T - H, T - H - 1, T - 2 - H, T - 2 - H - 1,
                                                       T - 2 * H, T - 2 * H - 1]
    for pos in singles:
        v = _noise(rng, N)
        v[pos] = -0.97 if pos % 2 else 0.97
        rows.append(v)
    for sep in (H, 2 * H, 2 * H + 1, 4 * H + 1, 4 * H + 3):       # merged, touching and separate dips
        v = _noise(rng, N)
        v[900] = 0.97
        v[900 + sep] = -0.99
        rows.append(v)
    x, lens, got, rec = _run(rows, fs, -16.0)
    assert np.all(np.isinf(rec[:, 0])) and np.all(rec[:, 1] == 1.0)
    _check_rows("lengths / positions / distances", x, lens, got, rec, fs, expect_bound=[True] * len(rows))
    # in place: the same bits
    _, _, got2, rec2 = _run(rows, fs, -16.0, in_place=True)
    assert np.array_equal(got2, got, equal_nan=True) and np.array_equal(rec2, rec)


def _short_peaks(rng, n):
    v = _noise(rng, n)
    v[n // 4] = 0.97
    v[n // 2] = -0.99
    v[n // 2 + 7] = 0.95
    return v


def _mixed_rows(fs, rng, k):
    """Rows of one loudness (so one target makes gL ~ k for all of them) and rows without one."""
    n = int(0.62 * fs) + 3
    base = rng.standard_normal(n)
    base *= 10.0 ** ((-34.0 - ref_loudness(base, fs)) / 20.0)
    click = base.copy()
    click[n // 3] = 0.6
    click[n // 3 + 2000] = -0.5
    click[n - 1] = 0.45
    first = base.copy()
    first[0] = -0.55
    rows = [click.astype(np.float32),
            np.zeros(int(0.5 * fs), np.float32),                       # silence: L = -inf, gL = 1, not bound
            base.astype(np.float32),                                   # no transient: not bound at k <= 4
            _short_peaks(rng, int(0.2 * fs)),                          # under 400 ms, peaks above the ceiling: bound at gL = 1
            _noise(rng, int(0.3 * fs), 0.3),                           # under 400 ms, not bound
            first.astype(np.float32)]
    T = ref_loudness(click.astype(np.float32), fs) + 20.0 * math.log10(k)
    return rows, T, [True, False, False, True, False, True]


@pytest.mark.parametrize("fs,k", [(8000, 4), (44100, 2), (48000, 4), (96000, 2), (192000, 4)])
def test_rates(fs, k):
    rng = np.random.default_rng(fs)
    rows, T, want = _mixed_rows(fs, rng, k)
    x, lens, got, rec = _run(rows, fs, T)
    assert abs(rec[0, 1] - k) <= 2e-3 * k       # gL is the k the target was chosen for (row 5: near it -- other clicks)
    assert np.isinf(rec[1, 0]) and rec[1, 1] == 1.0 and np.isinf(rec[3, 0]) and rec[3, 1] == 1.0
    worst = _check_rows("%d Hz (R = %d, H = %d)" % (fs, loudness.oversampling(fs), loudness.limiter_window(fs)[0]), x, lens, got,
                        rec, fs, expect_bound=want)
    assert worst > 0.0
    # a row that is not bound: the bits of the static path, and its record
    lib = _lib.lib()
    xd = torch.from_numpy(x).cuda()
    n_rows = torch.tensor(lens, dtype=torch.int32, device="cuda")
    out = torch.full(x.shape, float("nan"), device="cuda")
    c0 = lib.vfx_launch_count()
    static = ops.loudness_rows(xd, n_rows, fs, T, -1.0, out=out, true_peak=True).cpu().numpy()
    assert lib.vfx_launch_count() - c0 == 4 + (1 if loudness.oversampling(fs) > 1 else 0)       # the existing path: as it was
    so = out.cpu().numpy()
    for r in (1, 2, 4):
        assert np.array_equal(got[r, :lens[r]], so[r, :lens[r]]), (fs, r)
        assert np.array_equal(rec[r, :4], static[r]) and list(rec[r, 4:7]) == [0.0, 1.0, 1.0], (fs, r)
    assert np.array_equal(rec[:, [0, 2, 3]], static[:, [0, 2, 3]])      # L, P, TP: the measurement's bits for every row
    # three rows alone: the bits they have inside the batch
    for r in (0, 3, 5):
        _, _, g1, r1 = _run([rows[r]], fs, T)
        assert np.array_equal(g1[0, :lens[r]], got[r, :lens[r]]) and np.array_equal(r1[0], rec[r]), (fs, r)


def test_sample_peak_limiter():
    fs = 44100
    rng = np.random.default_rng(77)
    rows, T, want = _mixed_rows(fs, rng, 4)
    x, lens, got, rec = _run(rows, fs, T, true_peak=False)
    assert np.array_equal(rec[:, 2], rec[:, 3])                          # TP is the sample peak
    _check_rows("44100 Hz, sample peak", x, lens, got, rec, fs, true_peak=False, expect_bound=want)
    for r in range(len(rows)):
        assert np.abs(got[r, :lens[r]]).max() <= 10 ** (-1 / 20) * (1 + 2.0 ** -22)
    # another look-ahead and ceiling
    x, lens, got, rec = _run(rows, fs, T, ceiling_db=-3.0, ms=1.0)
    _check_rows("44100 Hz, 1 ms, -3 dBTP", x, lens, got, rec, fs, ceiling_db=-3.0, ms=1.0)


def test_plateau():
    """fs / 4 at 45 degrees, faded, amplitude 0.9, gL = 2: every interior position is bound and g is constant there."""
    fs = 44100
    x0 = _quarter_sine(int(0.6 * fs), 0.9, fade=True)
    T = ref_loudness(x0, fs) + 20.0 * math.log10(2.0)
    x, lens, got, rec = _run([x0], fs, T)
    assert abs(rec[0, 1] - 2.0) <= 4e-3
    _check_rows("plateau", x, lens, got, rec, fs, expect_bound=[True])
    gL, Cl = rec[0, 1], 10 ** (-1 / 20)
    ref = ref_limit(x0, fs, gL)
    n = x0.size
    mid = slice(n // 4, 3 * n // 4)
    assert np.all(ref["c"][mid] < 1.0) and np.ptp(ref["g"][mid]) < 1e-4
    g_dev = got[0, mid].astype(np.float64) / (gL * rec[0, 6] * x0[mid].astype(np.float64))
    want = Cl / (gL * 0.9)
    assert np.abs(g_dev - want).max() <= 1e-3 * want and abs(rec[0, 5] - ref["g"].min()) <= _bound(132, gL, Cl) / Cl


def test_programme_of_two_channels():
    fs = 44100
    rng = np.random.default_rng(9)
    n = int(0.7 * fs)
    a = rng.standard_normal(n)
    a *= 10.0 ** ((-30.0 - ref_loudness(a, fs)) / 20.0)
    b = 0.7 * rng.standard_normal(n) * np.std(a)
    a[n // 2] = 0.7                                                      # the peak is in channel 0 only
    a[5] = -0.6
    prog = np.stack([a, b]).astype(np.float32)
    mono = prog[0, :n - 777].copy()
    Cl = 10 ** (-1 / 20)
    for rows, groups in (([prog[0], prog[1]], [2]), ([mono, prog[0], prog[1]], [1, 2])):
        # the programme's loudness is the sum over both channels: take the target from its own measurement
        x, lens = _stage(rows)
        L = ops.loudness_groups(torch.from_numpy(x).cuda(), lens, groups, fs).cpu().numpy()[-1, 0]
        x, lens, got, rec = _run(rows, fs, L + 20.0 * math.log10(2.0), groups=groups)
        assert rec.shape == (len(groups), 8) and abs(rec[-1, 1] - 2.0) <= 1e-9 and rec[-1, 4] == 1.0
        gL, t = rec[-1, 1], rec[-1, 6]
        ref = ref_limit(prog, fs, gL)
        tol = _bound(132, gL, Cl)
        assert ref["bound"] and ref["t"] > 0.9999 and abs(t - ref["t"]) <= tol / Cl
        o = got[-2:, :n].astype(np.float64)
        assert np.abs(o - ref["out"]).max() <= tol
        keep = np.abs(prog[1]) > 1e-3                                    # both channels get the same gain curve
        assert np.abs(o[1, keep] / prog[1, keep] - gL * ref["g"][keep] * ref["t"]).max() <= tol / 1e-3
        assert max(ref_true_peak(got[-2, :n], fs), ref_true_peak(got[-1, :n], fs)) <= Cl * (1 + TP_BOUND)
        if len(groups) == 2:                                             # the mono row beside it: its own programme
            _check_rows("mono beside a programme", x[:1], lens[:1], got[:1], rec[:1], fs)


def test_launch_count_does_not_depend_on_the_batch():
    fs = 44100
    rng = np.random.default_rng(3)
    one = _noise(rng, 5000, 0.99)
    _run([one], fs, -16.0)                                               # (B = 1: _run asserts the count)
    _run([_noise(rng, 3000 + 511 * i, 0.99) for i in range(7)], fs, -16.0)
    _run([one], 192000, -16.0)
    _run([one], fs, -16.0, true_peak=False)


def test_bad_arguments_launch_nothing():
    import ctypes as C
    fs = 44100
    rng = np.random.default_rng(4)
    x, lens = _stage([_noise(rng, 4000, 0.99), _noise(rng, 4000, 0.99)])
    B, W = x.shape
    xd = torch.from_numpy(np.nan_to_num(x)).cuda()
    n_rows = torch.tensor(lens, dtype=torch.int32, device="cuda")
    p = loudness.plan(fs)
    coef = (C.c_double * 10)(*p["coef"])
    bank, J, c = ops.true_peak_bank("cuda", 4)
    lib = _lib.lib()
    nb = lib.vfx_loudness_limit_workspace_bytes(B, W, p["hop"], p["S"], 4, J)
    ws = torch.empty((nb // 8 + 1,), dtype=torch.float64, device="cuda")
    mp = torch.from_numpy(p["mpow"]).cuda()
    out = torch.zeros((B, W), device="cuda")
    rec = torch.zeros((B, 8), dtype=torch.float64, device="cuda")
    start = torch.tensor([0, 2], dtype=torch.int32, device="cuda")
    wt = torch.ones(2, dtype=torch.float64, device="cuda")
    P = ops._ptr
    args = [P(xd), W, P(n_rows), B, W, None, None, 0, coef, P(mp), p["S"], p["hop"], p["lookback"], -16.0, -1.0, P(bank), J, 4, c,
            P(out), W, 132, 1, P(rec), P(ws), nb, None]
    before = lib.vfx_launch_count()
    for i, bad in ((21, 0), (21, 4097), (22, 2), (13, float("nan")), (25, nb - 1), (19, None), (23, None), (15, None), (16, 0),
                   (17, 3), (18, 4 * J), (7, 1), (5, P(start)), (6, P(wt)), (7, 3), (14, float("inf")), (1, W - 1), (20, W - 1),
                   (19, C.c_void_p(xd.data_ptr() + 64))):
        a = list(args)
        a[i] = bad
        assert lib.vfx_loudness_limit_f32(*a) == _lib.EINVAL, (i, bad)
    assert lib.vfx_launch_count() == before
    assert lib.vfx_loudness_limit_f32(*args) == 0                        # ... and the same arguments, unbroken, run
    a = list(args)
    a[5], a[6], a[7] = P(start), P(wt), 1                                # ... as one programme, too
    assert lib.vfx_loudness_limit_f32(*a) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ops.loudness_limit(xd, n_rows, fs, None)
    with pytest.raises(ValueError):
        ops.loudness_limit(xd, n_rows, 768000, -16.0, lookahead_ms=10.0)
    assert lib.vfx_launch_count() == before + 20


# ---- the public surface ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def vf(seeded_states):
    return voicefixer_amd.VoiceFixer.from_state(*seeded_states)


def _utterance(seed, n, click=True):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 44100.0
    x = 0.03 * rng.standard_normal(n) * (1 + np.sin(2 * np.pi * 1.5 * t)) + 0.1 * np.sin(2 * np.pi * 180 * t)
    if click:
        x[n // 2] = 0.9
    return x.astype(np.float32)


def _limit_alone(plain, target, **kw):
    """ops.loudness_limit on restored rows (C, N): what the public call must return bit for bit."""
    x = torch.from_numpy(np.ascontiguousarray(plain)).cuda()
    C, n = plain.shape
    if C == 1:
        res = ops.loudness_limit(x, torch.tensor([n], dtype=torch.int32, device="cuda"), 44100, target, -1.0, True, 3.0, **kw)
    else:
        res = ops.loudness_limit(x, [n] * C, 44100, target, -1.0, True, 3.0, groups=[C], **kw)
    return x.cpu().numpy(), res.cpu().numpy()


def test_restore_inmem_and_batch_with_the_limiter(vf):
    lib = _lib.lib()
    x = _utterance(1, 50000)
    plain = vf.restore_inmem(x, cuda=True)
    L = voicefixer_amd.measure_loudness(plain[0])
    T = min(-1.0, L + 16.0)                                              # high enough for the ceiling to bind
    c0 = lib.vfx_launch_count()
    static = vf.restore_inmem(x, cuda=True, loudness=T, true_peak=True)
    c1 = lib.vfx_launch_count()
    same = vf.restore_inmem(x, cuda=True, loudness=T, true_peak=True, limiter=False)
    c2 = lib.vfx_launch_count()
    got = vf.restore_inmem(x, cuda=True, loudness=T, true_peak=True, limiter=True)
    c3 = lib.vfx_launch_count()
    assert c2 - c1 == c1 - c0 and np.array_equal(same, static)           # limiter=False: today's path, launch for launch
    assert (c3 - c2) - (c1 - c0) == 5                                    # 10 launches in place of 5
    want, rec = _limit_alone(plain, T)
    assert rec[0, 4] == 1.0 and rec[0, 5] < 1.0
    assert got.shape == plain.shape and np.array_equal(got, want)
    Cl = 10 ** (-1 / 20)
    assert ref_true_peak(got[0], 44100) <= Cl * (1 + TP_BOUND)
    Ls, Ll = voicefixer_amd.measure_loudness(static[0]), voicefixer_amd.measure_loudness(got[0])
    print("restore_inmem: target %.2f LUFS, static ceiling %.2f LUFS, limiter %.2f LUFS (min g %.4f, t %.7f)"
          % (T, Ls, Ll, rec[0, 5], rec[0, 6]))
    assert Ll > Ls
    # the sample-peak limiter
    sp = vf.restore_inmem(x, cuda=True, loudness=T, limiter=True, limiter_lookahead_ms=1.5)
    assert np.abs(sp).max() <= Cl * (1 + 2.0 ** -22) and not np.array_equal(sp, got)
    # three ragged inputs: each is what its own call returns
    wavs = [x, _utterance(2, 36000), _utterance(3, 61000, click=False)]
    outs = vf.restore_batch(wavs, batch_size=8, loudness=T, true_peak=True, limiter=True)
    plains = vf.restore_batch(wavs, batch_size=8)
    for p, o in zip(plains, outs):
        assert np.array_equal(o, _limit_alone(p, T)[0])
    # two channels: one gain curve, the ratio between the channels is kept
    x2 = np.stack([x, 0.5 * _utterance(4, 50000, click=False)])
    plain2 = vf.restore_inmem(x2, cuda=True, channels="all")
    got2 = vf.restore_inmem(x2, cuda=True, channels="all", loudness=T, true_peak=True, limiter=True)
    want2, rec2 = _limit_alone(plain2, T)
    assert rec2.shape == (1, 8) and np.array_equal(got2, want2)
    keep = (np.abs(plain2[0]) > 1e-3) & (np.abs(plain2[1]) > 1e-3)
    r0, r1 = got2[0, keep] / plain2[0, keep], got2[1, keep] / plain2[1, keep]
    assert np.abs(r0 / r1 - 1.0).max() <= 5 * 2.0 ** -24            # one float32 factor per sample for both: four roundings apart
    with pytest.raises(NotImplementedError):
        vf.restore_stream(x, loudness=T, limiter=True)


def test_folder_job_and_cli(vf, seeded_states, tmp_path, monkeypatch):
    from scipy.io import wavfile
    ind = str(tmp_path / "in")
    os.makedirs(ind)
    for k in range(3):
        v = _utterance(10 + k, 40000 + 5000 * k, click=k == 0)
        wavfile.write(os.path.join(ind, "f%d.wav" % k), 44100, np.round(v * 32767).astype(np.int16))
    T = -8.0
    st, st0 = {}, {}
    names = vf.restore_folder(ind, str(tmp_path / "lim"), batch_size=8, io_threads=2, stats=st, loudness=T, true_peak=True,
                              limiter=True)
    vf.restore_folder(ind, str(tmp_path / "static"), batch_size=8, io_threads=2, stats=st0, loudness=T, true_peak=True)
    assert len(names) == 3 and st["failed"] == [] and "limiter" not in st0
    assert [e[0] for e in st["limiter"]] == names == [e[0] for e in st["loudness"]] == [e[0] for e in st["true_peak"]]
    bound = 0
    for (name, red, trim, after), (_, before, after_tp) in zip(st["limiter"], st["true_peak"]):
        assert red <= 0.0 and -0.1 <= trim <= 0.0 and after <= -1.0 + 1e-4 and after == after_tp
        if red == 0.0:
            assert trim == 0.0
            continue
        bound += 1
        sr, a = wavfile.read(os.path.join(str(tmp_path / "lim"), name))
        sr, b = wavfile.read(os.path.join(str(tmp_path / "static"), name))
        La = voicefixer_amd.measure_loudness(a.astype(np.float32) / 32768.0)
        Lb = voicefixer_amd.measure_loudness(b.astype(np.float32) / 32768.0)
        print("folder %s: target %.1f, static ceiling %.2f LUFS, limiter %.2f LUFS (reduction %.2f dB, trim %.2e dB)"
              % (name, T, Lb, La, red, trim))
        assert T - Lb > T - La                                           # the static ceiling lands further under the target
        assert ref_true_peak(a.astype(np.float64) / 32768.0, sr) <= 10 ** (-1 / 20) * (1 + 1e-3)
    assert bound >= 1
    from voicefixer_amd import __main__ as cli
    vsd, rsd = seeded_states
    home = str(tmp_path / "home")
    a = os.path.join(home, ".cache/voicefixer/analysis_module/checkpoints")
    v = os.path.join(home, ".cache/voicefixer/synthesis_module/44100")
    os.makedirs(a)
    os.makedirs(v)
    torch.save({"generator": vsd}, os.path.join(v, "model.ckpt-1490000_trimed.pt"))
    torch.save({"generator." + k: t for k, t in rsd.items()}, os.path.join(a, "vf.ckpt"))
    monkeypatch.setenv("HOME", home)
    out = str(tmp_path / "cli")
    assert cli.main(["-ifdr", ind, "-ofdr", out, "--loudness", str(T), "--true-peak", "--limiter", "--silent"]) == 0
    for name in names:                                                   # the CLI writes what the API wrote
        assert open(os.path.join(out, name), "rb").read() == open(os.path.join(str(tmp_path / "lim"), name), "rb").read()
    one = str(tmp_path / "one.wav")
    assert cli.main(["-i", os.path.join(ind, "f0.wav"), "-o", one, "--loudness", str(T), "--true-peak", "--limiter",
                     "--limiter-lookahead-ms", "3", "--silent"]) == 0
    sr, pcm = wavfile.read(one)
    assert sr == 44100 and ref_true_peak(pcm.astype(np.float64) / 32768.0, sr) <= 10 ** (-1 / 20) * (1 + 1e-3)
