"""Loudness normalisation of restored audio (ITU-R BS.1770-4 integrated loudness): the host half.

The measurement and the gain run on the device (``vfx_loudness_rows_f32``, csrc/vfx_loudness.hip; ``ops.loudness_rows``);
this module designs what the kernel is given, in float64, once per rate:

  * the K-weighting biquads from their analog parameters (the shelf and the high-pass of BS.1770; at 48 kHz the formulas
    reproduce the tables of the recommendation),
  * ``hop`` = 100 ms of samples (a quarter of the 400 ms gating block) and the chunk length S of the filter scan,
  * the powers M^(2^i) of the one-chunk state transition M = A^S (A: one sample of both biquads with zero input, built from
    the fp32-rounded coefficients the kernel runs), and how many 256-chunk spans back the carried state still matters,

and checks the user's parameters.  DESIGN.md 3.10 has the definition, the scan and the measured cost.

True peak (``true_peak=True``; ours, after ITU-R BS.1770-4 Annex 2).  A row of n samples at fs is
oversampled R(fs) times -- 4 below 96 kHz, 2 from 96 kHz to below 192 kHz, 1 from 192 kHz -- by the project's one
Kaiser design, ``audio_io.hq_filter(R, 1)``: its float32 taps g in the ``audio_io.polyphase_bank`` layout (751 taps, J = 188
per phase at R = 4),

    y[m] = sum_i bank[p][i] * x[lo + i],   m in [0, R n),   pos = c + m, p = pos mod R, lo = pos // R - J + 1,

the sum ``vfx_resample_rows_f32`` evaluates with down = 1, samples outside [0, n) taken as zero; TP = max(P, max |y[m]|)
with P the sample peak, so a true-peak ceiling is never looser than the sample-peak one; R = 1 or n = 0: TP = P and
nothing is oversampled.  dBTP = 20 log10 TP (-inf for 0).  The device never stores y (``vfx_loudness_tp_rows_f32``).

Loudness report (``vfx_loudness_report_rows_f32``; EBU Tech 3341 / 3342): on the quarters of ``hop`` samples of the
integrated measurement, the maximum momentary loudness is the largest -0.691 + 10 log10 z_j over ALL 400 ms blocks
(ungated), the short-term blocks are 30 consecutive quarters from every quarter j in [0, nq - 30], the maximum short-term
loudness the largest of theirs, and the loudness range LRA is taken over the short-term values above -70 LUFS and above
the loudness of their mean energy - 20 LU: sorted ascending (n values s), LRA = s[((n-1) 95 + 50) // 100] -
s[((n-1) + 5) // 10]; 0.0 when no block survives, -inf for a maximum without a block.

Programmes of several channels (``vfx_loudness_groups_f32``, ``vfx_loudness_report_groups_f32``).  A
programme is C rows of equal length n at fs, 1 <= C <= 8, with weights G_c >= 0.  With q_{c,i} the quarter sums, P_c the
sample peak and TP_c the true peak of channel c as defined above:

  * block energy  z_j = (sum_c G_c (q_{c,j} + q_{c,j+1} + q_{c,j+2} + q_{c,j+3})) * 1/(4 hop), channels summed in ascending
    c in float64 (C = 1, G = 1.0: bit for bit the z_j of one row); both gates and L exactly as for one row on these z_j,
    L = -inf when no block passes;
  * P = max_c P_c, TP = max_c TP_c -- channels of weight 0 included: an LFE channel can clip too;
  * g = min(10^((T - L)/20), 10^(ceiling/20) / (TP or P)), 1 when L = -inf; every channel's output is float32(g) x_c, ONE
    factor for the programme: the balance between the channels is kept;
  * report: the programme quarter sums are Q_i = sum_c G_c q_{c,i} (ascending c, float64); the maximum short-term loudness
    and the LRA are the recipe above on Q, the maximum momentary loudness the largest z_j (ungated), the peaks P and TP.

``channel_weights(C)`` are the weights of BS.1770-4 Table 4 in the WAVE / FLAC channel order (L R C LFE Ls Rs ...: the
surrounds weigh 1.41, the LFE 0).  Two identical channels therefore read 10 log10 2 = 3.0103 LU above the same signal as
one channel: that is the recommendation's sum over channels, not an error.

Look-ahead peak limiter (``limiter=True`` with a loudness target; ``vfx_loudness_limit_f32``).  Per row of N
samples at fs, or per programme of linked channels, after the measurement above has produced L, P and TP:

  1. gL = 10^((T - L)/20) (1 when L = -inf), Cl = 10^(peak_ceiling/20).  The row is BOUND iff gL TP > Cl (TP is the sample
     peak P with ``true_peak=False``); a row that is not bound is written as float32(gL) x, exactly as without the limiter.
  2. Peak envelope: e[n] = |x[n]| with ``true_peak=False`` or at R = 1; otherwise, with y[m] the interpolation above
     (m in [0, R N), bank centre c), e[n] = max(|x[n]|, max{|y[m]| : n(m) = n}), n(m) = min((m + c mod R) // R, N - 1).  For both
     banks c mod R = R - 1 (c = 375 at R = 4, 187 at R = 2), so sample n collects the interpolated values at times in
     (n - 1, n].  For a programme e[n] is the maximum over its channels.
  3. Required gain: c[n] = min(1, Cl / (gL e[n])), 1 when e[n] = 0.
  4. Look-ahead: H = round(fs lookahead_ms / 1000), lookahead_ms in [0.1, 10] (default 3.0), H in [1, 4096];
     m[n] = min{c[j] : |j - n| <= H, 0 <= j < N}.
  5. Smoothing: w[k] = (1 + cos(pi k / (H + 1))) / (2 H + 2) for |k| <= H (all positive, summing to exactly 1);
     g[n] = 1 - sum_{|k| <= H} w[k] (1 - m[clamp(n + k, 0, N - 1)]).  The deficit form gives g[n] = 1 EXACTLY wherever the
     window holds only ones; every m in the window of n covers n, so g[n] <= c[n].
  6. Limited row: v[n] = gL g[n] x[n].
  7. Trim: the interpolated peak of a gain-modulated row is not bounded exactly by step 5.  TPv is the true peak of v by the
     same definition (the sample peak in the sample-peak mode, where t = 1 always); t = min(1, Cl / TPv); the output is t v.
  8. Result record per row or programme, device float64: {L, gL, P, TP, bound (0/1), min_n g[n], t, TPv t}; a row that is
     not bound records {L, gL, P, TP, 0, 1, 1, float32(gL) TP}.

Fixed-gain limiter of a streaming session (``open_stream(gain_db=..., limiter=True)``, ``voicefixer_amd.limit``;
``vfx_limit_span_f32``).  F is steps 2-6 above on one row x[0..N) at fs with a GIVEN gain
gL = 10^(gain_db/20): nothing is measured, there is no bound test and no trim (step 7 needs the whole row).  R = R(fs) with
``true_peak=True``, else 1; H = ``limiter_window(fs, lookahead_ms)[0]``; Cl = 10^(peak_ceiling/20); thr = float32(Cl / gL);
c[n] = thr / e[n] where e[n] > thr, else 1; out[n] = x[n] (float32(gL) g[n]).  Hence

  * where no sample within reach exceeds thr, g = 1 exactly and out = float32(gL) x, the bits of a plain product;
  * |out[n]| <= Cl up to fp32 rounding (g[n] <= c[n] and e[n] >= |x[n]|).  The INTER-SAMPLE peak of a gain-modulated row is
    bounded only approximately, and a session cannot trim: whoever needs a margin lowers ``peak_ceiling``.

Output n depends on the input within 2 H + Bk behind and 2 H + Fw ahead of n: (H, Bk, Fw) = ``limiter_reach(fs, lookahead_ms,
true_peak)``, Fw = c // R = 93 and Bk = J - 1 - c // R = 94 for both banks, 0 and 0 at R = 1.  The span form computes outputs
[m0, m1) from a window of the row, every value a function of global positions, clipped and clamped against [0, N) only: the
bits of the whole row, whatever the split.  Ready rule: with n_known samples seen and the end unknown, outputs
[0, ``limiter_ready(n_known, H, Fw)``) = [0, max(0, n_known - 2 H - Fw)) are final whatever arrives later and whatever N turns
out to be (m[j] is read for j <= n + H and reads c up to n + 2 H, whose interpolated values read x up to n + 2 H + Fw; the
clamp at the row's end and the values behind the last sample change nothing below N - 1 - H >= that bound).  At the end all
N are final.  The added latency is 2 H + Fw samples of the output rate.
"""
import math

import numpy as np

SHELF_F0, SHELF_G_DB, SHELF_Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
SHELF_VB_EXP = 0.4996667741545416
HP_F0, HP_Q = 38.13547087602444, 0.5003270373238773
MIN_RATE, MAX_RATE = 4000, 768000
SPAN = 256                    # chunks per workgroup of the kernel (LK_T)
NPOW = 16                     # M^(2^i), i < NPOW (LK_NPOW)
TARGET_RANGE = (-70.0, 0.0)   # LUFS, [lo, hi)
CEILING_RANGE = (-20.0, 0.0)  # dBFS, [lo, hi]
MAX_CHANNELS = 8
LOOKAHEAD_MS_RANGE = (0.1, 10.0)   # ms, [lo, hi]
LOOKAHEAD_MAX = 4096               # samples (LM_HMAX of the kernel)
_SURROUND = 1.41              # BS.1770-4 Table 4 (Ls, Rs)
_TABLE4 = {1: [1.0], 2: [1.0, 1.0], 3: [1.0, 1.0, 1.0], 4: [1.0, 1.0, _SURROUND, _SURROUND],
           5: [1.0, 1.0, 1.0, _SURROUND, _SURROUND], 6: [1.0, 1.0, 1.0, 0.0, _SURROUND, _SURROUND],
           7: [1.0, 1.0, 1.0, 0.0, 1.0, _SURROUND, _SURROUND], 8: [1.0, 1.0, 1.0, 0.0, 1.0, 1.0, _SURROUND, _SURROUND]}
CHANNEL_MODES = ("mix", "first", "all")


def oversampling(fs):
    """R(fs) of the true-peak measurement: 4 below 96 kHz, 2 below 192 kHz, else 1."""
    fs = _check_rate(fs)
    return 4 if fs < 96000 else (2 if fs < 192000 else 1)


def check_true_peak(flag):
    """``true_peak`` is a bool."""
    if not isinstance(flag, (bool, np.bool_)):
        raise ValueError("true_peak must be True or False (got %r)" % (flag,))
    return bool(flag)


def to_db(v):
    """20 log10 v; -inf for 0."""
    v = float(v)
    return 20.0 * math.log10(v) if v > 0.0 else -math.inf


def _check_rate(fs):
    if isinstance(fs, bool) or int(fs) != fs or not MIN_RATE <= int(fs) <= MAX_RATE:
        raise ValueError("loudness: sample rate must be an integer in [%d, %d] (got %r)" % (MIN_RATE, MAX_RATE, fs))
    return int(fs)


def k_weighting(fs):
    """(shelf_b, shelf_a, hp_b, hp_a) of the K-weighting at ``fs`` Hz, float64, a[0] = 1."""
    fs = _check_rate(fs)
    K = math.tan(math.pi * SHELF_F0 / fs)
    Vh = 10.0 ** (SHELF_G_DB / 20.0)
    Vb = Vh ** SHELF_VB_EXP
    a0 = 1.0 + K / SHELF_Q + K * K
    sb = np.array([(Vh + Vb * K / SHELF_Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / SHELF_Q + K * K) / a0])
    sa = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / SHELF_Q + K * K) / a0])
    K = math.tan(math.pi * HP_F0 / fs)
    d = 1.0 + K / HP_Q + K * K
    hb = np.array([1.0, -2.0, 1.0])
    ha = np.array([1.0, 2.0 * (K * K - 1.0) / d, (1.0 - K / HP_Q + K * K) / d])
    return sb, sa, hb, ha


def hop_length(fs):
    """Samples of one 100 ms quarter block: (fs + 5) // 10 (1103 at 11025 Hz)."""
    return (_check_rate(fs) + 5) // 10


def chunk_length(fs):
    """Samples one lane filters: a multiple of 32 near fs / 200 (224 at 44.1 kHz: a 32 x 10 s batch is ~63 K lanes), never
    more than a quarter block, so a chunk straddles at most one quarter boundary."""
    return 32 * max(1, (_check_rate(fs) + 3200) // 6400)


def coefficients(fs):
    """The 10 float64 values the kernel takes: shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2."""
    sb, sa, hb, ha = k_weighting(fs)
    return np.concatenate([sb, sa[1:], hb, ha[1:]])


def transition(fs):
    """A: the 4x4 zero-input state transition of one sample, state (shelf z1, z2, high-pass z1, z2) of the transposed
    direct form II, with the coefficients rounded to fp32 as the kernel runs them."""
    c = coefficients(fs).astype(np.float32).astype(np.float64)
    b0s, b1s, b2s, a1s, a2s, b0h, b1h, b2h, a1h, a2h = c
    A = np.zeros((4, 4))
    for j in range(4):
        s = np.zeros(4)
        s[j] = 1.0
        ys = s[0]                                      # zero input
        t0, t1 = -a1s * ys + s[1], -a2s * ys
        yh = b0h * ys + s[2]
        t2, t3 = b1h * ys - a1h * yh + s[3], b2h * ys - a2h * yh
        A[:, j] = (t0, t1, t2, t3)
    return A


_PLANS = {}


def plan(fs):
    """Everything the kernel needs at ``fs`` (cached): dict with coef (float64[10]), S, hop, mpow (float64[16, 4, 4]:
    M^(2^i)) and lookback (spans whose carry is summed: the first p with max|Mspan^p| < 2^-80, Mspan = M^256)."""
    fs = _check_rate(fs)
    hit = _PLANS.get(fs)
    if hit is not None:
        return hit
    S, hop = chunk_length(fs), hop_length(fs)
    M = np.linalg.matrix_power(transition(fs), S)
    pw = [M]
    for _ in range(NPOW - 1):
        pw.append(pw[-1] @ pw[-1])
    mpow = np.ascontiguousarray(np.stack(pw))
    span = pw[8]                                       # M^256
    lookback, p = 1, span
    while np.abs(p).max() >= 2.0 ** -80:
        lookback += 1
        p = p @ span
        if lookback >= SPAN:
            raise ValueError("loudness: the filter state does not decay at %d Hz" % fs)
    hit = {"coef": coefficients(fs), "S": S, "hop": hop, "mpow": mpow, "lookback": lookback}
    _PLANS[fs] = hit
    return hit


def _number(v, what):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError("%s must be a number (got %r)" % (what, v))
    v = float(v)
    if not math.isfinite(v):
        raise ValueError("%s must be finite (got %r)" % (what, v))
    return v


def check_target(target):
    """None (no normalisation) or a loudness target in [-70, 0) LUFS."""
    if target is None:
        return None
    v = _number(target, "loudness")
    if not TARGET_RANGE[0] <= v < TARGET_RANGE[1]:
        raise ValueError("loudness must be in [-70, 0) LUFS (got %r)" % target)
    return v


def check_ceiling(ceiling_db):
    """A sample-peak ceiling in [-20, 0] dBFS."""
    v = _number(ceiling_db, "peak_ceiling")
    if not CEILING_RANGE[0] <= v <= CEILING_RANGE[1]:
        raise ValueError("peak_ceiling must be in [-20, 0] dBFS (got %r)" % ceiling_db)
    return v


def check_channel_count(C):
    """A channel count in 1..8."""
    if isinstance(C, (bool, np.bool_)) or not isinstance(C, (int, np.integer)) or not 1 <= int(C) <= MAX_CHANNELS:
        raise ValueError("a programme has 1..%d channels (got %r)" % (MAX_CHANNELS, C))
    return int(C)


def channel_weights(C, override=None):
    """The channel weights G_c of a programme of C channels: BS.1770-4 Table 4 in the WAVE / FLAC channel order, or
    ``override``: a list of C finite floats >= 0 (anything else raises ValueError)."""
    C = check_channel_count(C)
    if override is None:
        return list(_TABLE4[C])
    if isinstance(override, (str, bytes)) or not isinstance(override, (list, tuple, np.ndarray)) or len(override) != C:
        raise ValueError("channel_weights must be a list of %d numbers >= 0 (got %r)" % (C, override))
    out = [_number(v, "channel_weights[%d]" % i) for i, v in enumerate(override)]
    if min(out) < 0.0:
        raise ValueError("channel_weights must be >= 0 (got %r)" % (override,))
    return out


def check_channels(channels, allow_none=True):
    """``channels``: None (only where a default exists), "mix", "first" or "all"."""
    if channels is None and allow_none:
        return None
    if not isinstance(channels, str) or channels not in CHANNEL_MODES:
        raise ValueError("channels must be 'mix', 'first' or 'all' (got %r)" % (channels,))
    return channels


def check_limiter(limiter, lookahead_ms=3.0):
    """(limiter, lookahead_ms): ``limiter`` is a bool, ``lookahead_ms`` a number in [0.1, 10]."""
    if not isinstance(limiter, (bool, np.bool_)):
        raise ValueError("limiter must be True or False (got %r)" % (limiter,))
    v = _number(lookahead_ms, "limiter_lookahead_ms")
    if not LOOKAHEAD_MS_RANGE[0] <= v <= LOOKAHEAD_MS_RANGE[1]:
        raise ValueError("limiter_lookahead_ms must be in [0.1, 10] ms (got %r)" % (lookahead_ms,))
    return bool(limiter), v


def limiter_window(fs, ms=3.0):
    """(H, w) of the limiter at ``fs`` Hz: H = round(fs ms / 1000) in [1, 4096] (ValueError otherwise) and the smoothing
    weights w[k], k = -H..H, float64[2 H + 1]: (1 + cos(pi k / (H + 1))) / (2 H + 2)."""
    fs = _check_rate(fs)
    ms = check_limiter(True, ms)[1]
    H = int(math.floor(fs * ms / 1000.0 + 0.5))
    if not 1 <= H <= LOOKAHEAD_MAX:
        raise ValueError("limiter: a look-ahead of %r ms at %d Hz is %d samples, outside [1, %d]" % (ms, fs, H, LOOKAHEAD_MAX))
    k = np.arange(-H, H + 1, dtype=np.float64)
    return H, (1.0 + np.cos(np.pi * k / (H + 1))) / (2.0 * H + 2.0)


GAIN_RANGE = (-60.0, 60.0)    # dB, [lo, hi]


def check_gain(gain_db):
    """None (no gain stage) or a fixed gain in [-60, 60] dB."""
    if gain_db is None:
        return None
    v = _number(gain_db, "gain_db")
    if not GAIN_RANGE[0] <= v <= GAIN_RANGE[1]:
        raise ValueError("gain_db must be in [-60, 60] dB (got %r)" % (gain_db,))
    return v


def limiter_reach(fs, lookahead_ms=3.0, true_peak=False):
    """(H, Bk, Fw) of the fixed-gain limiter at ``fs`` Hz: the look-ahead in samples and how far the peak envelope of a sample
    reads behind and ahead of it -- Bk = J - 1 - c // R and Fw = c // R of the true-peak bank (94 and 93 at R = 4 and at R = 2),
    0 and 0 at R = 1 and with ``true_peak=False``.  Output n reads the input in [n - 2 H - Bk, n + 2 H + Fw]."""
    H = limiter_window(fs, lookahead_ms)[0]
    R = oversampling(fs) if check_true_peak(true_peak) else 1
    if R == 1:
        return H, 0, 0
    from . import audio_io
    _, J, c = audio_io.hq_bank(R, 1)
    return H, J - 1 - c // R, c // R


def limiter_ready(n_known, H, Fw):
    """How many outputs of the fixed-gain limiter are final once ``n_known`` samples of a row of unknown length are known:
    max(0, n_known - 2 H - Fw)."""
    return max(0, int(n_known) - 2 * int(H) - int(Fw))
