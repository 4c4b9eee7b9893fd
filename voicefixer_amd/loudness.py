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

Streaming loudness leveller (``open_stream(leveller=T)``, ``voicefixer_amd.level``; ``vfx_level_span_f32``): a
slowly moving gain that follows the short-term loudness (EBU Tech 3341: 3 s) where no whole-file measurement exists.  Per row
x[0..N) at fs <= 192 kHz: hop = ``hop_length(fs)``, quarter q = [q hop, (q + 1) hop), Q = N // hop complete quarters (a partial
last quarter is never measured).  Parameters: the target T (``check_target``), ``max_gain_db`` in [0, 40] (default 12), ``gate``
(LUFS) in [-70, T) (default -50).  LEVELLER_WARMUP = 2, LEVELLER_BEHIND = 20, LEVELLER_AHEAD = 10 quarters, LEVELLER_MAX_CUT = 40 dB.

  1. Local quarter energy: E_q = the sum over quarter q of y^2 (float64 sum), y the K-weighting (the fp32 coefficients of
     ``coefficients(fs)``, as the kernels run them) started from ZERO state at sample max(0, (q - 2) hop).  The truncated warm-up
     is the definition: ``transition(fs)^(2 hop)`` has no entry above 1.4e-16 for 4 kHz <= fs <= 192 kHz (7e-19 at 4 kHz, 1.4e-17
     at 44.1 kHz, 9e-18 at 48 kHz, 1.4e-16 at 192 kHz), far below fp32 resolution; at 768 kHz it is 3.5e-5, so the leveller
     refuses fs > 192000 (ValueError).  E_q depends on x[(q - 2) hop .. (q + 1) hop) only.
  2. Anchor loudness: anchor q sits at sample q hop, q = 0..Q; its window is the quarters j in [q - 20, q + 9] within [0, Q);
     z_q = (sum of E_j, ascending j, float64, a direct sum per anchor) / (count hop); l_q = -0.691 + 10 log10 z_q.  An empty
     window or z_q = 0 counts as gated.
  3. Anchor gain: G_q = clamp(T - l_q, -40, max_gain_db) if l_q > gate, else G_{q-1} (hold), G_{-1} = 0 dB;
     a_q = float32(10^(G_q / 20)), evaluated in float64 and rounded once.
  4. Output: for t in quarter q <= Q - 1, with r = t - q hop, in float32 and every operation rounded once, in this order:
         f = float32(r) / float32(hop);   d = a_{q+1} - a_q;   p = d * f;   g = a_q + p;   out[t] = x[t] * g
     (no fused multiply-add; ``level_reference`` is this in numpy float32); for the partial tail t >= Q hop: out[t] = x[t] * a_Q.
     N < hop: Q = 0, the one anchor is gated, a_0 = 1 and out = x exactly.
  5. Ready rule: with n_known samples seen and the end unknown, outputs [0, ``leveller_ready(n_known, hop)``) =
     [0, max(0, (n_known // hop - 10) hop)) are final whatever arrives later and whatever N turns out to be: every window they
     read consists of complete, existing quarters.  At the end all N are final.  Added latency: less than 11 quarters (1.1 s).
  6. Record (device float64): {min G, max G, anchors evaluated, anchors gated} and G of the last anchor (what the hold carries);
     exact folds (min, max, integer counts): the values of one call over the whole row.

The span form takes its calls in order; after outputs [0, m) the anchors [0, na) are evaluated and the energies [0, ne) computed,
(na, ne) = ``leveller_counts(m, hop, Q)``, which is what the caller's device state then holds (the last 32 energies, the last four
anchor gains, the carried G and the record).
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


# ---- streaming loudness leveller (module docstring) ---------------------------------------------------------------
LEVELLER_WARMUP = 2           # quarters the filter runs from zero before a measured quarter
LEVELLER_BEHIND = 20          # quarters of an anchor's window behind it
LEVELLER_AHEAD = 10           # ... and from it on
LEVELLER_MAX_CUT = 40.0       # dB
LEVELLER_MAX_RATE = 192000
LEVELLER_MAX_GAIN_RANGE = (0.0, 40.0)   # dB, [lo, hi]
LEVELLER_GATE_MIN = -70.0     # LUFS; gate in [-70, T)
LEVELLER_STATE = 64           # float64 values of the device state (VFX_LEVEL_STATE)


def check_leveller(target, max_gain_db=12.0, gate=-50.0, fs=None):
    """(T, max_gain_db, gate) of the leveller as floats: T in [-70, 0) LUFS (not None), ``max_gain_db`` in [0, 40] dB, ``gate``
    in [-70, T) LUFS; ``fs`` (when given) an integer rate in [4000, 192000].  ValueError otherwise."""
    T = check_target(target)
    if T is None:
        raise ValueError("leveller: the target must be a number in [-70, 0) LUFS (got None)")
    g = _number(max_gain_db, "leveller_max_gain_db")
    if not LEVELLER_MAX_GAIN_RANGE[0] <= g <= LEVELLER_MAX_GAIN_RANGE[1]:
        raise ValueError("leveller_max_gain_db must be in [0, 40] dB (got %r)" % (max_gain_db,))
    gt = _number(gate, "leveller_gate")
    if not LEVELLER_GATE_MIN <= gt < T:
        raise ValueError("leveller_gate must be in [-70, target) LUFS (got %r with a target of %r)" % (gate, target))
    if fs is not None and _check_rate(fs) > LEVELLER_MAX_RATE:
        raise ValueError("leveller: rates above %d Hz are refused -- the two-quarter warm-up of the K-weighting no longer decays "
                         "below fp32 resolution (got %r)" % (LEVELLER_MAX_RATE, fs))
    return T, g, gt


def leveller_chunk(fs):
    """Samples one lane of the quarter kernel filters: 32 ceil(3 hop / 8192), so that 256 chunks cover a region of 3 hop."""
    return 32 * ((3 * hop_length(fs) + 8191) // 8192)


_LEVELLER_PLANS = {}


def leveller_plan(fs):
    """What the leveller's kernels need at ``fs`` (cached): dict with coef (float64[10]), hop, S = ``leveller_chunk(fs)`` and
    mpow (float64[8, 4, 4]: M^(2^i), M = ``transition(fs)``^S)."""
    check_leveller(-16.0, fs=fs)
    fs = int(fs)
    hit = _LEVELLER_PLANS.get(fs)
    if hit is None:
        S = leveller_chunk(fs)
        pw = [np.linalg.matrix_power(transition(fs), S)]
        for _ in range(7):
            pw.append(pw[-1] @ pw[-1])
        hit = {"coef": coefficients(fs), "hop": hop_length(fs), "S": S, "mpow": np.ascontiguousarray(np.stack(pw))}
        _LEVELLER_PLANS[fs] = hit
    return hit


def leveller_ready(n_known, hop):
    """How many outputs of the leveller are final once ``n_known`` samples of a row of unknown length are known:
    max(0, (n_known // hop - 10) hop)."""
    return max(0, (int(n_known) // int(hop) - LEVELLER_AHEAD) * int(hop))


def leveller_counts(m, hop, Q=None):
    """(na, ne): the anchors evaluated and the energies computed once outputs [0, m) of a row of Q complete quarters are done
    (None: the end is unknown): na = min(Q, (m - 1) // hop + 1) + 1, ne = min(Q, na + 9); (0, 0) for m = 0."""
    m, hop = int(m), int(hop)
    if m <= 0:
        return 0, 0
    a = (m - 1) // hop + 1
    na = (a if Q is None else min(a, Q)) + 1
    ne = na + LEVELLER_AHEAD - 1
    return na, (ne if Q is None else min(ne, Q))


def leveller_energies(x, fs):
    """E_q, q < N // hop, of one row (step 1 of the definition) in float64: scipy.signal.lfilter over every quarter's own region
    [max(0, (q - 2) hop), (q + 1) hop) from zero state, with the fp32-rounded coefficients."""
    from scipy.signal import lfilter
    check_leveller(-16.0, fs=fs)
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 1:
        raise ValueError("leveller_energies: a row is a 1-D array (got shape %r)" % (x.shape,))
    hop = hop_length(fs)
    c = coefficients(fs).astype(np.float32).astype(np.float64)
    sb, sa, hb, ha = c[0:3], np.array([1.0, c[3], c[4]]), c[5:8], np.array([1.0, c[8], c[9]])
    Q = x.shape[0] // hop
    E = np.zeros(Q)
    for q in range(Q):
        r0 = max(0, (q - LEVELLER_WARMUP) * hop)
        y = lfilter(hb, ha, lfilter(sb, sa, x[r0:(q + 1) * hop]))[q * hop - r0:]
        E[q] = float(np.dot(y, y))
    return E


def leveller_gains(E, N, fs, T, max_gain_db=12.0, gate=-50.0):
    """Steps 2 and 3 on the quarter energies ``E`` (N // hop of them) of a row of N samples: dict with l (float64[Q + 1], the
    anchors' loudness; -inf for an empty or silent window), held (bool[Q + 1]: gated), G (float64[Q + 1], dB) and a (float32[Q + 1])."""
    T, max_gain_db, gate = check_leveller(T, max_gain_db, gate, fs)
    hop = hop_length(fs)
    Q = int(N) // hop
    E = np.asarray(E, dtype=np.float64)
    if E.shape != (Q,):
        raise ValueError("leveller_gains: %d samples at %d Hz have %d quarters (got %r energies)" % (N, fs, Q, E.shape))
    l = np.full(Q + 1, -np.inf)
    G = np.zeros(Q + 1)
    gated = np.zeros(Q + 1, dtype=bool)
    prev = 0.0
    for q in range(Q + 1):
        j0, j1 = max(0, q - LEVELLER_BEHIND), min(Q, q + LEVELLER_AHEAD)
        z = 0.0
        for j in range(j0, j1):
            z += float(E[j])
        if j1 > j0 and z > 0.0:
            l[q] = -0.691 + 10.0 * math.log10(z / (float(j1 - j0) * float(hop)))
        if l[q] > gate:
            prev = min(max(T - l[q], -LEVELLER_MAX_CUT), max_gain_db)
        else:
            gated[q] = True
        G[q] = prev
    a = np.array([np.float32(10.0 ** (g / 20.0)) for g in G], dtype=np.float32)
    return {"l": l, "held": gated, "G": G, "a": a}


def leveller_apply(x, a, hop):
    """Step 4 in numpy float32, in the operation order of the definition: x (N,) float32, a (N // hop + 1,) float32."""
    x = np.asarray(x, dtype=np.float32)
    a = np.asarray(a, dtype=np.float32)
    N = x.shape[0]
    Q = N // hop
    t = np.arange(N, dtype=np.int64)
    q = np.minimum(t // hop, Q)
    body = q < Q
    f = (t - q * hop).astype(np.float32) / np.float32(hop)
    a0 = a[q]
    a1 = a[np.minimum(q + 1, Q)]
    d = a1 - a0
    p = d * f
    g = np.where(body, a0 + p, a0).astype(np.float32)
    return x * g


def level_reference(x, fs, target=-16.0, max_gain_db=12.0, gate=-50.0, stats=None):
    """The leveller of one row on the host: float64 energies and gains, the float32 output of step 4.  ``stats``: a dict that
    receives {"min_gain_db", "max_gain_db", "anchors", "gated"} and the arrays of ``leveller_gains``."""
    x = np.asarray(x, dtype=np.float32)
    r = leveller_gains(leveller_energies(x, fs), x.shape[0], fs, target, max_gain_db, gate)
    if stats is not None:
        stats.update(r, min_gain_db=float(r["G"].min()), max_gain_db=float(r["G"].max()), anchors=int(r["G"].shape[0]),
                     gated=int(r["held"].sum()))
    return leveller_apply(x, r["a"], hop_length(fs))


def leveller_energies_linked(x, fs, weights=None):
    """The LINKED quarter energies of a programme x (C, N): E_q = sum_c w_c E_{q,c} with E_{q,c} =
    ``leveller_energies(x[c], fs)`` and w = ``channel_weights(C, weights)``, in float64, c ascending from 0.0, every product and
    every sum rounded on its own (what vfx_level_span_rows_f32 does with its per-channel energies)."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError("leveller_energies_linked: a programme is a (C, N) array (got shape %r)" % (x.shape,))
    w = channel_weights(int(x.shape[0]), weights)
    E = np.zeros(x.shape[1] // hop_length(fs))
    for c in range(x.shape[0]):
        E = E + np.float64(w[c]) * leveller_energies(x[c], fs)
    return E


def level_reference_linked(x, fs, target=-16.0, max_gain_db=12.0, gate=-50.0, weights=None, stats=None):
    """``level_reference`` of a programme x (C, N) with ONE gain for all channels: the gains of ``leveller_gains`` on the linked
    energies, the float32 ramp of step 4 applied to every channel.  Returns float32 (C, N); ``stats`` as there."""
    x = np.asarray(x, dtype=np.float32)
    r = leveller_gains(leveller_energies_linked(x, fs, weights), x.shape[1], fs, target, max_gain_db, gate)
    if stats is not None:
        stats.update(r, min_gain_db=float(r["G"].min()), max_gain_db=float(r["G"].max()), anchors=int(r["G"].shape[0]),
                     gated=int(r["held"].sum()))
    hop = hop_length(fs)
    return np.stack([leveller_apply(x[c], r["a"], hop) for c in range(x.shape[0])])


# ---- streaming loudness meter --------------------------------------------------------------------------------
# ``open_stream(meter=True)``, ``voicefixer_amd.LoudnessMeter``; ``vfx_meter_span_rows_f32``, ``vfx_meter_report_f32``.  What a
# session delivered, in EBU R 128 terms, without keeping it: per programme x (C, N) at fs <= 192 kHz (a row is the programme of one
# channel with the weight 1), hop = ``hop_length(fs)``, the meter carries
#   * the quarter energies E_q, q < N // hop: the leveller's LINKED quarter energies (``leveller_energies_linked``), 8 bytes per
#     100 ms, from which ``meter_report`` takes every loudness figure by the recipe of the whole-row report (module docstring) --
#     the 400 ms blocks z_j = (E_j + E_{j+1} + E_{j+2} + E_{j+3}) / (4 hop), both gates, the 3 s blocks from every quarter, the LRA
#     -- and the two live figures ``momentary`` / ``short_term``: the loudness of the last 4 / 30 complete quarters;
#   * the sample peak P = max_c max |x_c| and the true peak TP = max(P, max |y|) of DESIGN.md 3.11, exact maxima.
# The filter of a quarter starts from zero two quarters earlier (the leveller's definition, which makes a quarter a function of
# 3 hop samples); the whole-row measurement filters the row once.  The two differ by the decayed state only (``transition(fs)^(2
# hop)`` < 1.4e-16), far below the bounds of DESIGN.md 3.10.
METER_STATE = 16              # float64 values of the device state (VFX_METER_STATE)
METER_KEYS = ("integrated", "loudness_range", "max_momentary", "max_short_term", "sample_peak", "true_peak", "momentary",
              "short_term", "seconds")


def check_meter(meter, fs=None):
    """``meter`` is a bool; ``fs`` (when given) an integer rate in [4000, 192000] -- the meter's quarters are the leveller's."""
    if not isinstance(meter, (bool, np.bool_)):
        raise ValueError("meter must be True or False (got %r)" % (meter,))
    if fs is not None and _check_rate(fs) > LEVELLER_MAX_RATE:
        raise ValueError("meter: rates above %d Hz are refused -- the two-quarter warm-up of the K-weighting no longer decays "
                         "below fp32 resolution (got %r)" % (LEVELLER_MAX_RATE, fs))
    return bool(meter)


def meter_reach(fs):
    """(R, Bk, Fw) of the meter's true peak at ``fs`` Hz: the oversampling and how far the interpolated values that belong to a
    sample read behind and ahead of it (``limiter_reach`` with true_peak=True: 94 and 93 at R = 4 and at R = 2, 0 and 0 at R = 1)."""
    R = oversampling(fs)
    if R == 1:
        return 1, 0, 0
    from . import audio_io
    _, J, c = audio_io.hq_bank(R, 1)
    return R, J - 1 - c // R, c // R


def meter_counts(m, hop):
    """nq: the quarters in the log once the samples [0, m) are metered: m // hop (never more than the row's N // hop)."""
    return max(int(m), 0) // int(hop)


def meter_ready(n_known, Fw):
    """How many samples can be metered once ``n_known`` samples of a row of unknown length are known: max(0, n_known - Fw) --
    the interpolated values of a sample read Fw samples ahead of it."""
    return max(0, int(n_known) - int(Fw))


def meter_keep(m1, hop, Bk):
    """The first sample that metering from m1 on still reads: max(0, min(m1 - Bk, (m1 // hop - 2) hop)) -- the interpolated values
    of sample m1 reach Bk behind it, the next quarter's filter starts two quarters before it."""
    m1, hop = int(m1), int(hop)
    return max(0, min(m1 - int(Bk), (m1 // hop - LEVELLER_WARMUP) * hop))


def _programme(x, what):
    x = np.asarray(x)
    if x.ndim == 1:
        x = x[None]
    if x.ndim != 2:
        raise ValueError("%s: a row is (N,), a programme (C, N) (got shape %r)" % (what, x.shape))
    check_channel_count(int(x.shape[0]))
    return x


def meter_energies(x, fs, weights=None):
    """The meter's quarter energies E_q, q < N // hop, of a row (N,) or a programme (C, N), float64: the leveller's linked quarter
    energies (``leveller_energies_linked``; one channel of weight 1: ``leveller_energies``, since 0 + 1 E = E)."""
    check_meter(True, fs)
    return leveller_energies_linked(_programme(x, "meter_energies"), fs, weights)


def _lufs(z):
    return -0.691 + 10.0 * math.log10(z) if z > 0.0 else -math.inf


def meter_report(E, hop):
    """The loudness figures of the quarter energies E[0..Q) at quarters of ``hop`` samples, float64, in the order of the device
    report (vfx_meter_report_f32): dict with ``integrated`` (both gates over the 400 ms blocks; -inf: no block passes),
    ``loudness_range`` (0.0: no short-term block survives), ``max_momentary`` (all blocks, ungated), ``max_short_term`` (-inf
    without a block) and the live ``momentary`` / ``short_term`` (the last 4 / 30 quarters; -inf with fewer)."""
    E = np.asarray(E, dtype=np.float64).reshape(-1)
    Q, hop = E.shape[0], int(hop)
    inv4, inv30 = 1.0 / (4.0 * hop), 1.0 / (30.0 * hop)
    z = np.array([(((E[j] + E[j + 1]) + E[j + 2]) + E[j + 3]) * inv4 for j in range(max(Q - 3, 0))])
    st = np.zeros(max(Q - 29, 0))
    for j in range(st.shape[0]):
        a = 0.0
        for i in range(30):
            a += float(E[j + i])
        st[j] = a * inv30
    lz = np.array([_lufs(v) for v in z])
    ls = np.array([_lufs(v) for v in st])
    L = -math.inf
    g1 = lz > -70.0
    if g1.any():
        gr = _lufs(float(z[g1].sum()) / int(g1.sum())) - 10.0
        g2 = g1 & (lz > gr)
        if g2.any():
            L = _lufs(float(z[g2].sum()) / int(g2.sum()))
    lra = 0.0
    g1 = ls > -70.0
    if g1.any():
        gr = _lufs(float(st[g1].sum()) / int(g1.sum())) - 20.0
        s = np.sort(st[g1 & (ls > gr)])
        n = s.shape[0]
        if n:
            lra = _lufs(float(s[((n - 1) * 95 + 50) // 100])) - _lufs(float(s[((n - 1) + 5) // 10]))
    return {"integrated": L, "loudness_range": lra,
            "max_momentary": _lufs(float(z.max())) if z.size else -math.inf,
            "max_short_term": _lufs(float(st.max())) if st.size else -math.inf,
            "momentary": float(lz[-1]) if z.size else -math.inf, "short_term": float(ls[-1]) if st.size else -math.inf}


def meter_reference(x, fs, weights=None, final=True):
    """The meter on the host, float64: the nine figures (``METER_KEYS``; peaks in dB as in ``loudness_report``) of a row (N,) or
    a programme (C, N) at ``fs``.  ``final=True``: the row is complete -- ``true_peak`` includes the interpolated values behind
    the last sample, as the whole-row measurement does.  ``final=False``: the report while the end is unknown, after N samples
    have been fed: quarters and sample peak cover every complete quarter and every sample, but ``true_peak`` covers only the
    interpolated values whose taps have all arrived, those that belong to the samples below N - Fw (``meter_reach``): the
    interpolator is a symmetric filter that reads Fw = 93 samples ahead of a value, and a value computed with zeros in place of
    samples still to come would be WRONG, not early -- so the mid-stream true peak is Fw samples late (2.1 ms at 44.1 kHz;
    never below the sample peak, which is not late)."""
    from scipy.signal import upfirdn
    from . import audio_io
    x = _programme(x, "meter_reference").astype(np.float64)
    C_, N = x.shape
    hop = hop_length(fs)
    out = meter_report(meter_energies(x, fs, weights), hop)
    P = float(np.abs(x).max()) if N else 0.0
    TP = P
    R, _, Fw = meter_reach(fs)
    if R > 1 and N:
        g = audio_io.hq_filter(R, 1)[1].astype(np.float64)
        c = (g.shape[0] - 1) // 2
        # value m in [0, R N) sits at c + m of the full convolution and belongs to sample (c + m) // R - c // R
        m1 = R * N if final else max(0, min(R * N, R * (N - Fw + c // R) - c))
        for ch in range(C_):
            y = upfirdn(g, x[ch], up=R)[c:c + m1]
            if y.size:
                TP = max(TP, float(np.abs(y).max()))
    out.update(sample_peak=to_db(P), true_peak=to_db(TP), seconds=N / float(fs))
    return {k: out[k] for k in METER_KEYS}
