"""Word-length reduction to 16- or 24-bit PCM with seeded dither: the specification ``vfx_quantize_rows_f32`` implements.

The device result is integer-identical to ``quantize_ref`` (numpy, float64).  Everything is a pure function of a sample's
ABSOLUTE index in its file, its channel and a 64-bit seed, so a row may be quantised in any number of pieces (the streaming
session does) and in any batch, and a run can be repeated.

For a row whose first sample has absolute index ``n0`` >= 0, channel ``c`` (0..7), seed ``s``, depth ``b`` in {16, 24} and
sample ``i`` of the row, n = n0 + i:

  * random words: k_t(n) = (word n % 4 of Philox4x32-10(counter = ((n // 4) & 0xffffffff, (n // 4) >> 32, c, t),
    dropout.key_of(s))) >> 8, a 24-bit integer; t in {0, 1} are two independent streams;
  * dither d(n), in LSB: "none": 0;  "tpdf": (k_0(n) - k_1(n)) * 2^-24 -- triangular on (-1, 1), white, variance 1/6 LSB^2;
    "hp": (k_0(n) - k_0(n - 1)) * 2^-24 for n >= 1, d(0) the "tpdf" value -- the same triangular PDF and variance, its
    spectrum rising with frequency as sin^2(w / 2); still a pure function of n.  Both integer differences are below 2^24 in
    magnitude: exact in float32 and float64;
  * v = float64(x) * 2^(b-1) + d(n) (the product is exact, the sum is ONE float64 rounding: a fused multiply-add gives the
    same bits);  NaN -> 0;  q = clamp(rint(v), -2^(b-1), 2^(b-1) - 1): round half to even; saturate, never wrap.

Per row: ``clipped``, the number of samples where the clamp changed the value or x was NaN, and ``peak`` = max |q|.

There is no error feedback (noise shaping): it is a serial recurrence through the quantiser; "hp" is the
parallel substitute.
"""
import numpy as np

from . import dropout

DEPTHS = (16, 24)
DITHERS = ("none", "tpdf", "hp")
MAX_CHANNELS = 8


def check_bit_depth(bit_depth, allow_none=False):
    """16 or 24 (an int, not a bool, not a string); None only with ``allow_none``."""
    if bit_depth is None and allow_none:
        return None
    if isinstance(bit_depth, bool) or not isinstance(bit_depth, (int, np.integer)):
        raise TypeError("bit_depth must be 16 or 24 (an int), got %r" % (bit_depth,))
    if int(bit_depth) not in DEPTHS:
        raise ValueError("bit_depth must be 16 or 24, got %d" % bit_depth)
    return int(bit_depth)


def check_dither(dither):
    if not isinstance(dither, str) or dither not in DITHERS:
        raise ValueError('dither must be "none", "tpdf" or "hp", got %r' % (dither,))
    return dither


def check_channel(channel):
    if isinstance(channel, bool) or not isinstance(channel, (int, np.integer)) or not 0 <= int(channel) < MAX_CHANNELS:
        raise ValueError("channel must be an int in 0..7, got %r" % (channel,))
    return int(channel)


def check_position(n0):
    if isinstance(n0, bool) or not isinstance(n0, (int, np.integer)) or not 0 <= int(n0) < 2 ** 62:
        raise ValueError("n0 must be an int in [0, 2**62), got %r" % (n0,))
    return int(n0)


def words(n0, N, channel, seed, stream):
    """k_stream(n) for n = n0 .. n0 + N - 1: int64 (N,) of 24-bit values."""
    key = dropout.key_of(seed)
    n = np.uint64(n0) + np.arange(N, dtype=np.uint64)
    q = n >> np.uint64(2)
    ctr = np.stack([(q & np.uint64(0xffffffff)).astype(np.uint32), (q >> np.uint64(32)).astype(np.uint32),
                    np.full(N, channel, np.uint32), np.full(N, stream, np.uint32)], axis=-1)
    w = dropout.philox4x32_10(ctr, key)[np.arange(N), (n & np.uint64(3)).astype(np.int64)]
    return (w >> np.uint32(8)).astype(np.int64)


def dither(kind, n0, N, channel, seed):
    """d(n) in LSB for n = n0 .. n0 + N - 1: float64 (N,)."""
    kind, n0, channel = check_dither(kind), check_position(n0), check_channel(channel)
    dropout.check_seed(seed)
    N = int(N)
    if kind == "none" or N == 0:
        return np.zeros(N, np.float64)
    if kind == "tpdf":
        diff = words(n0, N, channel, seed, 0) - words(n0, N, channel, seed, 1)
    else:
        lo = max(n0 - 1, 0)                              # k_0 from n0 - 1 on (from 0 when the row starts the file)
        k0 = words(lo, N + (n0 - lo), channel, seed, 0)
        if n0 == 0:
            diff = np.empty(N, np.int64)
            diff[1:] = k0[1:] - k0[:-1]
            diff[0] = k0[0] - words(0, 1, channel, seed, 1)[0]
        else:
            diff = k0[1:] - k0[:-1]
    return diff.astype(np.float64) * 2.0 ** -24


_dither_values = dither      # (quantize_ref's ``dither`` keyword is the KIND)


def quantize_ref(x, bit_depth, dither="tpdf", seed=0, n0=0, channel=0):
    """One row: float samples (N,) -> (int32 (N,), clipped, peak) as defined above."""
    b = check_bit_depth(bit_depth)
    x = np.asarray(x)
    if x.ndim != 1:
        raise ValueError("quantize_ref takes one row (N,), got shape %r" % (x.shape,))
    d = _dither_values(dither, n0, x.shape[0], channel, seed)
    with np.errstate(invalid="ignore", over="ignore"):
        v = x.astype(np.float64) * 2.0 ** (b - 1) + d
    nan = np.isnan(v)
    r = np.rint(np.where(nan, 0.0, v))
    q = np.clip(r, -2.0 ** (b - 1), 2.0 ** (b - 1) - 1.0)
    clipped = int(np.count_nonzero((q != r) | nan))
    q = q.astype(np.int32)
    peak = int(np.max(np.abs(q.astype(np.int64)))) if q.size else 0
    return q, clipped, peak


def peak_db(peak, bit_depth):
    """A row's ``peak`` (max |q|) in dBFS of its depth; -inf for an all-zero row."""
    return 20.0 * float(np.log10(peak / 2.0 ** (bit_depth - 1))) if peak > 0 else -float("inf")
