"""Seeded dropout of the train-mode restorer (mode 2): the specification ``vfx_dropout_f32`` implements.

The reference's two active ``nn.Dropout(0.5)`` layers (restorer/model.py:75 ``denoiser.5`` after Linear 4, and :92
``denoiser.12`` after Linear 11) draw from torch's unseeded generator, so no run of the reference can be repeated.  Here the
masks are a documented function of a 64-bit seed instead:

  * Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11), key = (seed & 0xffffffff,
    seed >> 32);
  * dropout layer ``l`` (0 = denoiser.5, 1 = denoiser.12), segment ``s`` of its file (30 s segments, 0-based), frame ``t``,
    feature ``c`` (0..511): i = t * 512 + c; the element uses word i % 4 of philox(counter = (i // 4, s, l, 0), key);
  * it is dropped (0) if that word is < 2**31, and kept x2 otherwise.

The masks depend on neither the batch position nor padding.  They cannot reproduce torch's own dropout stream (which the
reference never seeds).  Tests and golden generation call ``mask``; the device kernel must agree with it bit for bit.
"""
import numpy as np

M0, M1 = np.uint32(0xD2511F53), np.uint32(0xCD9E8D57)
W0, W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
FEATURES = 512
LAYERS = ("denoiser.5", "denoiser.12")


def _mulhilo(a, b):
    p = a.astype(np.uint64) * np.uint64(b)
    return (p >> np.uint64(32)).astype(np.uint32), (p & np.uint64(0xffffffff)).astype(np.uint32)


def philox4x32_10(ctr, key):
    """Philox4x32-10 on counters ``ctr`` (uint32 array (..., 4)) with ``key`` (two uint32, broadcast): uint32 (..., 4)."""
    c = np.array(ctr, dtype=np.uint32)
    c0, c1, c2, c3 = (c[..., k].copy() for k in range(4))
    k0, k1 = np.uint32(key[0]), np.uint32(key[1])
    with np.errstate(over="ignore"):
        for r in range(10):
            hi0, lo0 = _mulhilo(c0, M0)
            hi1, lo1 = _mulhilo(c2, M1)
            c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
            k0, k1 = np.uint32(k0 + W0), np.uint32(k1 + W1)
    return np.stack([c0, c1, c2, c3], axis=-1)


def key_of(seed):
    """The Philox key of a seed (an int in [0, 2**64))."""
    seed = check_seed(seed)
    return seed & 0xffffffff, seed >> 32


def check_seed(seed):
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
        raise TypeError("seed must be an int in [0, 2**64), got %r" % (seed,))
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError("seed must be in [0, 2**64), got %d" % seed)
    return seed


def mask(seed, segment, layer, T, C=FEATURES):
    """Keep-mask of dropout layer ``layer`` for ``segment`` of a file: float32 (T, C), 0 (dropped) or 2 (kept, scaled)."""
    key = key_of(seed)
    i = np.arange(T * C, dtype=np.uint64)
    q = (i // np.uint64(4)).astype(np.uint32)
    ctr = np.stack([q, np.full_like(q, segment), np.full_like(q, layer), np.zeros_like(q)], axis=-1)
    words = philox4x32_10(ctr, key)
    w = words[np.arange(T * C), (i % np.uint64(4)).astype(np.int64)]
    return np.where(w < np.uint32(1 << 31), 0.0, 2.0).astype(np.float32).reshape(T, C)
