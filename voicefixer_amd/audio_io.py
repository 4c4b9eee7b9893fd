"""File I/O at the edge of the path (host side, not timed, not on the kernel path).

Mirrors voicefixer/tools/wav.py: ``save_wave`` (:9-37, int16 truncation) and the
``librosa.load(path, sr=44100)`` call of voicefixer/base.py:47-49.  librosa / soundfile are not
available offline, so WAV files are read with scipy/stdlib, FLAC files (the format of the reference's own
test fixtures, test/test.py:45-75) with the decoder / encoder of ``flac.py``, and other sample rates are resampled with a
linear-phase polyphase filter designed to the published soxr "HQ" recipe librosa.load uses by default (pass band to
0.913 of the lower Nyquist frequency, stop band from that Nyquist frequency on, 125 dB rejection: ``resample_hq``).  Same
grade, not the same coefficients: resampled inputs agree with the reference's to the filter ripple, not bit for bit;
44.1 kHz inputs are untouched.
"""
import struct

import numpy as np

SR = 44100
FORMATS = (".wav", ".flac")   # what ``save_wave`` can write (the reference asks soundfile.available_formats())


def to_int16(frames):
    """voicefixer/tools/wav.py:27-34: x * 2^15 if max <= 1, then a truncating astype(np.short)
    (no rounding, no dither; values outside int16 wrap exactly like numpy's cast)."""
    frames = np.array(frames, copy=True)
    if np.max(frames) <= 1 and frames.dtype in (np.float32, np.float16, np.float64):
        frames = frames * 2 ** 15
    with np.errstate(invalid="ignore"):
        return frames.astype(np.short)


def save_wave(frames, fname, sample_rate=SR, channels_first=False):
    """(1, N) or (N,) float waveform -> PCM16 WAV or FLAC by extension (voicefixer/tools/wav.py:9-37 writes through
    soundfile, which picks the container from the extension the same way).  ``channels_first=True``: ``frames`` is
    (channels, N) with 1..8 channels whatever N (what ``load_wav(mono=False)`` and the multichannel restore calls return);
    without it only (1, N) and (2, N) are recognised as channels-first, as the reference does."""
    frames = np.asarray(frames)
    if channels_first:
        if frames.ndim != 2 or not 1 <= frames.shape[0] <= 8:
            raise ValueError("save_wave: channels_first takes (channels, N) with 1..8 channels (got shape %r)" % (frames.shape,))
        frames = frames.T
    elif frames.ndim == 1:
        frames = frames[..., None]
    elif frames.ndim == 2 and frames.shape[0] < frames.shape[1] and frames.shape[0] <= 2:
        frames = frames.T  # (channels, N) -> (N, channels), as the reference's (1, N) output
    pcm = to_int16(frames)
    low = str(fname).lower()
    if low.endswith(".flac"):
        from . import flac
        flac.write(fname, pcm, sample_rate, 16)
        return
    if not low.endswith(".wav"):
        raise RuntimeError("output format not supported offline (WAV and FLAC are; the reference writes via "
                           "soundfile): %s" % fname)
    from scipy.io import wavfile
    wavfile.write(fname, sample_rate, pcm if pcm.shape[1] > 1 else pcm[:, 0])


def _write_wav24(fname, pcm, sample_rate):
    """int (N, channels) inside the signed 24-bit range -> RIFF/WAVE with packed 3-byte little-endian samples: a plain PCM
    ``fmt `` chunk for one or two channels, WAVE_FORMAT_EXTENSIBLE (sub-format PCM, no speaker positions assigned) for more."""
    n, nch = pcm.shape
    raw = np.ascontiguousarray(pcm, dtype="<i4").view(np.uint8).reshape(n, nch, 4)[:, :, :3].tobytes()
    align = 3 * nch
    if nch <= 2:
        fmt = struct.pack("<HHIIHH", 1, nch, sample_rate, sample_rate * align, align, 24)
    else:
        pcm_guid = b"\x01\x00\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71"
        fmt = struct.pack("<HHIIHHHHI", 0xFFFE, nch, sample_rate, sample_rate * align, align, 24, 22, 24, 0) + pcm_guid
    pad = b"\x00" * (len(raw) & 1)
    if 4 + 8 + len(fmt) + 8 + len(raw) + len(pad) > 0xFFFFFFFF:
        raise RuntimeError("too long for a RIFF/WAVE file (4 GB): %s" % fname)
    with open(fname, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 4 + 8 + len(fmt) + 8 + len(raw) + len(pad)) + b"WAVE")
        f.write(b"fmt " + struct.pack("<I", len(fmt)) + fmt)
        f.write(b"data" + struct.pack("<I", len(raw)))
        f.write(raw)
        f.write(pad)


def save_pcm(pcm, fname, sample_rate, bit_depth, channels_first=False):
    """Integer PCM (what the restore calls return with ``bit_depth=``: int16 at 16 bits, int32 at 24) -> WAV or FLAC of that
    depth by extension, sample for sample: nothing is scaled, rounded or truncated here (``save_wave`` is the float path and
    stays the reference's).  Shapes as ``save_wave``: (N,), (1, N), (2, N), or with ``channels_first`` (channels, N), 1..8
    channels.  Values outside the signed ``bit_depth``-bit range raise ValueError."""
    from . import wordlength
    bit_depth = wordlength.check_bit_depth(bit_depth)
    pcm = np.asarray(pcm)
    if pcm.dtype.kind != "i":
        raise ValueError("save_pcm takes integer PCM (got %s); float waveforms go through save_wave" % pcm.dtype)
    if channels_first:
        if pcm.ndim != 2 or not 1 <= pcm.shape[0] <= 8:
            raise ValueError("save_pcm: channels_first takes (channels, N) with 1..8 channels (got shape %r)" % (pcm.shape,))
        pcm = pcm.T
    elif pcm.ndim == 1:
        pcm = pcm[..., None]
    elif pcm.ndim == 2 and pcm.shape[0] < pcm.shape[1] and pcm.shape[0] <= 2:
        pcm = pcm.T
    if pcm.ndim != 2:
        raise ValueError("save_pcm: PCM is (N,) or two-dimensional (got shape %r)" % (pcm.shape,))
    if pcm.size and (pcm.min() < -(1 << (bit_depth - 1)) or pcm.max() > (1 << (bit_depth - 1)) - 1):
        raise ValueError("save_pcm: samples outside the signed %d-bit range" % bit_depth)
    low = str(fname).lower()
    if low.endswith(".flac"):
        from . import flac
        flac.write(fname, pcm, sample_rate, bit_depth)
        return
    if not low.endswith(".wav"):
        raise RuntimeError("output format not supported offline (WAV and FLAC are): %s" % fname)
    if bit_depth == 16:
        from scipy.io import wavfile
        pcm = pcm.astype(np.int16)
        wavfile.write(fname, sample_rate, pcm if pcm.shape[1] > 1 else pcm[:, 0])
        return
    _write_wav24(fname, pcm, int(sample_rate))


def _riff_info(path, channels=False):
    """(sample_rate, frames, frames the header promises) of a RIFF/WAVE file from its ``fmt `` and ``data`` chunk headers alone
    -- any bit depth (scipy's memory-mapped read refuses 24-bit PCM, a very common studio format).  ``channels``: the channel
    count of the ``fmt `` chunk instead."""
    with open(path, "rb") as f:
        head = f.read(12)
        if len(head) < 12 or head[:4] not in (b"RIFF", b"RF64") or head[8:12] != b"WAVE":
            raise RuntimeError("not a RIFF/WAVE file: %s" % path)
        sr = block_align = None
        while True:
            ck = f.read(8)
            if len(ck) < 8:
                raise RuntimeError("WAV file without a data chunk: %s" % path)
            cid, size = ck[:4], struct.unpack("<I", ck[4:])[0]
            if cid == b"fmt ":
                fmt = f.read(size + (size & 1))
                _, nch, sr, _, block_align, _ = struct.unpack("<HHIIHH", fmt[:16])
                if channels:
                    return int(nch)
            elif cid == b"data":
                if not block_align:
                    raise RuntimeError("WAV data chunk before the fmt chunk: %s" % path)
                # the header PLANS (staging width of the folder job): never believe more than the file can hold -- a streamed /
                # RF64 file says 0xFFFFFFFF, a truncated or lying one promises bytes that are not there
                pos = f.tell()
                f.seek(0, 2)
                real = min(size, f.tell() - pos)
                return int(sr), int(real // block_align), int((real if size == 0xFFFFFFFF else size) // block_align)
            else:
                f.seek(size + (size & 1), 1)


def wav_info(path):
    """(sample rate, samples, samples the header PROMISES) of a WAV / FLAC file at its own rate, from the header (and the
    file size) alone."""
    promised = None
    if str(path).lower().endswith(".flac"):
        from . import flac
        sr, _, _, n = flac.info(path)
        # STREAMINFO's total is a promise; a frame holds at most 65535 samples per channel in no fewer than ~8 bytes, which bounds
        # what a file of this size can decode to (the folder job sizes pinned staging from this number)
        import os
        if n == 0 or n > (os.path.getsize(path) // 8 + 1) * 65535:      # 0: legal for streamed encoders (unknown length)
            n = flac.read(path)[1].shape[0]     # count what is really there
    else:
        sr, n, promised = _riff_info(path)
    return int(sr), n, (n if promised is None else promised)


def wav_channels(path):
    """Channel count of a WAV / FLAC file from its header alone."""
    if str(path).lower().endswith(".flac"):
        from . import flac
        return int(flac.info(path)[1])
    return _riff_info(path, channels=True)


def select_channels(x, channels):
    """What a ``channels=`` argument makes of a decoded file (``load_wav(mono=False)``: (N,) or (C, N)): None / "mix": the
    average of the channels (librosa's down-mix), (N,); "first": channel 0, (N,); "all": every channel, (C, N)."""
    x = np.asarray(x)
    if channels == "all":
        return x[None] if x.ndim == 1 else x
    if x.ndim == 1:
        return x
    return np.ascontiguousarray(x[0]) if channels == "first" else x.mean(axis=0)


def wav_length(path, sample_rate=SR, with_promise=False):
    """Number of samples ``load_wav(path, sample_rate)`` will return, from the file header (and the file size) alone;
    ``with_promise``: (that number, the number the header PROMISES) -- they differ for a truncated recording."""
    sr, n, promised = wav_info(path)
    if sr != sample_rate:
        n, promised = converted_length(n, sr, sample_rate), converted_length(promised, sr, sample_rate)  # ceil(n * up / down)
    return (n, promised) if with_promise else n


_HQ_FILTERS = {}

# largest max(up, down) the device resampler takes (api: larger reduced ratios -- no standard rate pair comes close -- are
# converted by resample_hq on the host, file by file)
DEVICE_MAX_RATIO = 1024


def rate_ratio(sr_in, sr_out):
    """(up, down): the reduced ratio sr_out / sr_in of a conversion."""
    from math import gcd
    g = gcd(int(sr_in), int(sr_out))
    return int(sr_out) // g, int(sr_in) // g


def converted_length(n, sr_in, sr_out):
    """Samples a conversion of n samples returns: ceil(n * up / down) (resample_poly's length)."""
    up, down = rate_ratio(sr_in, sr_out)
    return -(-int(n) * up // down)


def hq_filter(up, down):
    """The Kaiser-windowed sinc behind ``resample_hq`` at the common rate up * fs_in: (h float64 with unit DC gain,
    g = float32(h * up)).  Pass band edge 0.913 and stop band edge 1.0 of the lower of the two Nyquist frequencies,
    125 dB (beta = 0.1102 (A - 8.7), length from Kaiser's estimate, odd: zero phase).  Cached per (up, down); the host
    resampler and the device bank (polyphase_bank) are built from this one design."""
    h = _HQ_FILTERS.get((up, down))
    if h is None:
        from scipy.signal import firwin
        m = max(up, down)                      # the lower Nyquist frequency is 1 / m of the common rate's
        att, f_pass, f_stop = 125.0, 0.913 / m, 1.0 / m
        taps = int(np.ceil((att - 7.95) / (2.285 * np.pi * (f_stop - f_pass)))) | 1    # odd: zero phase
        h = firwin(taps, 0.5 * (f_pass + f_stop), window=("kaiser", 0.1102 * (att - 8.7)))       # (unit DC gain; the gain `up` is applied below)
        h = (h, np.ascontiguousarray(h * up, dtype=np.float32))
        _HQ_FILTERS[(up, down)] = h
    return h


def polyphase_bank(g, up):
    """The per-phase tap layout of the polyphase sum (csrc_host/vfx_resample.c, vfx_resample_rows_f32): bank [up, J],
    bank[p][i] = g[p + (J - 1 - i) * up] (phase p's taps reversed, zero past the filter's end), J = ceil(L / up) taps per
    phase, c = (L - 1) / 2 the filter's centre.  Returns (bank in g's dtype, J, c)."""
    g = np.asarray(g)
    L = g.shape[0]
    J = -(-L // up)
    gp = np.zeros(up * J, dtype=g.dtype)
    gp[:L] = g
    bank = np.ascontiguousarray(gp.reshape(J, up).T[:, ::-1])      # [p][j] = g[p + j*up], then j -> J - 1 - i
    return bank, J, (L - 1) // 2


def hq_bank(up, down):
    """(bank float32 [up, J], J, c): the per-phase layout of ``hq_filter(up, down)``'s float32 taps -- exactly what the host
    resampler builds from the same taps inside vfx_resample_poly_f32; ops.resample_rows uploads it once per device."""
    return polyphase_bank(hq_filter(up, down)[1], up)


def ready_outputs(avail, up, down, c):
    """Leading outputs of the polyphase sum (vfx_resample_rows_f32) that read nothing at or past sample ``avail``: those with
    kmax(m) = (c + m * down) // up < avail.  A streaming converter may emit them before the row's end is known."""
    t = int(avail) * up - 1 - c
    return 0 if t < 0 else t // down + 1


def span_window(m0, m1, up, down, J, c):
    """(lo(m0), kmax(m1 - 1) + 1): the unclipped range of input samples that outputs [m0, m1), m1 > m0, of the polyphase sum
    read (lo(m) = kmax(m) - J + 1; both grow with m)."""
    return (c + int(m0) * down) // up - J + 1, (c + (int(m1) - 1) * down) // up + 1


def resample_hq(x, sr_in, sr_out, use_native=None):
    """Band-limited rate conversion along the last axis, ceil(n * sr_out / sr_in) samples (librosa.load(sr=...) ->
    soxr_hq).  The filter of ``hq_filter`` applied as a polyphase filter: one dot product per output sample in
    libvfx_audio.so (vfx_resample_poly_f32: float32, several times scipy's speed and without the interpreter lock, so the
    folder driver's workers scale), or scipy's upfirdn in float64 when that library is not built / ``use_native=False``
    (the two agree to float32 rounding).  The device form of the same sum is ops.resample_rows."""
    up, down = rate_ratio(sr_in, sr_out)
    h = hq_filter(up, down)
    from . import flac
    lib = flac.native() if use_native in (None, True) else None
    x = np.asarray(x)
    if lib is not None and x.shape[-1] > 0:
        import ctypes
        f32p = ctypes.POINTER(ctypes.c_float)
        xin = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, x.shape[-1])
        n = xin.shape[1]
        ny = -(-n * up // down)
        out = np.empty((xin.shape[0], ny), dtype=np.float32)
        for r in range(xin.shape[0]):
            rc = lib.vfx_resample_poly_f32(xin[r].ctypes.data_as(f32p), n, h[1].ctypes.data_as(f32p), h[1].shape[0], up, down,
                                           out[r].ctypes.data_as(f32p), ny)
            if rc:
                raise RuntimeError("vfx_resample_poly_f32 failed (%d)" % rc)
        return out.reshape(x.shape[:-1] + (ny,))
    from scipy.signal import resample_poly
    return resample_poly(np.asarray(x, dtype=np.float64), up, down, axis=-1, window=h[0]).astype(np.float32)


def load_wav_native(path, mono=True):
    """Decode + downmix at the file's own rate: (float32 samples in [-1, 1], sample rate)."""
    low = str(path).lower()
    if low.endswith(".flac"):
        from . import flac
        sr, pcm, bps = flac.read(path)
        x = pcm.astype(np.float32) / float(1 << (bps - 1))     # soundfile's float conversion
        x = x[:, 0] if x.shape[1] == 1 else x
    elif low.endswith(".wav"):
        from scipy.io import wavfile
        sr, data = wavfile.read(path)
        if data.dtype == np.int16:
            x = data.astype(np.float32) / 32768.0
        elif data.dtype == np.int32:
            x = data.astype(np.float32) / 2147483648.0      # (scipy delivers 24-bit PCM left-justified in int32)
        elif data.dtype == np.uint8:
            x = (data.astype(np.float32) - 128.0) / 128.0
        else:
            x = data.astype(np.float32)
    else:
        raise RuntimeError("input format not supported offline (WAV and FLAC are): %s" % path)
    if x.ndim == 2:
        x = x.mean(axis=1) if mono else x.T
    return x, int(sr)


def load_wav(path, sample_rate=SR, mono=True):
    """Decode + (if needed) resample + downmix, float32 in [-1, 1] (librosa.load semantics)."""
    x, sr = load_wav_native(path, mono)
    if sr != sample_rate:
        x = resample_hq(x, sr, sample_rate)
    return np.ascontiguousarray(x, dtype=np.float32)
