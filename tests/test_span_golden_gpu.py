"""The span limiter and leveller against the bits their kernels gave before the mono and the linked kernel bodies became one
(DESIGN.md 3.18): tests/golden/span_kernels_parent.npz holds, from the build whose ``vfx_build_id`` it names, the float32 outputs,
the limiter records and the leveller states of every case of ``CASES`` -- ops.limit_span / ops.level_span, the ``_rows`` functions
at C = 1 and at C = 3 (limiter) / C = 2 (leveller); whole rows and spans from misaligned windows -- and a SHA-256 of every input.
A case first proves its inputs by their digests, so a drifting generator is not taken for a kernel difference; then every bit
must match.  tools/record_span_golden.py writes the fixture from ``CASES``; it is rerun only when the DEFINITION of a stage changes.

At the recording build a mono call and the ``_rows`` call at C = 1 gave the same bytes (the recorder asserts it), so the fixture
stores each such pair once, under the ``-mono`` name, and both entry points are compared with it.  The leveller's outputs are
stored as a digest plus their first and last ``EDGE`` samples per channel (the file stays small); the limiter's outputs, the
records and the states are stored whole."""
import hashlib
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from voicefixer_amd import _lib, loudness, ops  # noqa: E402
from test_stream_channels_gpu import PAD, _bits, _lspan, _noise, _steps, _vrun, _window  # noqa: E402

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "span_kernels_parent.npz")
EDGE = 4096


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _mono_in(x, lo, hi, off):
    """x[lo:hi] on the device, ``off`` floats past a 16-byte boundary."""
    d = torch.zeros((PAD + 4 + hi - lo,), device="cuda")
    assert d.data_ptr() % 16 == 0
    d[PAD + off:PAD + off + hi - lo] = torch.from_numpy(x[lo:hi]).cuda()
    return d[PAD + off:PAD + off + hi - lo]


def _mono_out(n, off):
    return torch.empty((PAD + 4 + n,), device="cuda")[PAD + off:PAD + off + n]


# ---- the limiter: N = 5000, +6 dB, ceiling -1 dB, 3 ms; peaks at 0, 1023, 2600, 4999 ---------------------------------------------

LN, LGAIN = 5000, 6.0
LMODES = {"tp44": (44100, True), "tp96": (96000, True), "sp44": (44100, False)}       # R = 4, 2, 1


def limiter_inputs():
    """(C = 3, N): the row of test_limiter_one_channel_is_the_mono_kernel, a row whose envelope stays under the threshold, and the
    row reversed."""
    x = _noise(np.random.default_rng(7), LN)
    x[0], x[1023], x[2600], x[4999] = 0.97, -0.95, 0.99, 0.9
    quiet = _noise(np.random.default_rng(8), LN, amp=0.02)
    return np.stack([x, quiet, x[::-1].copy()])


def _limiter_case(mode, span, rows):
    fs, true_peak = LMODES[mode]
    X = limiter_inputs()
    assert (loudness.oversampling(fs) if true_peak else 1) == {"tp44": 4, "tp96": 2, "sp44": 1}[mode]
    if span == "whole":
        m0, m1, lo, hi, known, xoff, ooff = 0, LN, 0, LN, True, 0, 0
    else:                                                     # an interior span, the end unknown, from its minimal window
        H, Bk, Fw = loudness.limiter_reach(fs, 3.0, true_peak)
        m0, m1, known, xoff, ooff = 900, 3000, False, 1, 3
        lo, hi = _window(LN, m0, m1, H, Bk, Fw, known)
    if rows == 0:                                             # ops.limit_span
        out = _mono_out(m1 - m0, ooff)
        rec = ops.limit_span(_mono_in(X[0], lo, hi, xoff), lo, LN if known else None, fs, LGAIN, m0, m1, out, -1.0, true_peak, 3.0)
        return {"out": out.cpu().numpy()[None], "rec": rec.cpu().numpy()}
    gap = 0
    if rows > 1:                                              # a row stride that is no multiple of 4 floats
        gap = 1 if (hi - lo + 1) % 4 else 2
        assert (hi - lo + gap) % 4 and (m1 - m0 + gap) % 4
    out, rec = _lspan(X[:rows], fs, LGAIN, m0, m1, lo, hi, known, true_peak=true_peak, gap=gap, xoff=xoff, ooff=ooff)
    return {"out": out, "rec": rec}


# ---- the leveller: fs = 8000, N = 33 hop + 17 (the state's ring of 32 quarters wraps), target -20 ---------------------------------

VFS, VHOP = 8000, 800
VN = 33 * VHOP + 17


def leveller_inputs():
    """[x, y] of test_leveller_exact."""
    rng = np.random.default_rng(60)
    return np.stack([_steps(rng, VN, VFS), _steps(rng, VN, VFS, (0.1, 0.01, 0.3))])


def _leveller_case(span, rows):
    X = leveller_inputs()
    cuts, gap, xoff, ooff = ((), 0, 0, 0) if span == "whole" else (range(VHOP + 1, VN, VHOP + 1), 5, 2, 3)
    if rows == 0:                                             # ops.level_span
        xw, out = _mono_in(X[0], 0, VN, xoff), _mono_out(VN, ooff)
        state = torch.full((loudness.LEVELLER_STATE,), 7.0, dtype=torch.float64, device="cuda")
        edges = [0] + list(cuts) + [VN]
        for m0, m1 in zip(edges[:-1], edges[1:]):
            ops.level_span(xw, 0, VN, VFS, -20.0, m0, m1, out[m0:m1], state)
        got, st = out.cpu().numpy()[None], state.cpu().numpy()
    else:
        got, st = _vrun(X[:rows], VFS, -20.0, weights=[1.0] if rows == 1 else None, cuts=cuts, gap=gap, xoff=xoff, ooff=ooff)
    return {"sha": np.array(_sha(got)), "head": got[:, :EDGE].copy(), "tail": got[:, -EDGE:].copy(), "state": st}


CASES = {}
for _mode in LMODES:
    for _span in ("whole", "interior"):
        for _rows, _tag in ((0, "mono"), (1, "rows1"), (3, "rows3")):
            CASES["limit-%s-%s-%s" % (_mode, _span, _tag)] = (_limiter_case, (_mode, _span, _rows))
for _span in ("whole", "cut"):
    for _rows, _tag in ((0, "mono"), (1, "rows1"), (2, "rows2")):
        CASES["level-%s-%s" % (_span, _tag)] = (_leveller_case, (_span, _rows))

INPUTS = {"limiter": limiter_inputs, "leveller": leveller_inputs}


def _stored(name):
    """The fixture's name of a case: the C = 1 cases share the arrays of their mono twins."""
    return name[:-len("rows1")] + "mono" if name.endswith("-rows1") else name


def record():
    """Every case's arrays from the build that is loaded (tools/record_span_golden.py saves them, each mono / C = 1 pair once)."""
    arrays = {"build_id": np.array(_lib.lib().vfx_build_id().decode())}
    for name, make in INPUTS.items():
        arrays["input/" + name] = np.array(_sha(make()))
    for name, (fn, args) in CASES.items():
        for key, v in fn(*args).items():
            arrays[name + "/" + key] = v
    return arrays


@pytest.fixture(scope="module")
def golden():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", sorted(CASES))
def test_span_kernels_give_the_recorded_bits(golden, name):
    kind = "limiter" if name.startswith("limit-") else "leveller"
    assert _sha(INPUTS[kind]()) == str(golden["input/" + kind]), "the test's own inputs drifted: not a kernel difference"
    fn, args = CASES[name]
    got = fn(*args)
    assert sorted(_stored(name) + "/" + k for k in got) == sorted(k for k in golden if k.startswith(_stored(name) + "/"))
    for key, v in got.items():
        want = golden[_stored(name) + "/" + key]
        if key == "sha":
            assert str(v) == str(want), (name, key)
        elif v.dtype == np.float32:
            assert v.shape == want.shape and np.array_equal(_bits(v), _bits(want)), (name, key)
        else:                                                 # records and states: float64, bit for bit
            assert v.dtype == want.dtype == np.float64 and np.array_equal(v.view(np.uint64), want.view(np.uint64)), (name, key)
