#!/usr/bin/env python
"""Record what the span limiter and leveller of the loaded build give on the cases of tests/test_span_golden_gpu.py (needs the
GPU): float32 outputs, limiter records, leveller states, a SHA-256 of every input and the build's ``vfx_build_id``.

    python tools/record_span_golden.py [--out tests/golden/span_kernels_parent.npz]

The committed fixture comes from the last build that had separate mono and linked kernel bodies; a change that is meant to keep
the bits runs the test against it and does NOT record again.  Record again only when the definition of a stage changes."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "span_kernels_parent.npz"))
    args = ap.parse_args(argv)
    import test_span_golden_gpu as cases
    arrays = cases.record()
    for key in [k for k in arrays if cases._stored(k.split("/")[0]) != k.split("/")[0]]:      # a C = 1 case: stored as its mono twin
        name = key.split("/")[0]
        a, b = arrays.pop(key), arrays[cases._stored(name) + key[len(name):]]
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (key, "mono and C = 1 differ")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **arrays)
    print("%s: %d arrays of %d cases, %d bytes, build %s" % (args.out, len(arrays), len(cases.CASES), os.path.getsize(args.out),
                                                            arrays["build_id"]))


if __name__ == "__main__":
    main()
