"""Worker of tests/test_lincomb_invariants.py: drives sr_lincomb_dev with the edge inputs of tests/test_lincomb_gpu.py -- every table
and coefficient word p - 1 over sixteen tables plus the constant (the largest sum a lazy accumulator of the call can hold), all-zero
coefficients, truncated tables with the non-canonical poison word behind them, masked rows whose dropped coefficients hold 0xFF..
words, both kernels, several launches, and the one-coefficient path at an odd 8-byte pointer -- and compares every output with
tools/model_lincomb.py.  `check`: the process was started with SR_LIB_PATH pointing at the checking build
(libstarkrings_hip_check.so), and after every ring the device counters must read zero -- no canonical routine saw a representative
>= p, no word >= p left the library.  `product`: the same calls on the product library, compared with the model alone."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import model_lincomb as LC  # noqa: E402

# (ring, log2 D, n): one ring per kernel family
RINGS = [("goldilocks", 6, 7), ("babybear", 5, 7), ("stark", 4, 5), ("goldilocks24", 0, 9), ("babybear72", 0, 9), ("frog16", 0, 9)]


def main():
    import torch

    from test_lincomb_gpu import draw, run
    from test_mle_gpu import model_for

    mode = sys.argv[1]
    checking = mode == "check"
    assert checking == os.environ.get("SR_LIB_PATH", "").endswith("_check.so"), "check: run with SR_LIB_PATH=<the checking build>"
    if checking:
        from rep_invariants_worker import counters, expect_clean
    for name, k, n in RINGS:
        m = model_for(name, k)
        w = m.w
        if checking:
            counters()   # building the context uses the same arithmetic: start from zero
        top = m.const(m.p - 1, 1)
        for K, M in ((16, 1), (16, 4), (4, 1), (4, 2)):
            tw = [np.tile(top, n) for _ in range(K)]
            run(torch, m, tw, np.tile(top, M * (K + 1)), [LC.full_mask(K)] * M, n)
            run(torch, m, tw, np.zeros(M * (K + 1) * w, dtype=np.uint64), [LC.full_mask(K)] * M, n)
        tw = [np.tile(top, e) for e in (0, 1, n - 1, n, n - 1)]
        run(torch, m, tw[:4], np.tile(top, 5), [LC.full_mask(4)], n)                       # truncated, poison behind the stored parts
        run(torch, m, tw, np.tile(top, 12), [0b110101, 0b001010], n)                       # masked: the dropped entries hold 0xFF.. words
        run(torch, m, tw, np.tile(top, 12), [0b110101, 0b001010], n, shift=1)              # the one-coefficient path
        tu, cu = draw(m, 3, 2, n, seed=0x1CB0)
        run(torch, m, tu, cu, [0b1011, 0b1101], n)
        if checking:
            expect_clean("%s linear combinations" % name)
        print("%-16s %s" % ("%s-%d" % (name, k), "clean" if checking else "agrees with the model"), flush=True)
    print("lincomb_invariants: OK", flush=True)


if __name__ == "__main__":
    main()
