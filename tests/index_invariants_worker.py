"""Worker of tests/test_index_invariants.py: drives sr_lincomb_index_dev with the edge inputs of tests/test_lincomb_index_gpu.py --
every column value >= p on Goldilocks (p, p + 1, 2^64 - 1 and a progression that ends at 2^64 - 1; the largest values elsewhere),
every table and coefficient word p - 1 at K + J = 16, truncated columns with poison behind them, masked rows whose dropped
coefficients hold 0xFF.. words, both kernels, several launches, and the one-coefficient path at an odd 8-byte pointer -- and compares
every output with tools/model_lincomb_index.py.  `check`: the process was started with SR_LIB_PATH pointing at the checking build
(libstarkrings_hip_check.so), and after every ring the device counters must read zero -- no canonical routine saw a representative
>= p, no word >= p left the library.  `product`: the same calls on the product library, compared with the model alone."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import model_lincomb_index as LI  # noqa: E402

# (ring, log2 D, n): one ring per kernel family
RINGS = [("goldilocks", 6, 7), ("babybear", 5, 7), ("stark", 4, 5), ("goldilocks24", 0, 9), ("babybear72", 0, 9), ("frog16", 0, 9)]
U64 = 1 << 64


def main():
    import torch

    from test_lincomb_index_gpu import draw, run, stored
    from test_mle_gpu import model_for

    mode = sys.argv[1]
    checking = mode == "check"
    assert checking == os.environ.get("SR_LIB_PATH", "").endswith("_check.so"), "check: run with SR_LIB_PATH=<the checking build>"
    if checking:
        from rep_invariants_worker import counters, expect_clean
    for name, k, n in RINGS:
        m = model_for(name, k)
        if checking:
            counters()   # building the context uses the same arithmetic: start from zero
        top = m.const(m.p - 1, 1)
        high = [m.p, m.p + 1, U64 - 1] if m.p < U64 else [U64 - 1, U64 - 2, 1 << 63]   # at or above p where a u64 can be
        big = [[high[(i + j) % 3] % U64 for i in range(n)] for j in range(8)]
        for K, J, M in ((8, 8, 1), (8, 8, 4), (15, 1, 1), (2, 2, 1), (1, 2, 2), (0, 1, 1)):
            T = K + J
            tw = [np.tile(top, n) for _ in range(K)]
            cols = big[:J - 1] + [LI.Progression(U64 - n)]
            run(torch, m, tw, cols, np.tile(top, M * (T + 1)), [(2 << T) - 1] * M, n)
        tw = [np.tile(top, e) for e in (n - 1, n)]
        cols = [stored(m, n, 0x77, e) for e in (0, 1, n - 1)]
        run(torch, m, tw, cols, np.tile(top, 6), [0b111111], n)                              # truncated, poison behind the stored parts
        run(torch, m, tw, cols, np.tile(top, 12), [0b110101, 0b001010], n)                   # masked: the dropped entries hold 0xFF.. words
        run(torch, m, tw, cols, np.tile(top, 12), [0b110101, 0b001010], n, shift=1)          # the one-coefficient path
        tu, cu = draw(m, 1, 2, 2, n, seed=0x1DB0)
        run(torch, m, tu, [LI.Progression(0), big[0]], cu, [0b1011, 0b1101], n)
        if checking:
            expect_clean("%s linear combinations with integer columns" % name)
        print("%-16s %s" % ("%s-%d" % (name, k), "clean" if checking else "agrees with the model"), flush=True)
    print("index_invariants: OK", flush=True)


if __name__ == "__main__":
    main()
