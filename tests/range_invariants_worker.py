"""Worker of tests/test_range_invariants.py: drives sr_range_wround_evals_dev with the largest inputs the call can hold -- every table,
weight and coefficient word p - 1, eight tables, bound 8, over enough pairs that every lazy sum is reduced in mid-pass -- plus a truncated
and a uniform case, and compares every output with tools/model_range.py.  `check`: the process was started with SR_LIB_PATH pointing at
the checking build (libstarkrings_hip_check.so), and after every ring the device counters must read zero -- no canonical routine saw a
representative >= p, no word >= p left the library.  `product`: the same calls on the product library, compared with the model alone."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import model_range as R  # noqa: E402

# (ring, log2 D, num_vars of the all-(p - 1) case: two records, sixteen pairs per lane): one ring per kernel family
RINGS = [("goldilocks", 1, 14), ("babybear", 1, 14), ("stark", 1, 13), ("goldilocks24", 0, 11), ("babybear72", 0, 11), ("frog16", 0, 12)]
LEADING, TRAILING = 0, 1


def main():
    import torch

    from test_mle_gpu import dev, host, model_for
    from test_range_gpu import model_message, range_dev
    from test_vpoly_gpu import one_of

    mode = sys.argv[1]
    checking = mode == "check"
    assert checking == os.environ.get("SR_LIB_PATH", "").endswith("_check.so"), "check: run with SR_LIB_PATH=<the checking build>"
    if checking:
        from rep_invariants_worker import counters, expect_clean
    for name, k, nv in RINGS:
        m = model_for(name, k)
        ring, w, bound = m.ring, m.w, 8
        if checking:
            counters()   # building the context uses the same arithmetic: start from zero
        pairs = 1 << (nv - 1)
        top = m.const(m.p - 1, 1)
        e = m.elems(top)[0]
        one_pair = R.wround_evals([[e, e]] * 8, bound, [e] * 8, [e], 1, LEADING, m.zero(), one_of(m), m.add, m.sub, m.mul)[0]
        want = m.words([(one_pair * pairs) % m.p]) if m.pow2 else ((one_pair.astype(object) * pairs) % m.p).astype(np.uint64)
        table = dev(torch, np.tile(top, 2 * pairs))
        for order in (LEADING, TRAILING):
            got = host(range_dev(torch, ring, table[:pairs * w], [table] * 8, bound, table[:8 * w], nv, order))
            assert np.array_equal(got, np.tile(want, 2 * bound)), (name, order)
        # truncated tables of p - 1 and uniform ones, three variables, against the model
        for words, cw, ww in (([np.tile(top, n) for n in (8, 5, 0, 3)], np.tile(top, 4), np.tile(top, 4)),
                              ([m.uniform(0x1A40 + j, n) for j, n in enumerate((8, 7, 1, 4))], m.uniform(0x1A50, 4), m.uniform(0x1A51, 4))):
            for order in (LEADING, TRAILING):
                for b in (2, 8):
                    got = range_dev(torch, ring, dev(torch, ww), [dev(torch, t) for t in words], b, dev(torch, cw), 3, order)
                    assert np.array_equal(host(got), m.words(model_message(m, words, b, cw, ww, 3, order))), (name, order, b)
        if checking:
            expect_clean("%s range-check rounds" % name)
        print("%-16s %s" % ("%s-%d" % (name, k), "clean" if checking else "agrees with the model"), flush=True)
    print("range_invariants: OK", flush=True)


if __name__ == "__main__":
    main()
