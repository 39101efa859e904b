"""Worker of tests/test_prod_tree_invariants.py: drives sr_prod_tree_dev with the edge leaves of tests/test_prod_tree_gpu.py -- every
leaf word p - 1, every leaf zero, every leaf one(), a single zero among ones and among uniform leaves, truncated leaves with the
non-canonical poison word behind them, and the one-coefficient path at an odd 8-byte pointer -- and compares every output with
tools/model_prod_tree.py.  `check`: the process was started with SR_LIB_PATH pointing at the checking build
(libstarkrings_hip_check.so), and after every ring the device counters must read zero -- no canonical routine saw a representative
>= p, no word >= p left the library.  `product`: the same calls on the product library, compared with the model alone."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import model_prod_tree as PT  # noqa: E402

# (ring, log2 D, num_vars): one ring per kernel family, two launches each
RINGS = [("goldilocks", 6, 5), ("babybear", 5, 5), ("stark", 4, 4), ("goldilocks24", 0, 5), ("babybear72", 0, 4), ("frog16", 0, 5)]


def main():
    import torch

    from test_mle_gpu import POISON, dev, host, model_for
    from test_prod_tree_gpu import GUARD, mul, one_elem

    mode = sys.argv[1]
    checking = mode == "check"
    assert checking == os.environ.get("SR_LIB_PATH", "").endswith("_check.so"), "check: run with SR_LIB_PATH=<the checking build>"
    if checking:
        from rep_invariants_worker import counters, expect_clean
    for name, k, nv in RINGS:
        m = model_for(name, k)
        ring, w, full = m.ring, m.w, 1 << nv
        if checking:
            counters()   # building the context uses the same arithmetic: start from zero
        assert ring.prod_tree_plan(nv)[1] == 2

        def run(words, n_leaves, what, shift=0):
            want_els = m.elems(words)[:n_leaves]
            buf = words.copy()
            buf[n_leaves * w:] = POISON
            src = torch.zeros(full * w + 2, dtype=torch.int64, device="cuda")
            src[shift:shift + full * w] = dev(torch, buf)
            n_out = (full - 1) * w
            for order in (PT.LEADING, PT.TRAILING):
                dst = torch.full((n_out + w,), GUARD, dtype=torch.int64, device="cuda")
                ring.prod_tree_dev(dst[:n_out], src[shift:shift + n_leaves * w], nv, order)
                torch.cuda.synchronize()
                want = m.words(PT.flat(PT.layers(want_els, nv, order, one_elem(m), mul(m))))
                got = host(dst)
                assert np.array_equal(got[:n_out], want), "%s %s order %d" % (name, what, order)
                assert (got[n_out:] == np.uint64(GUARD)).all(), "%s %s order %d: guard" % (name, what, order)

        one = m.one()
        uniform = m.uniform(0x1D00 + nv, full)
        for what, leaf in (("all p - 1", m.const(m.p - 1, 1)), ("all zero", np.zeros(w, dtype=np.uint64)), ("all one", one)):
            run(np.tile(leaf, full), full, what)
        for z in (0, full - 1):
            words = np.tile(one, full)
            words[z * w:(z + 1) * w] = 0
            run(words, full, "a zero at %d among ones" % z)
        words = uniform.copy()
        words[5 * w:6 * w] = 0
        run(words, full, "a zero among uniform leaves")
        run(np.tile(m.const(m.p - 1, 1), full), full - 3, "truncated p - 1 leaves, poison behind them")
        run(uniform, 1, "one stored leaf")
        run(np.tile(m.const(m.p - 1, 1), full), full, "p - 1 leaves at an odd 8-byte pointer", shift=1)
        if checking:
            expect_clean("%s product trees" % name)
        print("%-16s %s" % ("%s-%d" % (name, k), "clean" if checking else "agrees with the model"), flush=True)
    print("prod_tree_invariants: OK", flush=True)


if __name__ == "__main__":
    main()
