"""Worker of tests/test_frac_tree_invariants.py: drives sr_frac_tree_dev with the edge leaves of tests/test_frac_tree_gpu.py -- every
leaf word p - 1, every leaf the neutral fraction (zero, one), a single zero denominator among ones and among uniform leaves,
truncated leaves with the non-canonical poison word behind them, no stored numerators, and the one-coefficient path at an odd 8-byte
pointer -- and compares every output with tools/model_frac_tree.py.  `check`: the process was started with SR_LIB_PATH pointing at
the checking build (libstarkrings_hip_check.so), and after every ring the device counters must read zero -- no canonical routine
saw a representative >= p, no word >= p left the library.  `product`: the same calls on the product library, compared with the model
alone."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import model_frac_tree as FT  # noqa: E402

# (ring, log2 D, num_vars): one ring per kernel family, at least two launches each
RINGS = [("goldilocks", 6, 5), ("babybear", 5, 5), ("stark", 4, 4), ("goldilocks24", 0, 5), ("babybear72", 0, 4), ("frog16", 0, 5)]


def main():
    import torch

    from stark_rings_amd import frac_tree_dev, frac_tree_plan
    from test_frac_tree_gpu import GUARD, model_tree
    from test_mle_gpu import POISON, dev, host, model_for

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
        assert frac_tree_plan(ring, nv)[1] >= 2

        def run(p_words, q_words, n, what, shift=0):
            p_els = None if p_words is None else m.elems(p_words)[:n]
            q_els = m.elems(q_words)[:n]
            srcs = []
            for words in (p_words, q_words):
                if words is None:
                    srcs.append(None)
                    continue
                buf = words.copy()
                buf[n * w:] = POISON
                src = torch.zeros(full * w + 2, dtype=torch.int64, device="cuda")
                src[shift:shift + full * w] = dev(torch, buf)
                srcs.append(src[shift:shift + n * w])
            n_out = (full - 1) * w
            for order in (FT.LEADING, FT.TRAILING):
                dst_p = torch.full((n_out + w,), GUARD, dtype=torch.int64, device="cuda")
                dst_q = torch.full((n_out + w,), GUARD, dtype=torch.int64, device="cuda")
                frac_tree_dev(ring, dst_p[:n_out], dst_q[:n_out], srcs[0], srcs[1], nv, order)
                torch.cuda.synchronize()
                want = model_tree(m, p_els, q_els, nv, order)
                for got, wanted, side in ((host(dst_p), want[0], "p"), (host(dst_q), want[1], "q")):
                    assert np.array_equal(got[:n_out], wanted), "%s %s order %d: %s" % (name, what, order, side)
                    assert (got[n_out:] == np.uint64(GUARD)).all(), "%s %s order %d: guard of %s" % (name, what, order, side)

        one, zero, top = m.one(), np.zeros(w, dtype=np.uint64), m.const(m.p - 1, 1)
        up, uq = m.uniform(0x1E00 + nv, full), m.uniform(0x1F00 + nv, full)
        run(np.tile(top, full), np.tile(top, full), full, "all p - 1")
        run(None, np.tile(top, full), full, "all p - 1, no numerators")
        run(np.tile(zero, full), np.tile(one, full), full, "all (zero, one)")
        for z in (0, full - 1):
            words = np.tile(one, full)
            words[z * w:(z + 1) * w] = 0
            run(None, words, full, "a zero denominator at %d among ones" % z)
        words = uq.copy()
        words[5 * w:6 * w] = 0
        run(up, words, full, "a zero denominator among uniform leaves")
        run(np.tile(top, full), np.tile(top, full), full - 3, "truncated p - 1 leaves, poison behind them")
        run(None, np.tile(top, full), full - 3, "truncated p - 1 leaves, no numerators")
        run(up, uq, 1, "one stored leaf")
        run(np.tile(top, full), np.tile(top, full), full, "p - 1 leaves at an odd 8-byte pointer", shift=1)
        if checking:
            expect_clean("%s fraction trees" % name)
        print("%-16s %s" % ("%s-%d" % (name, k), "clean" if checking else "agrees with the model"), flush=True)
    print("frac_tree_invariants: OK", flush=True)


if __name__ == "__main__":
    main()
