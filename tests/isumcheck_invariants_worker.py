"""Worker of tests/test_isumcheck_invariants.py: drives sr_vpoly_iwround_evals_dev and sr_vpoly_iwround_fold_evals_dev with the edge
inputs -- every table, weight and coefficient word p - 1, every column value at or above p where a u64 can be (p, p + 1, 2^64 - 1 and a
progression that ends at 2^64 - 1; the largest values elsewhere), a truncated column -- over the 8-slot and the 4-slot kernels in both
orders, and compares every message and every folded slot with tools/model_isumcheck.py.  `check`: the process was started with
SR_LIB_PATH pointing at the checking build (libstarkrings_hip_check.so), and after every ring the device counters must read zero -- no
canonical routine saw a representative >= p, no word >= p left the library.  `product`: the same calls on the product library,
compared with the model alone."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import model_isumcheck as IS  # noqa: E402

# (ring, log2 D, num_vars): one ring per kernel family
RINGS = [("goldilocks", 6, 3), ("babybear", 5, 3), ("stark", 4, 3), ("goldilocks24", 0, 3), ("babybear72", 0, 2), ("frog16", 0, 3)]
U64 = 1 << 64


def main():
    import torch

    from stark_rings_amd import IndexColumn
    from test_isumcheck_gpu import ints_dev, iwfold, iwround
    from test_mle_gpu import dev, host, model_for
    from test_vpoly_gpu import one_of

    mode = sys.argv[1]
    checking = mode == "check"
    assert checking == os.environ.get("SR_LIB_PATH", "").endswith("_check.so"), "check: run with SR_LIB_PATH=<the checking build>"
    if checking:
        from rep_invariants_worker import counters, expect_clean
    for name, k, nv in RINGS:
        m = model_for(name, k)
        ring = m.ring
        if checking:
            counters()   # building the context uses the same arithmetic: start from zero
        full = 1 << nv
        top = m.const(m.p - 1, 1)
        top_elem = m.elems(top)[0]
        high = [m.p, m.p + 1, U64 - 1] if m.p < U64 else [U64 - 1, U64 - 2, 1 << 63]   # at or above p where a u64 can be
        ops = (m.zero(), one_of(m), m.add, m.sub, m.mul)
        same = lambda t, elems: len(m.elems(host(t))) == len(elems) and all(np.array_equal(a, b) for a, b in zip(m.elems(host(t)), elems))  # noqa: E731
        for sname in ("PLONK", "ALLCOL", "MIXED"):
            K, J, terms = IS.STRUCTURES[sname]
            ints = [[high[(i + j) % 3] % U64 for i in range(full if j != 1 else full - 1)] for j in range(J - 1)] + [IS.Progression(U64 - full)]
            cols = [IndexColumn(start=c.start) if isinstance(c, IS.Progression) else IndexColumn(ints_dev(torch, c)) for c in ints]
            tables = [dev(torch, np.tile(top, full)) for _ in range(K)]
            coeffs = None if sname == "MIXED" else dev(torch, np.tile(top, len(terms)))
            dw, dwf, r = dev(torch, np.tile(top, full // 2)), dev(torch, np.tile(top, full // 4)), dev(torch, top)
            t_el, c_el = [[top_elem] * full for _ in range(K)], None if coeffs is None else [top_elem] * len(terms)
            for order in (0, 1):
                got = iwround(torch, ring, dw, tables, cols, terms, coeffs, nv, order)
                assert same(got, IS.iwround_evals(t_el, ints, terms, c_el, [top_elem] * (full // 2), nv, order, *ops)), (name, sname, order)
                msg, folded, _ = iwfold(torch, ring, dwf, tables, cols, terms, coeffs, nv, r, order)
                want_folded, want_msg = IS.iwfold_round(t_el, ints, terms, c_el, [top_elem] * (full // 4), nv, top_elem, order, *ops)
                assert same(msg, want_msg), (name, sname, order)
                assert len(folded) == K + J and all(same(g, f) for g, f in zip(folded, want_folded)), (name, sname, order)
        if checking:
            expect_clean("%s weighted rounds with integer columns" % name)
        print("%-16s %s" % ("%s-%d" % (name, k), "clean" if checking else "agrees with the model"), flush=True)
    print("isumcheck_invariants: OK", flush=True)


if __name__ == "__main__":
    main()
