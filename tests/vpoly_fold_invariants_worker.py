"""Worker of tests/test_vpoly_fold_invariants.py: drives sr_vpoly_round_fold_evals_dev with operands that put its INTERMEDIATE words on
the borders of their number formats and compares every output with the integer models.  `check`: the process was started with
SR_LIB_PATH pointing at the checking build (libstarkrings_hip_check.so), and after every group the device counters must read zero --
no canonical routine saw a representative >= p, no lazy sum wrapped twice, no word >= p left the library.  `product`: the same calls
on the product library, compared with the model alone.

The operands come from tests/crafted_poly_operands.py: the folded tables of a call are craft_vpoly's tables of num_vars - 1 variables,
the tables handed in are their preimages under a crafted challenge r (what craft_fold_round does for a product); and the all-(p - 1)
edge tables with r = p - 1 and every coefficient p - 1, through R1CS and the eight terms of model_vpoly.MIXED."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import crafted_poly_operands as C  # noqa: E402
import model_vpoly_fold as VF  # noqa: E402

LEADING, TRAILING = C.LEADING, C.TRAILING
SMALL_NV = 5    # the eight-term structure and the short tables: a single record in every ring


def craft_vpoly_fold(o, nv, structure, order, seed=0):
    """-> (tables of 2^nv, terms, coeffs, r): the fused call's folded tables are craft_vpoly(nv - 1)'s.  In the rings of slots the
    tables that multiply stay per-slot scalars because hi is scalarised with them (craft_fold_round)."""
    folded, terms, coeffs, _ = C.craft_vpoly(o, nv - 1, structure, order, seed)
    rng = C.rng_for("vpolyfold", o.name, o.k, nv, structure, order, seed)
    r = o.scalar(o.rnd(rng, nonzero=True))
    r = np.where(r == o.ONE, 2, r) if o.slotw == 1 else r
    tables = []
    for j, f in enumerate(folded):
        t = C.preimage(o, f, nv - 1, r, order, seed + j)
        if 0 < j < 4 and o.slotw > 1:   # a, b, c multiply; e is the full factor and g (THREE) stands alone
            rr = o.eff(r) * o.Rinv % o.p
            den = o.inv((1 - rr) % o.p)
            for b, (lo_i, hi_i) in enumerate(C.first_pairs(nv, order)):
                t[hi_i] = o.scalar(t[hi_i])
                t[lo_i] = o.scalar((f[b] - rr * t[hi_i]) * den % o.p)
        tables.append(t)
    return tables, terms, coeffs, r


def main():
    import torch

    import crafted_poly_driver as D
    from test_vpoly_fold_gpu import vfold_dev

    mode = sys.argv[1]
    checking = mode == "check"
    assert checking == os.environ.get("SR_LIB_PATH", "").endswith("_check.so"), "check: run with SR_LIB_PATH=<the checking build>"
    if checking:
        from rep_invariants_worker import counters, expect_clean
    paths = set()
    for name, k, nv in C.POLY_CASES:
        run = D.Run(torch, name, k)
        o, ring, cols = run.o, run.ring, run.cols
        if checking:
            counters()   # building the context uses the same arithmetic: start from zero

        def call(tables, terms, coeffs, nv_, r, order, what, put=D.dev):
            msg, got, _ = vfold_dev(torch, ring, [put(torch, o.words(t)) for t in tables], terms, put(torch, o.words(coeffs)), nv_,
                                    D.dev(torch, o.words([r])), order)
            torch.cuda.synchronize()
            paths.add(ring.vpoly_round_fold_plan(nv_, len(tables), len(terms), max(len(t) for t in terms), order)[1] == 1)
            folded, message = VF.fold_round([C.cut(o, t, cols) for t in tables], terms, C.cut(o, coeffs, cols), nv_, C.cut(o, [r], cols)[0], order,
                                            o.zero, o.one, o.add, o.sub, o.mul)
            run.same(msg, message, what + " (message)")
            for g, f in zip(got, folded):
                run.same(g, f, what + " (folded table)")

        for structure in ("R1CS", "THREE"):
            for order in (LEADING, TRAILING):
                tables, terms, coeffs, r = craft_vpoly_fold(o, nv, structure, order)
                call(tables, terms, coeffs, nv, r, order, "crafted %s order %d" % (structure, order))
        tables, terms, coeffs, r = craft_vpoly_fold(o, nv, "R1CS", TRAILING, seed=1)
        call([t[:(1 << nv) - 3] for t in tables], terms, coeffs, nv, r, TRAILING, "truncated crafted R1CS")
        tables, terms, coeffs, r = craft_vpoly_fold(o, SMALL_NV, "R1CS", LEADING, seed=2)
        call(tables, terms, coeffs, SMALL_NV, r, LEADING, "short crafted R1CS")
        tables, terms, coeffs, r = craft_vpoly_fold(o, nv, "R1CS", LEADING, seed=3)
        call(tables, terms, coeffs, nv, r, LEADING, "crafted R1CS at odd 8-byte pointers", put=D.shifted)
        if checking:
            expect_clean("%s crafted operands" % name)
        # every table word, every word of r and of every coefficient p - 1: the largest operands of every product and lazy sum
        top = o.lanes_of(o.p - 1)
        edge = [top] * (1 << nv)
        for order in (LEADING, TRAILING):
            call([edge] * 4, C.VP.R1CS, [top, top], nv, top, order, "all-(p - 1) R1CS order %d" % order)
            call([[top] * (1 << SMALL_NV)] * 8, C.VP.MIXED, [top] * 8, SMALL_NV, top, order, "all-(p - 1) eight terms order %d" % order)
        if checking:
            expect_clean("%s edge operands" % name)
        print("%-40s %s" % (run.tag, "clean" if checking else "agrees with the model"), flush=True)
    assert paths == {True, False}, paths
    print("vpoly_fold_invariants: OK", flush=True)


if __name__ == "__main__":
    main()
