"""Worker of tests/test_inverse_invariants.py: drives sr_inverse_batch_dev on the rings whose slots are Goldilocks arithmetic with the
inputs that stress its representatives -- every word p - 1 (the product of a chunk is then +-1 and every intermediate is p - 1 or 1),
every word one, a uniform table with planted zero units, an all-zero table, each with and without numerators, and the one-coefficient
path at an odd 8-byte pointer -- and checks every output as tests/test_inverse_gpu.py does (integers, or the slot products of
oracle/pyref.py).  `check`: the process was started with SR_LIB_PATH pointing at the checking build (libstarkrings_hip_check.so), and
after every ring the device counters must read zero -- no canonical routine saw a representative >= p, no word >= p left the library.
`product`: the same calls on the product library, compared with the model alone."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

# (ring, log2 D)
RINGS = [("goldilocks", 0), ("goldilocks", 6), ("goldilocks24", 0)]


def main():
    import torch

    from stark_rings_amd import inverse_dev
    from test_inverse_gpu import Placed, check, plant, table, units_of
    from test_mle_gpu import host, model_for

    mode = sys.argv[1]
    checking = mode == "check"
    assert checking == os.environ.get("SR_LIB_PATH", "").endswith("_check.so"), "check: run with SR_LIB_PATH=<the checking build>"
    if checking:
        from rep_invariants_worker import counters, expect_clean
    for name, k in RINGS:
        m = model_for(name, k)
        if checking:
            counters()   # building the context uses the same arithmetic: start from zero
        c = m.ring.inverse_plan(1, False)[2]
        n = 5 * c + 3
        nu, uw = units_of(m)
        m.ring.inverse_zero_count()
        uniform = table(m, 0x7A00, n)
        planted = {(0, 0), (c + c // 2, nu - 1), (2 * c - 1, 0)} | {(e, nu // 2) for e in range(3 * c, 4 * c)}
        inputs = [("p - 1", m.const(m.p - 1, n), 0), ("one", np.tile(m.one(), n), 0),
                  ("planted zeros", plant(m, uniform.copy(), planted), len(planted)), ("all zero", np.zeros(n * m.w, dtype=np.uint64), n * nu)]
        for label, den, zeros in inputs:
            for num in (None, m.const(m.p - 1, n), uniform):
                for odd in (False, True):
                    out = Placed(torch, np.full(n * m.w, 0x22, dtype=np.uint64), odd)
                    t_den = Placed(torch, den, odd)
                    t_num = Placed(torch, num, False) if num is not None else None
                    inverse_dev(m.ring, out.t, t_den.t, t_num.t if t_num is not None else None)
                    torch.cuda.synchronize()
                    check(m, host(out.t), den, num)
                    assert out.guards_intact() and t_den.guards_intact(), (name, label, odd)
                    assert m.ring.inverse_zero_count() == zeros, (name, label)
        if checking:
            expect_clean("%s batch inversion" % name)
        print("%-16s %s" % ("%s-%d" % (name, k), "clean" if checking else "agrees with the model"), flush=True)
    print("inverse_invariants: OK", flush=True)


if __name__ == "__main__":
    main()
