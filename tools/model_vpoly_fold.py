"""Pure-Python restatement of the fused sum-check round over a SUM OF PRODUCTS (sr_vpoly_round_fold_evals): every distinct table folded
at the challenge r of the round that has just ended, and the message of the round that follows over the folded tables.  It composes
tools/model_mle.py (fold) per table and tools/model_vpoly.py (round_evals) and holds no arithmetic of its own; generic over the
element type like them.  No kernel, no library call.

  fold_round   folded_j = fold(f_j, [r]) cut to the truncated length the device writes;
               message = model_vpoly.round_evals(folded, terms, coeffs, num_vars - 1)

`python tools/model_vpoly_fold.py` rewrites tests/golden/vpoly_fold_kats.json.
"""
import json
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import model_mle as M  # noqa: E402
import model_sumcheck as SC  # noqa: E402
import model_sumcheck_fold as SF  # noqa: E402
import model_vpoly as VP  # noqa: E402

LEADING, TRAILING = M.LEADING, M.TRAILING
folded_len = SF.folded_len


def fold_round(tables, terms, coeffs, num_vars, r, order, zero, one, add, sub, mul):
    """tables: lists of at most 2^num_vars elements (the missing tail is zero), num_vars >= 2; terms, coeffs: as in model_vpoly.
    Returns (folded, message): the folded tables in truncated storage and [p(0), .., p(d)] of the next round."""
    assert num_vars >= 2
    folded = []
    for f in tables:
        g = M.fold(M.pad(f, num_vars, zero), num_vars, [r], order, add, sub, mul)
        folded.append(g[:folded_len(len(f), num_vars, order)])
    return folded, VP.round_evals(folded, terms, coeffs, num_vars - 1, order, zero, one, add, sub, mul)


# ---- the pinned vectors ----------------------------------------------------------------------------------------------------------
KAT_LOG2_DEGREE, KAT_NUM_VARS = 1, 3


def make_kats():
    cases = []
    d_ring = 1 << KAT_LOG2_DEGREE
    for ring, p in sorted(SC.PRIMES.items()):
        add, sub, mul = SC.vec_ops(p)
        zero, one = (0,) * d_ring, (1,) * d_ring
        rng = random.Random("vpoly fold kats " + ring)
        elem = lambda: tuple(rng.choice((0, 1, p - 1, rng.randrange(p))) for _ in range(d_ring))
        for name, terms in (("R1CS", VP.R1CS), ("REPEAT", VP.REPEAT)):
            full = 1 << KAT_NUM_VARS
            n_evals = [full] * VP.n_tables(terms)
            n_evals[-1] = full - 3  # a truncated table: odd, beyond the half
            tables = [[elem() for _ in range(n)] for n in n_evals]
            coeffs = [elem() for _ in terms]
            if name == "R1CS":
                coeffs[1] = sub(zero, one)
            r = tuple(rng.randrange(p) for _ in range(d_ring))
            case = {"ring": ring, "structure": name, "log2_degree": KAT_LOG2_DEGREE, "num_vars": KAT_NUM_VARS, "terms": terms,
                    "n_evals": n_evals, "tables": [[list(e) for e in f] for f in tables], "coeffs": [list(c) for c in coeffs], "r": list(r)}
            for key, order in (("leading", LEADING), ("trailing", TRAILING)):
                folded, msg = fold_round(tables, terms, coeffs, KAT_NUM_VARS, r, order, zero, one, add, sub, mul)
                case[key] = {"folded": [[list(e) for e in g] for g in folded], "message": [list(e) for e in msg]}
            cases.append(case)
    return {"source": "tools/model_vpoly_fold.py: standard-form integers, one list of D per ring element; terms: table indices per term; "
                      "per order the folded tables in truncated storage and the next round's p(0) .. p(d)",
            "cases": cases}


if __name__ == "__main__":
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "vpoly_fold_kats.json")
    with open(path, "w") as f:
        json.dump(make_kats(), f, indent=1)
        f.write("\n")
    print("wrote", path)
