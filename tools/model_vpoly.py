"""Pure-Python restatement of the prover's message of a sum-check round over a SUM OF PRODUCTS of dense multilinear extensions with
ring coefficients (HyperPlonk's VirtualPolynomial), on top of tools/model_mle.py and tools/model_sumcheck.py and generic over the
element type like them: the caller supplies zero, one, add, sub and mul (`r * a`), so the same code runs on Python integers modulo a
prime (tests/test_vpoly_host.py pins it against the sum-check identities), on ring elements of the power-of-two rings held as numpy
object arrays and on memory images of the reference's own rings with the oracle's slot products (the expected values of
tests/test_vpoly_gpu.py).  No kernel, no library call.

  g(x) = sum_k c_k prod_s f_{terms[k][s]}(x)      terms: lists of table indices; coeffs: one element per term, or None for one()
  round_evals   p(t) = sum_b g(t, b) for t = 0 .. d, d the longest term: every table folded with the point [R::from(t)] by
                model_mle.fold, multiplied term by term, scaled by the coefficient and summed
  poly_sum      sum_b g(b)

`python tools/model_vpoly.py` rewrites tests/golden/vpoly_kats.json.
"""
import json
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import model_mle as M  # noqa: E402
import model_sumcheck as SC  # noqa: E402

LEADING, TRAILING = M.LEADING, M.TRAILING

# the term structures of the tests: lists of table indices per term
SINGLE = [[0, 1, 2]]                                    # no coefficients: the message of model_sumcheck.round_evals
R1CS = [[0, 1, 2], [0, 3]]                              # tables e, a, b, c; coefficients (c0, -one()): eq (a b - c)
REPEAT = [[0, 0, 1, 1], [1], [2, 3]]                    # a table twice in a term, a lone factor
MIXED = [[0], [0, 1], [0, 2, 3], [0, 4, 5, 6], [1, 2, 7, 7], [3, 5, 0], [6, 7], [4]]  # 1,2,3,4,4,3,2,1 factors; table 0 in five terms
CANCEL = [[0, 1], [1, 0]]                               # coefficients (c, -c): every point is zero


def degree(terms):
    return max(len(t) for t in terms)


def n_tables(terms):
    return 1 + max(j for t in terms for j in t)


def _sum_of_terms(tables, terms, coeffs, zero, add, mul):
    """tables: equal-length lists of elements; sum_b sum_k c_k prod_s tables[terms[k][s]][b]"""
    total = zero
    for k, term in enumerate(terms):
        part = zero
        for b in range(len(tables[term[0]])):
            pr = tables[term[0]][b]
            for j in term[1:]:
                pr = mul(tables[j][b], pr)
            part = add(part, pr)
        total = add(total, part if coeffs is None else mul(coeffs[k], part))
    return total


def poly_sum(tables, terms, coeffs, num_vars, zero, add, mul):
    """tables: lists of at most 2^num_vars elements (the missing tail is zero)"""
    return _sum_of_terms([M.pad(f, num_vars, zero) for f in tables], terms, coeffs, zero, add, mul)


def round_evals(tables, terms, coeffs, num_vars, order, zero, one, add, sub, mul):
    """returns [p(0), .., p(d)]"""
    padded = [M.pad(f, num_vars, zero) for f in tables]
    out = []
    for t in range(degree(terms) + 1):
        r = SC.constant(t, zero, one, add)
        folded = [M.fold(f, num_vars, [r], order, add, sub, mul) for f in padded]
        out.append(_sum_of_terms(folded, terms, coeffs, zero, add, mul))
    return out


def evaluate(values, terms, coeffs, zero, add, mul):
    """g at a point, from the values of the tables there: sum_k c_k prod_s values[terms[k][s]]"""
    return _sum_of_terms([[v] for v in values], terms, coeffs, zero, add, mul)


# ---- the pinned vectors ----------------------------------------------------------------------------------------------------------
PRIMES = SC.PRIMES
KAT_LOG2_DEGREE, KAT_NUM_VARS = 1, 3


def make_kats():
    cases = []
    d_ring = 1 << KAT_LOG2_DEGREE
    for ring, p in sorted(PRIMES.items()):
        add, sub, mul = SC.vec_ops(p)
        zero, one = (0,) * d_ring, (1,) * d_ring
        rng = random.Random("vpoly kats " + ring)
        elem = lambda: tuple(rng.choice((0, 1, p - 1, rng.randrange(p))) for _ in range(d_ring))
        for name, terms in (("R1CS", R1CS), ("REPEAT", REPEAT), ("MIXED", MIXED)):
            full = 1 << KAT_NUM_VARS
            n_evals = [full] * n_tables(terms)
            n_evals[-1] = full - 3  # a truncated table: odd, beyond the half
            tables = [[elem() for _ in range(n)] for n in n_evals]
            coeffs = [elem() for _ in terms]
            if name == "R1CS":
                coeffs[1] = sub(zero, one)
            case = {"ring": ring, "structure": name, "log2_degree": KAT_LOG2_DEGREE, "num_vars": KAT_NUM_VARS, "terms": terms,
                    "n_evals": n_evals, "tables": [[list(e) for e in f] for f in tables], "coeffs": [list(c) for c in coeffs],
                    "sum": list(poly_sum(tables, terms, coeffs, KAT_NUM_VARS, zero, add, mul))}
            for key, order in (("leading", LEADING), ("trailing", TRAILING)):
                case[key] = [list(e) for e in round_evals(tables, terms, coeffs, KAT_NUM_VARS, order, zero, one, add, sub, mul)]
            cases.append(case)
    return {"source": "tools/model_vpoly.py: standard-form integers, one list of D per ring element; terms: table indices per term; "
                      "leading / trailing: p(0) .. p(d)",
            "cases": cases}


if __name__ == "__main__":
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "vpoly_kats.json")
    with open(path, "w") as f:
        json.dump(make_kats(), f, indent=1)
        f.write("\n")
    print("wrote", path)
