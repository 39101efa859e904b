"""Pure-Python restatement of the prover's message of a sum-check round over a product of dense multilinear extensions, on top of
tools/model_mle.py and generic over the element type like it: the caller supplies zero, one, add, sub and mul (`r * a`), so the same
code runs on Python integers modulo a prime (tests/test_sumcheck_host.py pins it against the sum-check identities), on ring elements
of the power-of-two rings held as numpy object arrays and on memory images of the reference's own rings with the oracle's slot
products (the expected values of tests/test_sumcheck_gpu.py).  No kernel, no library call.

  round_evals   p(t) = sum_b prod_j f_j(t, b) for t = 0 .. d: every table folded with the point [R::from(t)] by model_mle.fold
                (mle/dense.rs:171-199, polynomials/multilinear_polynomial.rs:251-286), multiplied element-wise and summed
  product_sum   sum_b prod_j f_j[b], the `sum` random_mle_list returns (multilinear_polynomial.rs:19-49)

`python tools/model_sumcheck.py` rewrites tests/golden/sumcheck_kats.json.
"""
import json
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import model_mle as M  # noqa: E402

LEADING, TRAILING = M.LEADING, M.TRAILING


def constant(t, zero, one, add):
    """R::from(t) = t * one()"""
    r = zero
    for _ in range(t):
        r = add(r, one)
    return r


def product_sum(tables, zero, add, mul):
    """tables: full-length lists of elements"""
    total = zero
    for b in range(len(tables[0])):
        term = tables[0][b]
        for f in tables[1:]:
            term = mul(f[b], term)
        total = add(total, term)
    return total


def round_evals(tables, num_vars, order, zero, one, add, sub, mul):
    """tables: lists of at most 2^num_vars elements (the missing tail is zero); returns [p(0), .., p(d)]"""
    padded = [M.pad(f, num_vars, zero) for f in tables]
    out = []
    for t in range(len(tables) + 1):
        r = constant(t, zero, one, add)
        folded = [M.fold(f, num_vars, [r], order, add, sub, mul) for f in padded]
        out.append(product_sum(folded, zero, add, mul))
    return out


def lagrange_at(values, r, p):
    """Prime field only: the polynomial of degree < len(values) through (t, values[t]), t = 0 .. len - 1, at r"""
    n, total = len(values), 0
    for i, v in enumerate(values):
        num, den = 1, 1
        for j in range(n):
            if j != i:
                num = num * (r - j) % p
                den = den * (i - j) % p
        total = (total + v * num * pow(den, p - 2, p)) % p
    return total


# ---- the pinned vectors ----------------------------------------------------------------------------------------------------------
PRIMES = {"goldilocks": 0xFFFFFFFF00000001, "babybear": 2013265921,
          "stark": 0x800000000000011000000000000000000000000000000000000000000000001}
KAT_LOG2_DEGREE, KAT_NUM_VARS = 1, 3


def vec_ops(p):
    """ring elements of a power-of-two ring as tuples of standard-form integers, slot-wise"""
    return ((lambda a, b: tuple((x + y) % p for x, y in zip(a, b))), (lambda a, b: tuple((x - y) % p for x, y in zip(a, b))),
            (lambda r, a: tuple(x * y % p for x, y in zip(r, a))))


def make_kats():
    cases = []
    d_ring = 1 << KAT_LOG2_DEGREE
    for ring, p in sorted(PRIMES.items()):
        add, sub, mul = vec_ops(p)
        zero, one = (0,) * d_ring, (1,) * d_ring
        rng = random.Random("sumcheck kats " + ring)
        for d in (1, 2, 3, 4):
            full = 1 << KAT_NUM_VARS
            n_evals = [full] * d
            n_evals[-1] = full - 3  # a truncated table: odd, beyond the half
            tables = [[tuple(rng.choice((0, 1, p - 1, rng.randrange(p))) for _ in range(d_ring)) for _ in range(n)] for n in n_evals]
            padded = [M.pad(f, KAT_NUM_VARS, zero) for f in tables]
            case = {"ring": ring, "log2_degree": KAT_LOG2_DEGREE, "num_vars": KAT_NUM_VARS, "n_evals": n_evals,
                    "tables": [[list(e) for e in f] for f in tables], "sum": list(product_sum(padded, zero, add, mul))}
            for name, order in (("leading", LEADING), ("trailing", TRAILING)):
                case[name] = [list(e) for e in round_evals(tables, KAT_NUM_VARS, order, zero, one, add, sub, mul)]
            cases.append(case)
    return {"source": "tools/model_sumcheck.py: standard-form integers, one list of D per ring element; leading / trailing: p(0) .. p(d)",
            "cases": cases}


if __name__ == "__main__":
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "sumcheck_kats.json")
    with open(path, "w") as f:
        json.dump(make_kats(), f, indent=1)
        f.write("\n")
    print("wrote", path)
