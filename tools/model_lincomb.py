"""Pure-Python restatement of the linear combination (sr_lincomb): M outputs over K tables of ring elements,

    out_m[e] = [bit K of uses[m]] coef[m][K]  +  sum_{k < K, bit k of uses[m]} coef[m][k] * T_k[e]        e < n

one term at a time, generic over the element type like tools/model_frac_tree.py -- the caller supplies zero, add and mul (mul(r, a):
the coefficient first), so the same code runs on Python integers modulo a prime (tests/test_lincomb_host.py pins it against closed
forms), on ring elements of the power-of-two rings held as tuples or numpy object arrays of standard-form integers, and on memory
images of the reference's own rings with the oracle's Fq3 / Fq9 / Fq4 slot products (the expected values of
tests/test_lincomb_gpu.py).  No kernel, no library call.

Table k stores n_evals[k] <= n elements; the rest of it is zero.  The constant goes to every one of the n elements.

composition() is the second formulation: the chain of DenseMultilinearExtension operators the call replaces (crates/poly
mle/dense.rs) -- copy, MulAssign<R> by the first coefficient, AddAssign<(R, &Self)> per further table, Add<R> of the constant.

`python tools/model_lincomb.py` rewrites tests/golden/lincomb_kats.json.
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import model_prod_tree as PT  # noqa: E402
import model_sumcheck as SC  # noqa: E402

MAX_TABLES, MAX_OUTPUTS = 16, 4


def full_mask(n_tables):
    """every table and the constant"""
    return (2 << n_tables) - 1


def pad(table, n, zero):
    assert len(table) <= n
    return list(table) + [zero] * (n - len(table))


def lincomb(tables, coef, uses, n, zero, add, mul):
    """tables: K lists of at most n elements; coef: M rows of K + 1 elements (an entry whose mask bit is clear is never touched and may
    be anything, None included); uses: M masks.  -> M lists of n elements"""
    K = len(tables)
    full = [pad(t, n, zero) for t in tables]
    outs = []
    for row, u in zip(coef, uses):
        assert u and not u >> (K + 1)
        out = []
        for e in range(n):
            acc = zero
            for k in range(K):
                if (u >> k) & 1:
                    acc = add(acc, mul(row[k], full[k][e]))
            if (u >> K) & 1:
                acc = add(acc, row[K])
            out.append(acc)
        outs.append(out)
    return outs


def composition(tables, coef, uses, n, zero, add, mul):
    """the same outputs from the operators the call replaces: out = copy of the first used table; out *= its coefficient; out += (c_k,
    T_k) for every further used table; out + const.  A row that uses no table is the constant alone."""
    K = len(tables)
    full = [pad(t, n, zero) for t in tables]
    outs = []
    for row, u in zip(coef, uses):
        used = [k for k in range(K) if (u >> k) & 1]
        if used:
            out = list(full[used[0]])                                     # copy
            out = [mul(row[used[0]], x) for x in out]                     # MulAssign<R>
            for k in used[1:]:
                out = [add(a, mul(row[k], x)) for a, x in zip(out, full[k])]   # AddAssign<(R, &Self)>
        else:
            out = [zero] * n
        if (u >> K) & 1:
            out = [add(a, row[K]) for a in out]                           # Add<R>, on every element
        outs.append(out)
    return outs


def traffic(n_tables, n_outputs, n=1):
    """(one pass, composition) in ring elements moved: every table read once and every output written once, against per output a copy
    (2 n), the in-place product (2 n), K - 1 accumulations of 3 n and the in-place constant (2 n)"""
    return (n_tables + n_outputs) * n, n_outputs * (3 * n_tables + 3) * n


# ---- the plan (csrc/lincomb.hpp: kRegTables, kRegOutputs, kRunOutputs; tests/test_lincomb_isa.py holds the register counts) ---------
REG_TABLES = 4
# ring id -> (outputs of the kernel that keeps its coefficients in registers, outputs per launch of the run-time-K kernel)
OUTPUTS = {0: (2, 3), 1: (2, 4), 2: (1, 1), 3: (1, 1), 4: (0, 1), 5: (0, 1)}


def plan(ring_id, n_tables, n_outputs):
    """(launches, outputs_per_launch, registers): registers -- the one launch keeps its coefficients in registers"""
    assert 1 <= n_tables <= MAX_TABLES and 1 <= n_outputs <= MAX_OUTPUTS
    reg_m, run_m = OUTPUTS[ring_id]
    if n_tables <= REG_TABLES and n_outputs <= reg_m:
        return 1, n_outputs, True
    per = min(n_outputs, run_m)
    return -(-n_outputs // per), per, False


# ---- the builders of lookup.py, on the model -------------------------------------------------------------------------------------
def permutation_leaves(f, ident, sigma, beta, gamma, one, zero, add, mul):
    """(num, den) = (beta + f + gamma id, beta + f + gamma sigma): tables (f, id, sigma), two rows whose masks leave out the table they
    do not use"""
    n = len(f)
    return lincomb([f, ident, sigma], [[one, gamma, None, beta], [one, None, gamma, beta]], [0b1011, 0b1101], n, zero, add, mul)


# ---- the pinned vectors ----------------------------------------------------------------------------------------------------------
KAT_LOG2_DEGREE = 1
KAT_N = 2
POW2_RINGS = PT.POW2_RINGS
SLOT_RINGS = PT.SLOT_RINGS
SLOT_PRIMES = {"goldilocks": SC.PRIMES["goldilocks"], "babybear": SC.PRIMES["babybear"], "frog": 15912092521325583641}
# (name, K, M, masks or None for everything, n_evals or None)
KAT_SHAPES = [("k1_m1", 1, 1, None, None), ("k3_m2", 3, 2, None, None), ("k16_m1", 16, 1, None, None),
              ("k3_m2_truncated", 3, 2, None, [0, 1, 2]), ("k3_m2_masked", 3, 2, [0b1011, 0b0101], None)]


def make_kats():
    import numpy as np

    import oracle_lib as O

    cases = []
    d_ring = 1 << KAT_LOG2_DEGREE

    def shapes(case, draw, zero, add, mul, out):
        for name, K, M, masks, n_evals in KAT_SHAPES:
            tables = [[draw() for _ in range(KAT_N if n_evals is None else n_evals[k])] for k in range(K)]
            coef = [[draw() for _ in range(K + 1)] for _ in range(M)]
            uses = masks if masks is not None else [full_mask(K)] * M
            outs = lincomb(tables, coef, uses, KAT_N, zero, add, mul)
            case[name] = {"n_tables": K, "n_outputs": M, "uses": uses, "n": KAT_N, "n_evals": [len(t) for t in tables],
                          "tables": [[out(e) for e in t] for t in tables], "coef": [[out(e) for e in row] for row in coef],
                          "outs": [[out(e) for e in o] for o in outs]}

    for ring, ring_id in sorted(POW2_RINGS.items(), key=lambda kv: kv[1]):
        p = SC.PRIMES[ring]
        add, _, mul = SC.vec_ops(p)
        rng = random.Random("lincomb kats " + ring)
        draw = lambda: tuple(rng.choice((1, p - 1, rng.randrange(p), rng.randrange(p))) for _ in range(d_ring))  # noqa: E731
        case = {"ring": ring, "ring_id": ring_id, "log2_degree": KAT_LOG2_DEGREE, "form": "standard"}
        shapes(case, draw, (0,) * d_ring, add, mul, list)
        cases.append(case)
    for ring, (ring_id, base, fn, d, slot_w) in sorted(SLOT_RINGS.items(), key=lambda kv: kv[1][0]):
        F = O.FIELD_ID[base]
        prime = SLOT_PRIMES[base]
        words = O.fill_uniform(F, 0xA700 + ring_id, 0, 256 * d)
        pos = [0]

        def draw():
            e = words[pos[0] * d:(pos[0] + 1) * d].copy()
            pos[0] += 1
            return e

        mul = lambda r, a: O.small(fn, a, r)  # noqa: E731
        add = lambda a, b: ((a.astype(object) + b.astype(object)) % prime).astype(np.uint64)  # noqa: E731
        ints = lambda e: [int(x) for x in e]  # noqa: E731
        case = {"ring": ring, "ring_id": ring_id, "log2_degree": 0, "form": "memory"}
        shapes(case, draw, np.zeros(d, dtype=np.uint64), add, mul, ints)
        assert pos[0] <= 256
        cases.append(case)
    return {"source": "tools/model_lincomb.py: one list of D words per ring element -- form `standard`: standard-form integers "
                      "(power-of-two rings); form `memory`: the u64 memory image (the reference's own rings, slot products of the "
                      "oracle); per shape: tables (the stored parts), coef (n_outputs rows of n_tables + 1 elements, the constant last), "
                      "uses (one mask per output) and outs (n_outputs lists of n elements)",
            "cases": cases}


def dump_kats():
    """the text of tests/golden/lincomb_kats.json"""
    return json.dumps(make_kats(), separators=(",", ":")) + "\n"


if __name__ == "__main__":
    root = os.path.dirname(HERE)
    sys.path.insert(0, os.path.join(root, "oracle"))
    path = os.path.join(root, "tests", "golden", "lincomb_kats.json")
    with open(path, "w") as f:
        f.write(dump_kats())
    print("wrote", path)
