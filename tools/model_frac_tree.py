"""Pure-Python restatement of the fraction tree (sr_frac_tree): every layer of the binary tree that sums fractions p_i / q_i without
dividing, one pair of children at a time, generic over the element type like tools/model_prod_tree.py -- the caller supplies zero(),
one(), add and mul, so the same code runs on Python integers modulo a prime (tests/test_frac_tree_host.py pins it against the closed
forms), on ring elements of the power-of-two rings held as tuples or numpy object arrays of standard-form integers, and on memory
images of the reference's own rings with the oracle's Fq3 / Fq9 / Fq4 slot products (the expected values of
tests/test_frac_tree_gpu.py).  No kernel, no library call.

A node is a pair (p, q); with children (l, r):   p = p_l * q_r + p_r * q_l     q = q_l * q_r
  leading    (l, r) = (2i, 2i + 1)        trailing   (l, r) = (i, i + half)        the pairs of tools/model_prod_tree.py

Layer 0 is the leaves, padded with the neutral fraction (zero(), one()) to 2^num_vars; layer k has 2^(num_vars - k) nodes.  Where no
numerators are stored (p_leaves None) every stored leaf has numerator one().

`python tools/model_frac_tree.py` rewrites tests/golden/frac_tree_kats.json.
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import model_prod_tree as PT  # noqa: E402
import model_sumcheck as SC  # noqa: E402

LEADING, TRAILING = 0, 1


def pad(p_leaves, q_leaves, num_vars, zero, one):
    """the truncated leaves written out, as (numerators, denominators): the leaves that are not stored are (zero(), one()); absent
    numerators are one() for every stored leaf"""
    n, full = len(q_leaves), 1 << num_vars
    assert n <= full and (p_leaves is None or len(p_leaves) == n)
    return (list(p_leaves) if p_leaves is not None else [one] * n) + [zero] * (full - n), list(q_leaves) + [one] * (full - n)


def layers(p_leaves, q_leaves, num_vars, order, zero, one, add, mul):
    """-> ([P_0, .., P_num_vars], [Q_0, .., Q_num_vars]): layer 0 the padded leaves, layer num_vars the one-node root"""
    p0, q0 = pad(p_leaves, q_leaves, num_vars, zero, one)
    ps, qs = [p0], [q0]
    for k in range(1, num_vars + 1):
        p, q, half = ps[-1], qs[-1], 1 << (num_vars - k)
        pairs = [(2 * i, 2 * i + 1) if order == LEADING else (i, i + half) for i in range(half)]
        ps.append([add(mul(p[l], q[r]), mul(p[r], q[l])) for l, r in pairs])
        qs.append([mul(q[l], q[r]) for l, r in pairs])
    return ps, qs


layer_offset = PT.layer_offset   # element offset of layer k (1 <= k <= num_vars) in either output: layer 1 first, the root last


def flat(tree):
    """(p_layers, q_layers): the layers 1 .. num_vars of each side one behind the other, as the call writes them"""
    return PT.flat(tree[0]), PT.flat(tree[1])


# ---- the pinned vectors ----------------------------------------------------------------------------------------------------------
# num_vars: one more than the levels a launch produces (tests/test_frac_tree_isa.py holds the table), so every case takes two
# launches.  n_leaves = 5 lies inside a group of the first launch in both orders.
KAT_LOG2_DEGREE = 1
POW2_RINGS = PT.POW2_RINGS
SLOT_RINGS = PT.SLOT_RINGS
LEVELS_PER_LAUNCH = {"goldilocks": 2, "babybear": 3, "stark": 2, "goldilocks24": 2, "babybear72": 1, "frog16": 2}
KAT_NUM_VARS = {ring: j + 1 for ring, j in LEVELS_PER_LAUNCH.items()}
KAT_NUM_VARS["babybear72"] = 3   # 5 leaves need three variables: three launches of one level
KAT_N_LEAVES = 5
SLOT_PRIMES = {"goldilocks": SC.PRIMES["goldilocks"], "babybear": SC.PRIMES["babybear"], "frog": 15912092521325583641}


def make_kats():
    import numpy as np

    import oracle_lib as O

    cases = []
    d_ring = 1 << KAT_LOG2_DEGREE

    def both(case, p_leaves, q_leaves, nv, zero, one, add, mul, out):
        for key, order in (("leading", LEADING), ("trailing", TRAILING)):
            for tag, pl in (("", p_leaves), ("_no_numerators", None)):
                p, q = flat(layers(pl, q_leaves, nv, order, zero, one, add, mul))
                case[key + tag] = {"p": [out(e) for e in p], "q": [out(e) for e in q]}

    for ring, ring_id in sorted(POW2_RINGS.items(), key=lambda kv: kv[1]):
        p = SC.PRIMES[ring]
        add, _, mul = SC.vec_ops(p)
        zero, one = (0,) * d_ring, (1,) * d_ring
        rng = random.Random("frac tree kats " + ring)
        nv = KAT_NUM_VARS[ring]
        draw = lambda: [tuple(rng.choice((1, p - 1, rng.randrange(p), rng.randrange(p))) for _ in range(d_ring))  # noqa: E731
                        for _ in range(KAT_N_LEAVES)]
        p_leaves, q_leaves = draw(), draw()
        case = {"ring": ring, "ring_id": ring_id, "log2_degree": KAT_LOG2_DEGREE, "num_vars": nv, "n_leaves": KAT_N_LEAVES,
                "form": "standard", "p_leaves": [list(e) for e in p_leaves], "q_leaves": [list(e) for e in q_leaves]}
        both(case, p_leaves, q_leaves, nv, zero, one, add, mul, list)
        cases.append(case)
    for ring, (ring_id, base, fn, d, slot_w) in sorted(SLOT_RINGS.items(), key=lambda kv: kv[1][0]):
        F = O.FIELD_ID[base]
        prime = SLOT_PRIMES[base]
        nv = KAT_NUM_VARS[ring]
        words = O.fill_uniform(F, 0x9E00 + ring_id, 0, 2 * KAT_N_LEAVES * d)
        p_leaves = [words[i * d:(i + 1) * d].copy() for i in range(KAT_N_LEAVES)]
        q_leaves = [words[i * d:(i + 1) * d].copy() for i in range(KAT_N_LEAVES, 2 * KAT_N_LEAVES)]
        zero = np.zeros(d, dtype=np.uint64)
        one = np.zeros(d, dtype=np.uint64)
        one[::slot_w] = O.to_mont(F, [1])[0]
        mul = lambda a, b: O.small(fn, a, b)  # noqa: E731
        add = lambda a, b: ((a.astype(object) + b.astype(object)) % prime).astype(np.uint64)  # noqa: E731
        ints = lambda e: [int(x) for x in e]  # noqa: E731
        case = {"ring": ring, "ring_id": ring_id, "log2_degree": 0, "num_vars": nv, "n_leaves": KAT_N_LEAVES, "form": "memory",
                "p_leaves": [ints(e) for e in p_leaves], "q_leaves": [ints(e) for e in q_leaves]}
        both(case, p_leaves, q_leaves, nv, zero, one, add, mul, ints)
        cases.append(case)
    return {"source": "tools/model_frac_tree.py: one list of D words per ring element -- form `standard`: standard-form integers "
                      "(power-of-two rings); form `memory`: the u64 memory image (the reference's own rings, slot products of the "
                      "oracle); leading / trailing: p and q, the 2^num_vars - 1 elements of the layers 1 .. num_vars of each side, the "
                      "root last; *_no_numerators: every stored numerator is one(); the leaves beyond n_leaves are (zero(), one())",
            "cases": cases}


def dump_kats():
    """the text of tests/golden/frac_tree_kats.json"""
    return json.dumps(make_kats(), separators=(",", ":")) + "\n"


if __name__ == "__main__":
    root = os.path.dirname(HERE)
    sys.path.insert(0, os.path.join(root, "oracle"))
    path = os.path.join(root, "tests", "golden", "frac_tree_kats.json")
    with open(path, "w") as f:
        f.write(dump_kats())
    print("wrote", path)
