"""Pure-Python restatement of the layered grand product (sr_prod_tree): every layer of the binary product tree over a table, one pair
at a time, generic over the element type like tools/model_mle.py -- the caller supplies one() and mul, so the same code runs on
Python integers modulo a prime (tests/test_prod_tree_host.py pins it against the closed form), on ring elements of the power-of-two
rings held as tuples or numpy object arrays of standard-form integers, and on memory images of the reference's own rings with the
oracle's Fq3 / Fq9 / Fq4 slot products (the expected values of tests/test_prod_tree_gpu.py).  No kernel, no library call.

  leading    L_k[i] = L_{k-1}[2i] * L_{k-1}[2i+1]        the pairs fix_variables folds (mle/dense.rs:171-199)
  trailing   L_k[i] = L_{k-1}[i] * L_{k-1}[i + half]     the pairs fix_last_variables folds (multilinear_polynomial.rs:227-286)

Layer 0 is the leaves, padded with one() to 2^num_vars; layer k has 2^(num_vars - k) elements.

`python tools/model_prod_tree.py` rewrites tests/golden/prod_tree_kats.json.
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import model_sumcheck as SC  # noqa: E402

LEADING, TRAILING = 0, 1


def pad(leaves, num_vars, one):
    """the truncated leaves written out: the leaves that are not stored are one()"""
    assert len(leaves) <= 1 << num_vars
    return list(leaves) + [one] * ((1 << num_vars) - len(leaves))


def layers(leaves, num_vars, order, one, mul):
    """-> [L_0, L_1, .., L_num_vars]: L_0 the padded leaves, L_num_vars the one-element root layer"""
    out = [pad(leaves, num_vars, one)]
    for k in range(1, num_vars + 1):
        below, half = out[-1], 1 << (num_vars - k)
        if order == LEADING:
            out.append([mul(below[2 * i], below[2 * i + 1]) for i in range(half)])
        else:
            out.append([mul(below[i], below[i + half]) for i in range(half)])
    return out


def layer_offset(num_vars, k):
    """element offset of layer k (1 <= k <= num_vars) in the buffer of a call: layer 1 first, the root last"""
    return (1 << num_vars) - (1 << (num_vars - k + 1))


def flat(tree):
    """the layers 1 .. num_vars one behind the other, as the call writes them: 2^num_vars - 1 elements"""
    return [e for layer in tree[1:] for e in layer]


# ---- the pinned vectors ----------------------------------------------------------------------------------------------------------
# num_vars: one more than the levels a launch produces (three; two for babybear72), so every case takes two launches.  n_leaves = 5
# lies strictly inside a group of the first launch in both orders: leading groups are 8 (babybear72: 4) consecutive leaves; trailing
# groups are the leaves of one index modulo 2, of which group 0 holds leaves 0, 2, 4 and misses leaf 6
KAT_LOG2_DEGREE = 1
POW2_RINGS = {"goldilocks": 0, "babybear": 1, "stark": 2}
SLOT_RINGS = {"goldilocks24": (3, "goldilocks", "sro_g24_ntt_mul", 24, 3), "babybear72": (4, "babybear", "sro_bb72_ntt_mul", 72, 9),
              "frog16": (5, "frog", "sro_frog16_ntt_mul", 16, 4)}
KAT_NUM_VARS = {"goldilocks": 4, "babybear": 4, "stark": 4, "goldilocks24": 4, "babybear72": 3, "frog16": 4}
KAT_N_LEAVES = 5


def make_kats():
    import numpy as np

    import oracle_lib as O

    cases = []
    d_ring = 1 << KAT_LOG2_DEGREE
    for ring, ring_id in sorted(POW2_RINGS.items(), key=lambda kv: kv[1]):
        p = SC.PRIMES[ring]
        mul = SC.vec_ops(p)[2]
        one = (1,) * d_ring
        rng = random.Random("prod tree kats " + ring)
        nv = KAT_NUM_VARS[ring]
        leaves = [tuple(rng.choice((1, p - 1, rng.randrange(p), rng.randrange(p))) for _ in range(d_ring)) for _ in range(KAT_N_LEAVES)]
        case = {"ring": ring, "ring_id": ring_id, "log2_degree": KAT_LOG2_DEGREE, "num_vars": nv, "n_leaves": KAT_N_LEAVES,
                "form": "standard", "leaves": [list(e) for e in leaves]}
        for key, order in (("leading", LEADING), ("trailing", TRAILING)):
            case[key] = [list(e) for e in flat(layers(leaves, nv, order, one, mul))]
        cases.append(case)
    for ring, (ring_id, base, fn, d, slot_w) in sorted(SLOT_RINGS.items(), key=lambda kv: kv[1][0]):
        F = O.FIELD_ID[base]
        nv = KAT_NUM_VARS[ring]
        words = O.fill_uniform(F, 0x9D00 + ring_id, 0, KAT_N_LEAVES * d)
        leaves = [words[i * d:(i + 1) * d].copy() for i in range(KAT_N_LEAVES)]
        one = np.zeros(d, dtype=np.uint64)
        one[::slot_w] = O.to_mont(F, [1])[0]
        mul = lambda a, b: O.small(fn, a, b)  # noqa: E731
        case = {"ring": ring, "ring_id": ring_id, "log2_degree": 0, "num_vars": nv, "n_leaves": KAT_N_LEAVES, "form": "memory",
                "leaves": [[int(x) for x in e] for e in leaves]}
        for key, order in (("leading", LEADING), ("trailing", TRAILING)):
            case[key] = [[int(x) for x in e] for e in flat(layers(leaves, nv, order, one, mul))]
        cases.append(case)
    return {"source": "tools/model_prod_tree.py: one list of D words per ring element -- form `standard`: standard-form integers "
                      "(power-of-two rings); form `memory`: the u64 memory image (the reference's own rings, slot products of the "
                      "oracle); leading / trailing: the 2^num_vars - 1 elements of the layers 1 .. num_vars, the root last; the "
                      "leaves beyond n_leaves are one()",
            "cases": cases}


def dump_kats():
    """the text of tests/golden/prod_tree_kats.json"""
    return json.dumps(make_kats(), separators=(",", ":")) + "\n"


if __name__ == "__main__":
    root = os.path.dirname(HERE)
    sys.path.insert(0, os.path.join(root, "oracle"))
    path = os.path.join(root, "tests", "golden", "prod_tree_kats.json")
    with open(path, "w") as f:
        f.write(dump_kats())
    print("wrote", path)
