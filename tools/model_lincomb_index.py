"""Pure-Python restatement of the linear combination with integer columns (sr_lincomb_index) and of the multiplicities
(sr_index_count):

    out_m[e] = [bit K+J of uses[m]] coef[m][K+J]  +  sum_{k < K, bit k} coef[m][k] * T_k[e]
             + sum_{j < J, bit K+j} coef[m][K+j] * R::from(col_j[e])                                   e < n

over the element operations of tools/model_lincomb.py (the caller supplies zero, add, mul and the ring's one()), one term at a time.
R::from(x) is built from one() by doubling and adding ONLY -- the binary expansion of x, most significant bit first -- so nothing
about the embedding of a base-field scalar is assumed: whatever one() is in the caller's element type (1 in every coefficient of a
power-of-two ring, (R, 0, ..) in every slot of the memory image of the reference's own rings), x one() is the reference's
R::from(x) = from_scalar(BaseRing::from(x)), reduced modulo p by the ring's own additions (x >= p included).  from_u64_repeated is the
second formulation, x additions of one(); tests/test_lincomb_index_host.py pins the two against each other for x <= 40 and against
the closed form (every coefficient x mod p) on the power-of-two rings.

A column is a list of at most n Python integers below 2^64 (the rest count as 0) or Progression(start): start + e.

`python tools/model_lincomb_index.py` rewrites tests/golden/lincomb_index_kats.json.
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import model_lincomb as LC  # noqa: E402
import model_sumcheck as SC  # noqa: E402

MAX_TABLES, MAX_COLUMNS, MAX_TERMS, MAX_OUTPUTS = 16, 8, 16, 4
U64 = 1 << 64


class Progression:
    def __init__(self, start):
        assert 0 <= start < U64
        self.start = start


def column_values(col, n):
    """the n integers of a column"""
    if isinstance(col, Progression):
        assert n == 0 or col.start + (n - 1) < U64, "the progression wraps"
        return [col.start + e for e in range(n)]
    assert len(col) <= n and all(0 <= x < U64 for x in col)
    return list(col) + [0] * (n - len(col))


def from_u64(x, one, zero, add):
    """x one() by doubling and adding, most significant bit first"""
    assert 0 <= x < U64
    acc = zero
    for bit in range(x.bit_length() - 1, -1, -1):
        acc = add(acc, acc)
        if (x >> bit) & 1:
            acc = add(acc, one)
    return acc


def from_u64_repeated(x, one, zero, add):
    """x one() as x additions"""
    acc = zero
    for _ in range(x):
        acc = add(acc, one)
    return acc


def lincomb_index(tables, columns, coef, uses, n, zero, one, add, mul, embed=None):
    """tables: K lists of at most n elements; columns: J columns; coef: M rows of K + J + 1 elements (an entry whose mask bit is clear
    is never touched and may be None); uses: M masks -- tables, columns, the constant.  -> M lists of n elements.  embed: x ->
    R::from(x), default from_u64 on the caller's operations (a caller that embeds the same integers again and again passes a
    memoised from_u64)"""
    if embed is None:
        embed = lambda x: from_u64(x, one, zero, add)  # noqa: E731
    K, J = len(tables), len(columns)
    T = K + J
    assert 0 <= K <= MAX_TABLES and 0 <= J <= MAX_COLUMNS and 1 <= T <= MAX_TERMS and 1 <= len(uses) <= MAX_OUTPUTS
    full = [LC.pad(t, n, zero) for t in tables]
    ints = [column_values(c, n) for c in columns]
    outs = []
    for row, u in zip(coef, uses):
        assert u and not u >> (T + 1)
        out = []
        for e in range(n):
            acc = zero
            for k in range(K):
                if (u >> k) & 1:
                    acc = add(acc, mul(row[k], full[k][e]))
            for j in range(J):
                if (u >> (K + j)) & 1:
                    acc = add(acc, mul(row[K + j], embed(ints[j][e])))
            if (u >> T) & 1:
                acc = add(acc, row[T])
            out.append(acc)
        outs.append(out)
    return outs


def index_count(idx, n_bins):
    """(counts, skipped): counts[t] = #{ i : idx[i] == t }; an index >= n_bins is skipped"""
    counts = [0] * n_bins
    skipped = 0
    for t in idx:
        if t < n_bins:
            counts[t] += 1
        else:
            skipped += 1
    return counts, skipped


def traffic(n=1):
    """a column of permutation leaves in ring elements moved: (f, id and sigma as integers, two outputs) against (f, id, sigma as
    tables, two outputs); the 8 bytes per row of sigma are not a ring element's worth"""
    return (1 + 2) * n, (3 + 2) * n


# ---- the plan (csrc/lincomb_index.hpp: kRegTerms, kRegOutputs, kRunOutputs; tests/test_lincomb_index_isa.py holds the registers) -----
REG_TERMS = 4
# ring id -> (outputs of the kernel that keeps its coefficients in registers, outputs per launch of the run-time kernel)
OUTPUTS = {0: (2, 3), 1: (2, 4), 2: (0, 1), 3: (1, 1), 4: (0, 1), 5: (0, 1)}
LDS_BINS = 4096


def plan(ring_id, n_tables, n_index, n_outputs):
    """(launches, outputs_per_launch, registers); no index column: the plan of sr_lincomb"""
    if n_index == 0:
        return LC.plan(ring_id, n_tables, n_outputs)
    terms = n_tables + n_index
    assert 0 <= n_tables <= MAX_TABLES and 1 <= n_index <= MAX_COLUMNS and terms <= MAX_TERMS and 1 <= n_outputs <= MAX_OUTPUTS
    reg_m, run_m = OUTPUTS[ring_id]
    if terms <= REG_TERMS and n_outputs <= reg_m:
        return 1, n_outputs, True
    per = min(n_outputs, run_m)
    return -(-n_outputs // per), per, False


# ---- the builders of lookup.py, on the model -------------------------------------------------------------------------------------
def permutation_leaves_indexed(f, id_start, sigma_idx, beta, gamma, one, zero, add, mul, embed=None):
    """(num, den) = (beta + f + gamma R::from(id_start + e), beta + f + gamma R::from(sigma_idx[e]))"""
    n = len(f)
    return lincomb_index([f], [Progression(id_start), list(sigma_idx)], [[one, gamma, None, beta], [one, None, gamma, beta]], [0b1011, 0b1101], n,
                         zero, one, add, mul, embed)


# ---- the pinned vectors ----------------------------------------------------------------------------------------------------------
KAT_LOG2_DEGREE = 1
KAT_N = 3
EDGE = [0, 1, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32, 1 << 63, U64 - 1]
# (name, K, columns as (kind, payload): ("p", start) or ("v", stored count), M, masks or None for everything)
KAT_SHAPES = [("k0_j1_m1", 0, [("v", 3)], 1, None), ("k1_j2_m2_leaves", 1, [("p", 0), ("v", 3)], 2, [0b1011, 0b1101]),
              ("k2_j2_m1_truncated", 2, [("v", 1), ("v", 0)], 1, None), ("k0_j8_m1", 0, [("p", U64 - 3)] + [("v", 3)] * 7, 1, None),
              ("k3_j2_m2", 3, [("v", 2), ("p", 1 << 32)], 2, None)]


def edge_values(p):
    return EDGE + ([p - 1, p, p + 1] if p < U64 else [])


def make_kats():
    import numpy as np

    import oracle_lib as O

    cases = []
    d_ring = 1 << KAT_LOG2_DEGREE

    def shapes(case, draw, prime, zero, one, add, mul, out):
        rng = random.Random("lincomb index kats " + case["ring"])
        for name, K, cols, M, masks in KAT_SHAPES:
            tables = [[draw() for _ in range(KAT_N)] for _ in range(K)]
            columns, described = [], []
            for kind, payload in cols:
                if kind == "p":
                    columns.append(Progression(payload))
                    described.append({"start": payload})
                else:
                    vals = [rng.choice(edge_values(prime)) for _ in range(payload)]
                    columns.append(vals)
                    described.append({"values": vals})
            T = K + len(cols)
            coef = [[draw() for _ in range(T + 1)] for _ in range(M)]
            uses = masks if masks is not None else [(2 << T) - 1] * M
            outs = lincomb_index(tables, columns, coef, uses, KAT_N, zero, one, add, mul)
            case[name] = {"n_tables": K, "n_index": len(cols), "n_outputs": M, "uses": uses, "n": KAT_N,
                          "tables": [[out(e) for e in t] for t in tables], "columns": described,
                          "coef": [[out(e) for e in row] for row in coef], "outs": [[out(e) for e in o] for o in outs]}

    for ring, ring_id in sorted(LC.POW2_RINGS.items(), key=lambda kv: kv[1]):
        p = SC.PRIMES[ring]
        add, _, mul = SC.vec_ops(p)
        rng = random.Random("lincomb index elements " + ring)
        draw = lambda: tuple(rng.choice((1, p - 1, rng.randrange(p), rng.randrange(p))) for _ in range(d_ring))  # noqa: E731
        case = {"ring": ring, "ring_id": ring_id, "log2_degree": KAT_LOG2_DEGREE, "form": "standard"}
        shapes(case, draw, p, (0,) * d_ring, (1,) * d_ring, add, mul, list)
        cases.append(case)
    for ring, (ring_id, base, fn, d, slot_w) in sorted(LC.SLOT_RINGS.items(), key=lambda kv: kv[1][0]):
        F = O.FIELD_ID[base]
        prime = LC.SLOT_PRIMES[base]
        words = O.fill_uniform(F, 0xA900 + ring_id, 0, 256 * d)
        pos = [0]

        def draw():
            e = words[pos[0] * d:(pos[0] + 1) * d].copy()
            pos[0] += 1
            return e

        mul = lambda r, a: O.small(fn, a, r)  # noqa: E731
        add = lambda a, b: ((a.astype(object) + b.astype(object)) % prime).astype(np.uint64)  # noqa: E731
        ints = lambda e: [int(x) for x in e]  # noqa: E731
        one = np.zeros(d, dtype=np.uint64)
        one[::slot_w] = O.to_mont(F, [1])[0]
        case = {"ring": ring, "ring_id": ring_id, "log2_degree": 0, "form": "memory"}
        shapes(case, draw, prime, np.zeros(d, dtype=np.uint64), one, add, mul, ints)
        assert pos[0] <= 256
        cases.append(case)
    return {"source": "tools/model_lincomb_index.py: one list of D words per ring element -- form `standard`: standard-form integers "
                      "(power-of-two rings); form `memory`: the u64 memory image (the reference's own rings, slot products of the "
                      "oracle); per shape: tables, columns ({values: the stored integers} or {start: of a progression}), coef "
                      "(n_outputs rows of n_tables + n_index + 1 elements: tables, columns, the constant), uses (one mask per output) "
                      "and outs (n_outputs lists of n elements)",
            "cases": cases}


def dump_kats():
    """the text of tests/golden/lincomb_index_kats.json"""
    return json.dumps(make_kats(), separators=(",", ":")) + "\n"


if __name__ == "__main__":
    root = os.path.dirname(HERE)
    sys.path.insert(0, os.path.join(root, "oracle"))
    path = os.path.join(root, "tests", "golden", "lincomb_index_kats.json")
    with open(path, "w") as f:
        f.write(dump_kats())
    print("wrote", path)
