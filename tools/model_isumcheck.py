"""Pure-Python restatement of the weighted sum-check rounds with INTEGER COLUMNS as factors (sr_vpoly_iwround_evals,
sr_vpoly_iwround_fold_evals), generic over the element type like tools/model_wsumcheck.py: the caller supplies zero, one, add, sub and
mul.  No kernel, no library call.

A slot of the sum of products is a table of ring elements or a column of u64 (a list of stored integers, the rest zero, or a
model_lincomb_index.Progression) that stands for the table R::from(col[e]); R::from is model_lincomb_index.from_u64.  Slots
0 .. K - 1 are the tables, K .. K + J - 1 the columns.

  iwround_evals   h(t) = sum_b w[b] sum_k c_k prod_s (lo_s[b] + t (hi_s[b] - lo_s[b])), t = 0 .. d, straight from the definition:
                  the pair of a slot is (x[2b], x[2b + 1]) in leading order and (x[b], x[b + half]) in trailing order, a column's x
                  embedded integer by integer -- no table is expanded and model_mle.fold is not used
  iwfold_round    every slot folded at r to lo + r (hi - lo) in truncated storage, then iwround_evals of the folded tables
  expand          the tables E_j = R::from(col_j[e]), e < n_evals_j: what the composition (from_u64_dev, then the weighted call) reads;
                  tests/test_isumcheck_host.py holds the two ways to each other through tools/model_wsumcheck.py

`python tools/model_isumcheck.py` rewrites tests/golden/isumcheck_kats.json.
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import model_lincomb_index as LI  # noqa: E402
import model_sumcheck as SC  # noqa: E402
import model_vpoly as VP  # noqa: E402
import model_vpoly_fold as VF  # noqa: E402
import model_wsumcheck as W  # noqa: E402

LEADING, TRAILING = W.LEADING, W.TRAILING
Progression = LI.Progression
U64 = 1 << 64

# the structures of tests/test_isumcheck_gpu.py: (K, J, terms); SHARED passes one column in both of its column slots
PLONK = (3, 5, [[3, 0], [4, 1], [5, 0, 1], [6, 2], [7]])  # q_L a + q_R b + q_M a b - q_O c + q_C: the -1 is the fourth coefficient
ALLCOL = (0, 2, [[0, 1]])
SQUARE = (1, 1, [[1, 1], [0, 1]])
SHARED = (1, 2, [[0, 1], [2]])
MIXED = (2, 2, [[0, 2], [1, 3], [0, 1]])
STRUCTURES = {"PLONK": PLONK, "ALLCOL": ALLCOL, "SQUARE": SQUARE, "SHARED": SHARED, "MIXED": MIXED}


def stored_len(col, num_vars):
    return 1 << num_vars if isinstance(col, Progression) else len(col)


def expand(columns, num_vars, zero, one, add):
    """the tables R::from(col_j[e]), e < n_evals_j (a progression: 2^num_vars)"""
    out = []
    for col in columns:
        n = stored_len(col, num_vars)
        assert n <= 1 << num_vars
        out.append([LI.from_u64(x, one, zero, add) for x in LI.column_values(col, n)])
    return out


def _slot_value(tables, columns, s, e, embed, zero):
    K = len(tables)
    if s < K:
        return tables[s][e] if e < len(tables[s]) else zero
    col = columns[s - K]
    if isinstance(col, Progression):
        assert col.start + e < U64
        return embed(col.start + e)
    return embed(col[e]) if e < len(col) else zero


def _pair(e_of, b, half, order):
    return (e_of(2 * b), e_of(2 * b + 1)) if order == LEADING else (e_of(b), e_of(b + half))


def iwround_evals(tables, columns, terms, coeffs, weights, num_vars, order, zero, one, add, sub, mul):
    """tables, columns: see above; weights: 2^(num_vars - 1) elements.  Returns [h(0), .., h(d)]."""
    assert num_vars >= 1 and len(weights) == 1 << (num_vars - 1)
    half, memo = 1 << (num_vars - 1), {}

    def embed(x):
        if x not in memo:
            memo[x] = LI.from_u64(x, one, zero, add)
        return memo[x]

    n_slots = len(tables) + len(columns)
    out = []
    for t in range(VP.degree(terms) + 1):
        tt = SC.constant(t, zero, one, add)
        total = [zero for _ in terms]
        for b, wb in enumerate(weights):
            at = []
            for s in range(n_slots):
                lo, hi = _pair(lambda e: _slot_value(tables, columns, s, e, embed, zero), b, half, order)
                at.append(add(lo, mul(tt, sub(hi, lo))))
            for k, term in enumerate(terms):
                pr = wb
                for s in term:
                    pr = mul(at[s], pr)
                total[k] = add(total[k], pr)
        h = zero
        for k, part in enumerate(total):
            h = add(h, part if coeffs is None else mul(coeffs[k], part))
        out.append(h)
    return out


def iwfold_round(tables, columns, terms, coeffs, weights, num_vars, r, order, zero, one, add, sub, mul):
    """num_vars >= 2; weights: 2^(num_vars - 2) elements.  Returns (the K + J folded slots in truncated storage, [h(0), .., h(d)])."""
    assert num_vars >= 2
    half = 1 << (num_vars - 1)
    embed = lambda x: LI.from_u64(x, one, zero, add)  # noqa: E731
    folded = []
    for s in range(len(tables) + len(columns)):
        n = len(tables[s]) if s < len(tables) else stored_len(columns[s - len(tables)], num_vars)
        g = []
        for b in range(VF.folded_len(n, num_vars, order)):
            lo, hi = _pair(lambda e: _slot_value(tables, columns, s, e, embed, zero), b, half, order)
            g.append(add(lo, mul(r, sub(hi, lo))))
        folded.append(g)
    return folded, W.wround_evals(folded, terms, coeffs, weights, num_vars - 1, order, zero, one, add, sub, mul)


# ---- pinned vectors ------------------------------------------------------------------------------------------------------------------------
KAT_STRUCTURES = ("PLONK", "ALLCOL")


def kat_columns(ring, name, nv):
    """the columns of a pinned case: 0/1 selectors, a progression from the last legal start, a truncated column and the values at and
    around p (2^64 - 1 on every ring)"""
    base = W.SLOT_RINGS[ring][1] if ring in W.SLOT_RINGS else ring
    p = W.SLOT_PRIMES[base] if ring in W.SLOT_RINGS else SC.PRIMES[ring]
    full = 1 << nv
    rng = random.Random("isumcheck columns %s %s" % (ring, name))
    edge = [x % U64 for x in (p - 1, p, p + 1)] + [U64 - 1]
    if name == "ALLCOL":
        return [(edge * full)[:full], Progression(U64 - full)]
    return [[rng.randrange(2) for _ in range(full)], (edge * full)[:full - 1], Progression(0), [rng.randrange(U64) for _ in range(full // 2 + 1)],
            Progression(U64 - full)]


def make_kats():
    cases = []
    for ring in W.RINGS:
        zero, one, add, sub, mul, draw, out, form = W.ring_ops(ring)
        rng = random.Random("isumcheck kats " + ring)
        nv = W.KAT_NUM_VARS if form == "standard" else W.KAT_SLOT_NUM_VARS
        full = 1 << nv
        for name in KAT_STRUCTURES:
            K, J, terms = STRUCTURES[name]
            n_evals = [full] * K
            if K:
                n_evals[-1] = full - 3
            columns = kat_columns(ring, name, nv)
            case = {"ring": ring, "form": form, "structure": name, "log2_degree": W.KAT_LOG2_DEGREE if form == "standard" else 0,
                    "num_vars": nv, "terms": terms, "n_evals": n_evals,
                    "columns": [{"start": c.start} if isinstance(c, Progression) else {"values": [str(x) for x in c]} for c in columns]}
            if form == "standard":
                tables = [draw(rng, n) for n in n_evals]
                coeffs = draw(rng, len(terms))
                w_round, w_fold, r = draw(rng, full // 2), draw(rng, full // 4), draw(rng, 1)[0]
            else:  # the inputs are not stored: model_wsumcheck.kat_inputs() makes them from the ring's name
                tables, coeffs, w_round, w_fold, r = W.kat_inputs(ring, n_evals, len(terms), nv)
            if name == "PLONK":
                coeffs[3] = sub(zero, one)
            if form == "standard":
                case.update({"tables": [[out(e) for e in f] for f in tables], "coeffs": [out(c) for c in coeffs],
                             "weights_round": [out(e) for e in w_round], "weights_fold": [out(e) for e in w_fold], "r": out(r)})
            for key, order in (("leading", LEADING), ("trailing", TRAILING)):
                msg = iwround_evals(tables, columns, terms, coeffs, w_round, nv, order, zero, one, add, sub, mul)
                folded, fmsg = iwfold_round(tables, columns, terms, coeffs, w_fold, nv, r, order, zero, one, add, sub, mul)
                case[key] = {"round": [out(e) for e in msg], "fold_message": [out(e) for e in fmsg]}
                if form == "standard":
                    case[key]["folded"] = [[out(e) for e in g] for g in folded]
            cases.append(case)
    return {"source": "tools/model_isumcheck.py: the layout of wsumcheck_kats.json; `columns` holds the integer columns (u64 as decimal "
                      "strings, or the start of a progression), slots K .. K + J - 1 of the terms; `folded` has K + J tables",
            "cases": cases}


def kat_column_values(case):
    """the columns of a pinned case as model objects"""
    return [Progression(int(c["start"])) if "start" in c else [int(x) for x in c["values"]] for c in case["columns"]]


def dump_kats():
    """the text of tests/golden/isumcheck_kats.json"""
    return json.dumps(make_kats(), separators=(",", ":")) + "\n"


if __name__ == "__main__":
    root = os.path.dirname(HERE)
    sys.path.insert(0, os.path.join(root, "oracle"))
    path = os.path.join(root, "tests", "golden", "isumcheck_kats.json")
    with open(path, "w") as f:
        f.write(dump_kats())
    print("wrote", path)
