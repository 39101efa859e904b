"""Pure-Python restatement of the WEIGHTED sum-check rounds (sr_vpoly_wround_evals, sr_vpoly_wround_fold_evals) and of a whole
sum-check of  sum_b eq(z, b) g(b)  that holds eq(z, .) as per-pair weights instead of a table (EqSumCheck), on the operations of
tools/model_vpoly.py / tools/model_vpoly_fold.py and generic over the element type like them: the caller supplies zero, one, add, sub
and mul.  No kernel, no library call.

  wround_evals   h(t) = sum_b w[b] * sum_k c_k prod_s f_{terms[k][s]}(t, b), t = 0 .. d: every table folded at R::from(t) by
                 model_mle.fold, multiplied term by term, by the pair's weight, scaled by the coefficient and summed.  The weight is no
                 factor: d is the longest term.
  wfold_round    the tables folded at r as model_vpoly_fold.fold_round folds them; h of the folded tables with the same weights
  eq_sumcheck    per round j: s_j(t) = [prod_{i bound} eq(z_i, r_i)] eq(z_v, t) h_j(t), t = 0 .. d + 1, with w = eq(z_rest, .);
                 h_j(d + 1) from h_j(0 .. d) by the finite-difference identity, which needs no division
  explicit       the same prover with eq(z, .) as one more factor of every term: model_vpoly.round_evals, then
                 model_vpoly_fold.fold_round -- what eq_sumcheck must send, element for element

`python tools/model_wsumcheck.py` rewrites tests/golden/wsumcheck_kats.json.
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import model_mle as M  # noqa: E402
import model_prod_tree as PT  # noqa: E402
import model_sparse_mle as SM  # noqa: E402
import model_sumcheck as SC  # noqa: E402
import model_vpoly as VP  # noqa: E402
import model_vpoly_fold as VF  # noqa: E402

LEADING, TRAILING = M.LEADING, M.TRAILING


def wround_evals(tables, terms, coeffs, weights, num_vars, order, zero, one, add, sub, mul):
    """tables: lists of at most 2^num_vars elements (the missing tail is zero), num_vars >= 1; weights: 2^(num_vars - 1) elements.
    Returns [h(0), .., h(d)]."""
    assert num_vars >= 1 and len(weights) == 1 << (num_vars - 1)
    padded = [M.pad(f, num_vars, zero) for f in tables]
    out = []
    for t in range(VP.degree(terms) + 1):
        r = SC.constant(t, zero, one, add)
        folded = [M.fold(f, num_vars, [r], order, add, sub, mul) for f in padded]
        total = zero
        for k, term in enumerate(terms):
            part = zero
            for b, wb in enumerate(weights):
                pr = wb
                for j in term:
                    pr = mul(folded[j][b], pr)
                part = add(part, pr)
            total = add(total, part if coeffs is None else mul(coeffs[k], part))
        out.append(total)
    return out


def wfold_round(tables, terms, coeffs, weights, num_vars, r, order, zero, one, add, sub, mul):
    """num_vars >= 2; weights: 2^(num_vars - 2) elements.  Returns (folded tables in truncated storage, [h(0), .., h(d)])."""
    assert num_vars >= 2
    folded = []
    for f in tables:
        g = M.fold(M.pad(f, num_vars, zero), num_vars, [r], order, add, sub, mul)
        folded.append(g[:VF.folded_len(len(f), num_vars, order)])
    return folded, wround_evals(folded, terms, coeffs, weights, num_vars - 1, order, zero, one, add, sub, mul)


def round_weights(z, j, order, sub, mul, one):
    """the weights of round j = 1 .. n: the eq table of z[j:] (leading) or z[:n - j] (trailing), 2^(n - j) elements"""
    n = len(z)
    return SM.precompute_eq(list(z[j:]) if order == LEADING else list(z[:n - j]), sub, mul, one)


def bound_coordinate(z, j, order):
    """the coordinate of z that round j binds"""
    return z[j - 1] if order == LEADING else z[len(z) - j]


def next_point(h, zero, add, sub):
    """h(d + 1) from h(0 .. d): sum_i (-1)^(d - i) C(d + 1, i) h(i), by additions and subtractions only"""
    d, c, total = len(h) - 1, 1, zero
    for i, hi in enumerate(h):
        for _ in range(c):
            total = add(total, hi) if (d - i) % 2 == 0 else sub(total, hi)
        c = c * (d + 1 - i) // (i + 1)
    return total


def eq_message(h, zv, prefix, zero, one, add, sub, mul):
    """s(0 .. d + 1) = prefix * eq(z_v, t) * h(t); eq(z_v, t) = (1 - z_v) + t (2 z_v - 1); the prefix product last"""
    hh = list(h) + [next_point(h, zero, add, sub)]
    e0 = sub(one, zv)
    step = sub(zv, e0)
    out, e = [], e0
    for ht in hh:
        out.append(mul(prefix, mul(e, ht)))
        e = add(e, step)
    return out


def eq_sumcheck(tables, terms, coeffs, z, challenges, order, zero, one, add, sub, mul):
    """the whole prover without an eq table.  tables in n = len(z) = len(challenges) variables.  Returns (messages: one list of
    d + 2 elements per round; the tables' values at the challenges; eq(z, r))."""
    n = len(z)
    assert n >= 1 and len(challenges) == n
    prefix, msgs = one, []
    h = wround_evals(tables, terms, coeffs, round_weights(z, 1, order, sub, mul, one), n, order, zero, one, add, sub, mul)
    for j in range(1, n + 1):
        zv, r = bound_coordinate(z, j, order), challenges[j - 1]
        msgs.append(eq_message(h, zv, prefix, zero, one, add, sub, mul))
        left = n - j + 1
        if left >= 2:
            tables, h = wfold_round(tables, terms, coeffs, round_weights(z, j + 1, order, sub, mul, one), left, r, order, zero, one, add, sub,
                                    mul)
        else:
            tables = [M.fold(M.pad(f, 1, zero), 1, [r], order, add, sub, mul) for f in tables]
        e0 = sub(one, zv)
        prefix = mul(prefix, add(e0, mul(r, sub(zv, e0))))
    return msgs, [f[0] for f in tables], prefix


def explicit(tables, terms, coeffs, z, challenges, order, zero, one, add, sub, mul):
    """the prover that holds eq(z, .) as table slot len(tables), a factor of every term.  Returns (messages of d + 2 elements; the
    values of the tables at the challenges, eq last)."""
    n = len(z)
    eq = SM.precompute_eq(list(z), sub, mul, one)
    tabs = list(tables) + [eq]
    eterms = [list(t) + [len(tables)] for t in terms]
    msgs = [VP.round_evals(tabs, eterms, coeffs, n, order, zero, one, add, sub, mul)]
    for j in range(1, n):
        tabs, msg = VF.fold_round(tabs, eterms, coeffs, n - j + 1, challenges[j - 1], order, zero, one, add, sub, mul)
        msgs.append(msg)
    tabs = [M.fold(M.pad(f, 1, zero), 1, [challenges[n - 1]], order, add, sub, mul) for f in tabs]
    return msgs, [f[0] for f in tabs]


# ---- the rings of the tests and of the pinned vectors ------------------------------------------------------------------------------
# the power-of-two rings slot-wise on standard-form integers; the reference's own rings on memory images with the oracle's slot products
POW2_RINGS = PT.POW2_RINGS
SLOT_RINGS = PT.SLOT_RINGS
SLOT_PRIMES = {"goldilocks": SC.PRIMES["goldilocks"], "babybear": SC.PRIMES["babybear"], "frog": 15912092521325583641}
FRACTION = [[0, 3], [1, 2], [2, 3]]  # tables p_lo, p_hi, q_lo, q_hi; coefficients (one, one, lambda): the layer claim of a fraction tree
# the pinned vectors, R1CS  c0 a b - c: D = 2 and three variables on the power-of-two rings; two variables (the smallest fold) and only
# the two messages on the reference's own rings, whose elements have 16 to 72 words (the folded tables are those of the unweighted call)
KAT_LOG2_DEGREE, KAT_NUM_VARS, KAT_SLOT_NUM_VARS = 1, 3, 2


def ring_ops(ring):
    """-> (zero, one, add, sub, mul, draw(rng-or-seed, n) -> n elements, out(element) -> list of ints, form)"""
    if ring in POW2_RINGS:
        p = SC.PRIMES[ring]
        d_ring = 1 << KAT_LOG2_DEGREE
        add, sub, mul = SC.vec_ops(p)
        draw = lambda rng, n: [tuple(rng.choice((0, 1, p - 1, rng.randrange(p))) for _ in range(d_ring)) for _ in range(n)]  # noqa: E731
        return (0,) * d_ring, (1,) * d_ring, add, sub, mul, draw, list, "standard"
    import numpy as np

    import oracle_lib as O

    ring_id, base, fn, d, slot_w = SLOT_RINGS[ring]
    F, prime = O.FIELD_ID[base], SLOT_PRIMES[base]
    zero = np.zeros(d, dtype=np.uint64)
    one = np.zeros(d, dtype=np.uint64)
    one[::slot_w] = O.to_mont(F, [1])[0]
    mul = lambda a, b: O.small(fn, a, b)  # noqa: E731
    add = lambda a, b: ((a.astype(object) + b.astype(object)) % prime).astype(np.uint64)  # noqa: E731
    sub = lambda a, b: ((a.astype(object) - b.astype(object)) % prime).astype(np.uint64)  # noqa: E731

    def draw(rng, n):
        words = O.fill_uniform(F, 0xA600 + ring_id + (rng.randrange(1 << 16) << 8), 0, n * d)
        return [words[i * d:(i + 1) * d].copy() for i in range(n)]

    return zero, one, add, sub, mul, draw, (lambda e: [int(x) for x in e]), "memory"


RINGS = sorted(POW2_RINGS, key=POW2_RINGS.get) + sorted(SLOT_RINGS, key=lambda r: SLOT_RINGS[r][0])


def kat_inputs(ring, n_evals, n_terms, nv):
    """the inputs of a pinned case of one of the reference's own rings, as memory images: (tables, coefficients -- R1CS sets the
    second to -one() --, the weights of the round call, the weights of the fused call, r), uniform from fixed seeds"""
    import oracle_lib as O

    ring_id, base, _, d, _ = SLOT_RINGS[ring]
    fill = lambda j, n: [e.copy() for e in O.fill_uniform(O.FIELD_ID[base], 0xA600 + 16 * ring_id + j, 0, n * d).reshape(n, d)]  # noqa: E731
    return [fill(j, n) for j, n in enumerate(n_evals)], fill(8, n_terms), fill(9, 1 << (nv - 1)), fill(10, 1 << (nv - 2)), fill(11, 1)[0]


def make_kats():
    cases = []
    for ring in RINGS:
        zero, one, add, sub, mul, draw, out, form = ring_ops(ring)
        rng = random.Random("wsumcheck kats " + ring)
        nv = KAT_NUM_VARS if form == "standard" else KAT_SLOT_NUM_VARS
        for name, terms in (("R1CS", [[0, 1], [2]]),):
            full = 1 << nv
            nt = VP.n_tables(terms)
            n_evals = [full] * nt
            n_evals[-1] = full - 3  # a truncated table: odd, beyond the half
            case = {"ring": ring, "form": form, "structure": name, "log2_degree": KAT_LOG2_DEGREE if form == "standard" else 0,
                    "num_vars": nv, "terms": terms, "n_evals": n_evals}
            if form == "standard":
                tables = [draw(rng, n) for n in n_evals]
                coeffs = draw(rng, len(terms))
                w_round, w_fold, r = draw(rng, full // 2), draw(rng, full // 4), draw(rng, 1)[0]
            else:  # the inputs are not stored: kat_inputs() makes them from the ring's name
                tables, coeffs, w_round, w_fold, r = kat_inputs(ring, n_evals, len(terms), nv)
            if name == "R1CS":
                coeffs[1] = sub(zero, one)
            if form == "standard":
                case.update({"tables": [[out(e) for e in f] for f in tables], "coeffs": [out(c) for c in coeffs],
                             "weights_round": [out(e) for e in w_round], "weights_fold": [out(e) for e in w_fold], "r": out(r)})
            for key, order in (("leading", LEADING), ("trailing", TRAILING)):
                msg = wround_evals(tables, terms, coeffs, w_round, nv, order, zero, one, add, sub, mul)
                folded, fmsg = wfold_round(tables, terms, coeffs, w_fold, nv, r, order, zero, one, add, sub, mul)
                case[key] = {"round": [out(e) for e in msg], "fold_message": [out(e) for e in fmsg]}
                if form == "standard":
                    case[key]["folded"] = [[out(e) for e in g] for g in folded]
            cases.append(case)
    return {"source": "tools/model_wsumcheck.py: one list of D words per ring element -- form `standard`: standard-form integers "
                      "(power-of-two rings); form `memory`: the u64 memory image (the reference's own rings, slot products of the "
                      "oracle); per order the weighted round h(0) .. h(d) with weights_round, and the folded tables in truncated "
                      "storage with the weighted message of the next round with weights_fold; form `memory` stores no inputs: "
                      "kat_inputs() makes them",
            "cases": cases}


def dump_kats():
    """the text of tests/golden/wsumcheck_kats.json"""
    return json.dumps(make_kats(), separators=(",", ":")) + "\n"


if __name__ == "__main__":
    root = os.path.dirname(HERE)
    sys.path.insert(0, os.path.join(root, "oracle"))
    path = os.path.join(root, "tests", "golden", "wsumcheck_kats.json")
    with open(path, "w") as f:
        f.write(dump_kats())
    print("wrote", path)
