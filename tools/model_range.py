"""Pure-Python restatement of the range-check round (sr_range_wround_evals) on the operations of tools/model_wsumcheck.py and generic
over the element type like it: the caller supplies zero, one, add, sub and mul.  No kernel, no library call.

  range_poly     P_B(x) = prod_{j = -(B-1)}^{B-1} (x - R::from(j)): the definition, literally -- all 2 B - 1 factors, no factoring;
                 R::from(j) from one() by additions or subtractions only
  wround_evals   h(t) = sum_b w[b] * sum_i mu_i * P_B(f_i(t, b)), t = 0 .. 2 B - 1: every table folded at R::from(t) by
                 model_mle.fold, P_B taken element by element, times the pair's weight, summed, scaled by the coefficient
  eq_sumcheck    the whole norm check sum_b eq(z, b) g(b) with eq as per-pair weights, round by round as model_wsumcheck.eq_sumcheck

`python tools/model_range.py` rewrites tests/golden/range_kats.json.
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import model_mle as M  # noqa: E402
import model_sumcheck as SC  # noqa: E402
import model_wsumcheck as WS  # noqa: E402

LEADING, TRAILING = M.LEADING, M.TRAILING


def from_int(j, zero, one, add, sub):
    """R::from(j) for a signed integer j"""
    x = zero
    for _ in range(abs(j)):
        x = add(x, one) if j > 0 else sub(x, one)
    return x


def range_poly(x, bound, zero, one, add, sub, mul):
    pr = None
    for j in range(-(bound - 1), bound):
        f = sub(x, from_int(j, zero, one, add, sub))
        pr = f if pr is None else mul(pr, f)
    return pr


def wround_evals(tables, bound, coeffs, weights, num_vars, order, zero, one, add, sub, mul):
    """tables: lists of at most 2^num_vars elements (the missing tail is zero), num_vars >= 1; weights: 2^(num_vars - 1) elements;
    coeffs: one element per table or None.  Returns [h(0), .., h(2 bound - 1)]."""
    assert num_vars >= 1 and len(weights) == 1 << (num_vars - 1)
    padded = [M.pad(f, num_vars, zero) for f in tables]
    out = []
    for t in range(2 * bound):
        r = SC.constant(t, zero, one, add)
        total = zero
        for i, f in enumerate(padded):
            g = M.fold(f, num_vars, [r], order, add, sub, mul)
            part = zero
            for b, wb in enumerate(weights):
                part = add(part, mul(wb, range_poly(g[b], bound, zero, one, add, sub, mul)))
            total = add(total, part if coeffs is None else mul(coeffs[i], part))
        out.append(total)
    return out


def eq_sumcheck(tables, bound, coeffs, z, challenges, order, zero, one, add, sub, mul):
    """the whole prover without an eq table.  Returns (messages: one list of 2 bound + 1 elements per round; the tables' values at the
    challenges; eq(z, r))."""
    n = len(z)
    assert n >= 1 and len(challenges) == n
    prefix, msgs = one, []
    for j in range(1, n + 1):
        left = n - j + 1
        h = wround_evals(tables, bound, coeffs, WS.round_weights(z, j, order, sub, mul, one), left, order, zero, one, add, sub, mul)
        zv, r = WS.bound_coordinate(z, j, order), challenges[j - 1]
        msgs.append(WS.eq_message(h, zv, prefix, zero, one, add, sub, mul))
        tables = [M.fold(M.pad(f, left, zero), left, [r], order, add, sub, mul) for f in tables]
        e0 = sub(one, zv)
        prefix = mul(prefix, add(e0, mul(r, sub(zv, e0))))
    return msgs, [f[0] for f in tables], prefix


# ---- the rings of the tests and of the pinned vectors: those of model_wsumcheck --------------------------------------------------------
ring_ops = WS.ring_ops
RINGS = WS.RINGS
POW2_RINGS, SLOT_RINGS = WS.POW2_RINGS, WS.SLOT_RINGS
# the pinned vectors: two tables, bound 3 (six points, five factors), coefficients; D = 2 and three variables on the power-of-two rings,
# two variables on the reference's own rings
KAT_LOG2_DEGREE, KAT_NUM_VARS, KAT_SLOT_NUM_VARS, KAT_BOUND = WS.KAT_LOG2_DEGREE, 3, 2, 3


def kat_inputs(ring, n_evals, nv):
    """the inputs of a pinned case of one of the reference's own rings, as memory images: (tables, coefficients, weights)"""
    import oracle_lib as O

    ring_id, base, _, d, _ = SLOT_RINGS[ring]
    fill = lambda j, n: [e.copy() for e in O.fill_uniform(O.FIELD_ID[base], 0xB700 + 16 * ring_id + j, 0, n * d).reshape(n, d)]  # noqa: E731
    return [fill(j, n) for j, n in enumerate(n_evals)], fill(8, len(n_evals)), fill(9, 1 << (nv - 1))


def make_kats():
    cases = []
    for ring in RINGS:
        zero, one, add, sub, mul, draw, out, form = ring_ops(ring)
        rng = random.Random("range kats " + ring)
        nv = KAT_NUM_VARS if form == "standard" else KAT_SLOT_NUM_VARS
        full = 1 << nv
        n_evals = [full, full - 1]  # a truncated table: odd, beyond the half
        case = {"ring": ring, "form": form, "log2_degree": KAT_LOG2_DEGREE if form == "standard" else 0, "num_vars": nv, "bound": KAT_BOUND,
                "n_evals": n_evals}
        if form == "standard":
            tables = [draw(rng, n) for n in n_evals]
            coeffs, weights = draw(rng, len(n_evals)), draw(rng, full // 2)
            case.update({"tables": [[out(e) for e in f] for f in tables], "coeffs": [out(c) for c in coeffs],
                         "weights": [out(e) for e in weights]})
        else:  # the inputs are not stored: kat_inputs() makes them from the ring's name
            tables, coeffs, weights = kat_inputs(ring, n_evals, nv)
        for key, order in (("leading", LEADING), ("trailing", TRAILING)):
            msg = wround_evals(tables, KAT_BOUND, coeffs, weights, nv, order, zero, one, add, sub, mul)
            case[key] = [out(e) for e in msg]
        cases.append(case)
    return {"source": "tools/model_range.py: one list of D words per ring element -- form `standard`: standard-form integers "
                      "(power-of-two rings); form `memory`: the u64 memory image (the reference's own rings, slot products of the "
                      "oracle); per order the range-check round h(0) .. h(2 bound - 1); form `memory` stores no inputs: kat_inputs() "
                      "makes them",
            "cases": cases}


def dump_kats():
    """the text of tests/golden/range_kats.json"""
    return json.dumps(make_kats(), separators=(",", ":")) + "\n"


if __name__ == "__main__":
    root = os.path.dirname(HERE)
    sys.path.insert(0, os.path.join(root, "oracle"))
    path = os.path.join(root, "tests", "golden", "range_kats.json")
    with open(path, "w") as f:
        f.write(dump_kats())
    print("wrote", path)
