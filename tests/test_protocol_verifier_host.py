"""The verifier of tests/protocol_verifier.py against the pure-Python provers (tools/model_wsumcheck.py eq_sumcheck and explicit,
tools/model_range.py eq_sumcheck, the layers of tools/model_prod_tree.py and tools/model_frac_tree.py with their layer claims built
by hand): every honest transcript is accepted, and every mutation below is rejected, in the round and for the reason it must be.
Without this file an accepting run of tests/test_protocols_gpu.py would say nothing.  The rings: Z_p for p = 97 and the Goldilocks
prime, Z_97[X] / (X^2 - 3) whose product is not slot-wise, and goldilocks24 on the oracle's Fq3 slot products.

Which mutation covers which check of verify_rounds / verify_eq_sumcheck (no other check sees it):
  msg[0] + msg[1] == claim        claim0 off by one()
  the number of points            one more point behind a message (the reason is asserted)
  finals from the raw tables      a raw table entry changed after the proof; a final dropped
  eq_r == eq(z, point)            an honest proof of a true zero claim for another z
  last claim == eq_r g(finals)    the last element of the last message off by one()
"""
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tools"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
import model_frac_tree as FT  # noqa: E402
import model_mle as M  # noqa: E402
import model_prod_tree as PT  # noqa: E402
import model_range as RG  # noqa: E402
import model_vpoly as VP  # noqa: E402
import model_vpoly_fold as VF  # noqa: E402
import model_wsumcheck as W  # noqa: E402
import protocol_verifier as PV  # noqa: E402
from protocol_verifier import CLAIM, EQ, FINAL, LEAVES, LENGTH, POINT, ROOT as BAD_ROOT, SUM, Rejected, same  # noqa: E402

LEADING, TRAILING = 0, 1
ORDERS = (LEADING, TRAILING)
GOLDILOCKS = 0xFFFFFFFF00000001
RINGS = ["z97", "zgoldilocks", "quadratic97", "goldilocks24"]
KINDS = {"product": [[0, 1]], "r1cs": [[0, 1], [2]], "fraction": W.FRACTION}


class Ring:
    """(the verifier over the ring, draw(rng, n) -> n uniform elements)"""

    def __init__(self, name):
        if name in ("z97", "zgoldilocks"):
            p = 97 if name == "z97" else GOLDILOCKS
            ops = (0, 1, lambda a, b: (a + b) % p, lambda a, b: (a - b) % p, lambda a, b: a * b % p)
            self.draw = lambda rng, n: [rng.randrange(p) for _ in range(n)]
        elif name == "quadratic97":
            p = 97
            ops = ((0, 0), (1, 0), lambda a, b: ((a[0] + b[0]) % p, (a[1] + b[1]) % p), lambda a, b: ((a[0] - b[0]) % p, (a[1] - b[1]) % p),
                   lambda r, a: ((r[0] * a[0] + 3 * r[1] * a[1]) % p, (r[0] * a[1] + r[1] * a[0]) % p))
            self.draw = lambda rng, n: [(rng.randrange(p), rng.randrange(p)) for _ in range(n)]
        else:
            zero, one, add, sub, mul, self.draw, _, _ = W.ring_ops(name)
            ops, p = (zero, one, add, sub, mul), W.SLOT_PRIMES[W.SLOT_RINGS[name][1]]
        self.ops = ops
        self.V = PV.Verifier(*ops, p)


_rings = {}


def ring_of(name):
    if name not in _rings:
        _rings[name] = Ring(name)
    return _rings[name]


def g_of_terms(V, terms, coeffs):
    """g of the tables' values, term by term"""
    def g(vals):
        return V.sum(V.mul(V.prod(vals[j] for j in term), V.one if coeffs is None else coeffs[k]) for k, term in enumerate(terms))
    return g


def claimed_sum(V, z, nv, g_at):
    """sum_b eq(z, b) g(b) over the cube, g_at(b) the value of g at index b"""
    return V.sum(V.mul(V.eq_eval(z, V.bits(b, nv)), g_at(b)) for b in range(1 << nv))


def rejects(call, round, reason, layer=None):
    with pytest.raises(Rejected) as e:
        call()
    assert (e.value.round, e.value.reason, e.value.layer) == (round, reason, layer), str(e.value)


def first_generic(name, body):
    """body(salt) builds the transcript of that seed and runs its mutations.  A mutated transcript is accepted, or fails a later check
    than the one named, where a challenge happens to be a root of the difference: the soundness error of the protocol itself, about
    degree / |field| per round.  Over the Goldilocks prime that never happens and the first seed has to do.  Over 97 it happens in
    several of a hundred mutations, so there the seed is the first of eight whose mutations all land where they must; an honest
    transcript that is rejected fails at once whatever the seed."""
    if name in ("zgoldilocks", "goldilocks24"):
        return body(0)
    failures = []
    for salt in range(8):
        try:
            return body(salt)
        except (AssertionError, pytest.fail.Exception) as e:
            failures.append(e)
    raise failures[0]


def bump(V, msgs, j, i):
    """the messages with element i of round j (1 ..) off by one()"""
    out = [list(m) for m in msgs]
    out[j - 1][i] = V.add(out[j - 1][i], V.one)
    return out


# ---- the verifier's own pieces, against closed forms on a prime field ---------------------------------------------------------------------
def test_scalars_interpolation_and_the_variable_order_of_the_extension():
    p = 97
    V = ring_of("z97").V
    assert [V.scalar(c) for c in (0, 1, 5, 96, 97, -1, 200)] == [0, 1, 5, 96, 0, 96, 6]
    assert all(V.scalar(c) * V.inv_scalar(c) % p == 1 for c in range(1, p))
    coeffs = [3, 0, 7, 11, 2]
    poly = lambda x: sum(c * x ** i for i, c in enumerate(coeffs)) % p  # noqa: E731
    assert all(V.interpolate([poly(t) for t in range(5)], r) == poly(r) for r in range(p))
    assert all(V.interpolate([poly(t) for t in range(7)], r) == poly(r) for r in (0, 6, 50))
    # variable 0 is the lowest index bit: the extension of the table b -> bit 0 of b is x_0
    assert V.mle_eval([0, 1, 0, 1, 0, 1, 0, 1], [10, 20, 30]) == 10 and V.mle_eval([0, 0, 0, 0, 1, 1, 1, 1], [10, 20, 30]) == 30
    assert V.mle_eval([5, 6, 7], [0, 1], pad=9) == 7 and V.mle_eval([5, 6, 7], [1, 1], pad=9) == 9 and V.mle_eval([5, 6, 7], [1, 1]) == 0
    assert all(V.eq_eval(V.bits(a, 3), V.bits(b, 3)) == (a == b) for a in range(8) for b in range(8))
    assert V.eq_eval([10, 20], [30, 40]) == (10 * 30 + 9 * 29) * (20 * 40 + 19 * 39) % p
    assert V.point_of([1, 2, 3], LEADING) == [1, 2, 3] and V.point_of([1, 2, 3], TRAILING) == [3, 2, 1]
    assert V.range_poly(5, 3) == (5 + 2) * (5 + 1) * 5 * (5 - 1) * (5 - 2) % p
    assert all((V.range_poly(V.scalar(j), 4) == 0) == (abs(j) < 4) for j in range(-6, 7))
    # on a ring whose product is not slot-wise the interpolation still goes through the points
    Q = ring_of("quadratic97").V
    rng = random.Random(3)
    c = ring_of("quadratic97").draw(rng, 4)
    qpoly = lambda x: Q.sum(Q.mul(ci, Q.prod([x] * i)) for i, ci in enumerate(c))  # noqa: E731
    r = (5, 17)
    assert Q.interpolate([qpoly(Q.scalar(t)) for t in range(4)], r) == qpoly(r)


# ---- the eq sum-check --------------------------------------------------------------------------------------------------------------------------
def eq_case(name, kind, nv, order, zero_claim=False, salt=0):
    """an honest transcript of model_wsumcheck.eq_sumcheck as the keyword arguments of verify_eq_sumcheck"""
    R = ring_of(name)
    V, rng = R.V, random.Random("verifier %s %s %d %d %d" % (name, kind, nv, order, salt))
    zero, one, add, sub, mul = R.ops
    terms = KINDS[kind]
    tables = [R.draw(rng, 1 << nv) for _ in range(VP.n_tables(terms))]
    if kind == "r1cs" and zero_claim:
        tables[2] = [mul(a, b) for a, b in zip(tables[0], tables[1])]
    coeffs = {"product": None, "r1cs": [one, sub(zero, one)], "fraction": [one, one] + R.draw(rng, 1)}[kind]
    z, rs = R.draw(rng, nv), R.draw(rng, nv)
    msgs, finals, eq_r = W.eq_sumcheck(tables, terms, coeffs, z, rs, order, zero, one, add, sub, mul)
    g = g_of_terms(V, terms, coeffs)
    claim0 = claimed_sum(V, z, nv, lambda b: g([t[b] for t in tables]))
    return V, dict(claim0=claim0, z=z, messages=msgs, challenges=rs, finals=finals, eq_r=eq_r, order=order, g_of=g, tables=tables,
                   points=VP.degree(terms) + 2)


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("nv", [3, 4])
@pytest.mark.parametrize("name", RINGS)
def test_honest_eq_sumchecks_are_accepted(name, nv, order, kind):
    V, case = eq_case(name, kind, nv, order)
    point = V.verify_eq_sumcheck(**case)
    assert len(point) == nv and same(point[0], case["challenges"][0 if order == LEADING else nv - 1])
    V, case = eq_case(name, "r1cs", nv, order, zero_claim=True)
    assert same(case["claim0"], V.zero)
    V.verify_eq_sumcheck(**case)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("nv", [3, 4])
@pytest.mark.parametrize("name", RINGS)
def test_every_mutation_of_an_eq_sumcheck_is_rejected_where_it_must_be(name, nv, order):
    first_generic(name, lambda salt: eq_mutations(name, nv, order, salt))


def eq_mutations(name, nv, order, salt):
    V, case = eq_case(name, "fraction", nv, order, salt=salt)
    V.verify_eq_sumcheck(**case)
    run = lambda **kw: (lambda: V.verify_eq_sumcheck(**dict(case, **kw)))  # noqa: E731
    msgs, rs, finals, tables, z = case["messages"], case["challenges"], case["finals"], case["tables"], case["z"]
    top = len(msgs[0]) - 1
    behind = lambda j: (j + 1, SUM) if j < nv else (None, CLAIM)  # noqa: E731  where an error that round j itself cannot see shows
    # one element off by one(), in the first, a middle and the last round: an element of the round's sum there, another one a round on
    for j in (1, 2, nv):
        rejects(run(messages=bump(V, msgs, j, 0)), j, SUM)
        rejects(run(messages=bump(V, msgs, j, 1)), j, SUM)
        rejects(run(messages=bump(V, msgs, j, top)), *behind(j))
    # msg[0] and msg[1] swapped: the round's sum holds, its polynomial is another one
    for j in (1, 2, nv):
        swapped = [list(m) for m in msgs]
        swapped[j - 1][0], swapped[j - 1][1] = msgs[j - 1][1], msgs[j - 1][0]
        rejects(run(messages=swapped), *behind(j))
    # a challenge of another round used to interpolate; behind the last round it shows in the point
    for j, k in ((1, 2), (2, nv), (nv, 1)):
        other = list(rs)
        other[j - 1] = rs[k - 1]
        rejects(run(challenges=other), *((j + 1, SUM) if j < nv else (None, FINAL)))
    rejects(run(order=1 - order), None, FINAL)                          # the point assembled in the other order
    rejects(run(claim0=V.add(case["claim0"], V.one)), 1, SUM)
    rejects(run(finals=[finals[1]] + finals[1:]), None, FINAL)          # the other table's final
    rejects(run(finals=finals[:-1]), None, FINAL)
    point = V.point_of(rs, order)
    rejects(run(eq_r=V.eq_eval(list(reversed(z)), point)), None, EQ)
    for at in (0, (1 << nv) - 1):                                       # a raw table entry changed after the proof
        changed = [list(t) for t in tables]
        changed[3][at] = V.add(changed[3][at], V.one)
        rejects(run(tables=changed), None, FINAL)
    rejects(run(messages=[m + [m[0]] if i == 1 else m for i, m in enumerate(msgs)]), 2, LENGTH)
    rejects(run(messages=[m[:1] for m in msgs], points=None), 1, LENGTH)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", RINGS)
def test_an_honest_proof_of_a_zero_claim_for_another_z_fails_only_the_eq_check(name, order):
    def body(salt):
        V, case = eq_case(name, "r1cs", 3, order, zero_claim=True, salt=salt)
        other = list(case["z"])
        other[1] = V.add(other[1], V.one)
        rejects(lambda: V.verify_eq_sumcheck(**dict(case, z=other)), None, EQ)

    first_generic(name, body)


# ---- the explicit prover and the plain sum-check -----------------------------------------------------------------------------------------------
def plain_prover(tables, terms, coeffs, rs, order, ops):
    """the messages of sum_b g(b) and the tables' values at the challenges: model_vpoly.round_evals, then model_vpoly_fold.fold_round"""
    zero, one, add, sub, mul = ops
    n = len(rs)
    tabs = list(tables)
    msgs = [VP.round_evals(tabs, terms, coeffs, n, order, zero, one, add, sub, mul)]
    for j in range(1, n):
        tabs, msg = VF.fold_round(tabs, terms, coeffs, n - j + 1, rs[j - 1], order, zero, one, add, sub, mul)
        msgs.append(msg)
    return msgs, [M.fold(M.pad(f, 1, zero), 1, [rs[n - 1]], order, add, sub, mul)[0] for f in tabs]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("nv", [3, 4])
@pytest.mark.parametrize("name", RINGS)
def test_the_explicit_prover_and_the_plain_sum_check(name, nv, order):
    first_generic(name, lambda salt: explicit_and_plain(name, nv, order, salt))


def explicit_and_plain(name, nv, order, salt):
    R = ring_of(name)
    V = R.V
    zero, one, add, sub, mul = R.ops
    # the explicit prover holds eq(z, .) as one more table: its final value stands behind the tables'
    rng = random.Random("explicit %s %d %d %d" % (name, nv, order, salt))
    terms = VP.R1CS[:1] + [[3]]   # a b c - d with coefficients
    tables = [R.draw(rng, (1 << nv) - (3 if i == 1 else 0)) for i in range(4)]   # one table truncated: its tail is zero
    coeffs, z, rs = R.draw(rng, 2), R.draw(rng, nv), R.draw(rng, nv)
    g = g_of_terms(V, terms, coeffs)
    at = lambda t, b: t[b] if b < len(t) else zero  # noqa: E731
    msgs, finals = W.explicit(tables, terms, coeffs, z, rs, order, zero, one, add, sub, mul)
    case = dict(claim0=claimed_sum(V, z, nv, lambda b: g([at(t, b) for t in tables])), z=z, messages=msgs, challenges=rs, finals=finals[:-1],
                eq_r=finals[-1], order=order, g_of=g, tables=tables, points=VP.degree(terms) + 2)
    V.verify_eq_sumcheck(**case)
    rejects(lambda: V.verify_eq_sumcheck(**dict(case, messages=bump(V, msgs, nv, 4))), None, CLAIM)
    rejects(lambda: V.verify_eq_sumcheck(**dict(case, pad=one)), None, FINAL)   # the tail of a truncated table is zero, not one
    # the plain sum-check of the same g
    msgs, finals = plain_prover(tables, terms, coeffs, rs, order, R.ops)
    plain = dict(claim0=V.sum(g([at(t, b) for t in tables]) for b in range(1 << nv)), messages=msgs, challenges=rs, finals=finals, order=order,
                 g_of=g, tables=tables, points=VP.degree(terms) + 1)
    V.verify_sumcheck(**plain)
    rejects(lambda: V.verify_sumcheck(**dict(plain, claim0=V.add(plain["claim0"], one))), 1, SUM)
    rejects(lambda: V.verify_sumcheck(**dict(plain, messages=bump(V, msgs, 1, 3))), 2, SUM)
    rejects(lambda: V.verify_sumcheck(**dict(plain, messages=bump(V, msgs, nv, 3))), None, CLAIM)
    rejects(lambda: V.verify_sumcheck(**dict(plain, order=1 - order)), None, FINAL)
    rejects(lambda: V.verify_sumcheck(**dict(plain, finals=finals[:-1])), None, FINAL)
    changed = [list(t) for t in tables]
    changed[2][5] = add(changed[2][5], one)
    rejects(lambda: V.verify_sumcheck(**dict(plain, tables=changed)), None, FINAL)


# ---- the range check -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("nv", [3, 4])
@pytest.mark.parametrize("name", RINGS)
def test_the_range_check_prover(name, nv, order):
    """model_range.eq_sumcheck at bound 2 (nv 3: bound 3 as well) over two tables with coefficients: in-range tables claim zero; one
    entry R::from(B) does not, and verifies against the true sum only"""
    first_generic(name, lambda salt: range_checks(name, nv, order, salt))


def range_checks(name, nv, order, salt):
    R = ring_of(name)
    V = R.V
    zero, one, add, sub, mul = R.ops
    rng = random.Random("range %s %d %d %d" % (name, nv, order, salt))
    for B in (2, 3) if nv == 3 else (2,):
        tables = [[V.scalar(rng.randrange(-(B - 1), B)) for _ in range(1 << nv)] for _ in range(2)]
        mu, z, rs = R.draw(rng, 2), R.draw(rng, nv), R.draw(rng, nv)
        g = lambda vals: V.sum(V.mul(m, V.range_poly(v, B)) for m, v in zip(mu, vals))  # noqa: E731
        msgs, finals, eq_r = RG.eq_sumcheck(tables, B, mu, z, rs, order, zero, one, add, sub, mul)
        case = dict(claim0=zero, z=z, messages=msgs, challenges=rs, finals=finals, eq_r=eq_r, order=order, g_of=g, tables=tables, points=2 * B + 1)
        V.verify_eq_sumcheck(**case)
        rejects(lambda: V.verify_eq_sumcheck(**dict(case, messages=bump(V, msgs, nv, 2 * B))), None, CLAIM)
        planted = [list(t) for t in tables]
        planted[1][5] = V.scalar(B)
        msgs, finals, eq_r = RG.eq_sumcheck(planted, B, mu, z, rs, order, zero, one, add, sub, mul)
        case.update(messages=msgs, finals=finals, eq_r=eq_r, tables=planted)
        rejects(lambda: V.verify_eq_sumcheck(**case), 1, SUM)
        true_sum = claimed_sum(V, z, nv, lambda b: g([t[b] for t in planted]))
        assert not same(true_sum, zero)
        V.verify_eq_sumcheck(**dict(case, claim0=true_sum))


# ---- the trees -------------------------------------------------------------------------------------------------------------------------------------
def descend(R, rng, nv, stop, halves_of, terms, with_lam, tau_first=False, no_lam_at=None):
    """the layer claims of a trailing-order tree by hand: per layer k = nv - 1 .. stop + 1 the tables halves_of(k) (the lower and upper
    halves of layer k - 1), model_wsumcheck.eq_sumcheck over them in trailing order, and the next point (point, tau) -- (tau, point)
    with tau_first, the mutation.  no_lam_at: the layer whose prover leaves lambda out.  Returns (z_top, layers)."""
    zero, one, add, sub, mul = R.ops
    z_top = R.draw(rng, 1)
    z, out = list(z_top), {}
    for k in range(nv - 1, stop, -1):
        m = nv - k
        rs, (tau,) = R.draw(rng, m), R.draw(rng, 1)
        t = {"z": list(z), "challenges": rs, "tau": tau}
        coeffs = None
        if with_lam:
            (t["lam"],) = R.draw(rng, 1)
            coeffs = [one, one, one if k == no_lam_at else t["lam"]]
        t["messages"], t["finals"], t["eq_r"] = W.eq_sumcheck(halves_of(k), terms, coeffs, z, rs, TRAILING, zero, one, add, sub, mul)
        out[k] = t
        point = list(reversed(rs))   # trailing order: the last challenge bound variable 0
        z = [tau] + point if tau_first else point + [tau]
    return z_top, out


def product_case(name, nv, n_leaves, stop, salt=0, **kw):
    R = ring_of(name)
    rng = random.Random("product tree %s %d %d %d" % (name, nv, n_leaves, salt))
    leaves = R.draw(rng, n_leaves)
    L = PT.layers(leaves, nv, TRAILING, R.ops[1], R.ops[4])
    halves = lambda k: [L[k - 1][:1 << (nv - k)], L[k - 1][1 << (nv - k):]]  # noqa: E731
    z_top, layers = descend(R, rng, nv, stop, halves, [[0, 1]], False, **kw)
    return R.V, leaves, dict(nv=nv, top=L[nv - 1], z_top=z_top, layers=layers, stop=stop)


def fraction_case(name, nv, n_leaves, stop, numerators=True, salt=0, **kw):
    R = ring_of(name)
    zero, one, add, sub, mul = R.ops
    rng = random.Random("fraction tree %s %d %d %d" % (name, nv, n_leaves, salt))
    p, q = (R.draw(rng, n_leaves) if numerators else None), R.draw(rng, n_leaves)
    Ps, Qs = FT.layers(p, q, nv, TRAILING, zero, one, add, mul)
    h = lambda k: 1 << (nv - k)  # noqa: E731
    halves = lambda k: [Ps[k - 1][:h(k)], Ps[k - 1][h(k):], Qs[k - 1][:h(k)], Qs[k - 1][h(k):]]  # noqa: E731
    z_top, layers = descend(R, rng, nv, stop, halves, W.FRACTION, True, **kw)
    top = ((Ps[nv - 1][0], Qs[nv - 1][0]), (Ps[nv - 1][1], Qs[nv - 1][1]))
    return R.V, p, q, dict(nv=nv, top=top, z_top=z_top, layers=layers, stop=stop)


def with_layer(case, k, **changes):
    layers = dict(case["layers"])
    layers[k] = dict(layers[k], **changes)
    return dict(case, layers=layers)


@pytest.mark.parametrize("nv,n_leaves,stop", [(3, 8, 0), (4, 16, 0), (4, 11, 1), (3, 5, 0)])
@pytest.mark.parametrize("name", RINGS)
def test_the_product_tree_descent(name, nv, n_leaves, stop):
    first_generic(name, lambda salt: product_descent(name, nv, n_leaves, stop, salt))


def product_descent(name, nv, n_leaves, stop, salt):
    V, leaves, case = product_case(name, nv, n_leaves, stop, salt)
    z = V.verify_product_tree(leaves, **case)
    assert len(z) == nv - stop
    run = lambda lv=leaves, **kw: (lambda: V.verify_product_tree(lv, **dict(case, **kw)))  # noqa: E731
    # a leaf changed after the tree was built: the root; two leaves exchanged keep the root and fail at the leaves
    changed = list(leaves)
    changed[2] = V.add(changed[2], V.one)
    rejects(run(changed), None, BAD_ROOT, nv)
    changed = list(leaves)
    changed[1], changed[2] = leaves[2], leaves[1]
    rejects(run(changed), None, LEAVES, stop)
    rejects(run(top=[V.add(case["top"][0], V.one), case["top"][1]]), None, BAD_ROOT, nv)
    for k in sorted(case["layers"]):
        t = case["layers"][k]
        nxt = (lambda r, why: (r, why, k - 1)) if k - 1 > stop else (lambda r, why: (None, LEAVES, stop))
        rejects(lambda: V.verify_product_tree(leaves, **with_layer(case, k, messages=bump(V, t["messages"], 1, 0))), 1, SUM, k)
        rejects(lambda: V.verify_product_tree(leaves, **with_layer(case, k, messages=bump(V, t["messages"], nv - k, 3))), None, CLAIM, k)
        rejects(lambda: V.verify_product_tree(leaves, **with_layer(case, k, eq_r=V.add(t["eq_r"], V.one))), None, EQ, k)
        if k - 1 > stop:   # a tau other than the one the next layer was proved at (behind the last layer tau is the verifier's own)
            rejects(lambda: V.verify_product_tree(leaves, **with_layer(case, k, tau=V.add(t["tau"], V.one))), None, POINT, k - 1)
        # lo and hi exchanged: the layer's own claim is symmetric in them and holds; the claim handed down does not
        rejects(lambda: V.verify_product_tree(leaves, **with_layer(case, k, finals=t["finals"][::-1])), *nxt(1, SUM))
    # tau at the wrong end of the next point, by a prover that is honest about that point from then on
    V, leaves, wrong = product_case(name, nv, n_leaves, stop, salt, tau_first=True)
    assert nv - 2 > stop   # there is a next layer whose point the prover states
    rejects(lambda: V.verify_product_tree(leaves, **wrong), None, POINT, nv - 2)


@pytest.mark.parametrize("nv,n_leaves,stop,numerators", [(3, 8, 0, True), (4, 16, 0, True), (4, 11, 1, True), (3, 8, 1, False), (4, 13, 1, False)])
@pytest.mark.parametrize("name", RINGS)
def test_the_fraction_tree_descent(name, nv, n_leaves, stop, numerators):
    first_generic(name, lambda salt: fraction_descent(name, nv, n_leaves, stop, numerators, salt))


def fraction_descent(name, nv, n_leaves, stop, numerators, salt):
    V, p, q, case = fraction_case(name, nv, n_leaves, stop, numerators, salt)
    z, (P, Q) = V.verify_fraction_tree(p, q, **case)
    assert len(z) == nv - stop
    # the root by the definition of a sum of fractions, once more in the open: Q = prod q_i, P = sum_i p_i prod_{j != i} q_j
    ps = p if p is not None else [V.one] * n_leaves
    assert same(Q, V.prod(q)) and same(P, V.sum(V.mul(ps[i], V.prod(q[j] for j in range(n_leaves) if j != i)) for i in range(n_leaves)))
    changed = list(q)
    changed[2] = V.add(changed[2], V.one)
    rejects(lambda: V.verify_fraction_tree(p, changed, **case), None, BAD_ROOT, nv)
    swapped = list(q)   # two fractions exchanged (with their numerators): the sum stays, the leaves do not
    swapped[1], swapped[2] = q[2], q[1]
    sp = None
    if p is not None:
        sp = list(p)
        sp[1], sp[2] = p[2], p[1]
    rejects(lambda: V.verify_fraction_tree(sp, swapped, **case), None, LEAVES, stop)
    if p is not None:
        rejects(lambda: V.verify_fraction_tree(None, q, **case), None, BAD_ROOT, nv)
    for k in sorted(case["layers"]):
        t = case["layers"][k]
        nxt = (lambda r, why: (r, why, k - 1)) if k - 1 > stop else (lambda r, why: (None, LEAVES, stop))
        rejects(lambda: V.verify_fraction_tree(p, q, **with_layer(case, k, messages=bump(V, t["messages"], 1, 1))), 1, SUM, k)
        rejects(lambda: V.verify_fraction_tree(p, q, **with_layer(case, k, messages=bump(V, t["messages"], nv - k, 3))), None, CLAIM, k)
        if k - 1 > stop:
            rejects(lambda: V.verify_fraction_tree(p, q, **with_layer(case, k, tau=V.add(t["tau"], V.one))), None, POINT, k - 1)
        # lambda used by the verifier, left out by the prover of this layer alone
        _, p2, q2, bad = fraction_case(name, nv, n_leaves, stop, numerators, salt, no_lam_at=k)
        rejects(lambda: V.verify_fraction_tree(p2, q2, **bad), 1, SUM, k)
        # lo and hi exchanged in all four finals: p_lo q_hi + p_hi q_lo + lam q_lo q_hi is symmetric, so the layer's claim holds ...
        p_lo, p_hi, q_lo, q_hi = t["finals"]
        exchanged = with_layer(case, k, finals=[p_hi, p_lo, q_hi, q_lo])
        g = lambda f: V.add(V.add(V.mul(f[0], f[3]), V.mul(f[1], f[2])), V.mul(t["lam"], V.mul(f[2], f[3])))  # noqa: E731
        assert same(g(t["finals"]), g([p_hi, p_lo, q_hi, q_lo]))
        # ... and the claim handed down is that of the wrong half: the next layer's first round, or the leaves, fail
        rejects(lambda: V.verify_fraction_tree(p, q, **exchanged), *nxt(1, SUM))
    V, p, q, wrong = fraction_case(name, nv, n_leaves, stop, numerators, salt, tau_first=True)
    if nv - 2 > stop:
        rejects(lambda: V.verify_fraction_tree(p, q, **wrong), None, POINT, nv - 2)
    else:   # one layer only: the prover states no next point, the verifier forms its own
        V.verify_fraction_tree(p, q, **wrong)
