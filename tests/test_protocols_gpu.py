"""Every protocol the library proves on the device, read by the plain verifier of tests/protocol_verifier.py (pinned by
tests/test_protocol_verifier_host.py, which shows that it rejects): EqSumCheck over a VirtualPolynomial and over a RangePolynomial, the
explicit and the fused round calls, ProductTree and FractionTree from the root to the leaves, a permutation check and a lookup from
integers -- for all six ring ids, in both orders where the call has both.  Every comparison is exact.

The device is the prover and nothing else: every expected value -- the claimed sums, the leaves, the tables' values at the final
point, eq(z, point), the roots -- is computed here from the raw inputs in Python integers (the oracle's Fq3 / Fq9 / Fq4 slot products
on the reference's own rings).  The one thing read from a tree is its layer of two nodes, which is the prover's first message.

The shapes are the smallest at which every kind of round occurs: four variables give a round of several launches, a round of one
record and the last round, which has no weights left.  The challenges of a case hold zero(), one() and R::from(p - 1) beside uniform
elements; z is uniform, or a point of the cube, where eq is an indicator and the claimed sum is one entry of g.
"""
import os
import random
import sys

import numpy as np
import pytest

import oracle_lib as O
from test_mle_gpu import SLOT_MUL, dev, host, model_for, ring_for
from test_wsumcheck_gpu import SIX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import model_vpoly as VP  # noqa: E402
import protocol_verifier as PV  # noqa: E402
from protocol_verifier import FINAL, SUM, Rejected, same  # noqa: E402

pytestmark = pytest.mark.gpu
LEADING, TRAILING = 0, 1
ORDERS = (LEADING, TRAILING)
ORDER_IDS = ["leading", "trailing"]
RING_IDS = [c[0] for c in SIX]
Z_KINDS = pytest.mark.parametrize("cube_z", [False, True], ids=["z-uniform", "z-on-the-cube"])
NV = 4
# the term shape MIXED of tools/model_vpoly.py -- coefficients, a table twice in one term, a table in several terms, one to four
# factors -- cut to seven tables and three factors, so that eq(z, .) fits in as the eighth table and the fourth factor of every term
MIXED_EQ = [[0], [0, 1], [0, 2, 3], [1, 4, 4], [3, 5, 0], [6, 4], [2]]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


class Env:
    """one ring: the model's elements and operations, the verifier over them, and the way to and from the device"""

    def __init__(self, torch, name, k):
        self.torch, self.name = torch, name
        self.m, self.ring = model_for(name, k), ring_for(name, k)
        self.zero, self.one = self.m.zero(), self.m.elems(self.m.one())[0]
        self.V = PV.Verifier(self.zero, self.one, self.m.add, self.m.sub, self.m.mul, self.m.p)

    def put(self, elems):
        return dev(self.torch, self.m.words(list(elems)))

    def get(self, t):
        return self.m.elems(host(t))

    def uniform(self, seed, n):
        return self.m.elems(self.m.uniform(seed, n))

    def n_slots(self):
        return self.ring.degree if self.m.pow2 else self.m.w // SLOT_MUL[self.name][1]

    def from_slots(self, js):
        """the element whose slot s is the base-field integer js[s]"""
        m = self.m
        if m.pow2:
            return np.array([int(j) % m.p for j in js], dtype=object)
        out = np.zeros(m.w, dtype=np.uint64)
        out[::SLOT_MUL[self.name][1]] = O.to_mont(m.F, [int(j) % m.p for j in js])
        return out


_envs = {}


def env_for(torch, name, k):
    if (name, k) not in _envs:
        _envs[(name, k)] = Env(torch, name, k)
    return _envs[(name, k)]


class Draw:
    """the seeded generator of one case"""

    def __init__(self, env, *key):
        self.env, self.rng, self.deck = env, random.Random(repr(key)), []

    def elems(self, n):
        return self.env.uniform(self.rng.randrange(1 << 24), n)

    def elem(self):
        return self.elems(1)[0]

    def challenge(self):
        """every four draws: zero(), one(), R::from(p - 1) and a uniform element, in a drawn order"""
        if not self.deck:
            V = self.env.V
            self.deck = [V.zero, V.one, V.scalar(V.p - 1), self.elem()]
            self.rng.shuffle(self.deck)
        return self.deck.pop()

    def challenges(self, n):
        return [self.challenge() for _ in range(n)]

    def z(self, n, cube):
        """(z, the index of the cube it is, or None)"""
        if not cube:
            return self.elems(n), None
        index = self.rng.randrange(1, (1 << n) - 1)   # not all zero(), not all one()
        return self.env.V.bits(index, n), index


def claimed_sum(V, z, nv, g_at):
    """sum_b eq(z, b) g(b) over the cube, g_at(b) the value of g at index b"""
    return V.sum(V.mul(V.eq_eval(z, V.bits(b, nv)), g_at(b)) for b in range(1 << nv))


def g_of_terms(V, terms, coeffs):
    def g(vals):
        return V.sum(V.mul(V.prod(vals[j] for j in term), V.one if coeffs[k] is None else coeffs[k]) for k, term in enumerate(terms))
    return g


def slots_of(g, mles):
    """per table slot of the VirtualPolynomial g, which of `mles` it holds"""
    ptrs = [t.evaluations.data_ptr() for t in mles]
    return [ptrs.index(t.evaluations.data_ptr()) for t in g.tables]


def drive(env, prover, challenges, slots):
    """message(), next(r) per round, then final(): (messages, the final values in the order of the caller's tables, eq(z, r))"""
    msgs = []
    for r in challenges:
        msgs.append(env.get(prover.message()))
        prover.next(env.put([r]))
    finals_dev, eq_dev = prover.final()
    assert len(finals_dev) == len(slots)
    finals = [None] * len(slots)
    for slot, t in zip(slots, finals_dev):
        finals[slot] = env.get(t)[0]
    return msgs, finals, env.get(eq_dev)[0]


def unchanged(env, mles, tables):
    return all(np.array_equal(host(t.evaluations), env.m.words(list(f))) for t, f in zip(mles, tables))


# ---- a. EqSumCheck over a VirtualPolynomial ------------------------------------------------------------------------------------------------------
KINDS = {"product": [[0, 1]], "r1cs": [[0, 1], [2]], "fraction": [[0, 3], [1, 2], [2, 3]]}


@Z_KINDS
@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("order", ORDERS, ids=ORDER_IDS)
@pytest.mark.parametrize("name,k", SIX, ids=RING_IDS)
def test_eq_sumcheck_over_a_virtual_polynomial_verifies(torch_cuda, name, k, order, kind, cube_z):
    """the claims of tests/test_wsumcheck_gpu.py: a b;  a b - c with c = a b element by element, a true zero claim;  the layer claim of
    a fraction tree p_lo q_hi + p_hi q_lo + lambda q_lo q_hi"""
    from stark_rings_amd import DenseMultilinearExtension as MLE, EqSumCheck, VirtualPolynomial

    env = env_for(torch_cuda, name, k)
    V, ring, d = env.V, env.ring, Draw(env, "eq", name, kind, order, cube_z)
    terms = KINDS[kind]
    tables = [d.elems(1 << NV) for _ in range(VP.n_tables(terms))]
    if kind == "r1cs":
        tables[2] = [V.mul(a, b) for a, b in zip(tables[0], tables[1])]
    coeffs = {"product": [None], "r1cs": [None, V.sub(V.zero, V.one)], "fraction": [None, None, d.elem()]}[kind]
    mles = [MLE(ring, NV, env.put(t)) for t in tables]
    g = VirtualPolynomial(ring, NV)
    for term, c in zip(terms, coeffs):
        g.add_mle_list([mles[j] for j in term], None if c is None else env.put([c]))
    g_of = g_of_terms(V, terms, coeffs)
    z, index = d.z(NV, cube_z)
    claim0 = claimed_sum(V, z, NV, lambda b: g_of([t[b] for t in tables]))
    if kind == "r1cs":
        assert same(claim0, V.zero)
    if cube_z:
        assert same(claim0, g_of([t[index] for t in tables]))
    challenges = d.challenges(NV)
    msgs, finals, eq_r = drive(env, EqSumCheck(g, env.put(z), order), challenges, slots_of(g, mles))
    V.verify_eq_sumcheck(claim0, z, msgs, challenges, finals, eq_r, order, g_of, tables, points=VP.degree(terms) + 2)
    # the order is no formality: the same transcript read with the point in the other variable order fails at the final values
    with pytest.raises(Rejected) as e:
        V.verify_eq_sumcheck(claim0, z, msgs, challenges, finals, eq_r, 1 - order, g_of, tables, points=VP.degree(terms) + 2)
    assert (e.value.round, e.value.reason) == (None, FINAL)
    assert unchanged(env, mles, tables)


# ---- b. the explicit and the fused paths ---------------------------------------------------------------------------------------------------------
@Z_KINDS
@pytest.mark.parametrize("order", ORDERS, ids=ORDER_IDS)
@pytest.mark.parametrize("name,k", SIX, ids=RING_IDS)
def test_round_evals_and_fold_round_evals_of_a_virtual_polynomial_verify(torch_cuda, name, k, order, cube_z):
    """VirtualPolynomial.round_evals, then fold_round_evals per round and fixed_variables behind the last: MIXED_EQ with
    DenseMultilinearExtension.eq multiplied in (eight tables, degree four), whose last table's final value is eq(z, point); and
    the whole MIXED of tools/model_vpoly.py as a plain sum-check of sum_b g(b)"""
    from stark_rings_amd import DenseMultilinearExtension as MLE, VirtualPolynomial

    env = env_for(torch_cuda, name, k)
    V, ring, d = env.V, env.ring, Draw(env, "explicit", name, order, cube_z)
    for terms, with_eq in ((MIXED_EQ, True), (VP.MIXED, False)):
        tables = [d.elems(1 << NV) for _ in range(VP.n_tables(terms))]
        coeffs = d.elems(len(terms))
        mles = [MLE(ring, NV, env.put(t)) for t in tables]
        e = VirtualPolynomial(ring, NV)
        for term, c in zip(terms, coeffs):
            e.add_mle_list([mles[j] for j in term], env.put([c]))
        slots = slots_of(e, mles)
        g_of = g_of_terms(V, terms, coeffs)
        z, _ = d.z(NV, cube_z)
        if with_eq:
            e.mul_by_mle(MLE.eq(ring, env.put(z)))
            assert len(e.tables) == 8 and e.degree == 4
        challenges = d.challenges(NV)
        msgs, msg = [], e.round_evals(order)
        for j, r in enumerate(challenges):
            msgs.append(env.get(msg))
            if j + 1 < NV:
                msg, e = e.fold_round_evals(env.put([r]), order)
            else:
                e = e.fixed_variables(env.put([r]), order)
        values = [env.get(t.evaluations)[0] for t in e.tables]
        finals = [None] * len(tables)
        for slot, v in zip(slots, values):
            finals[slot] = v
        if with_eq:
            claim0 = claimed_sum(V, z, NV, lambda b: g_of([t[b] for t in tables]))
            V.verify_eq_sumcheck(claim0, z, msgs, challenges, finals, values[-1], order, g_of, tables, points=5)
        else:
            claim0 = V.sum(g_of([t[b] for t in tables]) for b in range(1 << NV))
            V.verify_sumcheck(claim0, msgs, challenges, finals, order, g_of, tables, points=5)
        assert unchanged(env, mles, tables)


@pytest.mark.parametrize("order", ORDERS, ids=ORDER_IDS)
@pytest.mark.parametrize("name,k", SIX, ids=RING_IDS)
def test_round_evals_and_fold_round_evals_of_three_tables_verify(torch_cuda, name, k, order):
    """DenseMultilinearExtension.round_evals, then fold_round_evals per round: sum_b a b c; the second table stores 11 of its 16
    evaluations, the rest are zero"""
    from stark_rings_amd import DenseMultilinearExtension as MLE

    env = env_for(torch_cuda, name, k)
    V, ring, d = env.V, env.ring, Draw(env, "three tables", name, order)
    tables = [d.elems(n) for n in (1 << NV, 11, 1 << NV)]
    mles = [MLE(ring, NV, env.put(t)) for t in tables]
    at = lambda t, b: t[b] if b < len(t) else V.zero  # noqa: E731
    claim0 = V.sum(V.prod(at(t, b) for t in tables) for b in range(1 << NV))
    challenges = d.challenges(NV)
    tabs, msgs, msg = mles, [], MLE.round_evals(mles, order)
    for j, r in enumerate(challenges):
        msgs.append(env.get(msg))
        rd = env.put([r])
        if j + 1 < NV:
            msg, tabs = MLE.fold_round_evals(tabs, rd, order)
        else:
            tabs = [t.fixed_variables(rd) if order == LEADING else t.fix_last_variables(rd) for t in tabs]
    finals = [env.get(t.evaluations)[0] for t in tabs]
    V.verify_sumcheck(claim0, msgs, challenges, finals, order, V.prod, tables, points=4)
    assert unchanged(env, mles, tables)


# ---- c, d. the trees, from the root to the leaves ---------------------------------------------------------------------------------------------------
def descend(env, d, tree, nv, stop, fraction):
    """the prover's side of the layered descent of a trailing-order tree: layer nv - 1 as it stands, then per layer k = nv - 1 ..
    stop + 1 the sum-check of layer_claim(k, z_k) and the next point (r_0, .., r_{m-1}, tau) -- hi is the upper half, the top
    variable.  Returns (top, z_top, layers) as verify_product_tree / verify_fraction_tree take them."""
    if fraction:
        p, q = (env.get(t.evaluations) for t in tree.layer(nv - 1))
        top = ((p[0], q[0]), (p[1], q[1]))
    else:
        top = env.get(tree.layer(nv - 1).evaluations)
    assert len(top) == 2
    z_top = [d.elem()]
    z, layers = list(z_top), {}
    for k in range(nv - 1, stop, -1):
        t = {"z": list(z), "challenges": d.challenges(nv - k), "tau": d.elem()}
        if fraction:
            t["lam"] = d.elem()
            claim = tree.layer_claim(k, env.put(z), env.put([t["lam"]]))
        else:
            claim = tree.layer_claim(k, env.put(z))
        assert claim.order == TRAILING
        t["messages"], t["finals"], t["eq_r"] = drive(env, claim, t["challenges"], slots_of(claim.g, tree.halves(k)))
        layers[k] = t
        z = list(reversed(t["challenges"])) + [t["tau"]]
    return top, z_top, layers


def product_tree_verifies(env, d, tree, leaves, nv):
    """the whole descent of one ProductTree whose stored leaves must be `leaves`"""
    from stark_rings_amd import RingError

    stop = 0 if len(leaves) == 1 << nv else 1
    if stop:   # layer 0 of a truncated tree is no table: its missing leaves are one(), a table's are zero()
        with pytest.raises(RingError):
            tree.halves(1)
        with pytest.raises(RingError):
            tree.layer_claim(1, env.put(d.elems(nv - 1)))
    top, z_top, layers = descend(env, d, tree, nv, stop, False)
    z = env.V.verify_product_tree(leaves, nv, top, z_top, layers, stop)
    assert len(z) == nv - stop and sorted(layers) == list(range(stop + 1, nv))
    assert same(env.get(tree.root())[0], env.V.prod(leaves))


def fraction_tree_verifies(env, d, tree, p_leaves, q_leaves, nv):
    """the whole descent of one FractionTree; returns its root (P, Q) by the definition"""
    from stark_rings_amd import RingError

    stop = 0 if len(q_leaves) == 1 << nv and p_leaves is not None else 1
    if stop:   # nor is layer 0 of a tree without stored numerators: they are one()
        with pytest.raises(RingError):
            tree.halves(1)
        with pytest.raises(RingError):
            tree.layer_claim(1, env.put(d.elems(nv - 1)), env.put(d.elems(1)))
    top, z_top, layers = descend(env, d, tree, nv, stop, True)
    z, (P, Q) = env.V.verify_fraction_tree(p_leaves, q_leaves, nv, top, z_top, layers, stop)
    assert len(z) == nv - stop and sorted(layers) == list(range(stop + 1, nv))
    rp, rq = tree.root()
    assert same(env.get(rp)[0], P) and same(env.get(rq)[0], Q)
    return P, Q


@pytest.mark.parametrize("n_leaves", [16, 11])
@pytest.mark.parametrize("name,k", SIX, ids=RING_IDS)
def test_a_product_tree_verifies_from_the_root_to_the_leaves(torch_cuda, name, k, n_leaves):
    from stark_rings_amd import ProductTree

    env = env_for(torch_cuda, name, k)
    d = Draw(env, "product tree", name, n_leaves)
    leaves = d.elems(n_leaves)
    tree = ProductTree(env.ring, env.put(leaves), NV)
    product_tree_verifies(env, d, tree, leaves, NV)
    assert np.array_equal(host(tree.leaves), env.m.words(leaves))


@pytest.mark.parametrize("numerators", [True, False], ids=["stored-numerators", "no-numerators"])
@pytest.mark.parametrize("name,k", SIX, ids=RING_IDS)
def test_a_fraction_tree_verifies_from_the_root_to_the_leaves(torch_cuda, name, k, numerators):
    from stark_rings_amd import FractionTree

    env = env_for(torch_cuda, name, k)
    V, d = env.V, Draw(env, "fraction tree", name, numerators)
    p, q = (d.elems(1 << NV) if numerators else None), d.elems(1 << NV)
    tree = FractionTree(env.ring, None if p is None else env.put(p), env.put(q), NV)
    P, Q = fraction_tree_verifies(env, d, tree, p, q, NV)
    # the root once more in the open: Q = prod q_i, P = sum_i p_i prod_{j != i} q_j -- 16 leaves, 256 products
    ps = p if p is not None else [V.one] * len(q)
    assert same(Q, V.prod(q)) and same(P, V.sum(V.mul(ps[i], V.prod(q[j] for j in range(len(q)) if j != i)) for i in range(len(q))))


# ---- e. a permutation check from integers ---------------------------------------------------------------------------------------------------------
CYCLES = [(0, 3, 7), (1, 2), (4, 9, 12, 15), (6, 8), (10, 11, 13, 5, 14)]   # sigma on 16 rows; every row is on a cycle


@pytest.mark.parametrize("column", [0, 1])
@pytest.mark.parametrize("name,k", SIX, ids=RING_IDS)
def test_a_permutation_check_from_integers_verifies(torch_cuda, name, k, column):
    """one wire column of 2^4 rows, f constant on the cycles of sigma; column 1 has id_start = 16, sigma within 16 .. 31, and -- where
    p + 31 is a u64 -- one entry of sigma given as p + its value, which R::from(u64) reduces"""
    from stark_rings_amd import PermutationCheck, permutation_leaves_indexed

    env = env_for(torch_cuda, name, k)
    V, d, n = env.V, Draw(env, "permutation", name, column), 1 << NV
    start = column * n
    sigma, cycle_of = list(range(n)), [0] * n
    for c, cyc in enumerate(CYCLES):
        for a, b in zip(cyc, cyc[1:] + cyc[:1]):
            sigma[a], cycle_of[a] = b, c
    assert sorted(sigma) == list(range(n)) and all(sigma[e] != e for e in range(n))
    values = d.elems(len(CYCLES))
    f = [values[cycle_of[e]] for e in range(n)]
    sent = [start + s for s in sigma]
    if column == 1 and V.p + start + n < 1 << 64:
        sent[5] += V.p
        assert sent[5] >= V.p
    elif column == 1 and name != "stark":
        raise AssertionError("every field here but Stark's has room for p + 31 in a u64")
    beta, gamma = d.elem(), d.elem()
    num, den = permutation_leaves_indexed(env.ring, env.put(f), dev(torch_cuda, np.array(sent, dtype=np.uint64)), env.put([beta]),
                                          env.put([gamma]), id_start=start)
    check = PermutationCheck(env.ring, num, den, NV)
    want_num = [V.add(V.add(beta, f[e]), V.mul(gamma, V.scalar(start + e))) for e in range(n)]
    want_den = [V.add(V.add(beta, f[e]), V.mul(gamma, V.scalar(start + sigma[e]))) for e in range(n)]
    assert same(V.prod(want_num), V.prod(want_den)) and check.holds()
    product_tree_verifies(env, d, check.num, want_num, NV)
    product_tree_verifies(env, d, check.den, want_den, NV)


# ---- f. a lookup from indices -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zero_denominator", [False, True], ids=["beta-uniform", "beta-a-fingerprint"])
@pytest.mark.parametrize("name,k", SIX, ids=RING_IDS)
def test_a_lookup_from_indices_verifies(torch_cuda, name, k, zero_denominator):
    """a witness of 2^4 rows taken from a table of 2^3 rows of two columns by u64 indices; q = beta - (col_0 + gamma col_1).  With beta
    the fingerprint of a table row that the witness uses, one denominator of the table and some of the witness are zero(): the
    protocol never divides, and the transcript still verifies"""
    from stark_rings_amd import LookupCheck, fingerprint

    env = env_for(torch_cuda, name, k)
    V, d = env.V, Draw(env, "lookup", name, zero_denominator)
    nw, nt = 4, 3
    cols = [d.elems(1 << nt) for _ in range(2)]
    idx = [d.rng.randrange((1 << nt) - 1) for _ in range(1 << nw)]   # the last table row is never used
    idx[:3] = [5, 5, 2]
    counts = [idx.count(j) for j in range(1 << nt)]
    assert 0 in counts and max(counts) >= 2   # a table row that no witness row uses, and one that several do
    gamma = d.elem()
    row = lambda j: V.add(cols[0][j], V.mul(gamma, cols[1][j]))  # noqa: E731
    beta = row(5) if zero_denominator else d.elem()
    coeffs, const = env.put([V.sub(V.zero, V.one), V.sub(V.zero, gamma)]), env.put([beta])
    q_t = fingerprint(env.ring, [env.put(c) for c in cols], coeffs, const)
    q_w = fingerprint(env.ring, [env.put([c[i] for i in idx]) for c in cols], coeffs, const)
    check = LookupCheck.from_indices(env.ring, q_w, q_t, dev(torch_cuda, np.array(idx, dtype=np.uint64)), nw, nt)
    want_qw = [V.sub(beta, row(i)) for i in idx]
    want_qt = [V.sub(beta, row(j)) for j in range(1 << nt)]
    want_pt = [V.scalar(c) for c in counts]
    assert same(want_qt[5], V.zero) == zero_denominator
    Pw, Qw = fraction_tree_verifies(env, d, check.witness, None, want_qw, nw)
    Pt, Qt = fraction_tree_verifies(env, d, check.table, want_pt, want_qt, nt)
    assert same(V.mul(Pw, Qt), V.mul(Pt, Qw)) and check.holds()
    assert env.ring.spmv_bad_index_count() == 0


# ---- g. the range check --------------------------------------------------------------------------------------------------------------------------------
@Z_KINDS
@pytest.mark.parametrize("bound", [2, 8])
@pytest.mark.parametrize("order", ORDERS, ids=ORDER_IDS)
@pytest.mark.parametrize("name,k", SIX, ids=RING_IDS)
def test_a_range_check_verifies_and_a_planted_bound_does_not(torch_cuda, name, k, order, bound, cube_z):
    """EqSumCheck(RangePolynomial) over two tables with coefficients mu; every slot of every entry is R::from(j), |j| < B: the claimed
    sum is zero().  Then R::from(B) in every slot of one entry: the same honest prover is rejected in round 1 against zero(), and
    accepted to the end against the true sum"""
    from stark_rings_amd import DenseMultilinearExtension as MLE, EqSumCheck, RangePolynomial

    env = env_for(torch_cuda, name, k)
    V, ring, d, B = env.V, env.ring, Draw(env, "range", name, order, bound, cube_z), bound
    tables = [[env.from_slots([d.rng.randrange(-(B - 1), B) for _ in range(env.n_slots())]) for _ in range(1 << NV)] for _ in range(2)]
    mu = d.elems(2)
    z, index = d.z(NV, cube_z)
    g_of = lambda vals: V.sum(V.mul(c, V.range_poly(v, B)) for c, v in zip(mu, vals))  # noqa: E731

    def transcript(tabs):
        mles = [MLE(ring, NV, env.put(t)) for t in tabs]
        prover = EqSumCheck(RangePolynomial(ring, mles, B, env.put(mu)), env.put(z), order)
        challenges = d.challenges(NV)
        msgs, finals, eq_r = drive(env, prover, challenges, [0, 1])
        assert all(len(m) == 2 * B + 1 for m in msgs) and unchanged(env, mles, tabs)
        return dict(z=z, messages=msgs, challenges=challenges, finals=finals, eq_r=eq_r, order=order, g_of=g_of, tables=tabs, points=2 * B + 1)

    assert same(claimed_sum(V, z, NV, lambda b: g_of([t[b] for t in tables])), V.zero)
    V.verify_eq_sumcheck(claim0=V.zero, **transcript(tables))
    at = index if cube_z else 5   # on the cube eq(z, .) is zero everywhere else
    planted = [tables[0], list(tables[1])]
    planted[1][at] = V.scalar(B)
    run = transcript(planted)
    with pytest.raises(Rejected) as e:
        V.verify_eq_sumcheck(claim0=V.zero, **run)
    assert (e.value.round, e.value.reason) == (1, SUM)
    true_sum = claimed_sum(V, z, NV, lambda b: g_of([t[b] for t in planted]))
    assert not same(true_sum, V.zero)
    V.verify_eq_sumcheck(claim0=true_sum, **run)
