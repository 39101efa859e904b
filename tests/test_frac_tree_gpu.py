"""GPU parity of the fraction-tree calls (sr_frac_tree[_dev], FractionTree) for all six ring ids.  Every comparison is bit-exact.
Expected values come from tools/model_frac_tree.py, the pair-at-a-time restatement of both orders (pinned against the closed forms by
tests/test_frac_tree_host.py): on standard-form Python integers for the power-of-two rings, on the oracle's Fq3 / Fq9 / Fq4 slot
products for the reference's own rings.  The cases are those of tests/test_prod_tree_gpu.py: the smallest tables at which a launch
split, a group boundary or an access width can go wrong."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

import oracle_lib as O
from test_mle_gpu import POISON, dev, host, model_for, ring_for
from test_sumcheck_gpu import _interp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import model_frac_tree as FT  # noqa: E402

pytestmark = pytest.mark.gpu
LEADING, TRAILING = 0, 1
ORDERS = (LEADING, TRAILING)
ORDER_IDS = ["leading", "trailing"]
# (ring, log2 D, num_vars)
CASES = [("goldilocks", 6, 7), ("goldilocks", 16, 4), ("babybear", 5, 7), ("stark", 4, 5), ("stark", 12, 3),
         ("goldilocks24", 0, 8), ("babybear72", 0, 7), ("frog16", 0, 8)]
IDS = ["%s-%d-nv%d" % c for c in CASES]
SMALL = [c for c in CASES if c[:2] not in {("goldilocks", 16), ("stark", 12)}]
SMALL_IDS = ["%s-%d-nv%d" % c for c in SMALL]
# the smallest ring of each family (and of each levels-per-launch bound), where every num_vars = 0 .. jmax + 1 is run
SMALLEST = [("goldilocks", 6), ("babybear", 5), ("stark", 4), ("goldilocks24", 0), ("babybear72", 0), ("frog16", 0)]
JMAX = FT.LEVELS_PER_LAUNCH   # levels per launch (tests/test_frac_tree_isa.py holds the register counts behind them)
GUARD = 0x6B6B6B6B6B6B6B6B
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "frac_tree_kats.json")))["cases"]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def one_elem(m):
    return m.elems(m.one())[0]


def model_tree(m, p_els, q_els, nv, order):
    """(p words, q words) of the layers 1 .. nv"""
    p, q = FT.flat(FT.layers(p_els, q_els, nv, order, m.zero(), one_elem(m), m.add, lambda a, b: m.mul(b, a)))
    return m.words(p), m.words(q)


_trees = {}


def want_tree(m, key, p_els, q_els, nv, order):
    """computed once per key"""
    k = (m.name, m.k, nv, order, key, p_els is None)
    if k not in _trees:
        _trees[k] = model_tree(m, p_els, q_els, nv, order)
    return _trees[k]


_leaves = {}


def leaves_for(m, nv):
    """the shared leaves of a case: (p words, q words, p elements, q elements)"""
    k = (m.name, m.k, nv)
    if k not in _leaves:
        p, q = m.uniform(0x9C00 + m.k + nv, 1 << nv), m.uniform(0x9D00 + m.k + nv, 1 << nv)
        _leaves[k] = (p, q, m.elems(p), m.elems(q))
    return _leaves[k]


def tree_dev(torch, ring, t_p, t_q, nv, order, stream=None):
    """the _dev call into two buffers with one guard element behind the 2^nv - 1 outputs each; returns (p view, q view, p buffer, q buffer)"""
    from stark_rings_amd import frac_tree_dev

    w = ring.words_per_elem
    n = ((1 << nv) - 1) * w
    bp = torch.full((n + w,), GUARD, dtype=torch.int64, device="cuda")
    bq = torch.full((n + w,), GUARD, dtype=torch.int64, device="cuda")
    frac_tree_dev(ring, bp[:n], bq[:n], t_p, t_q, nv, order, stream=stream)
    return bp[:n], bq[:n], bp, bq


def guards_intact(w, *bufs):
    return all(bool((host(b[-w:]) == np.uint64(GUARD)).all()) for b in bufs)


def check(torch, m, got, want, where):
    gp, gq, bp, bq = got
    torch.cuda.synchronize()
    assert np.array_equal(host(gq), want[1]), ("q", where)
    assert np.array_equal(host(gp), want[0]), ("p", where)
    assert guards_intact(m.w, bp, bq), where


@pytest.mark.parametrize("name,k,nv", CASES, ids=IDS)
@pytest.mark.parametrize("order", ORDERS, ids=ORDER_IDS)
def test_full_tables_match_the_restatement(torch_cuda, name, k, nv, order):
    torch = torch_cuda
    from stark_rings_amd import frac_tree_plan

    m = model_for(name, k)
    ring = m.ring
    pw, qw, pe, qe = leaves_for(m, nv)
    t_p, t_q = dev(torch, pw), dev(torch, qw)
    for numer in (True, False):
        want = want_tree(m, "full", pe if numer else None, qe, nv, order)
        got = tree_dev(torch, ring, t_p if numer else None, t_q, nv, order)
        check(torch, m, got, want, (name, nv, order, numer))
        assert ring.count_noncanonical_dev(got[0]) == 0 and ring.count_noncanonical_dev(got[1]) == 0
    assert np.array_equal(host(t_p), pw) and np.array_equal(host(t_q), qw), "the leaves were written"
    elems, launches = frac_tree_plan(ring, nv, order)
    assert elems == (1 << nv) - 1 and launches == -(-nv // JMAX[name])


@pytest.mark.parametrize("name,k", SMALLEST, ids=["%s-%d" % c for c in SMALLEST])
def test_every_num_vars_up_to_one_past_a_launch(torch_cuda, name, k):
    torch = torch_cuda
    from stark_rings_amd import frac_tree_plan

    m = model_for(name, k)
    ring = m.ring
    for nv in range(JMAX[name] + 2):
        full = 1 << nv
        pw, qw = m.uniform(0x9B00 + nv, full), m.uniform(0x9B80 + nv, full)
        pe, qe = m.elems(pw), m.elems(qw)
        for order in ORDERS:
            for n in sorted({full, full - 1, 0}):
                for numer in (True, False):
                    want = model_tree(m, pe[:n] if numer else None, qe[:n], nv, order)
                    got = tree_dev(torch, ring, dev(torch, pw)[:n * m.w] if numer else None, dev(torch, qw)[:n * m.w], nv, order)
                    check(torch, m, got, want, (name, nv, n, order, numer))   # num_vars = 0 writes nothing at all
            assert frac_tree_plan(ring, nv, order) == (full - 1, -(-nv // JMAX[name]))


def truncations(name, nv):
    """0, 1, a value inside a group of the first launch, one below a group boundary, 2^nv - 1"""
    g, full = 1 << JMAX[name], 1 << nv
    inside = g + 3 if g + 3 < full else 3
    if inside % g == 0:
        inside += 1
    below = 2 * g - 1 if 2 * g <= full else g - 1
    return sorted({0, 1, inside, below, full - 1})


@pytest.mark.parametrize("name,k,nv", CASES, ids=IDS)
def test_truncated_tables_poison_behind_the_leaves_and_guards_behind_the_layers(torch_cuda, name, k, nv):
    torch = torch_cuda
    m = model_for(name, k)
    ring = m.ring
    pw, qw, pe, qe = leaves_for(m, nv)
    for n in truncations(name, nv):
        bp, bq = pw.copy(), qw.copy()
        bp[n * m.w:] = POISON   # not canonical in any of the fields: a kernel that read it would show it
        bq[n * m.w:] = POISON
        t_p, t_q = dev(torch, bp), dev(torch, bq)
        for order in ORDERS:
            for numer in (True, False):
                want = want_tree(m, n, pe[:n] if numer else None, qe[:n], nv, order)
                got = tree_dev(torch, ring, t_p[:n * m.w] if numer else None, t_q[:n * m.w], nv, order)
                check(torch, m, got, want, (name, n, order, numer))
                assert ring.count_noncanonical_dev(got[0]) == 0 and ring.count_noncanonical_dev(got[1]) == 0
        assert np.array_equal(host(t_p), bp) and np.array_equal(host(t_q), bq), "the leaves (or the poison behind them) were written"


@pytest.mark.parametrize("name,k,nv", SMALL, ids=SMALL_IDS)
def test_edge_leaves_and_a_single_zero_denominator(torch_cuda, name, k, nv):
    torch = torch_cuda
    m = model_for(name, k)
    ring = m.ring
    full = 1 << nv
    top = m.const(m.p - 1, 1)   # every coefficient the memory word p - 1
    one, zero = m.one(), np.zeros(m.w, dtype=np.uint64)
    words = np.tile(top, full)
    for order in ORDERS:
        for numer in (True, False):
            want = want_tree(m, "p - 1", m.elems(words) if numer else None, m.elems(words), nv, order)
            got = tree_dev(torch, ring, dev(torch, words) if numer else None, dev(torch, words), nv, order)
            check(torch, m, got, want, (name, "p - 1", order, numer))
    # every leaf the neutral fraction (zero, one), stored or not: every node is (zero, one)
    for n in (full, 3, 0):
        for order in ORDERS:
            gp, gq, _, _ = tree_dev(torch, ring, dev(torch, np.tile(zero, n)), dev(torch, np.tile(one, n)), nv, order)
            torch.cuda.synchronize()
            assert not host(gp).any(), (name, n, order)
            assert np.array_equal(host(gq), np.tile(one, full - 1)), (name, n, order)
    # a single zero denominator among ones (numerators one()): exactly the nodes above it have q = 0
    for z in sorted({0, 5, full // 2, full - 1}):
        qw = np.tile(one, full)
        qw[z * m.w:(z + 1) * m.w] = 0
        for order in ORDERS:
            _, gq, _, _ = tree_dev(torch, ring, None, dev(torch, qw), nv, order)
            torch.cuda.synchronize()
            gq = host(gq)
            for lvl in range(1, nv + 1):
                above = z >> lvl if order == LEADING else z & ((1 << (nv - lvl)) - 1)
                off = FT.layer_offset(nv, lvl)
                for i in range(1 << (nv - lvl)):
                    e = gq[(off + i) * m.w:(off + i + 1) * m.w]
                    assert np.array_equal(e, np.zeros_like(e) if i == above else one), (name, order, z, lvl, i)
    # and among uniform leaves: the model
    pw, qw, _, _ = leaves_for(m, nv)
    qw = qw.copy()
    qw[5 * m.w:6 * m.w] = 0
    for order in ORDERS:
        want = want_tree(m, "zero at 5", m.elems(pw), m.elems(qw), nv, order)
        check(torch, m, tree_dev(torch, ring, dev(torch, pw), dev(torch, qw), nv, order), want, (name, "zero at 5", order))


@pytest.mark.parametrize("name,k,nv", [("goldilocks", 6, 5), ("babybear", 5, 5), ("stark", 4, 4), ("goldilocks", 0, 5), ("babybear", 0, 4),
                                       ("goldilocks24", 0, 4)],
                         ids=["goldilocks-6", "babybear-5", "stark-4", "goldilocks-0", "babybear-0", "goldilocks24"])
def test_the_one_coefficient_path_at_odd_eight_byte_pointers_and_at_degree_one(torch_cuda, name, k, nv):
    """any of the four buffers 8 bytes past a 16-byte boundary takes the one-coefficient path of the one-limb kernels, as does D = 1;
    guards on both sides of both outputs"""
    torch = torch_cuda
    from stark_rings_amd import frac_tree_dev

    m = model_for(name, k)
    ring = m.ring
    w, full = m.w, 1 << nv
    pw, qw, pe, qe = leaves_for(m, nv)
    n_out = (full - 1) * w
    for n in (full, full - 3):
        for order in ORDERS:
            for numer in (True, False):
                want = want_tree(m, n if n != full else "full", pe[:n] if numer else None, qe[:n], nv, order)
                for shifts in ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 1, 1, 1), (0, 0, 0, 0)):
                    if not numer and shifts == (0, 0, 1, 0):
                        continue
                    s_po, s_qo, s_pi, s_qi = shifts
                    src_p = torch.zeros(full * w + 2, dtype=torch.int64, device="cuda")
                    src_q = torch.zeros(full * w + 2, dtype=torch.int64, device="cuda")
                    assert src_p.data_ptr() % 16 == 0 and src_q.data_ptr() % 16 == 0
                    src_p[s_pi:s_pi + full * w] = dev(torch, pw)
                    src_q[s_qi:s_qi + full * w] = dev(torch, qw)
                    dst_p = torch.full((n_out + w + 2,), GUARD, dtype=torch.int64, device="cuda")
                    dst_q = torch.full((n_out + w + 2,), GUARD, dtype=torch.int64, device="cuda")
                    frac_tree_dev(ring, dst_p[s_po:s_po + n_out], dst_q[s_qo:s_qo + n_out], src_p[s_pi:s_pi + n * w] if numer else None,
                                  src_q[s_qi:s_qi + n * w], nv, order)
                    torch.cuda.synchronize()
                    for got, s, wanted in ((host(dst_p), s_po, want[0]), (host(dst_q), s_qo, want[1])):
                        assert np.array_equal(got[s:s + n_out], wanted), (name, n, order, numer, shifts)
                        assert (got[:s] == np.uint64(GUARD)).all() and (got[s + n_out:] == np.uint64(GUARD)).all(), (name, shifts)


@pytest.mark.parametrize("name,k,nv", CASES, ids=IDS)
def test_existing_calls_are_a_second_witness(torch_cuda, name, k, nv):
    """d_q_layers is sr_prod_tree_dev of the q leaves in both orders; in trailing order every p layer is ntt_mul_dev / add_dev on the
    halves of the layers below"""
    torch = torch_cuda
    m = model_for(name, k)
    ring = m.ring
    w, full = m.w, 1 << nv
    pw, qw, _, _ = leaves_for(m, nv)
    for n in (full, full - 3):
        t_p, t_q = dev(torch, pw)[:n * w], dev(torch, qw)[:n * w]
        for numer in (True, False):
            for order in ORDERS:
                gp, gq, _, _ = tree_dev(torch, ring, t_p if numer else None, t_q, nv, order)
                prod = torch.zeros((full - 1) * w, dtype=torch.int64, device="cuda")
                ring.prod_tree_dev(prod, t_q, nv, order)
                torch.cuda.synchronize()
                assert torch.equal(gq, prod), (name, n, order, numer)
            # trailing: gp and gq still hold the trailing tree
            pad_q = dev(torch, np.tile(m.one(), full - n))
            pad_p = torch.zeros_like(pad_q)
            below_p = torch.cat([t_p if numer else dev(torch, np.tile(m.one(), n)), pad_p])
            below_q = torch.cat([t_q, pad_q])
            for lvl in range(1, nv + 1):
                half = (1 << (nv - lvl)) * w
                a = below_p[:half].clone()
                ring.ntt_mul_dev(a, below_q[half:2 * half])
                b = below_p[half:2 * half].clone()
                ring.ntt_mul_dev(b, below_q[:half])
                ring.add_dev(a, b)
                off = FT.layer_offset(nv, lvl) * w
                assert torch.equal(gp[off:off + half], a), (name, n, numer, lvl)
                below_p, below_q = gp[off:off + half], gq[off:off + half]


@pytest.mark.parametrize("name,k,nv", SMALL, ids=SMALL_IDS)
def test_permuted_leaf_pairs_have_one_root_in_both_orders(torch_cuda, name, k, nv):
    torch = torch_cuda
    from stark_rings_amd import FractionTree

    m = model_for(name, k)
    ring = m.ring
    w, full = m.w, 1 << nv
    pw, qw, _, _ = leaves_for(m, nv)
    perm = np.random.RandomState(nv).permutation(full)
    assert not np.array_equal(perm, np.arange(full))
    sp, sq = (x.reshape(full, w)[perm].reshape(-1).copy() for x in (pw, qw))
    roots = []
    for order in ORDERS:
        a = FractionTree(ring, dev(torch, pw), dev(torch, qw), nv, order=order)
        b = FractionTree(ring, dev(torch, sp), dev(torch, sq), nv, order=order)
        torch.cuda.synchronize()
        for x, y in zip(a.root(), b.root()):
            assert torch.equal(x, y), (name, order)
        assert not torch.equal(a.p_layers, b.p_layers)
        changed = sp.copy()
        changed[3 * w:4 * w] = m.uniform(0x5151, 1)
        c = FractionTree(ring, dev(torch, changed), dev(torch, sq), nv, order=order)
        torch.cuda.synchronize()
        assert not torch.equal(a.root()[0], c.root()[0]) and torch.equal(a.root()[1], c.root()[1]), (name, order)
        roots.append(a.root())
    assert torch.equal(roots[0][0], roots[1][0]) and torch.equal(roots[0][1], roots[1][1])


@pytest.mark.parametrize("name,k,nv", [("goldilocks", 6, 7), ("babybear", 5, 7), ("stark", 4, 5), ("goldilocks24", 0, 5), ("babybear72", 0, 4),
                                       ("frog16", 0, 5)], ids=["goldilocks", "babybear", "stark", "goldilocks24", "babybear72", "frog16"])
def test_the_layer_claim_of_the_fractional_sumcheck(torch_cuda, name, k, nv):
    """The GKR layer the feature exists for: with a trailing tree, a point z and a batching coefficient lambda,
    P_k(z) + lambda Q_k(z) = sum_b eq(z, b) (p_lo(b) q_hi(b) + p_hi(b) q_lo(b) + lambda q_lo(b) q_hi(b)) for every k, the four operands
    being the halves of layer k - 1 as they lie; and one run of all rounds of that sum-check at layer 1 ends at the five tables at the
    point of the challenges."""
    torch = torch_cuda
    from stark_rings_amd import DenseMultilinearExtension as MLE, FractionTree, RingError, VirtualPolynomial

    m = model_for(name, k)
    ring = m.ring
    w = m.w
    pw, qw, _, _ = leaves_for(m, nv)
    tree = FractionTree(ring, dev(torch, pw), dev(torch, qw), nv, order=TRAILING)
    z = dev(torch, m.uniform(0x2B2B, nv))
    lam = dev(torch, m.uniform(0x2C2C, 1))

    def claim_poly(n, zk):
        eq = MLE.eq(ring, zk)
        p_lo, p_hi, q_lo, q_hi = tree.halves(nv - n)
        g = VirtualPolynomial(ring, n)
        g.add_mle_list([eq, p_lo, q_hi])
        g.add_mle_list([eq, p_hi, q_lo])
        g.add_mle_list([eq, q_lo, q_hi], lam)
        return g, (eq, p_lo, q_hi, p_hi, q_lo)   # the table slots in the order of their first appearance

    def claimed(lvl, zk):
        big_p, big_q = tree.layer(lvl)
        value = big_q.evaluate(zk).clone()
        ring.ntt_mul_dev(value, lam)
        ring.add_dev(value, big_p.evaluate(zk))
        return value

    for lvl in range(1, nv + 1):
        n = nv - lvl
        zk = z[:n * w]
        g, tables = claim_poly(n, zk)
        assert all(t.num_vars == n for t in tables)
        torch.cuda.synchronize()
        assert torch.equal(g.sum(), claimed(lvl, zk)), (name, lvl)
    # all rounds at layer 1: n = nv - 1 variables, trailing order (round i fixes variable n - 1 - i at challenge i)
    n = nv - 1
    zk = z[:n * w]
    g, tables = claim_poly(n, zk)
    claim_t = claimed(1, zk)
    challenges = [dev(torch, m.uniform(0x7200 + i, 1)) for i in range(n)]
    msgs = [g.round_evals(TRAILING)]
    for rnd in range(1, n):
        msg, g = g.fold_round_evals(challenges[rnd - 1], TRAILING)
        msgs.append(msg)
    last = g.fixed_variables(challenges[n - 1], TRAILING)
    torch.cuda.synchronize()
    point = torch.cat(list(reversed(challenges)))   # variable j of the point is the challenge of round n - 1 - j
    finals = [t.evaluations for t in last.tables]
    assert last.num_vars == 0 and len(finals) == 5
    for f, table in zip(finals, tables):
        assert torch.equal(f, table.evaluate(point)), name
    if m.pow2:  # prime-field slots: p(0) + p(1) is the running claim, and the last claim is the summand at the point
        claim = m.elems(host(claim_t))[0]
        for rnd, msg in enumerate(msgs):
            p = m.elems(host(msg))
            assert np.array_equal(m.add(p[0], p[1]), claim), (name, rnd)
            claim = _interp(m, host(msg), host(challenges[rnd]), 3)
        e, pl, qh, ph, ql = [m.elems(host(f))[0] for f in finals]
        lm = m.elems(host(lam))[0]
        inner = m.add(m.add(m.mul(pl, qh), m.mul(ph, ql)), m.mul(lm, m.mul(ql, qh)))
        assert np.array_equal(m.mul(e, inner), claim)
    with pytest.raises(RingError, match="trailing"):
        FractionTree(ring, dev(torch, pw), dev(torch, qw), nv, order=LEADING).halves(1)


@pytest.mark.parametrize("name,k", [("goldilocks", 6), ("babybear", 5), ("stark", 4)])
def test_logup_end_to_end(torch_cuda, name, k):
    """sum_j m_j / (alpha - t_j) - sum_i 1 / (alpha - a_i) = 0 on ring elements (slot by slot): 8 table values with multiplicities and
    20 lookups are 28 stored leaves of 32, built on the host with the model's arithmetic; the root numerator is the zero element, and
    is not after one lookup is moved off the table"""
    torch = torch_cuda
    from stark_rings_amd import FractionTree

    m = model_for(name, k)
    ring = m.ring
    rs = np.random.RandomState(k)
    table = m.elems(m.uniform(0x10C0, 8))
    alpha = m.elems(m.uniform(0x10C1, 1))[0]
    picks = [int(x) for x in rs.randint(0, 8, 20)]
    count = lambda c: np.array([c % m.p] * ring.degree, dtype=object)  # noqa: E731

    def roots(lookups):
        p_els = [count(picks.count(j)) for j in range(8)] + [count(m.p - 1)] * 20
        q_els = [m.sub(alpha, t) for t in table] + [m.sub(alpha, a) for a in lookups]
        out = []
        for order in ORDERS:
            tree = FractionTree(ring, dev(torch, m.words(p_els)), dev(torch, m.words(q_els)), 5, order=order)
            torch.cuda.synchronize()
            assert tree.n_leaves == 28
            out.append([host(t) for t in tree.root()])
        assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
        return out[0]

    num, den = roots([table[j] for j in picks])
    assert not num.any() and den.any(), name
    off = [table[j] for j in picks]
    off[7] = m.add(off[7], count(1))   # leaves the table in every slot (a collision has probability 8 / p per slot)
    assert all(not np.array_equal(off[7], t) for t in table)
    num, den = roots(off)
    assert num.reshape(ring.degree, -1).any(axis=1).all(), name


@pytest.mark.parametrize("name,k,nv", [("goldilocks", 6, 7), ("stark", 4, 5), ("babybear72", 0, 7)], ids=["goldilocks", "stark", "babybear72"])
@pytest.mark.parametrize("order", ORDERS, ids=ORDER_IDS)
def test_a_tree_is_capturable_on_a_fresh_context(torch_cuda, name, k, nv, order):
    """Captured into a graph on a non-default stream on a context that has never run the call (or anything else) eagerly; replayed
    twice on new leaves in the same buffers.  One branch, nothing forked: later launches read what earlier ones wrote."""
    torch = torch_cuda
    from stark_rings_amd import CyclotomicRing, frac_tree_dev, frac_tree_plan

    m = model_for(name, k)
    fresh = CyclotomicRing(name, k, device=0)
    w, full = m.w, 1 << nv
    n = full - 3
    assert frac_tree_plan(fresh, nv, order)[1] >= 2
    t_p, t_q = dev(torch, m.uniform(0x88, full)), dev(torch, m.uniform(0x89, full))
    out_p = torch.zeros((full - 1) * w, dtype=torch.int64, device="cuda")
    out_q = torch.zeros_like(out_p)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        frac_tree_dev(fresh, out_p, out_q, t_p[:n * w], t_q[:n * w], nv, order, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    for seed in (0x91, 0x93):
        pw, qw = m.uniform(seed, full), m.uniform(seed + 1, full)
        t_p.copy_(dev(torch, pw))
        t_q.copy_(dev(torch, qw))
        wp, wq, _, _ = tree_dev(torch, m.ring, t_p[:n * w], t_q[:n * w], nv, order)     # eager, on the long-lived context
        torch.cuda.synchronize()
        out_p.zero_()
        out_q.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(host(out_p), host(wp)) and np.array_equal(host(out_q), host(wq)), (name, order, seed)
    want = model_tree(m, m.elems(pw)[:n], m.elems(qw)[:n], nv, order)
    assert np.array_equal(host(out_p), want[0]) and np.array_equal(host(out_q), want[1])
    del g
    fresh.close()


@pytest.mark.parametrize("name,k,nv", CASES, ids=IDS)
def test_the_host_pointer_form_and_the_class_agree_with_the_device_call(torch_cuda, name, k, nv):
    torch = torch_cuda
    from stark_rings_amd import FractionTree, RingError
    from stark_rings_amd.frac_tree import frac_tree

    m = model_for(name, k)
    ring = m.ring
    w, full = m.w, 1 << nv
    pw, qw, _, _ = leaves_for(m, nv)
    t_p, t_q = dev(torch, pw), dev(torch, qw)
    for n in (full, full - 3, 0):
        for order in ORDERS:
            for numer in (True, False):
                wp, wq, _, _ = tree_dev(torch, ring, t_p[:n * w] if numer else None, t_q[:n * w], nv, order)
                torch.cuda.synchronize()
                hp, hq = frac_tree(ring, pw[:n * w] if numer else None, qw[:n * w], nv, order)
                assert np.array_equal(hp, host(wp)) and np.array_equal(hq, host(wq)), (name, n, order, numer)
                tree = FractionTree(ring, t_p if numer else None, t_q, nv, n_leaves=n, order=order)
                torch.cuda.synchronize()
                assert tree.num_vars == nv and tree.n_leaves == n
                assert torch.equal(tree.p_layers, wp) and torch.equal(tree.q_layers, wq)
                end = 0
                for lvl in range(1, nv + 1):
                    big_p, big_q = tree.layer(lvl)
                    assert tree.layer_offset(lvl) == end and big_p.num_vars == big_q.num_vars == nv - lvl and len(big_p) == len(big_q) == 1 << (nv - lvl)
                    assert torch.equal(big_p.evaluations, wp[end * w:(end + len(big_p)) * w])
                    assert torch.equal(big_q.evaluations, wq[end * w:(end + len(big_q)) * w])
                    assert big_p.evaluations.data_ptr() == tree.p_layers.data_ptr() + end * w * 8, "a view, not a copy"
                    assert big_q.evaluations.data_ptr() == tree.q_layers.data_ptr() + end * w * 8, "a view, not a copy"
                    end += len(big_p)
                root_p, root_q = tree.root()
                assert torch.equal(root_p, wp[-w:]) and torch.equal(root_q, wq[-w:])
                assert root_p.data_ptr() == tree.p_layers.data_ptr() + (full - 2) * w * 8
                if order == TRAILING and nv >= 2:
                    ops = tree.halves(2)
                    below = tree.layer_offset(1) * w * 8
                    quarter = (full // 4) * w * 8
                    assert [t.evaluations.data_ptr() for t in ops] == [tree.p_layers.data_ptr() + below, tree.p_layers.data_ptr() + below + quarter,
                                                                        tree.q_layers.data_ptr() + below, tree.q_layers.data_ptr() + below + quarter]
                if n == full and numer:
                    l0 = tree.layer(0)
                    assert l0[0].evaluations.data_ptr() == t_p.data_ptr() and l0[1].evaluations.data_ptr() == t_q.data_ptr()
                elif n != full:
                    with pytest.raises(RingError, match="truncated"):
                        tree.layer(0)
                else:
                    with pytest.raises(RingError, match="without stored numerators"):
                        tree.layer(0)
                with pytest.raises(RingError, match="out of range"):
                    tree.layer(nv + 1)
    single = FractionTree(ring, t_p[:w], t_q[:w], 0)
    assert single.p_layers.numel() == 0 and torch.equal(single.root()[0], t_p[:w]) and torch.equal(single.root()[1], t_q[:w])
    with pytest.raises(RingError, match="no variables"):
        FractionTree(ring, None, t_q[:w], 0).root()


def test_the_pinned_vectors(torch_cuda):
    torch = torch_cuda
    for c in KATS:
        name, k, nv, n = c["ring"], c["log2_degree"], c["num_vars"], c["n_leaves"]
        m = model_for(name, k)
        to_words = (lambda els: O.to_mont(m.F, [int(x) for e in els for x in e])) if c["form"] == "standard" else \
            (lambda els: np.array([x for e in els for x in e], dtype=np.uint64))
        t_p, t_q = dev(torch, to_words(c["p_leaves"])), dev(torch, to_words(c["q_leaves"]))
        assert t_p.numel() == t_q.numel() == n * m.w
        for key, order in (("leading", LEADING), ("trailing", TRAILING)):
            for tag, numer in (("", True), ("_no_numerators", False)):
                got = tree_dev(torch, m.ring, t_p if numer else None, t_q, nv, order)
                check(torch, m, got, (to_words(c[key + tag]["p"]), to_words(c[key + tag]["q"])), (name, key, tag))


def test_every_refusal_names_its_reason(torch_cuda):
    torch = torch_cuda
    from stark_rings_amd import FractionTree, RingError, _lib, frac_tree_dev

    ring = ring_for("goldilocks", 6)
    w = ring.words_per_elem
    nv = 4
    lib, ctx = ring._lib, ring._ctx
    bufs = [torch.zeros(16 * w, dtype=torch.int64, device="cuda") for _ in range(4)]
    po, qo, pi, qi = [ctypes.c_void_p(b.data_ptr()) for b in bufs]
    null = ctypes.c_void_p(0)

    def refused(args, reason):
        assert lib.sr_frac_tree_dev(ctx, *args, None) == 1, args
        assert reason in _lib.last_error(), (reason, _lib.last_error())

    refused((po, qo, pi, qi, 16, nv, 2), "unknown order")
    refused((po, qo, pi, qi, 17, nv, TRAILING), "n_leaves exceeds 2^num_vars")
    refused((po, qo, pi, qi, 16, 48, TRAILING), "num_vars must be below 48")
    refused((po, qo, pi, qi, 16, 47, TRAILING), "element count too large")
    refused((null, qo, pi, qi, 16, nv, TRAILING), "null output buffer")
    refused((po, null, pi, qi, 16, nv, TRAILING), "null output buffer")
    refused((po, qo, pi, null, 16, nv, TRAILING), "null denominator leaves")
    # any overlap of either output with either stored input, or of the two outputs: the first and the last word of either range
    both = torch.zeros(64 * w, dtype=torch.int64, device="cuda")
    base = both.data_ptr()
    at = lambda words: ctypes.c_void_p(base + words * 8)  # noqa: E731
    far = [at(32 * w), at(48 * w)]
    refused((at(0), at(15 * w - 1), far[0], far[1], 16, nv, TRAILING), "d_p_layers overlaps d_q_layers")
    refused((at(15 * w - 1), at(0), far[0], far[1], 16, nv, TRAILING), "d_p_layers overlaps d_q_layers")
    refused((at(0), far[0], far[1], at(15 * w - 1), 16, nv, TRAILING), "d_p_layers overlaps d_q_leaves")
    refused((at(16 * w - 1), far[0], far[1], at(0), 16, nv, TRAILING), "d_p_layers overlaps d_q_leaves")
    refused((far[0], at(0), far[1], at(15 * w - 1), 16, nv, TRAILING), "d_q_layers overlaps d_q_leaves")
    refused((far[0], at(16 * w - 1), far[1], at(0), 16, nv, LEADING), "d_q_layers overlaps d_q_leaves")
    refused((at(0), far[0], at(15 * w - 1), far[1], 16, nv, TRAILING), "d_p_layers overlaps d_p_leaves")
    refused((at(16 * w - 1), far[0], at(0), far[1], 16, nv, TRAILING), "d_p_layers overlaps d_p_leaves")
    refused((far[0], at(0), at(15 * w - 1), far[1], 16, nv, TRAILING), "d_q_layers overlaps d_p_leaves")
    refused((far[0], at(16 * w - 1), at(0), far[1], 16, nv, LEADING), "d_q_layers overlaps d_p_leaves")
    # back to back is no overlap (15, 15, 16 and 16 elements in a row); neither are leaves that are not stored; the inputs may coincide
    assert lib.sr_frac_tree_dev(ctx, at(0), at(15 * w), at(30 * w), at(46 * w), 16, nv, TRAILING, None) == 0
    assert lib.sr_frac_tree_dev(ctx, at(0), at(15 * w), at(0), at(0), 0, nv, TRAILING, None) == 0
    assert lib.sr_frac_tree_dev(ctx, at(0), at(15 * w), at(30 * w), at(30 * w), 16, nv, LEADING, None) == 0
    assert lib.sr_frac_tree_dev(ctx, at(0), at(15 * w), null, at(30 * w), 16, nv, LEADING, None) == 0   # no numerators stored
    assert lib.sr_frac_tree_dev(ctx, null, null, null, null, 0, 0, TRAILING, None) == 0   # num_vars = 0: nothing written
    torch.cuda.synchronize()
    host_buf = np.zeros(64 * w, dtype=np.uint64)
    hp = lambda words: ctypes.cast(ctypes.c_void_p(host_buf.ctypes.data + words * 8), _lib.u64p)  # noqa: E731
    assert lib.sr_frac_tree(ctx, hp(0), hp(16 * w), hp(32 * w), hp(0), 16, nv, TRAILING) == 1 and "overlaps" in _lib.last_error()
    assert lib.sr_frac_tree(ctx, hp(0), hp(16 * w), hp(32 * w), hp(48 * w), 1, nv, 7) == 1 and "unknown order" in _lib.last_error()
    # the mirror
    layers = torch.zeros(15 * w, dtype=torch.int64, device="cuda")
    with pytest.raises(RingError, match="must hold"):
        frac_tree_dev(ring, layers[:14 * w], bufs[1][:15 * w], bufs[2], bufs[3], nv)
    with pytest.raises(RingError, match="more leaves"):
        frac_tree_dev(ring, layers, bufs[1][:15 * w], bufs[2], bufs[3], 3)
    with pytest.raises(RingError, match="same number"):
        frac_tree_dev(ring, layers, bufs[1][:15 * w], bufs[2][:8 * w], bufs[3], nv)
    with pytest.raises(RingError, match="unknown order"):
        FractionTree(ring, bufs[2], bufs[3], nv, order=2)
    with pytest.raises(RingError, match="n_leaves"):
        FractionTree(ring, bufs[2], bufs[3], nv, n_leaves=17)
    with pytest.raises(RingError, match="num_vars"):
        FractionTree(ring, bufs[2], bufs[3], 48)
