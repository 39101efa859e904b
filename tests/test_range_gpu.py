"""GPU parity of the range-check rounds (sr_range_wround_evals[_dev], RangePolynomial, EqSumCheck over it) for all six ring ids.  Every
comparison is bit-exact.  Expected values come from tools/model_range.py (pinned by tests/test_range_host.py), which evaluates the
definition literally, and from three device-side compositions of the older entry points:
  bound 2        vpoly_wround_evals_dev on (f, f - 1, f + 1), made with add_scalar_dev, one term of three factors per table (at most two
                 tables: eight slots); those tables are full, so this oracle is compared on full tables only
  any bound      point by point: every table folded at R::from(t) (sr_mle_fix_variables_dev), shifted by every j (add_scalar_dev),
                 multiplied up with the weights (ntt_mul_dev), summed (sum_dev), times the coefficient (mul_elem_dev)
  a whole check  EqSumCheck over the VirtualPolynomial of (f, f - 1, f + 1) at bound 2
The shapes are those of tests/test_sumcheck_fold_gpu.py: several lane-groups on one element, records and the workspace."""
import ctypes
import json
import math
import os
import sys

import numpy as np
import pytest

import oracle_lib as O
from stark_rings_amd import RangePolynomial, range_wround_evals, range_wround_evals_dev, range_wround_plan
from test_mle_gpu import POISON, dev, fold_dev, host, model_for, ring_for
from test_sumcheck_fold_gpu import CASES, IDS, challenge, elems_agree
from test_vpoly_gpu import one_of
from test_wsumcheck_gpu import wround_dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import model_range as R  # noqa: E402

pytestmark = pytest.mark.gpu
LEADING, TRAILING = 0, 1
ORDERS = (LEADING, TRAILING)
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "range_kats.json")))
POISON_I64 = POISON - (1 << 64)
SIX = [("goldilocks", 6), ("babybear", 5), ("stark", 4), ("goldilocks24", 0), ("babybear72", 0), ("frog16", 0)]
# points per launch (csrc/range_check.hpp): bound 2 is one launch for the one-limb fields and several for the others, bound 8 several
# for every ring
PER_LAUNCH = {"goldilocks": 7, "babybear": 8, "stark": 3, "goldilocks24": 2, "babybear72": 2, "frog16": 2}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


_words = {}


def words_for(name, k, nv):
    """eight full tables, eight coefficients and the weights of a case, made once and never changed"""
    if (name, k, nv) not in _words:
        m = model_for(name, k)
        _words[(name, k, nv)] = ([m.uniform(0x7A000 + j, 1 << nv) for j in range(8)], m.uniform(0x7AC0, 8), m.uniform(0x7AE0 + nv, 1 << (nv - 1)))
    return _words[(name, k, nv)]


def range_dev(torch, ring, weights, tables, bound, coeffs, nv, order, stream=None, work_fill=0x3C3C3C3C3C3C3C3C):
    """the _dev call with a workspace of exactly the planned size, pre-filled with a pattern; two elements of poison behind the message"""
    w, n = ring.words_per_elem, 2 * bound
    buf = torch.full(((n + 2) * w,), POISON_I64, dtype=torch.int64, device="cuda")
    work_elems, launches = range_wround_plan(ring, nv, len(tables), bound, order)
    assert (work_elems == 0) == (launches == 1)
    work = torch.full((work_elems * w,), work_fill, dtype=torch.int64, device="cuda") if work_elems else None
    range_wround_evals_dev(ring, buf[:n * w], weights, tables, bound, coeffs, nv, order, work, stream=stream)
    assert bool((buf[n * w:] == POISON_I64).all())
    return buf[:n * w]


def image(m, j):
    """the memory image of the base-field element j (signed), as add_scalar_dev takes it"""
    return O.to_mont(m.F, [j % m.p])


def shifted_tables(torch, m, ring, t):
    """(f, f - 1, f + 1) of a full table"""
    return [t, ring.add_scalar_dev(t.clone(), image(m, -1), True), ring.add_scalar_dev(t.clone(), image(m, 1), True)]


def composed_bound_two(torch, m, ring, weights, tables, coeffs, nv, order):
    slots = [s for t in tables for s in shifted_tables(torch, m, ring, t)]
    terms = [[3 * i, 3 * i + 1, 3 * i + 2] for i in range(len(tables))]
    return wround_dev(torch, ring, weights, slots, terms, coeffs, nv, order)


def composed_points(torch, m, ring, weights, tables, bound, coeffs, nv, order):
    """any bound and any storage, from the older entry points, point by point; a folded table is whole (its truncated tail is zero, and
    P_B(0) = 0)"""
    w, out = ring.words_per_elem, []
    t_elem = m.zero()
    for t in range(2 * bound):
        point = dev(torch, m.words([t_elem]))
        total = torch.zeros(w, dtype=torch.int64, device="cuda")
        for i, f in enumerate(tables):
            if f.numel() == 0:
                continue
            folded = fold_dev(torch, ring, f, nv, point, order)[0]
            acc = weights.clone()
            for j in range(-(bound - 1), bound):
                x = folded.clone()
                if j:
                    ring.add_scalar_dev(x, image(m, -j), True)
                ring.ntt_mul_dev(acc, x)
            o = torch.empty(w, dtype=torch.int64, device="cuda")
            ring.sum_dev(o, acc)
            if coeffs is not None:
                ring.mul_elem_dev(o, coeffs[i * w:(i + 1) * w].clone())
            ring.add_dev(total, o)
        out.append(total)
        t_elem = m.add(t_elem, one_of(m))
    return torch.cat(out)


def model_message(m, tables_words, bound, coeff_words, weight_words, nv, order):
    els = [m.elems(t) for t in tables_words]
    ce = None if coeff_words is None else m.elems(coeff_words)
    return R.wround_evals(els, bound, ce, m.elems(weight_words), nv, order, m.zero(), one_of(m), m.add, m.sub, m.mul)


def cut(tables, sizes, w):
    return [t[:n * w] for t, n in zip(tables, sizes)]


# ---- the plans the cases reach ----------------------------------------------------------------------------------------------------------
def test_the_cases_reach_single_launches_several_launches_and_records():
    seen = set()
    for name, k, nv in CASES:
        ring = ring_for(name, k)
        for bound in (2, 3, 8):
            work, launches = range_wround_plan(ring, nv, 3, bound, LEADING)
            points = -(-2 * bound // PER_LAUNCH[name])
            records = ring.mle_round_plan(nv, 1, LEADING)[0] // 2
            assert work == max(records, 2 if points > 1 else 0) * 2 * bound and launches == points + (1 if work else 0)
            seen.add((points > 1, records > 1))
    assert seen == {(False, False), (False, True), (True, False), (True, True)}, seen


# ---- against the compositions -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k,nv", CASES, ids=IDS)
def test_the_call_matches_the_compositions_in_both_orders(torch_cuda, name, k, nv):
    """1, 3 and 8 tables at bounds 2, 3 and 8, with and without coefficients, full and truncated; bound 2 on one and two full tables
    against the weighted round of the shifted tables as well"""
    torch = torch_cuda
    m, ring = model_for(name, k), ring_for(name, k)
    w, full = ring.words_per_elem, 1 << nv
    half = full // 2
    tw, cw, ww = words_for(name, k, nv)
    dt, dc, dw = [dev(torch, t) for t in tw], dev(torch, cw), dev(torch, ww)
    trunc3 = (full - 1, half + 1, full) if nv >= 2 else (1, 2, 2)
    trunc8 = (full, full - 3, half, half + 1, 1, full, 0, full - 1) if nv >= 3 else (full,) * 8
    for order in ORDERS:
        for nt in (1, 2):
            for coeffs in (dc[:nt * w], None):
                got = range_dev(torch, ring, dw, dt[:nt], 2, coeffs, nv, order)
                assert torch.equal(got, composed_bound_two(torch, m, ring, dw, dt[:nt], coeffs, nv, order)), (name, nt, order)
                if nt == 1:
                    assert torch.equal(got, composed_points(torch, m, ring, dw, dt[:nt], 2, coeffs, nv, order)), (name, nt, order)
        for nt, bound, coeffs, sizes in ((3, 3, dc[:3 * w], None), (3, 8, None, trunc3), (8, 3, None, trunc8), (8, 8, dc, None), (3, 2, dc[:3 * w], trunc3)):
            tabs = dt[:nt] if sizes is None else cut(dt, sizes[:nt], w)
            got = range_dev(torch, ring, dw, tabs, bound, coeffs, nv, order)
            assert torch.equal(got, composed_points(torch, m, ring, dw, tabs, bound, coeffs, nv, order)), (name, nt, bound, order)


# ---- against the model -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nv", [1, 2, 3])
@pytest.mark.parametrize("name,k", SIX, ids=[c[0] for c in SIX])
def test_small_shapes_match_the_model(torch_cuda, name, k, nv):
    """one and two variables and the smallest shape with truncations of every kind: odd n_evals in leading order, n_evals <= half and
    half < n_evals < 2^num_vars in trailing order, one empty table among full ones, all empty"""
    torch = torch_cuda
    m, ring = model_for(name, k), ring_for(name, k)
    w, full = ring.words_per_elem, 1 << nv
    half = full // 2
    tw, cw, ww = words_for(name, k, nv)
    dw, dc = dev(torch, ww), dev(torch, cw)
    shapes = [(1, 2, (full,), True), (3, 3, (full, full, full), False), (8, 8, (full,) * 8, True)]
    if nv == 3:
        shapes += [(3, 3, (5, 1, 7), True), (3, 8, (3, 4, 5), False), (3, 2, (full, 0, full), True), (8, 3, (2, 8, 0, 3, 6, 1, 7, 5), True),
                   (2, 3, (0, 0), True)]
    for nt, bound, sizes, with_coeffs in shapes:
        words = cut(tw, sizes, w)
        tabs = [dev(torch, t) for t in words]
        for order in ORDERS:
            got = range_dev(torch, ring, dw, tabs, bound, dc[:nt * w] if with_coeffs else None, nv, order)
            want = model_message(m, words, bound, cw[:nt * w] if with_coeffs else None, ww, nv, order)
            assert elems_agree(m, host(got), want, None), (name, nv, nt, bound, sizes, order)
            if not any(sizes):
                assert not host(got).any()


def test_the_pinned_vectors_on_the_device(torch_cuda):
    torch = torch_cuda
    for case in KATS["cases"]:
        ring = ring_for(case["ring"], case["log2_degree"])
        nv, bound = case["num_vars"], case["bound"]
        if case["form"] == "standard":
            F = O.FIELD_ID[case["ring"]]
            put = lambda elems: dev(torch, O.to_mont(F, [x for e in elems for x in e]))  # noqa: E731
            get = lambda t: [int(x) for x in O.from_mont(F, host(t))]  # noqa: E731
            inputs = (case["tables"], case["coeffs"], case["weights"])
        else:
            put = lambda elems: dev(torch, np.array([x for e in elems for x in e], dtype=np.uint64))  # noqa: E731
            get = lambda t: [int(x) for x in host(t)]  # noqa: E731
            inputs = R.kat_inputs(case["ring"], case["n_evals"], nv)
        dt, dc, dw = [put(f) for f in inputs[0]], put(inputs[1]), put(inputs[2])
        for key, order in (("leading", LEADING), ("trailing", TRAILING)):
            assert get(range_dev(torch, ring, dw, dt, bound, dc, nv, order)) == [x for e in case[key] for x in e], (case["ring"], key)


# ---- truncated storage reads nothing beyond it --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k,nv", CASES[:8], ids=IDS[:8])
def test_weights_and_tables_beyond_the_visited_pairs_are_not_read(torch_cuda, name, k, nv):
    """the tables end in poison right behind their stored part and the weights beyond the last visited pair are poison, which is not
    canonical in any field and would show"""
    torch = torch_cuda
    m, ring = model_for(name, k), ring_for(name, k)
    w, full = ring.words_per_elem, 1 << nv
    half = full // 2
    tw, cw, ww = words_for(name, k, nv)
    dw, dc = dev(torch, ww), dev(torch, cw)
    for sizes in ((full - 3, half + 1, 5), (half - 1, 1, 3), (0, 0, 0)):
        tabs = []
        for t, n in zip(tw, sizes):
            buf = torch.full(((n + 1) * w,), POISON_I64, dtype=torch.int64, device="cuda")
            buf[:n * w] = dev(torch, t[:n * w])
            tabs.append(buf[:n * w])
        for order in ORDERS:
            pairs = lambda n: (n + 1) // 2 if order == LEADING else min(n, half)  # noqa: E731
            visited = max(pairs(n) for n in sizes)
            poisoned = dw.clone()
            poisoned[visited * w:] = POISON_I64
            got = range_dev(torch, ring, poisoned, tabs, 3, dc[:3 * w], nv, order)
            assert torch.equal(got, range_dev(torch, ring, dw, [dev(torch, t[:n * w]) for t, n in zip(tw, sizes)], 3, dc[:3 * w], nv, order)), (name, sizes, order)
            if not any(sizes):
                assert not host(got).any()


# ---- all p - 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k,nv", [("goldilocks", 1, 14), ("babybear", 1, 14), ("stark", 1, 13), ("goldilocks24", 0, 11), ("babybear72", 0, 11),
                                       ("frog16", 0, 12)], ids=[c[0] for c in SIX])
def test_all_p_minus_one_inputs_pass_several_lazy_reduction_intervals(torch_cuda, name, k, nv):
    """every table, weight and coefficient word is p - 1, the largest canonical image; eight tables add eight terms per pair, so the
    sums are reduced every eight pairs and a lane of these shapes (two records) takes 16.  lo == hi, so h(t) = pairs * g(e) at every t,
    which the model computes from one pair."""
    torch = torch_cuda
    m, ring = model_for(name, k), ring_for(name, k)
    w, bound = ring.words_per_elem, 8
    pairs = 1 << (nv - 1)
    top = m.p - 1 if m.p - 1 < 1 << 63 else m.p - 1 - (1 << 64)
    if ring.limbs == 1:
        table = torch.full((2 * pairs * w,), top, dtype=torch.int64, device="cuda")
        e_words = np.full(w, m.p - 1, dtype=np.uint64)
    else:
        e_words = m.const(m.p - 1, 1)
        table = dev(torch, np.tile(e_words, 2 * pairs))
    e = m.elems(e_words)[0]
    one_pair = R.wround_evals([[e, e]] * 8, bound, [e] * 8, [e], 1, LEADING, m.zero(), one_of(m), m.add, m.sub, m.mul)[0]
    want = m.words([(one_pair * pairs) % m.p]) if m.pow2 else ((one_pair.astype(object) * pairs) % m.p).astype(np.uint64)
    dc, dw = table[:8 * w].clone(), table[:pairs * w].clone()
    for order in ORDERS:
        got = host(range_dev(torch, ring, dw, [table] * 8, bound, dc, nv, order))
        assert np.array_equal(got, np.tile(want, 2 * bound)), (name, order)


# ---- eight bytes off --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k,nv", [("goldilocks", 6, 10), ("babybear", 5, 11), ("goldilocks", 8, 8), ("babybear", 9, 7), ("goldilocks24", 0, 5)])
def test_every_buffer_off_by_eight_bytes_gives_the_same_result(torch_cuda, name, k, nv):
    """pointers 8 bytes behind a 16-byte boundary, with a word of poison in front (the guard) and poison behind d_out (range_dev); the
    one-limb fields take the one-coefficient path"""
    torch = torch_cuda
    ring = ring_for(name, k)
    w, full = ring.words_per_elem, 1 << nv
    tw, cw, ww = words_for(name, k, nv)
    aligned = [dev(torch, t[:n * w]) for t, n in zip(tw, (full, full - 3, full // 2 + 1))]
    dc, dw = dev(torch, cw[:3 * w]), dev(torch, ww)

    def shift(t):
        buf = torch.full((t.numel() + 2,), POISON_I64, dtype=torch.int64, device="cuda")
        buf[1:-1] = t
        assert buf[1:-1].data_ptr() % 16 == 8
        return buf[1:-1]

    for order in ORDERS:
        for bound in (2, 8):
            want = range_dev(torch, ring, dw, aligned, bound, dc, nv, order)
            for tabs, wts, cc in (([shift(t) for t in aligned], shift(dw), shift(dc)), (aligned, shift(dw), dc), ([aligned[0], shift(aligned[1]), aligned[2]], dw, dc)):
                assert torch.equal(range_dev(torch, ring, wts, tabs, bound, cc, nv, order), want), (name, bound, order)
            # d_out itself 8 bytes off, poison on both sides
            n = 2 * bound
            buf = torch.full(((n + 2) * w + 2,), POISON_I64, dtype=torch.int64, device="cuda")
            out = buf[1:1 + n * w]
            assert out.data_ptr() % 16 == 8
            work_elems, _ = range_wround_plan(ring, nv, 3, bound, order)
            work = torch.full((work_elems * w + 1,), POISON_I64, dtype=torch.int64, device="cuda")[1:] if work_elems else None
            range_wround_evals_dev(ring, out, dw, aligned, bound, dc, nv, order, work)
            assert torch.equal(out, want) and int(buf[0]) == POISON_I64 and bool((buf[1 + n * w:] == POISON_I64).all()), (name, bound, order)


# ---- the workspace, the host-pointer form, the class ----------------------------------------------------------------------------------------
def test_workspace_contents_do_not_matter_and_the_host_pointer_form_and_the_class_agree(torch_cuda):
    torch = torch_cuda
    from stark_rings_amd import DenseMultilinearExtension as MLE, MLE_TRAILING, RingError

    for name, k, nv in (("goldilocks", 6, 10), ("stark", 4, 11), ("babybear72", 0, 3), ("frog16", 0, 13)):
        m, ring = model_for(name, k), ring_for(name, k)
        w, full = ring.words_per_elem, 1 << nv
        tw, cw, ww = words_for(name, k, nv)
        words = cut(tw, (full, full - 5, full // 2 + 1), w)
        tabs, dc, dw = [dev(torch, t) for t in words], dev(torch, cw[:3 * w]), dev(torch, ww)
        r = challenge(torch, m, 0x4A04)
        for order in ORDERS:
            for bound in (2, 5):
                a = range_dev(torch, ring, dw, tabs, bound, dc, nv, order, work_fill=0)
                assert torch.equal(a, range_dev(torch, ring, dw, tabs, bound, dc, nv, order, work_fill=POISON_I64))
                assert np.array_equal(range_wround_evals(ring, ww, words, bound, cw[:3 * w], nv, order), host(a))
                assert np.array_equal(range_wround_evals(ring, ww, words[:1], bound, None, nv, order),
                                      host(range_dev(torch, ring, dw, tabs[:1], bound, None, nv, order)))
                g = RangePolynomial(ring, [MLE(ring, nv, t) for t in tabs], bound, dc)
                assert g.degree == 2 * bound - 1 and g.num_vars == nv and g.terms
                assert torch.equal(g.round_evals_weighted(dw, order), a)
                msg, h = g.fold_round_evals_weighted(r, dw[:dw.numel() // 2], order)
                folded = [fold_dev(torch, ring, t, nv, r, order)[0] for t in tabs]
                assert h.num_vars == nv - 1 and all(torch.equal(t.evaluations, f) for t, f in zip(h.tables, folded))
                assert torch.equal(msg, range_dev(torch, ring, dw[:dw.numel() // 2], folded, bound, dc, nv - 1, order))
        with pytest.raises(RingError):
            g.round_evals_weighted(dw, MLE_TRAILING + 1)
        with pytest.raises(RingError):
            g.round_evals_weighted(dw[:dw.numel() // 2])  # half the weights
        with pytest.raises(RingError):
            RangePolynomial(ring, [MLE(ring, nv, t) for t in tabs], 9)


# ---- capture ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k,nv", [("goldilocks", 6, 10), ("frog16", 0, 13)])
def test_capture_on_a_fresh_context_and_two_replays_agree(torch_cuda, name, k, nv):
    torch = torch_cuda
    from stark_rings_amd import CyclotomicRing

    ring = CyclotomicRing(name, k, device=0)  # fresh: nothing has run on it, so nothing is warm
    try:
        w, bound, order = ring.words_per_elem, 8, LEADING
        tw, cw, ww = words_for(name, k, nv)
        tabs, dc, dw = [dev(torch, t) for t in tw[:3]], dev(torch, cw[:3 * w]), dev(torch, ww).clone()
        out = torch.empty(2 * bound * w, dtype=torch.int64, device="cuda")
        work_elems, launches = range_wround_plan(ring, nv, 3, bound, order)
        assert work_elems and launches >= 3
        work = torch.full((work_elems * w,), POISON_I64, dtype=torch.int64, device="cuda")
        side = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            range_wround_evals_dev(ring, out, dw, tabs, bound, dc, nv, order, work, stream=side)
        graph.replay()
        torch.cuda.synchronize()
        first = out.clone()
        assert torch.equal(first, range_dev(torch, ring_for(name, k), dw, tabs, bound, dc, nv, order))
        out.fill_(POISON_I64)
        work.fill_(0x1111111111111111)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, first)
        dw.copy_(dev(torch, model_for(name, k).uniform(0x77AA, 1 << (nv - 1))))  # the graph holds pointers, not values
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, range_dev(torch, ring_for(name, k), dw, tabs, bound, dc, nv, order))
    finally:
        ring.close()


# ---- an honest instance, and a planted violation ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bound", [2, 3, 8])
@pytest.mark.parametrize("name,k", SIX, ids=[c[0] for c in SIX])
def test_an_honest_witness_gives_zero_and_a_planted_bound_gives_the_factorial(torch_cuda, name, k, bound):
    """every slot an in-range constant: h(0) = h(1) = 0.  The value B planted in every slot of one first-of-pair element, weights one():
    h(0) = R::from((2 B - 1)!), nonzero for every prime here."""
    torch = torch_cuda
    m, ring = model_for(name, k), ring_for(name, k)
    nv, w = 5, ring.words_per_elem
    rng = np.random.RandomState(0xB0 + bound)

    def constant(j):
        return ring.add_scalar_dev(torch.zeros(w, dtype=torch.int64, device="cuda"), image(m, j), True)

    consts = {j: constant(j) for j in range(-(bound - 1), bound + 1)}
    ones = constant(1).repeat(1 << (nv - 1))
    fact = constant(math.factorial(2 * bound - 1) % m.p)
    assert bool(fact.any())
    dw = dev(torch, words_for(name, k, nv)[2])
    for order in ORDERS:
        tabs = [torch.cat([consts[int(j)] for j in rng.randint(-(bound - 1), bound, 1 << nv)]) for _ in range(2)]
        h = range_dev(torch, ring, dw, tabs, bound, None, nv, order)
        assert not bool(h[:2 * w].any()), (name, bound, order)
        planted = tabs[1].clone()
        at = 6 if order == LEADING else 3  # a first-of-pair position in either order
        planted[at * w:(at + 1) * w] = consts[bound]
        h = range_dev(torch, ring, ones, [tabs[0], planted], bound, None, nv, order)
        assert torch.equal(h[:w], fact) and not bool(h[w:2 * w].any()), (name, bound, order)


# ---- a whole norm check -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name,k", SIX, ids=[c[0] for c in SIX])
def test_a_whole_norm_check_sends_the_messages_of_the_virtual_polynomial_of_shifted_tables(torch_cuda, name, k, order):
    """EqSumCheck(RangePolynomial) at bound 2 and four variables against EqSumCheck over the VirtualPolynomial of (f, f - 1, f + 1):
    every message and every final value, bit for bit"""
    torch = torch_cuda
    from stark_rings_amd import DenseMultilinearExtension as MLE, EqSumCheck, VirtualPolynomial

    m, ring = model_for(name, k), ring_for(name, k)
    nv, w = 4, ring.words_per_elem
    tw, cw, _ = words_for(name, k, nv)
    tabs = [dev(torch, t) for t in tw[:2]]
    dc = dev(torch, cw[:2 * w])
    z = dev(torch, m.uniform(0x2E7, nv))
    rs = [challenge(torch, m, 0x7200 + i) for i in range(nv)]
    g = VirtualPolynomial(ring, nv)
    for i, t in enumerate(tabs):
        g.add_mle_list([MLE(ring, nv, s) for s in shifted_tables(torch, m, ring, t)], dc[i * w:(i + 1) * w])
    want = EqSumCheck(g, z, order)
    got = EqSumCheck(RangePolynomial(ring, [MLE(ring, nv, t) for t in tabs], 2, dc), z, order)
    assert got.degree == want.degree == 3
    for j in range(nv):
        assert torch.equal(got.message(), want.message()), (name, order, j)
        got.next(rs[j])
        want.next(rs[j])
    (gf, ge), (wf, we) = got.final(), want.final()
    assert torch.equal(ge, we) and len(gf) == 2 and len(wf) == 6
    for i in range(2):
        assert torch.equal(gf[i], wf[3 * i]), (name, order, i)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_every_device_refusal_names_its_reason_and_launches_nothing(torch_cuda):
    torch = torch_cuda
    from stark_rings_amd import _lib

    ring = ring_for("goldilocks", 6)
    lib, ctx = ring._lib, ring._ctx
    nv, w, bound = 10, ring.words_per_elem, 8
    canary = 0x0123456789ABCDEF
    full, half = 1 << nv, 1 << (nv - 1)
    f = torch.full((w << nv,), 7, dtype=torch.int64, device="cuda")
    f2 = torch.full((w << nv,), 7, dtype=torch.int64, device="cuda")
    wt = torch.full((w * half,), 9, dtype=torch.int64, device="cuda")
    out = torch.full((2 * bound * w,), canary, dtype=torch.int64, device="cuda")
    co = torch.full((32 * w,), 3, dtype=torch.int64, device="cuda")[:2 * w]  # room behind it for a misplaced d_out
    need, launches = range_wround_plan(ring, nv, 2, bound, LEADING)
    assert 0 < need <= 64 and launches == 4
    work = torch.full((64 * w,), canary, dtype=torch.int64, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    fp, f2p, wtp, op, cp, wp = (t.data_ptr() for t in (f, f2, wt, out, co, work))
    eb = 8 * w
    pa, sa = (ctypes.c_void_p * 8)(fp, f2p), (ctypes.c_size_t * 8)(full, full)

    def call(out_p=op, wts=wtp, tables=pa, sizes=sa, n_tables=2, b=bound, num_vars=nv, order=LEADING, work_p=wp, work_n=64):
        rc = lib.sr_range_wround_evals_dev(ctx, out_p, wts, tables, sizes, n_tables, b, cp, num_vars, order, work_p, work_n, st)
        return rc, _lib.last_error()

    for kw, msg in ((dict(wts=None), "null pointer (d_weights)"), (dict(out_p=None), "null pointer"), (dict(tables=None), "null pointer"),
                    (dict(sizes=None), "null pointer"), (dict(order=2), "unknown order"), (dict(num_vars=0), "num_vars >= 1"),
                    (dict(num_vars=48), "num_vars must be below 48"), (dict(b=1), "bound must be 2 .. 8"), (dict(b=9), "bound must be 2 .. 8"),
                    (dict(n_tables=0), "n_tables must be 1 .. 8"), (dict(n_tables=9), "n_tables must be 1 .. 8"),
                    (dict(sizes=(ctypes.c_size_t * 8)(full, full + 1)), "n_evals exceeds 2^num_vars"),
                    (dict(tables=(ctypes.c_void_p * 8)(fp, None)), "null pointer (a table)"),
                    (dict(work_p=None), "null pointer (d_work)"), (dict(work_n=need - 1), "workspace too small"),
                    (dict(out_p=wtp + eb), "d_out overlaps d_weights"), (dict(work_p=wtp), "d_work overlaps d_weights"),
                    (dict(out_p=fp + eb), "d_out overlaps a table"), (dict(work_p=f2p), "d_work overlaps a table"),
                    (dict(out_p=wp + eb), "d_out overlaps d_work"), (dict(out_p=cp + eb), "d_out overlaps d_coeffs"),
                    (dict(work_p=cp), "d_work overlaps d_coeffs")):
        rc, err = call(**kw)
        assert rc == 1 and msg in err and err.startswith("range_wround: "), (kw, rc, err)
    rc, err = call(num_vars=47, sizes=(ctypes.c_size_t * 8)(1 << 45, 1 << 45))  # within 2^num_vars, beyond what a context addresses
    assert rc == 1 and err == "element count too large", (rc, err)
    torch.cuda.synchronize()
    for t in (out, work):
        assert bool((t == canary).all())
    assert bool((f == 7).all()) and bool((wt == 9).all())
    assert call()[0] == 0
    torch.cuda.synchronize()
    assert not bool((out == canary).any())
