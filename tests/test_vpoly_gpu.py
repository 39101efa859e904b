"""GPU parity of the sum-of-products round calls (sr_vpoly_round_evals[_dev], stark_rings_amd.VirtualPolynomial) for all six ring
ids.  Every comparison is bit-exact.  Expected values come from tools/model_vpoly.py (every table folded with the point [R::from(t)]
by tools/model_mle.py, multiplied term by term, scaled and summed; pinned by tests/test_vpoly_host.py), from sr_mle_round_evals_dev
where the claim is a single product, and from the composition of the entry points that were there before.  The shapes, the element
types and the helpers are those of tests/test_sumcheck_gpu.py and tests/test_mle_gpu.py.

Structures (tools/model_vpoly.py): SINGLE (f0 f1 f2, no coefficients), R1CS c0 e a b - e c, REPEAT c0 f0 f0 f1 f1 + c1 f1 + c2 f2 f3,
MIXED (8 terms of 1,2,3,4,4,3,2,1 factors over 8 tables), CANCEL c f0 f1 - c f1 f0."""
import ctypes
import json
import os
import random
import sys

import numpy as np
import pytest

import oracle_lib as O
from test_mle_gpu import POISON, dev, host, model_for, ring_for
from test_sumcheck_gpu import CASES, FAMILY, IDS, columns, poisoned, round_dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import model_sumcheck as SC  # noqa: E402
import model_vpoly as VP  # noqa: E402

pytestmark = pytest.mark.gpu
LEADING, TRAILING, ROUND_SUM = 0, 1, 2
MODES = (LEADING, TRAILING, ROUND_SUM)
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "vpoly_kats.json")))
STRUCTURES = {"SINGLE": VP.SINGLE, "R1CS": VP.R1CS, "REPEAT": VP.REPEAT, "MIXED": VP.MIXED, "CANCEL": VP.CANCEL}
SMALL = [("goldilocks", 6), ("babybear", 5), ("stark", 4), ("goldilocks24", 0), ("babybear72", 0), ("frog16", 0)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def n_out(mode, terms):
    return 1 if mode == ROUND_SUM else VP.degree(terms) + 1


def vp_dev(torch, ring, tables, terms, coeffs, nv, mode, stream=None, work_fill=0x3C3C3C3C3C3C3C3C):
    """the _dev call with a workspace of exactly the planned size"""
    w = ring.words_per_elem
    out = torch.full((n_out(mode, terms) * w,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    work_elems, _ = ring.vpoly_round_plan(nv, len(tables), len(terms), VP.degree(terms), mode)
    work = torch.full((work_elems * w,), work_fill, dtype=torch.int64, device="cuda") if work_elems else None
    ring.vpoly_round_evals_dev(out, tables, terms, coeffs, nv, mode, work, stream=stream)
    return out


def one_of(m):
    return m.elems(m.one())[0]


def message(m, els, terms, coeffs, nv, mode, zero=None, one=None):
    zero = m.zero() if zero is None else zero
    one = one_of(m) if one is None else one
    if mode == ROUND_SUM:
        return [VP.poly_sum(els, terms, coeffs, nv, zero, m.add, m.mul)]
    return VP.round_evals(els, terms, coeffs, nv, mode, zero, one, m.add, m.sub, m.mul)


def agrees(m, got_words, els, terms, coeffs, nv, mode):
    """els, coeffs: model elements; at D > 2^10 the round modes compare the 96 columns of tests/test_sumcheck_gpu.py::columns (the model
    holds a ring element as D Python integers); the other columns are covered by the composition test at the same kernels"""
    cols = columns(m, 2, mode)
    if cols is None:
        return np.array_equal(got_words, m.words(message(m, els, terms, coeffs, nv, mode)))
    cut = lambda e: e[cols]  # noqa: E731
    want = message(m, [[cut(e) for e in f] for f in els], terms, None if coeffs is None else [cut(c) for c in coeffs], nv, mode,
                   np.array([0] * cols.size, dtype=object), np.array([1] * cols.size, dtype=object))
    got = m.elems(got_words)
    return len(got) == len(want) and all(np.array_equal(g[cols], x) for g, x in zip(got, want))


_tables, _elems, _coeffs = {}, {}, {}


def tables_for(name, k, nv):
    """eight full tables per shape, made once and never changed"""
    if (name, k, nv) not in _tables:
        m = model_for(name, k)
        _tables[(name, k, nv)] = [m.uniform(0x7B000 + j, 1 << nv) for j in range(8)]
    return _tables[(name, k, nv)]


def elems_for(name, k, nv):
    if (name, k, nv) not in _elems:
        m = model_for(name, k)
        _elems[(name, k, nv)] = [m.elems(t) for t in tables_for(name, k, nv)]
    return _elems[(name, k, nv)]


def coeffs_for(name, k, structure):
    """the coefficient words of a structure: seeded uniform ones; R1CS: c1 = -one(); MIXED: 0, one(), p - 1 in every word, uniform;
    CANCEL: (c, -c); SINGLE: none"""
    if (name, k, structure) not in _coeffs:
        m = model_for(name, k)
        terms = STRUCTURES[structure]
        if structure == "SINGLE":
            c = None
        else:
            c = [m.uniform(0xC0EF0 + j, 1) for j in range(len(terms))]
            neg = lambda words: m.words([m.sub(m.zero(), m.elems(words)[0])])  # noqa: E731
            if structure == "R1CS":
                c[1] = neg(m.one())
            if structure == "CANCEL":
                c[1] = neg(c[0])
            if structure == "MIXED":
                c[0], c[1], c[2] = np.zeros(m.w, dtype=np.uint64), m.one(), m.const(m.p - 1, 1)
            c = np.concatenate(c)
        _coeffs[(name, k, structure)] = c
    return _coeffs[(name, k, structure)]


def setup(torch, name, k, nv, structure):
    """(device tables, terms, device coefficients or None, model tables, model coefficients or None) of a structure on full tables"""
    m = model_for(name, k)
    terms = STRUCTURES[structure]
    nt = VP.n_tables(terms)
    cw = coeffs_for(name, k, structure)
    return ([dev(torch, t) for t in tables_for(name, k, nv)[:nt]], terms, None if cw is None else dev(torch, cw),
            elems_for(name, k, nv)[:nt], None if cw is None else m.elems(cw))


def test_the_cases_reach_the_single_launch_and_the_split_path_of_the_new_plan():
    """babybear72 and frog16 take one point per launch (csrc/sumcheck_vpoly.hpp, points_of), so a round message of theirs is never a
    single launch: they reach the single launch through the plain sum, whose kernel is the same instantiation pattern without pairs"""
    rounds, every = {}, {}
    for name, k, nv in CASES:
        ring = ring_for(name, k)
        for nt in (3, 4, 8):
            for d in (1, 2, 3, 4):
                for mode in MODES:
                    work, launches = ring.vpoly_round_plan(nv, nt, 2, d, mode)
                    assert (work == 0) == (launches == 1)
                    every.setdefault(FAMILY.get(name, name), set()).add(launches == 1)
                    if mode != ROUND_SUM:
                        rounds.setdefault(FAMILY.get(name, name), set()).add(launches == 1)
    assert every == {f: {True, False} for f in ("one-limb", "stark", "goldilocks24", "babybear72", "frog16")}, every
    assert rounds == {"one-limb": {True, False}, "stark": {True, False}, "goldilocks24": {True, False}, "babybear72": {False},
                      "frog16": {False}}, rounds


# ---- 1. SINGLE ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k,nv", CASES, ids=IDS)
def test_a_single_product_without_coefficients_is_the_round_call_bit_for_bit(torch_cuda, name, k, nv):
    torch = torch_cuda
    ring = ring_for(name, k)
    dt, terms, _, _, _ = setup(torch, name, k, nv, "SINGLE")
    for mode in MODES:
        assert torch.equal(vp_dev(torch, ring, dt, terms, None, nv, mode), round_dev(torch, ring, dt, nv, mode)), (name, mode)


# ---- 2. R1CS and REPEAT against the model ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("structure", ["R1CS", "REPEAT"])
@pytest.mark.parametrize("name,k,nv", CASES, ids=IDS)
def test_r1cs_and_repeat_match_the_model_in_all_three_modes(torch_cuda, name, k, nv, structure):
    torch = torch_cuda
    m, ring = model_for(name, k), ring_for(name, k)
    dt, terms, dc, els, ce = setup(torch, name, k, nv, structure)
    for mode in MODES:
        assert agrees(m, host(vp_dev(torch, ring, dt, terms, dc, nv, mode)), els, terms, ce, nv, mode), (name, structure, mode)


def test_the_pinned_vectors_on_the_device(torch_cuda):
    torch = torch_cuda
    for case in KATS["cases"]:
        ring = ring_for(case["ring"], case["log2_degree"])
        F = O.FIELD_ID[case["ring"]]
        nv = case["num_vars"]
        dt = [dev(torch, O.to_mont(F, [x for e in f for x in e])) for f in case["tables"]]
        dc = dev(torch, O.to_mont(F, [x for c in case["coeffs"] for x in c]))
        for key, mode in (("leading", LEADING), ("trailing", TRAILING), ("sum", ROUND_SUM)):
            want = case[key] if mode != ROUND_SUM else [case[key]]
            got = O.from_mont(F, host(vp_dev(torch, ring, dt, case["terms"], dc, nv, mode)))
            assert [int(x) for x in got] == [x for e in want for x in e], (case["ring"], case["structure"], key)


# ---- 3. MIXED -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nv", [3, 4, 5])
@pytest.mark.parametrize("name,k", SMALL, ids=[c[0] for c in SMALL])
def test_mixed_matches_the_model_on_small_tables(torch_cuda, name, k, nv):
    torch = torch_cuda
    m, ring = model_for(name, k), ring_for(name, k)
    dt, terms, dc, els, ce = setup(torch, name, k, nv, "MIXED")
    for mode in MODES:
        assert agrees(m, host(vp_dev(torch, ring, dt, terms, dc, nv, mode)), els, terms, ce, nv, mode), (name, nv, mode)


def composed_vpoly(torch, m, tables, terms, coeffs, nv, mode):
    """the message from the entry points that were there before.  Per point: every table folded at t * one (sr_mle_fix_variables_dev);
    per term: the element-wise products (ntt_mul_dev), their sum (sum_dev), times the coefficient (mul_elem_dev), added (add_dev)"""
    ring = m.ring
    w = ring.words_per_elem
    outs = []
    for t in ([None] if mode == ROUND_SUM else range(VP.degree(terms) + 1)):
        cols = []
        for f in tables:
            if t is None:
                full = torch.zeros(w << nv, dtype=torch.int64, device="cuda")
                full[:f.numel()] = f
                cols.append(full)
            else:
                pt = dev(torch, m.words([SC.constant(t, m.zero(), one_of(m), m.add)]))
                o = torch.empty(w << (nv - 1), dtype=torch.int64, device="cuda")
                ring.mle_fix_variables_dev(o, f, nv, pt, mode, None)
                cols.append(o)
        total = torch.zeros(w, dtype=torch.int64, device="cuda")
        for k, term in enumerate(terms):
            acc = cols[term[0]].clone()
            for j in term[1:]:
                ring.ntt_mul_dev(acc, cols[j])
            o = torch.empty(w, dtype=torch.int64, device="cuda")
            ring.sum_dev(o, acc)
            if coeffs is not None:
                ring.mul_elem_dev(o, coeffs[k * w:(k + 1) * w].clone())
            ring.add_dev(total, o)
        outs.append(total)
    return torch.cat(outs)


@pytest.mark.parametrize("name,k,nv", CASES, ids=IDS)
def test_mixed_agrees_with_the_composition_of_the_older_entry_points(torch_cuda, name, k, nv):
    torch = torch_cuda
    m, ring = model_for(name, k), ring_for(name, k)
    dt, terms, dc, _, _ = setup(torch, name, k, nv, "MIXED")
    for mode in MODES:
        got = vp_dev(torch, ring, dt, terms, dc, nv, mode)
        assert torch.equal(got, composed_vpoly(torch, m, dt, terms, dc, nv, mode)), (name, mode)  # every column


# ---- 4. CANCEL, 5. p(0) + p(1) --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k,nv", CASES[:8], ids=IDS[:8])
def test_cancelling_terms_give_zeros(torch_cuda, name, k, nv):
    torch = torch_cuda
    ring = ring_for(name, k)
    dt, terms, dc, _, _ = setup(torch, name, k, nv, "CANCEL")
    for mode in MODES:
        assert not host(vp_dev(torch, ring, dt, terms, dc, nv, mode)).any(), (name, mode)


@pytest.mark.parametrize("structure", ["SINGLE", "R1CS", "REPEAT", "MIXED", "CANCEL"])
@pytest.mark.parametrize("name,k,nv", CASES[:8], ids=IDS[:8])
def test_p0_plus_p1_is_the_plain_sum(torch_cuda, name, k, nv, structure):
    torch = torch_cuda
    m, ring = model_for(name, k), ring_for(name, k)
    dt, terms, dc, _, _ = setup(torch, name, k, nv, structure)
    total = m.elems(host(vp_dev(torch, ring, dt, terms, dc, nv, ROUND_SUM)))[0]
    for mode in (LEADING, TRAILING):
        msg = m.elems(host(vp_dev(torch, ring, dt, terms, dc, nv, mode)))
        assert len(msg) == VP.degree(terms) + 1
        assert np.array_equal(m.add(msg[0], msg[1]), total), (name, structure, mode)


# ---- 6. truncation, 7. empty tables -----------------------------------------------------------------------------------------------------
def truncations(structure, nv):
    """stored sizes per table for which one term ends before another"""
    full, half = 1 << nv, 1 << (nv - 1)
    if structure == "R1CS":  # e, a, b, c: the second term ends at c, long before the first ends at a
        return [(full, full - 1, full, 5), (half + 1, full, 3, full)]
    if structure == "REPEAT":
        return [(5, full, full - 1, half + 1), (full, half, 1, full)]
    return [(full, full - 1, half + 1, 5, full, 1, half, full - 3)]


@pytest.mark.parametrize("structure", ["R1CS", "REPEAT", "MIXED"])
@pytest.mark.parametrize("name,k,nv", CASES[:8], ids=IDS[:8])
def test_truncated_tables_are_never_read_past_their_stored_part(torch_cuda, name, k, nv, structure):
    torch = torch_cuda
    m, ring = model_for(name, k), ring_for(name, k)
    w, full = ring.words_per_elem, 1 << nv
    _, terms, dc, els, ce = setup(torch, name, k, nv, structure)
    tabs = tables_for(name, k, nv)
    for sizes in truncations(structure, nv):
        keep = [poisoned(torch, tabs[j][:n * w], full * w) for j, n in enumerate(sizes)]
        cut = [els[j][:n] for j, n in enumerate(sizes)]
        for mode in MODES:
            got = vp_dev(torch, ring, [v for v, _ in keep], terms, dc, nv, mode)
            if structure == "MIXED" and name not in ("goldilocks", "babybear", "stark"):
                # the slot products of the model run through the oracle one element at a time: MIXED at these sizes is compared with
                # the composition of the older entry points, which honour the same truncated storage
                assert torch.equal(got, composed_vpoly(torch, m, [v for v, _ in keep], terms, dc, nv, mode)), (name, sizes, mode)
            else:
                assert agrees(m, host(got), cut, terms, ce, nv, mode), (name, structure, sizes, mode)


@pytest.mark.parametrize("name,k,nv", CASES[:8], ids=IDS[:8])
def test_an_empty_table_silences_its_terms_only(torch_cuda, name, k, nv):
    """R1CS with an empty c: the message of c0 e a b alone.  e is full; the empty table is a zero-length tensor"""
    torch = torch_cuda
    m, ring = model_for(name, k), ring_for(name, k)
    w, full = ring.words_per_elem, 1 << nv
    _, terms, dc, _, _ = setup(torch, name, k, nv, "R1CS")
    tabs = tables_for(name, k, nv)
    keep = [poisoned(torch, tabs[j][:n * w], full * w) for j, n in enumerate((full, full - 1, full - 2))]
    empty = torch.empty(0, dtype=torch.int64, device="cuda")
    for mode in MODES:
        got = vp_dev(torch, ring, [v for v, _ in keep] + [empty], terms, dc, nv, mode)
        first = vp_dev(torch, ring, [v for v, _ in keep], [terms[0]], dc[:w], nv, mode)
        assert torch.equal(got, first), (name, mode)
        # and that message is c0 times the message of the product e a b from the call that was there before
        want = round_dev(torch, ring, [v for v, _ in keep], nv, mode)
        ring.mul_elem_dev(want, dc[:w].clone())
        assert torch.equal(got, want), (name, mode)


@pytest.mark.parametrize("name,k,nv", CASES[:8], ids=IDS[:8])
def test_every_term_empty_gives_zeros_and_loads_nothing(torch_cuda, name, k, nv):
    torch = torch_cuda
    ring = ring_for(name, k)
    w = ring.words_per_elem
    poison = torch.full((w << nv,), POISON - (1 << 64), dtype=torch.int64, device="cuda")
    empty = torch.empty(0, dtype=torch.int64, device="cuda")
    dc = dev(torch, coeffs_for(name, k, "R1CS"))
    for mode in MODES:
        # e is in both terms of R1CS; REPEAT: f1 is in the first two terms, f3 in the third
        assert not host(vp_dev(torch, ring, [empty, poison, poison, poison], VP.R1CS, dc, nv, mode)).any(), (name, mode)
        assert not host(vp_dev(torch, ring, [poison, empty, poison, empty], VP.REPEAT, None, nv, mode)).any(), (name, mode)


# ---- 8. lazy sums -----------------------------------------------------------------------------------------------------------------------
LAZY = [("goldilocks", 1), ("babybear", 1), ("goldilocks24", 0), ("babybear72", 0), ("frog16", 0)]


@pytest.mark.parametrize("name,k", LAZY, ids=[c[0] for c in LAZY])
def test_all_p_minus_one_inputs_pass_two_lazy_reduction_intervals(torch_cuda, name, k):
    """csrc/sumcheck_vpoly.hpp reduces its lazy sums before they would hold more than kFlush = 64 products, and a pair adds one per
    term.  A plan has at most 1024 records of 256 lanes, i.e. 2^18 / units lane-groups, so 17 * 2^18 / units pairs give every lane 17
    of them: with the 8 terms of MIXED 136 products, two intervals and one pair more.  One table in all 8 slots (at most 612 MiB, for
    babybear72).  Every table word and every coefficient word is p - 1, the largest canonical image; lo == hi, so p(t) = pairs * g(e)
    at every t, which the model computes from one pair."""
    torch = torch_cuda
    m, ring = model_for(name, k), ring_for(name, k)
    w = ring.words_per_elem
    terms = VP.MIXED
    units = {"goldilocks": 1, "babybear": 1, "goldilocks24": 8, "babybear72": 8, "frog16": 4}[name]
    pairs = 17 * (1 << 18) // units
    nv = (2 * pairs - 1).bit_length()
    assert ring.vpoly_round_plan(nv, 8, 8, 4, LEADING)[0] == 1024 * 5
    top = m.p - 1 if m.p - 1 < 1 << 63 else m.p - 1 - (1 << 64)  # the word p - 1 as torch's signed 64-bit integer
    table = torch.full((2 * pairs * w,), top, dtype=torch.int64, device="cuda")
    dc = torch.full((8 * w,), top, dtype=torch.int64, device="cuda")
    e = m.elems(np.full(w, m.p - 1, dtype=np.uint64))[0]
    g = VP.evaluate([e] * 8, terms, [e] * 8, m.zero(), m.add, m.mul)
    for mode, count, copies in ((LEADING, pairs, 5), (ROUND_SUM, 2 * pairs, 1)):
        if m.pow2:
            want = m.words([(g * count) % m.p])
        else:
            want = ((g.astype(object) * count) % m.p).astype(np.uint64)
        got = host(vp_dev(torch, ring, [table] * 8, terms, dc, nv, mode))
        assert np.array_equal(got, np.tile(want, copies)), (name, mode)
    del table
    torch.cuda.empty_cache()


# ---- 9. alignment -----------------------------------------------------------------------------------------------------------------------
def shifted(torch, t):
    buf = torch.empty(t.numel() + 1, dtype=torch.int64, device="cuda")
    buf[1:] = t
    assert buf[1:].data_ptr() % 16 == 8
    return buf[1:]


# The last two plan two records and sit on the boundaries of the launch geometry (test_sumcheck_gpu.py: OFF_BY_EIGHT).
@pytest.mark.parametrize("name,k,nv", [("goldilocks", 6, 10), ("babybear", 5, 9), ("goldilocks", 8, 7), ("babybear", 9, 6)])
def test_buffers_off_by_eight_bytes_take_the_one_coefficient_path_to_the_same_result(torch_cuda, name, k, nv):
    torch = torch_cuda
    ring = ring_for(name, k)
    dt, terms, dc, _, _ = setup(torch, name, k, nv, "R1CS")
    st, sc = [shifted(torch, t) for t in dt], shifted(torch, dc)
    for mode in MODES:
        a = vp_dev(torch, ring, dt, terms, dc, nv, mode)
        assert torch.equal(vp_dev(torch, ring, st, terms, sc, nv, mode), a), (name, mode)
        assert torch.equal(vp_dev(torch, ring, dt, terms, sc, nv, mode), a), (name, mode)           # the coefficients alone
        assert torch.equal(vp_dev(torch, ring, [dt[0], st[1], dt[2], dt[3]], terms, dc, nv, mode), a), (name, mode)  # one table alone


# ---- 10. a whole sum-check ----------------------------------------------------------------------------------------------------------------
def _interp(m, msg_words, r_words, d):
    """p(r) from the d + 1 message elements, slot by slot on standard-form integers (power-of-two rings)"""
    vals = m.elems(msg_words)
    r = m.elems(r_words)[0]
    deg = m.ring.degree
    return np.array([SC.lagrange_at([int(vals[t][c]) for t in range(d + 1)], int(r[c]), m.p) for c in range(deg)], dtype=object)


def _fold_all(torch, ring, tabs, left, r_t, order):
    w = ring.words_per_elem
    folded = []
    for f in tabs:
        o = torch.empty(w << (left - 1), dtype=torch.int64, device="cuda")
        work_elems, _ = ring.mle_plan(left, 1, order)
        ring.mle_fix_variables_dev(o, f, left, r_t, order, torch.empty(work_elems * w, dtype=torch.int64, device="cuda") if work_elems else None)
        folded.append(o)
    return folded


@pytest.mark.parametrize("name,k,nv", [("goldilocks", 4, 6), ("stark", 2, 5)])
@pytest.mark.parametrize("order", [LEADING, TRAILING])
def test_a_whole_sum_check_of_r1cs(torch_cuda, name, k, nv, order):
    torch = torch_cuda
    m, ring = model_for(name, k), ring_for(name, k)
    terms = VP.R1CS
    tabs = [dev(torch, m.uniform(0xABD0 + j, 1 << nv)) for j in range(4)]
    cw = coeffs_for(name, k, "R1CS")
    dc, ce = dev(torch, cw), m.elems(cw)
    claim = m.elems(host(vp_dev(torch, ring, tabs, terms, dc, nv, ROUND_SUM)))[0]
    rng = random.Random("vpoly %s %d" % (name, order))
    for rnd in range(nv):
        left = nv - rnd
        msg = host(vp_dev(torch, ring, tabs, terms, dc, left, order))
        p = m.elems(msg)
        assert np.array_equal(m.add(p[0], p[1]), claim), (name, rnd)
        r_words = m.words([np.array([rng.randrange(m.p) for _ in range(ring.degree)], dtype=object)])
        claim = _interp(m, msg, r_words, 3)
        tabs = _fold_all(torch, ring, tabs, left, dev(torch, r_words), order)
    # the folded tables are the values of e, a, b, c at the challenge point: the final claim is g there
    values = [m.elems(host(f))[0] for f in tabs]
    assert np.array_equal(VP.evaluate(values, terms, ce, m.zero(), m.add, m.mul), claim)


@pytest.mark.parametrize("name,nv", [("goldilocks24", 5), ("babybear72", 4), ("frog16", 5)])
def test_the_round_loop_of_r1cs_on_the_reference_rings(torch_cuda, name, nv):
    """no interpolation on extension-field slots here: p(0) + p(1) is the plain sum over the tables as they stand in every round"""
    torch = torch_cuda
    m, ring = model_for(name, 0), ring_for(name, 0)
    tabs = [dev(torch, m.uniform(0xDEE0 + j, 1 << nv)) for j in range(4)]
    dc = dev(torch, coeffs_for(name, 0, "R1CS"))
    for rnd in range(nv):
        left = nv - rnd
        msg = m.elems(host(vp_dev(torch, ring, tabs, VP.R1CS, dc, left, LEADING)))
        total = m.elems(host(vp_dev(torch, ring, tabs, VP.R1CS, dc, left, ROUND_SUM)))[0]
        assert np.array_equal(m.add(msg[0], msg[1]), total), (name, rnd)
        tabs = _fold_all(torch, ring, tabs, left, dev(torch, m.uniform(0x7100 + rnd, 1)), LEADING)


# ---- 11. capture ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k,nv", [("goldilocks", 6, 10), ("stark", 4, 10), ("babybear72", 0, 11)])
def test_capture_on_a_fresh_context_and_replay_after_tables_and_coefficients_change(torch_cuda, name, k, nv):
    torch = torch_cuda
    from stark_rings_amd import CyclotomicRing

    m = model_for(name, k)
    ring = CyclotomicRing(name, k, device=0)  # fresh: nothing has run on it, so nothing is warm
    try:
        w = ring.words_per_elem
        terms, mode = VP.R1CS, TRAILING
        first, c_first = tables_for(name, k, nv)[:4], coeffs_for(name, k, "R1CS")
        second = [m.uniform(0x9910 + j, 1 << nv) for j in range(4)]
        c_second = m.uniform(0x9920, 2)
        tabs, dc = [dev(torch, t) for t in first], dev(torch, c_first)
        out = torch.empty(4 * w, dtype=torch.int64, device="cuda")
        work_elems, launches = ring.vpoly_round_plan(nv, 4, 2, 3, mode)
        assert work_elems and launches >= 2
        work = torch.full((work_elems * w,), POISON - (1 << 64), dtype=torch.int64, device="cuda")
        side = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            ring.vpoly_round_evals_dev(out, tabs, terms, dc, nv, mode, work, stream=side)
        graph.replay()
        torch.cuda.synchronize()
        assert agrees(m, host(out), [m.elems(t) for t in first], terms, m.elems(c_first), nv, mode)
        for t, new in zip(tabs, second):
            t.copy_(dev(torch, new))
        dc.copy_(dev(torch, c_second))
        work.fill_(0x1111111111111111)
        graph.replay()
        torch.cuda.synchronize()
        assert agrees(m, host(out), [m.elems(t) for t in second], terms, m.elems(c_second), nv, mode)
    finally:
        ring.close()


def test_workspace_contents_do_not_matter(torch_cuda):
    torch = torch_cuda
    for name, k, nv in (("goldilocks", 6, 10), ("frog16", 0, 12)):
        ring = ring_for(name, k)
        dt, terms, dc, _, _ = setup(torch, name, k, nv, "REPEAT")
        a = vp_dev(torch, ring, dt, terms, dc, nv, LEADING, work_fill=0)
        b = vp_dev(torch, ring, dt, terms, dc, nv, LEADING, work_fill=POISON - (1 << 64))
        assert torch.equal(a, b)


# ---- 12. the class ----------------------------------------------------------------------------------------------------------------------
def test_the_virtual_polynomial_class(torch_cuda):
    torch = torch_cuda
    from stark_rings_amd import DenseMultilinearExtension as MLE, MLE_TRAILING, RingError, VirtualPolynomial

    for name, k, nv in (("goldilocks", 6, 10), ("stark", 4, 10), ("goldilocks24", 0, 11)):
        m, ring = model_for(name, k), ring_for(name, k)
        w, full = ring.words_per_elem, 1 << nv
        words = [t[:n * w] for t, n in zip(tables_for(name, k, nv), (full, full - 5, full // 2 + 1, full))]
        els = [m.elems(t) for t in words]
        e, a, b, c = [MLE(ring, nv, dev(torch, t)) for t in words]
        cw = coeffs_for(name, k, "R1CS")
        ce = m.elems(cw)
        # eq (c0 a b - c) built as HyperPlonk builds it: the products first, then eq on every term
        vp = VirtualPolynomial(ring, nv)
        vp.add_mle_list([a, b], dev(torch, cw[:w]))
        vp.add_mle_list([c], dev(torch, cw[w:]))
        assert (len(vp.tables), vp.degree) == (3, 2)
        vp.mul_by_mle(e)
        assert (len(vp.tables), vp.degree, vp.terms) == (4, 3, [[0, 1, 3], [2, 3]])  # a, b, c, e: one slot each, e shared
        slots = [els[1], els[2], els[3], els[0]]
        assert agrees(m, host(vp.round_evals()), slots, vp.terms, ce, nv, LEADING)
        assert agrees(m, host(vp.round_evals(order=MLE_TRAILING)), slots, vp.terms, ce, nv, TRAILING)
        assert agrees(m, host(vp.sum()), slots, vp.terms, ce, nv, ROUND_SUM)
        # a coefficient of None among given ones is one(); the same tensor in another MLE object is the same slot
        vq = VirtualPolynomial(ring, nv)
        vq.add_mle_list([e, a, a], None)
        vq.add_mle_list([MLE(ring, nv, a.evaluations), b], dev(torch, cw[:w]))
        assert len(vq.tables) == 3 and vq.terms == [[0, 1, 1], [1, 2]]
        assert agrees(m, host(vq.round_evals()), [els[0], els[1], els[2]], vq.terms, [one_of(m), ce[0]], nv, LEADING)
        # the host-pointer form stages the same tables
        got = ring.vpoly_round_evals(words, VP.R1CS, cw, nv, TRAILING)
        assert agrees(m, got, els, VP.R1CS, ce, nv, TRAILING)
        assert np.array_equal(ring.vpoly_round_evals(words[:3], VP.SINGLE, None, nv, LEADING), ring.mle_round_evals(words[:3], nv, LEADING))
        # the limits
        many = [MLE(ring, nv, dev(torch, words[0])) for _ in range(9)]
        v8 = VirtualPolynomial(ring, nv)
        for j in range(4):
            v8.add_mle_list(many[2 * j:2 * j + 2])
        with pytest.raises(RingError, match="distinct tables"):
            v8.add_mle_list([many[8]])
        assert len(v8.tables) == 8 and len(v8.terms) == 4  # a refused call leaves the polynomial as it was
        for j in range(4):
            v8.add_mle_list([many[j]])
        with pytest.raises(RingError, match="products"):
            v8.add_mle_list([many[0]])
        with pytest.raises(RingError, match="factors"):
            VirtualPolynomial(ring, nv).add_mle_list([e] * 5)
        v4 = VirtualPolynomial(ring, nv).add_mle_list([e, a, b, c])
        with pytest.raises(RingError, match="factors"):
            v4.mul_by_mle(e)
        with pytest.raises(RingError, match="num_vars"):
            VirtualPolynomial(ring, nv).add_mle_list([e, MLE(ring, nv - 1, dev(torch, words[0][:w << (nv - 1)]))])


# ---- 13. refusals -----------------------------------------------------------------------------------------------------------------------
def test_every_refusal_names_its_reason_and_launches_nothing(torch_cuda):
    torch = torch_cuda
    from stark_rings_amd import _lib

    ring = ring_for("goldilocks", 6)
    lib, ctx = ring._lib, ring._ctx
    nv, w = 10, ring.words_per_elem
    canary = 0x0123456789ABCDEF
    f = torch.full((w << nv,), 7, dtype=torch.int64, device="cuda")
    coef = torch.full((2 * w,), 9, dtype=torch.int64, device="cuda")
    out = torch.full((4 * w,), canary, dtype=torch.int64, device="cuda")
    need, _ = ring.vpoly_round_plan(nv, 4, 2, 3, LEADING)
    assert need
    work = torch.full((need * w,), canary, dtype=torch.int64, device="cuda")
    arena = torch.full(((need + 2) * w,), canary, dtype=torch.int64, device="cuda")  # a workspace and coefficients that overlap
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    fp, op, wp, cp, full = f.data_ptr(), out.data_ptr(), work.data_ptr(), coef.data_ptr(), 1 << nv
    good = dict(out=op, ptrs=[fp] * 4, sizes=[full] * 4, nt=4, terms=VP.R1CS, n_terms=2, coef=cp, nv=nv, mode=LEADING, work=wp, need=need)

    def call(**change):
        a = dict(good, **change)
        pa = (ctypes.c_void_p * 8)(*a["ptrs"]) if a["ptrs"] is not None else None
        sa = (ctypes.c_size_t * 8)(*a["sizes"]) if a["sizes"] is not None else None
        ta = None
        if a["terms"] is not None:
            ta = (_lib.VPolyTerm * 9)()
            for i, t in enumerate(a["terms"]):
                ta[i].n_factors = t[0] if isinstance(t, tuple) else len(t)  # (n_factors, indices): a count that is not the length
                for s, j in enumerate((t[1] if isinstance(t, tuple) else t)[:4]):
                    ta[i].table[s] = j
        rc = lib.sr_vpoly_round_evals_dev(ctx, a["out"], pa, sa, a["nt"], ta, a["n_terms"], a["coef"], a["nv"], a["mode"], a["work"], a["need"], st)
        return rc, _lib.last_error()

    bad = [
        (dict(out=None), "null pointer"),
        (dict(ptrs=None), "null pointer"),
        (dict(sizes=None), "null pointer"),
        (dict(terms=None), "null pointer"),
        (dict(ptrs=[fp, None, fp, fp]), "null pointer"),
        (dict(work=None), "null pointer"),
        (dict(nt=0), "n_tables must be 1 .. 8"),
        (dict(nt=9), "n_tables must be 1 .. 8"),
        (dict(n_terms=0), "n_terms must be 1 .. 8"),
        (dict(n_terms=9, terms=[[0, 1, 2], [0, 3]] + [[0]] * 7), "n_terms must be 1 .. 8"),
        (dict(terms=[[0, 1, 2], (0, [0, 3])]), "n_factors must be 1 .. 4"),
        (dict(terms=[[0, 1, 2], (5, [0, 3, 0, 0])]), "n_factors must be 1 .. 4"),
        (dict(terms=[[0, 1, 2], [0, 4]]), "table index outside"),
        (dict(terms=[[0, 1, 2], [0, -1]]), "table index outside"),
        (dict(terms=[[0, 1, 2], [0, 1]]), "a table that no term uses"),
        (dict(mode=3), "unknown mode"),
        (dict(nv=48), "num_vars must be below 48"),
        (dict(nv=0, sizes=[1] * 4, mode=TRAILING), "num_vars >= 1"),
        (dict(sizes=[full, full, full + 1, full]), "n_evals exceeds 2^num_vars"),
        (dict(nv=47, sizes=[1 << 45] * 4), "element count too large"),
        (dict(need=need - 1), "workspace too small"),
        (dict(out=fp + 8 * w), "d_out overlaps a table"),
        (dict(work=fp), "d_work overlaps a table"),
        (dict(coef=fp + 8 * w), "d_coeffs overlaps a table"),
        (dict(out=wp + 8 * w), "d_out overlaps d_work"),
        (dict(out=cp + 8 * w), "d_out overlaps d_coeffs"),
        (dict(work=arena.data_ptr(), coef=arena.data_ptr() + 8 * w * (need - 1)), "d_work overlaps d_coeffs"),
    ]
    for change, msg in bad:
        rc, err = call(**change)
        assert rc == 1 and msg in err, (change, rc, err)
    # the plan refuses a degree that is not the largest n_factors of the call it is asked about
    assert lib.sr_vpoly_round_plan(ring.ring, 6, nv, 4, 2, 5, LEADING, ctypes.byref(ctypes.c_size_t()), ctypes.byref(ctypes.c_int())) == 1
    assert "degree" in _lib.last_error()
    torch.cuda.synchronize()
    assert bool((out == canary).all()) and bool((work == canary).all()) and bool((arena == canary).all())
    assert bool((f == 7).all()) and bool((coef == 9).all())
    rc, err = call()
    assert rc == 0, err
    torch.cuda.synchronize()
    assert not bool((out == canary).any())
