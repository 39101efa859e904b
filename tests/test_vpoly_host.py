"""CPU checks of the sum-of-products round entry points (include/stark_rings_hip.h: sr_vpoly_round_plan, sr_vpoly_round_evals[_dev]):
the exports, the plan arithmetic for every ring, the refusals that need no context (the others need one and live in
tests/test_vpoly_gpu.py), and the pure-Python restatement (tools/model_vpoly.py, the oracle of the GPU tests) against the sum-check
identities, against tools/model_sumcheck.py and against the pinned vectors of tests/golden/vpoly_kats.json."""
import ctypes
import json
import os
import random
import re
import sys

import numpy as np
import pytest

from stark_rings_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import model_mle as M  # noqa: E402
import model_sumcheck as SC  # noqa: E402
import model_vpoly as VP  # noqa: E402

NEW = ("sr_vpoly_round_plan", "sr_vpoly_round_evals_dev", "sr_vpoly_round_evals")
LEADING, TRAILING, ROUND_SUM = 0, 1, 2
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "vpoly_kats.json")))
STRUCTURES = {"SINGLE": VP.SINGLE, "R1CS": VP.R1CS, "REPEAT": VP.REPEAT, "MIXED": VP.MIXED, "CANCEL": VP.CANCEL}


def _header():
    return open(os.path.join(ROOT, "include", "stark_rings_hip.h")).read()


def test_header_library_and_ctypes_table_carry_the_new_names():
    lib = _lib.load()
    header = _header()
    declared = set(re.findall(r"\b(sr_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared, "%s is not declared in the header" % name
        assert name in _lib.SYMBOLS, "%s is missing from _lib.SYMBOLS" % name
        assert hasattr(lib, name), "the library does not export %s" % name
    for macro, value in (("SR_VPOLY_MAX_TABLES", 8), ("SR_VPOLY_MAX_TERMS", 8), ("SR_VPOLY_MAX_FACTORS", 4)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), header), macro
    assert (_lib.VPOLY_MAX_TABLES, _lib.VPOLY_MAX_TERMS, _lib.VPOLY_MAX_FACTORS) == (8, 8, 4)
    assert ctypes.sizeof(_lib.VPolyTerm) == 5 * ctypes.sizeof(ctypes.c_int)  # { int n_factors; int table[4]; }
    import stark_rings_amd

    assert stark_rings_amd.VirtualPolynomial.MAX_TABLES == 8


def test_the_structures_of_the_tests_are_what_the_issue_lists():
    assert [len(t) for t in VP.MIXED] == [1, 2, 3, 4, 4, 3, 2, 1]
    assert {j for t in VP.MIXED for j in t} == set(range(8))
    assert max(sum(j in t for t in VP.MIXED) for j in range(8)) >= 4
    assert (VP.degree(VP.SINGLE), VP.n_tables(VP.SINGLE)) == (3, 3)
    assert (VP.degree(VP.R1CS), VP.n_tables(VP.R1CS)) == (3, 4)
    assert (VP.degree(VP.REPEAT), VP.n_tables(VP.REPEAT)) == (4, 4)
    assert (VP.degree(VP.MIXED), VP.n_tables(VP.MIXED)) == (4, 8)


def _plan(ring, k, nv, nt, terms, degree, mode):
    lib = _lib.load()
    work, launches = ctypes.c_size_t(1 << 60), ctypes.c_int(-1)
    rc = lib.sr_vpoly_round_plan(ring, k, nv, nt, terms, degree, mode, ctypes.byref(work), ctypes.byref(launches))
    return rc, work.value, launches.value


@pytest.mark.parametrize("ring,k", [(0, 0), (0, 6), (0, 10), (0, 16), (1, 5), (1, 16), (2, 4), (2, 12), (3, 0), (4, 0), (5, 0)])
def test_plan_bounds_for_every_ring_mode_table_count_term_count_and_degree(ring, k):
    lib = _lib.load()
    max_groups = int(re.search(r"#define\s+SR_MLE_ROUND_MAX_GROUPS\s+(\d+)", _header()).group(1))
    split = single = 0
    for mode in (LEADING, TRAILING, ROUND_SUM):
        for nv in range(25):
            for nt in range(1, 9):
                for degree in (1, 2, 3, 4):
                    answers = {_plan(ring, k, nv, nt, n_terms, degree, mode) for n_terms in (1, 2, 5, 8)}
                    assert len(answers) == 1  # the term count is checked, it does not move the plan
                    rc, work, launches = answers.pop()
                    where = "ring %d k %d nv %d tables %d degree %d mode %d: work %d launches %d" % (ring, k, nv, nt, degree, mode, work, launches)
                    if nv == 0 and mode != ROUND_SUM:
                        assert rc == 1 and "num_vars >= 1" in _lib.last_error(), where
                        continue
                    assert rc == 0, where
                    assert launches >= 1, where
                    assert (work == 0) == (launches == 1), where
                    assert work <= max_groups * (degree + 1), where
                    if mode == ROUND_SUM:
                        assert launches <= 2 and work <= max_groups, where
                    else:
                        assert work % (degree + 1) == 0, where
                        # the records are those of sr_mle_round_plan: same fill target, cap and minimum of pairs per lane
                        w1, l1 = ctypes.c_size_t(), ctypes.c_int()
                        assert lib.sr_mle_round_plan(ring, k, nv, 1, mode, ctypes.byref(w1), ctypes.byref(l1)) == 0
                        assert work // (degree + 1) in (w1.value // 2, max(w1.value // 2, 2)), where
                    if ring <= 1:  # the one-limb fields take all d + 1 points at once: every table is read exactly once per call
                        assert launches <= 2, where
                    split += work > 0
                    single += work == 0
    assert split and single


def test_plan_depends_on_the_shape_only_and_needs_no_device():
    """pure host arithmetic: the same answer every time, with no context anywhere in sight"""
    assert _plan(0, 10, 20, 4, 2, 3, LEADING) == _plan(0, 10, 20, 4, 2, 3, LEADING)
    assert _plan(0, 10, 20, 4, 2, 3, LEADING) == _plan(0, 10, 20, 4, 2, 3, TRAILING)
    rc, work, launches = _plan(0, 10, 20, 4, 2, 3, LEADING)
    assert (rc, launches) == (0, 2) and work % 4 == 0 and work > 0
    assert _plan(0, 16, 4, 4, 2, 3, LEADING) == (0, 0, 1)


def test_plan_refuses_bad_arguments_and_names_the_reason():
    lib = _lib.load()
    work, launches = ctypes.c_size_t(), ctypes.c_int()
    for args, msg in (((0, 10, 4, 0, 2, 3, LEADING), "n_tables must be 1 .. 8"), ((0, 10, 4, 9, 2, 3, LEADING), "n_tables must be 1 .. 8"),
                      ((0, 10, 4, 4, 0, 3, LEADING), "n_terms must be 1 .. 8"), ((0, 10, 4, 4, 9, 3, LEADING), "n_terms must be 1 .. 8"),
                      ((0, 10, 4, 4, 2, 0, LEADING), "degree"), ((0, 10, 4, 4, 2, 5, LEADING), "degree"),
                      ((0, 10, 4, 4, 2, 3, 3), "unknown mode"), ((0, 10, 4, 4, 2, 3, -1), "unknown mode"),
                      ((0, 10, 48, 4, 2, 3, LEADING), "num_vars must be below 48"), ((0, 10, 0, 4, 2, 3, LEADING), "num_vars >= 1"),
                      ((0, 10, 0, 4, 2, 3, TRAILING), "num_vars >= 1"), ((6, 0, 4, 4, 2, 3, LEADING), "unknown ring"),
                      ((0, 25, 4, 4, 2, 3, LEADING), "log2_degree")):
        assert lib.sr_vpoly_round_plan(*args, ctypes.byref(work), ctypes.byref(launches)) == 1, args
        assert msg in _lib.last_error(), (args, _lib.last_error())
    assert lib.sr_vpoly_round_plan(0, 10, 4, 4, 2, 3, LEADING, None, ctypes.byref(launches)) == 1 and "null" in _lib.last_error()
    assert lib.sr_vpoly_round_plan(0, 10, 4, 4, 2, 3, LEADING, ctypes.byref(work), None) == 1 and "null" in _lib.last_error()
    assert lib.sr_vpoly_round_plan(0, 10, 0, 4, 2, 3, ROUND_SUM, ctypes.byref(work), ctypes.byref(launches)) == 0


def test_entry_points_refuse_a_null_context_before_anything_else():
    lib = _lib.load()
    buf = np.zeros(16, dtype=np.uint64)
    # every other argument is bad as well: the context is looked at first
    assert lib.sr_vpoly_round_evals(None, None, None, None, 99, None, 99, None, 99, 7) == 1 and "null context" in _lib.last_error()
    assert lib.sr_vpoly_round_evals_dev(None, None, None, None, 99, None, 99, None, 99, 7, None, 0, None) == 1
    assert "null context" in _lib.last_error()
    ptrs, sizes = (ctypes.c_void_p * 1)(buf.ctypes.data), (ctypes.c_size_t * 1)(1)
    term = (_lib.VPolyTerm * 1)()
    term[0].n_factors = 1
    assert lib.sr_vpoly_round_evals(None, buf.ctypes.data_as(_lib.u64p), ptrs, sizes, 1, term, 1, None, 1, LEADING) == 1
    assert "null context" in _lib.last_error()


# ---- the restatement the GPU tests use as their oracle, pinned by the sum-check identities on Python integers -------------------------
def _int_ops(p):
    return (lambda a, b: (a + b) % p), (lambda a, b: (a - b) % p), (lambda r, a: r * a % p)


def _random_tables(rng, p, terms, nv):
    full = 1 << nv
    return [[rng.choice((0, 1, p - 1, rng.randrange(p))) for _ in range(rng.choice((full, full, full - 1, 1)))] for _ in range(VP.n_tables(terms))]


@pytest.mark.parametrize("field", ["goldilocks", "babybear", "stark"])
@pytest.mark.parametrize("structure", sorted(STRUCTURES))
def test_model_round_messages_satisfy_the_sum_check_identities(field, structure):
    p = SC.PRIMES[field]
    terms = STRUCTURES[structure]
    d = VP.degree(terms)
    add, sub, mul = _int_ops(p)
    rng = random.Random("%s %s" % (field, structure))
    for nv in (1, 2, 4):
        tables = _random_tables(rng, p, terms, nv)
        padded = [M.pad(f, nv, 0) for f in tables]
        for coeffs in (None, [rng.choice((0, 1, p - 1, rng.randrange(p))) for _ in terms]):
            if structure == "CANCEL" and coeffs is not None:
                coeffs[1] = (p - coeffs[0]) % p
            claim = VP.poly_sum(tables, terms, coeffs, nv, 0, add, mul)
            for order in (LEADING, TRAILING):
                msg = VP.round_evals(tables, terms, coeffs, nv, order, 0, 1, add, sub, mul)
                assert len(msg) == d + 1
                assert (msg[0] + msg[1]) % p == claim
                r = rng.randrange(p)
                folded = [M.fold(f, nv, [r], order, add, sub, mul) for f in padded]
                assert SC.lagrange_at(msg, r, p) == VP.poly_sum(folded, terms, coeffs, nv - 1, 0, add, mul)
                if structure == "CANCEL" and coeffs is not None:
                    assert msg == [0] * (d + 1)


@pytest.mark.parametrize("field", ["goldilocks", "babybear", "stark"])
def test_model_messages_are_linear_in_the_coefficients(field):
    p = SC.PRIMES[field]
    add, sub, mul = _int_ops(p)
    rng = random.Random("linear " + field)
    for terms in (VP.R1CS, VP.REPEAT, VP.MIXED):
        nv = 3
        tables = _random_tables(rng, p, terms, nv)
        a = [rng.randrange(p) for _ in terms]
        b = [rng.randrange(p) for _ in terms]
        lam = rng.randrange(p)
        both = [(x + lam * y) % p for x, y in zip(a, b)]
        for order in (LEADING, TRAILING):
            ma, mb, mab = (VP.round_evals(tables, terms, c, nv, order, 0, 1, add, sub, mul) for c in (a, b, both))
            assert mab == [(x + lam * y) % p for x, y in zip(ma, mb)]
        # no coefficients means one() everywhere
        ones = VP.round_evals(tables, terms, [1] * len(terms), nv, LEADING, 0, 1, add, sub, mul)
        assert ones == VP.round_evals(tables, terms, None, nv, LEADING, 0, 1, add, sub, mul)


@pytest.mark.parametrize("field", ["goldilocks", "babybear", "stark"])
@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_model_with_one_term_and_unit_coefficient_is_the_product_model(field, d):
    p = SC.PRIMES[field]
    add, sub, mul = _int_ops(p)
    rng = random.Random("%s single %d" % (field, d))
    terms = [list(range(d))]
    for nv in (1, 3):
        tables = _random_tables(rng, p, terms, nv)
        for order in (LEADING, TRAILING):
            want = SC.round_evals(tables, nv, order, 0, 1, add, sub, mul)
            assert VP.round_evals(tables, terms, None, nv, order, 0, 1, add, sub, mul) == want
            assert VP.round_evals(tables, terms, [1], nv, order, 0, 1, add, sub, mul) == want
        assert VP.poly_sum(tables, terms, None, nv, 0, add, mul) == SC.product_sum([M.pad(f, nv, 0) for f in tables], 0, add, mul)


def test_model_p0_plus_p1_is_the_sum_on_slot_products_too():
    """the identity that needs no interpolation, on a ring whose product is not slot-wise: Z_p[X] / (X^2 - 3)"""
    p = 97
    add = lambda a, b: ((a[0] + b[0]) % p, (a[1] + b[1]) % p)  # noqa: E731
    sub = lambda a, b: ((a[0] - b[0]) % p, (a[1] - b[1]) % p)  # noqa: E731
    mul = lambda r, a: ((r[0] * a[0] + 3 * r[1] * a[1]) % p, (r[0] * a[1] + r[1] * a[0]) % p)  # noqa: E731
    rng = random.Random(5)
    for terms in (VP.R1CS, VP.REPEAT, VP.MIXED):
        tables = [[(rng.randrange(p), rng.randrange(p)) for _ in range(8)] for _ in range(VP.n_tables(terms))]
        coeffs = [(rng.randrange(p), rng.randrange(p)) for _ in terms]
        claim = VP.poly_sum(tables, terms, coeffs, 3, (0, 0), add, mul)
        for order in (LEADING, TRAILING):
            msg = VP.round_evals(tables, terms, coeffs, 3, order, (0, 0), (1, 0), add, sub, mul)
            assert add(msg[0], msg[1]) == claim


def test_model_reproduces_the_pinned_vectors():
    assert KATS == VP.make_kats(), "tests/golden/vpoly_kats.json is not what tools/model_vpoly.py writes"
    seen = set()
    for case in KATS["cases"]:
        p = SC.PRIMES[case["ring"]]
        add, sub, mul = SC.vec_ops(p)
        dr = 1 << case["log2_degree"]
        zero, one = (0,) * dr, (1,) * dr
        tables = [[tuple(e) for e in f] for f in case["tables"]]
        coeffs = [tuple(c) for c in case["coeffs"]]
        terms = case["terms"]
        assert terms == STRUCTURES[case["structure"]]
        assert [len(f) for f in tables] == case["n_evals"]
        nv = case["num_vars"]
        assert (dr, nv) == (2, 3)
        assert [list(e) for e in VP.round_evals(tables, terms, coeffs, nv, LEADING, zero, one, add, sub, mul)] == case["leading"]
        assert [list(e) for e in VP.round_evals(tables, terms, coeffs, nv, TRAILING, zero, one, add, sub, mul)] == case["trailing"]
        assert list(VP.poly_sum(tables, terms, coeffs, nv, zero, add, mul)) == case["sum"]
        seen.add((case["ring"], case["structure"], min(case["n_evals"]) < 1 << nv))
    assert seen == {(r, s, True) for r in ("goldilocks", "babybear", "stark") for s in ("R1CS", "REPEAT", "MIXED")}
