"""CPU checks of the fused fold-and-round entry points of a sum of products (include/stark_rings_hip.h: sr_vpoly_round_fold_plan,
sr_vpoly_round_fold_evals[_dev]): the exports, the plan arithmetic for every ring, the refusals that need no context (the others need
one and live in tests/test_vpoly_fold_gpu.py), and the pure-Python restatement (tools/model_vpoly_fold.py, the oracle of the GPU tests)
against model_mle.fold, model_vpoly.round_evals, model_sumcheck_fold.fold_round, the sum-check identities and the pinned vectors of
tests/golden/vpoly_fold_kats.json."""
import ctypes
import json
import os
import random
import re
import sys

import pytest

from stark_rings_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import model_mle as M  # noqa: E402
import model_sumcheck as SC  # noqa: E402
import model_sumcheck_fold as SF  # noqa: E402
import model_vpoly as VP  # noqa: E402
import model_vpoly_fold as VF  # noqa: E402

NEW = ("sr_vpoly_round_fold_plan", "sr_vpoly_round_fold_evals_dev", "sr_vpoly_round_fold_evals")
LEADING, TRAILING = 0, 1
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "vpoly_fold_kats.json")))
# points the fused launch takes over 4 / 8 table slots (csrc/sumcheck_vpoly_fold.hpp: fused_points_of) and points per launch of the
# round kernels that take the remaining ones (csrc/sumcheck_vpoly.hpp: points_of), per ring id
FUSED = {0: {4: 5, 8: 4}, 1: {4: 5, 8: 3}, 2: {4: 2, 8: 1}, 3: {4: 2, 8: 1}, 4: {4: 1, 8: 0}, 5: {4: 1, 8: 1}}
PER_LAUNCH = {0: {4: 5, 8: 5}, 1: {4: 5, 8: 5}, 2: {4: 2, 8: 1}, 3: {4: 2, 8: 1}, 4: {4: 1, 8: 1}, 5: {4: 1, 8: 1}}


def _header():
    return open(os.path.join(ROOT, "include", "stark_rings_hip.h")).read()


def test_header_library_and_ctypes_table_carry_the_new_names():
    lib = _lib.load()
    declared = set(re.findall(r"\b(sr_[a-z0-9_]+)\s*\(", _header()))
    for name in NEW:
        assert name in declared, "%s is not declared in the header" % name
        assert name in _lib.SYMBOLS, "%s is missing from _lib.SYMBOLS" % name
        assert hasattr(lib, name), "the library does not export %s" % name


def _plan(ring, k, nv, nt, n_terms, degree, order):
    lib = _lib.load()
    work, launches = ctypes.c_size_t(1 << 60), ctypes.c_int(-1)
    rc = lib.sr_vpoly_round_fold_plan(ring, k, nv, nt, n_terms, degree, order, ctypes.byref(work), ctypes.byref(launches))
    return rc, work.value, launches.value


@pytest.mark.parametrize("ring,k", [(0, 0), (0, 6), (0, 10), (0, 16), (1, 5), (1, 16), (2, 4), (2, 12), (3, 0), (4, 0), (5, 0)])
def test_plan_bounds_for_every_ring_size_table_count_degree_and_order(ring, k):
    max_groups = int(re.search(r"#define\s+SR_MLE_ROUND_MAX_GROUPS\s+(\d+)", _header()).group(1))
    split = single = 0
    for order in (LEADING, TRAILING):
        for nv in range(2, 25):
            for nt in (4, 8):
                for degree in (1, 2, 3, 4):
                    rc, work, launches = _plan(ring, k, nv, nt, 3, degree, order)
                    where = "ring %d k %d nv %d tables %d degree %d order %d: work %d launches %d" % (ring, k, nv, nt, degree, order, work, launches)
                    assert rc == 0, where
                    assert launches >= 1, where
                    assert (work == 0) == (launches == 1), where
                    assert work <= max_groups * (degree + 1), where
                    assert work % (degree + 1) == 0, where
                    fused, per = min(FUSED[ring][nt], degree + 1), min(PER_LAUNCH[ring][nt], degree + 1)
                    rest = -(-(degree + 1 - fused) // per)  # launches of the remaining points
                    assert launches in (1 + rest, 2 + rest), where
                    if rest:
                        assert work > 0, where  # several launches meet in the workspace
                    # the records are those of the sum-of-products round in num_vars - 1 variables
                    rwork, rlaunches = ctypes.c_size_t(), ctypes.c_int()
                    assert _lib.load().sr_vpoly_round_plan(ring, k, nv - 1, nt, 3, degree, order, ctypes.byref(rwork), ctypes.byref(rlaunches)) == 0
                    assert work == rwork.value or (rest and rwork.value == 0 and work == 2 * (degree + 1)), where
                    split += work > 0
                    single += work == 0
    assert split and (single or ring >= 4)  # babybear72 and frog16 fuse one point at most: their plans always split


def test_plan_depends_on_the_shape_only_and_needs_no_device():
    assert _plan(0, 10, 20, 4, 2, 3, LEADING) == _plan(0, 10, 20, 4, 2, 3, LEADING)
    assert _plan(0, 10, 20, 4, 2, 3, LEADING) == _plan(0, 10, 20, 4, 8, 3, TRAILING)
    rc, work, launches = _plan(0, 10, 20, 4, 2, 3, LEADING)
    assert (rc, launches) == (0, 2) and work % 4 == 0 and work > 0
    assert _plan(0, 16, 4, 4, 2, 3, LEADING) == (0, 0, 1)
    # Goldilocks over 8 slots: four points fused, the fifth from the round kernel, then the sum over the records
    assert _plan(0, 16, 4, 8, 2, 4, LEADING)[2] == 3 and _plan(0, 16, 4, 8, 2, 3, LEADING) == (0, 0, 1)


def test_plan_refuses_bad_arguments_and_names_the_reason():
    lib = _lib.load()
    work, launches = ctypes.c_size_t(), ctypes.c_int()
    for args, msg in (((0, 10, 0, 2, 2, 3, LEADING), "num_vars >= 2"), ((0, 10, 1, 2, 2, 3, TRAILING), "num_vars >= 2"),
                      ((0, 10, 48, 2, 2, 3, LEADING), "num_vars must be below 48"),
                      ((0, 10, 4, 0, 2, 3, LEADING), "n_tables must be 1 .. 8"), ((0, 10, 4, 9, 2, 3, LEADING), "n_tables must be 1 .. 8"),
                      ((0, 10, 4, 2, 0, 3, LEADING), "n_terms must be 1 .. 8"), ((0, 10, 4, 2, 9, 3, LEADING), "n_terms must be 1 .. 8"),
                      ((0, 10, 4, 2, 2, 0, LEADING), "degree"), ((0, 10, 4, 2, 2, 5, LEADING), "degree"),
                      ((0, 10, 4, 2, 2, 3, 2), "unknown order"), ((0, 10, 4, 2, 2, 3, -1), "unknown order"),
                      ((6, 0, 4, 2, 2, 3, LEADING), "unknown ring"), ((-1, 0, 4, 2, 2, 3, LEADING), "unknown ring"),
                      ((0, 25, 4, 2, 2, 3, LEADING), "log2_degree")):
        assert lib.sr_vpoly_round_fold_plan(*args, ctypes.byref(work), ctypes.byref(launches)) == 1, args
        assert msg in _lib.last_error(), (args, _lib.last_error())
        if "ring" not in msg and "log2" not in msg:
            assert _lib.last_error().startswith("vpoly_round_fold: "), _lib.last_error()
    assert lib.sr_vpoly_round_fold_plan(0, 10, 4, 2, 2, 3, LEADING, None, ctypes.byref(launches)) == 1 and "null" in _lib.last_error()
    assert lib.sr_vpoly_round_fold_plan(0, 10, 4, 2, 2, 3, LEADING, ctypes.byref(work), None) == 1 and "null" in _lib.last_error()
    for ring in range(6):
        assert lib.sr_vpoly_round_fold_plan(ring, 4 if ring < 3 else 0, 2, 4, 2, 3, LEADING, ctypes.byref(work), ctypes.byref(launches)) == 0
        assert lib.sr_vpoly_round_fold_plan(ring, 4 if ring < 3 else 0, 47, 4, 2, 3, LEADING, ctypes.byref(work), ctypes.byref(launches)) == 0
        assert lib.sr_vpoly_round_fold_plan(ring, 4 if ring < 3 else 0, 1, 4, 2, 3, LEADING, ctypes.byref(work), ctypes.byref(launches)) == 1
        assert lib.sr_vpoly_round_fold_plan(ring, 4 if ring < 3 else 0, 48, 4, 2, 3, LEADING, ctypes.byref(work), ctypes.byref(launches)) == 1


def test_entry_points_refuse_a_null_context_before_anything_else():
    lib = _lib.load()
    assert lib.sr_vpoly_round_fold_evals(None, None, None, None, None, None, 9, None, 9, None, 99, None, 7) == 1
    assert "null context" in _lib.last_error()
    assert lib.sr_vpoly_round_fold_evals_dev(None, None, None, None, None, None, 9, None, 9, None, 99, None, 7, None, 0, None) == 1
    assert "null context" in _lib.last_error()


# ---- the restatement the GPU tests use as their oracle ---------------------------------------------------------------------------------
def _int_ops(p):
    return (lambda a, b: (a + b) % p), (lambda a, b: (a - b) % p), (lambda r, a: r * a % p)


def test_model_reproduces_the_pinned_vectors():
    assert KATS == VF.make_kats(), "tests/golden/vpoly_fold_kats.json is not what tools/model_vpoly_fold.py writes"
    seen = set()
    for case in KATS["cases"]:
        p = SC.PRIMES[case["ring"]]
        add, sub, mul = SC.vec_ops(p)
        dr = 1 << case["log2_degree"]
        zero, one = (0,) * dr, (1,) * dr
        tables = [[tuple(e) for e in f] for f in case["tables"]]
        coeffs = [tuple(c) for c in case["coeffs"]]
        assert [len(f) for f in tables] == case["n_evals"]
        nv = case["num_vars"]
        for key, order in (("leading", LEADING), ("trailing", TRAILING)):
            folded, msg = VF.fold_round(tables, case["terms"], coeffs, nv, tuple(case["r"]), order, zero, one, add, sub, mul)
            assert [[list(e) for e in g] for g in folded] == case[key]["folded"]
            assert [list(e) for e in msg] == case[key]["message"]
            assert [len(g) for g in folded] == [VF.folded_len(n, nv, order) for n in case["n_evals"]]
        seen.add((case["ring"], case["structure"], min(case["n_evals"]) < 1 << nv))
    assert seen == {(r, s, True) for r in ("goldilocks", "babybear", "stark") for s in ("R1CS", "REPEAT")}
    size = os.path.getsize(os.path.join(ROOT, "tests", "golden", "vpoly_fold_kats.json"))
    assert 24 << 10 <= size <= 48 << 10, size


@pytest.mark.parametrize("field", ["goldilocks", "babybear", "stark"])
@pytest.mark.parametrize("name", ["SINGLE", "R1CS", "REPEAT", "MIXED", "CANCEL"])
def test_model_folds_like_model_mle_and_continues_the_sum_check(field, name):
    p = SC.PRIMES[field]
    add, sub, mul = _int_ops(p)
    terms = getattr(VP, name)
    rng = random.Random("vpoly fold %s %s" % (field, name))
    for nv in (2, 3, 5):
        full = 1 << nv
        tables = [[rng.choice((0, 1, p - 1, rng.randrange(p))) for _ in range(rng.choice((full, full, full - 1, full // 2 + 1, 1)))]
                  for _ in range(VP.n_tables(terms))]
        coeffs = None if name == "SINGLE" else [rng.randrange(p) for _ in terms]
        if name == "CANCEL":
            coeffs[1] = (p - coeffs[0]) % p
        for order in (LEADING, TRAILING):
            prev = VP.round_evals(tables, terms, coeffs, nv, order, 0, 1, add, sub, mul)
            r = rng.randrange(p)
            folded, msg = VF.fold_round(tables, terms, coeffs, nv, r, order, 0, 1, add, sub, mul)
            for f, g in zip(tables, folded):
                whole = M.fold(M.pad(f, nv, 0), nv, [r], order, add, sub, mul)
                assert g == whole[:len(g)] and not any(whole[len(g):])
                assert len(g) == VF.folded_len(len(f), nv, order)
            assert msg == VP.round_evals(folded, terms, coeffs, nv - 1, order, 0, 1, add, sub, mul)
            assert len(msg) == VP.degree(terms) + 1
            # the sum-check identity: p(0) + p(1) of the new message is the previous message interpolated at r
            assert (msg[0] + msg[1]) % p == SC.lagrange_at(prev, r, p)
            if name == "CANCEL":
                assert not any(msg)
            if name == "SINGLE":  # one term without coefficients: the fused round of a product
                assert (folded, msg) == SF.fold_round([tables[j] for j in terms[0]], nv, r, order, 0, 1, add, sub, mul)


@pytest.mark.parametrize("order", [LEADING, TRAILING])
def test_model_whole_r1cs_prover_ends_at_g_of_the_evaluations(order):
    p = SC.PRIMES["goldilocks"]
    add, sub, mul = _int_ops(p)
    rng = random.Random(order)
    nv, terms = 5, VP.R1CS
    orig = [[rng.randrange(p) for _ in range(n)] for n in (32, 29, 17, 32)]
    coeffs = [rng.randrange(p), p - 1]
    tables = orig
    claim = VP.poly_sum(tables, terms, coeffs, nv, 0, add, mul)
    msg = VP.round_evals(tables, terms, coeffs, nv, order, 0, 1, add, sub, mul)  # round 0
    point = []
    for left in range(nv, 1, -1):  # rounds 1 .. nv - 1 through the fused step
        assert (msg[0] + msg[1]) % p == claim
        r = rng.randrange(p)
        point.append(r)
        claim = SC.lagrange_at(msg, r, p)
        tables, msg = VF.fold_round(tables, terms, coeffs, left, r, order, 0, 1, add, sub, mul)
    assert (msg[0] + msg[1]) % p == claim
    r = rng.randrange(p)
    point.append(r)
    claim = SC.lagrange_at(msg, r, p)
    finals = [M.fold(M.pad(f, 1, 0), 1, [r], order, add, sub, mul)[0] for f in tables]
    assert VP.evaluate(finals, terms, coeffs, 0, add, mul) == claim
    full_point = point if order == LEADING else point[::-1]
    assert finals == [M.fix_variables(M.pad(f, nv, 0), nv, full_point, add, sub, mul)[0] for f in orig]
