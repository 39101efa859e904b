"""CPU checks of the weighted sum-check rounds (include/stark_rings_hip.h: sr_vpoly_wround_plan, sr_vpoly_wround_evals[_dev],
sr_vpoly_wround_fold_plan, sr_vpoly_wround_fold_evals[_dev]): the exports, the plan arithmetic for every ring with the points-per-launch
table, the refusals that need no device, and the pure-Python restatement (tools/model_wsumcheck.py, the oracle of the GPU tests) against
model_vpoly.round_evals, the explicit prover that holds eq(z, .) as one more table, the round identity and the pinned vectors of
tests/golden/wsumcheck_kats.json."""
import ctypes
import json
import os
import random
import re
import sys

import pytest

from stark_rings_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tools"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
import model_mle as M  # noqa: E402
import model_sparse_mle as SM  # noqa: E402
import model_vpoly as VP  # noqa: E402
import model_vpoly_fold as VF  # noqa: E402
import model_wsumcheck as W  # noqa: E402

NEW = ("sr_vpoly_wround_plan", "sr_vpoly_wround_evals_dev", "sr_vpoly_wround_evals", "sr_vpoly_wround_fold_plan",
       "sr_vpoly_wround_fold_evals_dev", "sr_vpoly_wround_fold_evals")
LEADING, TRAILING, ROUND_SUM = 0, 1, 2
# points per launch of the weighted round kernels and points the weighted fused launch takes, over 4 / 8 table slots, per ring id
# (csrc/sumcheck_weighted.hpp: points_of, fused_points_of; tests/test_wsumcheck_isa.py holds the register counts behind them)
PER_LAUNCH = {0: {4: 5, 8: 5}, 1: {4: 5, 8: 5}, 2: {4: 4, 8: 1}, 3: {4: 3, 8: 1}, 4: {4: 1, 8: 1}, 5: {4: 1, 8: 1}}
FUSED = {0: {4: 5, 8: 4}, 1: {4: 5, 8: 3}, 2: {4: 2, 8: 1}, 3: {4: 2, 8: 1}, 4: {4: 1, 8: 0}, 5: {4: 1, 8: 1}}
SHAPES = [(0, 0), (0, 6), (0, 10), (0, 16), (1, 5), (1, 16), (2, 4), (2, 12), (3, 0), (4, 0), (5, 0)]


def _header():
    return open(os.path.join(ROOT, "include", "stark_rings_hip.h")).read()


def test_header_library_and_ctypes_table_carry_the_new_names():
    lib = _lib.load()
    declared = set(re.findall(r"\b(sr_[a-z0-9_]+)\s*\(", _header()))
    for name in NEW:
        assert name in declared, "%s is not declared in the header" % name
        assert name in _lib.SYMBOLS, "%s is missing from _lib.SYMBOLS" % name
        assert hasattr(lib, name), "the library does not export %s" % name


def _plan(fn, ring, k, nv, nt, n_terms, degree, order):
    work, launches = ctypes.c_size_t(1 << 60), ctypes.c_int(-1)
    rc = getattr(_lib.load(), fn)(ring, k, nv, nt, n_terms, degree, order, ctypes.byref(work), ctypes.byref(launches))
    return rc, work.value, launches.value


@pytest.mark.parametrize("ring,k", SHAPES)
def test_round_plan_for_every_ring_slot_count_degree_and_order(ring, k):
    max_groups = int(re.search(r"#define\s+SR_MLE_ROUND_MAX_GROUPS\s+(\d+)", _header()).group(1))
    for order in (LEADING, TRAILING):
        for nv in range(1, 25):
            for nt in (1, 4, 5, 8):
                slots = 4 if nt <= 4 else 8
                for degree in (1, 2, 3, 4):
                    rc, work, launches = _plan("sr_vpoly_wround_plan", ring, k, nv, nt, 3, degree, order)
                    where = "ring %d k %d nv %d tables %d degree %d order %d: work %d launches %d" % (ring, k, nv, nt, degree, order, work, launches)
                    assert rc == 0, where
                    assert (work == 0) == (launches == 1), where
                    assert work <= max_groups * (degree + 1) and work % (degree + 1) == 0, where
                    points = -(-(degree + 1) // min(PER_LAUNCH[ring][slots], degree + 1))  # launches of the points
                    assert launches in (points, points + 1), where
                    if points > 1:
                        assert work > 0 and launches == points + 1, where
                    # the records are those of the unweighted round (at least two where the points go in several launches)
                    urc, uwork, _ = _plan("sr_vpoly_round_plan", ring, k, nv, nt, 3, degree, order)
                    assert urc == 0 and (work == uwork or {work, uwork} == {0, 2 * (degree + 1)}), where


@pytest.mark.parametrize("ring,k", SHAPES)
def test_fold_plan_for_every_ring_slot_count_degree_and_order(ring, k):
    split = single = 0
    for order in (LEADING, TRAILING):
        for nv in range(2, 25):
            for nt in (4, 8):
                for degree in (1, 2, 3, 4):
                    rc, work, launches = _plan("sr_vpoly_wround_fold_plan", ring, k, nv, nt, 3, degree, order)
                    where = "ring %d k %d nv %d tables %d degree %d order %d: work %d launches %d" % (ring, k, nv, nt, degree, order, work, launches)
                    assert rc == 0 and launches >= 1, where
                    assert (work == 0) == (launches == 1), where
                    fused, per = min(FUSED[ring][nt], degree + 1), min(PER_LAUNCH[ring][nt], degree + 1)
                    rest = -(-(degree + 1 - fused) // per)  # launches of the remaining points
                    assert launches in (1 + rest, 2 + rest), where
                    if rest:
                        assert work > 0, where  # several launches meet in the workspace
                    rrc, rwork, _ = _plan("sr_vpoly_wround_plan", ring, k, nv - 1, nt, 3, degree, order)
                    assert rrc == 0 and (work == rwork or {work, rwork} <= {0, 2 * (degree + 1)}), where
                    split += work > 0
                    single += work == 0
    assert split and (single or ring >= 4)  # babybear72 and frog16 fuse one point at most: their plans always split


def test_plans_depend_on_the_shape_only():
    assert _plan("sr_vpoly_wround_plan", 0, 10, 20, 4, 2, 3, LEADING) == _plan("sr_vpoly_wround_plan", 0, 10, 20, 4, 8, 3, TRAILING)
    assert _plan("sr_vpoly_wround_plan", 0, 16, 4, 8, 2, 4, LEADING) == (0, 0, 1)       # all five points in one launch, one record
    assert _plan("sr_vpoly_wround_plan", 2, 4, 3, 4, 2, 4, LEADING)[2] == 3             # Stark: 4 + 1 points, then the records
    assert _plan("sr_vpoly_wround_plan", 2, 4, 3, 4, 2, 3, LEADING) == (0, 0, 1)        # four points over four slots in one launch
    assert _plan("sr_vpoly_wround_plan", 3, 0, 3, 4, 2, 2, LEADING) == (0, 0, 1)        # goldilocks24: three
    assert _plan("sr_vpoly_wround_fold_plan", 0, 16, 4, 8, 2, 4, LEADING)[2] == 3       # four fused, the fifth, the records
    assert _plan("sr_vpoly_wround_fold_plan", 0, 16, 4, 8, 2, 3, LEADING) == (0, 0, 1)


def test_device_free_refusals_name_their_reason():
    lib = _lib.load()
    work, launches = ctypes.c_size_t(), ctypes.c_int()
    by = ctypes.byref
    # a weight of a plain sum is just a table
    assert lib.sr_vpoly_wround_plan(0, 10, 4, 2, 2, 3, ROUND_SUM, by(work), by(launches)) == 1
    assert _lib.last_error().startswith("vpoly_wround: ") and "SR_MLE_ROUND_SUM" in _lib.last_error()
    assert lib.sr_vpoly_wround_fold_plan(0, 10, 4, 2, 2, 3, ROUND_SUM, by(work), by(launches)) == 1
    assert _lib.last_error().startswith("vpoly_wround_fold: ") and "unknown order" in _lib.last_error()
    for order in (3, -1):
        assert lib.sr_vpoly_wround_plan(0, 10, 4, 2, 2, 3, order, by(work), by(launches)) == 1 and "unknown order" in _lib.last_error()
    for ring in range(6):
        k = 4 if ring < 3 else 0
        assert lib.sr_vpoly_wround_plan(ring, k, 0, 4, 2, 3, LEADING, by(work), by(launches)) == 1
        assert "num_vars >= 1" in _lib.last_error() and _lib.last_error().startswith("vpoly_wround: ")
        assert lib.sr_vpoly_wround_plan(ring, k, 1, 4, 2, 3, LEADING, by(work), by(launches)) == 0
        assert lib.sr_vpoly_wround_plan(ring, k, 47, 4, 2, 3, TRAILING, by(work), by(launches)) == 0
        assert lib.sr_vpoly_wround_plan(ring, k, 48, 4, 2, 3, LEADING, by(work), by(launches)) == 1
        assert lib.sr_vpoly_wround_fold_plan(ring, k, 1, 4, 2, 3, LEADING, by(work), by(launches)) == 1
        assert "num_vars >= 2" in _lib.last_error() and _lib.last_error().startswith("vpoly_wround_fold: ")
        assert lib.sr_vpoly_wround_fold_plan(ring, k, 2, 4, 2, 3, TRAILING, by(work), by(launches)) == 0
    for args, msg in (((0, 10, 4, 0, 2, 3, LEADING), "n_tables must be 1 .. 8"), ((0, 10, 4, 9, 2, 3, LEADING), "n_tables must be 1 .. 8"),
                      ((0, 10, 4, 2, 0, 3, LEADING), "n_terms must be 1 .. 8"), ((0, 10, 4, 2, 2, 5, LEADING), "degree"),
                      ((6, 0, 4, 2, 2, 3, LEADING), "unknown ring"), ((0, 25, 4, 2, 2, 3, LEADING), "log2_degree")):
        for fn in (lib.sr_vpoly_wround_plan, lib.sr_vpoly_wround_fold_plan):
            assert fn(*args, by(work), by(launches)) == 1 and msg in _lib.last_error(), (args, _lib.last_error())
    assert lib.sr_vpoly_wround_plan(0, 10, 4, 2, 2, 3, LEADING, None, by(launches)) == 1 and "null" in _lib.last_error()
    # null weights are refused before anything else, a null context next
    one = ctypes.c_uint64(0)
    wp = ctypes.cast(by(one), ctypes.c_void_p)
    assert lib.sr_vpoly_wround_evals_dev(None, None, None, None, None, 9, None, 9, None, 99, 7, None, 0, None) == 1
    assert _lib.last_error() == "vpoly_wround: null pointer (d_weights)"
    assert lib.sr_vpoly_wround_evals(None, None, None, None, None, 9, None, 9, None, 99, 7) == 1
    assert _lib.last_error() == "vpoly_wround: null pointer (weights)"
    assert lib.sr_vpoly_wround_fold_evals_dev(None, None, None, None, None, None, None, 9, None, 9, None, 99, None, 7, None, 0, None) == 1
    assert _lib.last_error() == "vpoly_wround_fold: null pointer (d_weights)"
    assert lib.sr_vpoly_wround_fold_evals(None, None, None, None, None, None, None, 9, None, 9, None, 99, None, 7) == 1
    assert _lib.last_error() == "vpoly_wround_fold: null pointer (weights)"
    assert lib.sr_vpoly_wround_evals_dev(None, None, wp, None, None, 9, None, 9, None, 99, 7, None, 0, None) == 1
    assert "null context" in _lib.last_error()
    assert lib.sr_vpoly_wround_fold_evals_dev(None, None, None, None, wp, None, None, 9, None, 9, None, 99, None, 7, None, 0, None) == 1
    assert "null context" in _lib.last_error()


# ---- the restatement the GPU tests use as their oracle ---------------------------------------------------------------------------------
def _same(a, b):
    import numpy as np

    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


STRUCTS = {"PRODUCT": ([[0, 1]], False), "R1CS": ([[0, 1], [2]], True), "FRACTION": (W.FRACTION, True), "MIXED3": ([[0, 0, 1], [2], [1, 2]], True)}


@pytest.mark.parametrize("ring", W.RINGS)
def test_all_one_weights_give_the_unweighted_round(ring):
    zero, one, add, sub, mul, draw, _, _ = W.ring_ops(ring)
    rng = random.Random("wsumcheck ones " + ring)
    for name, (terms, with_coeffs) in sorted(STRUCTS.items()):
        for nv in (1, 3):
            full = 1 << nv
            tables = [draw(rng, rng.choice((full, full, full - 1, full // 2 + 1, 1))) for _ in range(VP.n_tables(terms))]
            coeffs = draw(rng, len(terms)) if with_coeffs else None
            for order in (LEADING, TRAILING):
                got = W.wround_evals(tables, terms, coeffs, [one] * (full // 2), nv, order, zero, one, add, sub, mul)
                assert _same(got, VP.round_evals(tables, terms, coeffs, nv, order, zero, one, add, sub, mul)), (ring, name, nv, order)


@pytest.mark.parametrize("order", [LEADING, TRAILING])
@pytest.mark.parametrize("ring", W.RINGS)
def test_the_eq_sumcheck_model_sends_the_messages_of_the_explicit_prover(ring, order):
    """in every round the d + 2 elements of the prover that holds eq(z, .) as one more factor; s_j(0) + s_j(1) = s_{j-1}(r_{j-1}),
    checked through the explicit prover's own messages (their degree is d + 1, so the d + 2 points pin the polynomial) and directly
    as the sum of the first two elements against the claimed sum of the round; the final values agree as well"""
    zero, one, add, sub, mul, draw, _, _ = W.ring_ops(ring)
    rng = random.Random("wsumcheck eq %s %d" % (ring, order))
    for name, (terms, with_coeffs) in sorted(STRUCTS.items()):
        for nv in (1, 4) if name == "R1CS" else (2,):
            full = 1 << nv
            tables = [draw(rng, rng.choice((full, full, full - 1))) for _ in range(VP.n_tables(terms))]
            coeffs = draw(rng, len(terms)) if with_coeffs else None
            z, rs = draw(rng, nv), draw(rng, nv)
            msgs, finals, eq_r = W.eq_sumcheck(tables, terms, coeffs, z, rs, order, zero, one, add, sub, mul)
            want_msgs, want_finals = W.explicit(tables, terms, coeffs, z, rs, order, zero, one, add, sub, mul)
            assert len(msgs) == len(want_msgs) == nv
            for j, (a, b) in enumerate(zip(msgs, want_msgs)):
                assert len(a) == VP.degree(terms) + 2 and _same(a, b), (ring, name, nv, j)
            assert _same(finals, want_finals[:-1]) and _same([eq_r], want_finals[-1:]), (ring, name, nv)
            # the claimed sum of round 1 is sum_b eq(z, b) g(b); the claim of round j + 1 is s_j(r_j), which the folded explicit
            # polynomial restates as its own plain sum
            eq = SM.precompute_eq(list(z), sub, mul, one)
            eterms = [list(t) + [len(tables)] for t in terms]
            claim = VP.poly_sum(list(tables) + [eq], eterms, coeffs, nv, zero, add, mul)
            tabs = list(tables) + [eq]
            for j in range(nv):
                assert _same([add(msgs[j][0], msgs[j][1])], [claim]), (ring, name, nv, j)
                tabs = [M.fold(M.pad(f, nv - j, zero), nv - j, [rs[j]], order, add, sub, mul) for f in tabs]
                claim = VP.poly_sum(tabs, eterms, coeffs, nv - j - 1, zero, add, mul)
            assert _same([claim], [mul(eq_r, VP.evaluate(finals, terms, coeffs, zero, add, mul))]), (ring, name, nv)


@pytest.mark.parametrize("ring", W.RINGS)
def test_the_fold_round_model_is_the_round_on_the_folded_tables(ring):
    zero, one, add, sub, mul, draw, _, _ = W.ring_ops(ring)
    rng = random.Random("wsumcheck fold " + ring)
    terms = W.FRACTION
    for nv in (2, 4):
        full = 1 << nv
        tables = [draw(rng, n) for n in (full, full - 1, full // 2 + 1, full)]
        coeffs, weights, r = draw(rng, 3), draw(rng, full // 4), draw(rng, 1)[0]
        for order in (LEADING, TRAILING):
            folded, msg = W.wfold_round(tables, terms, coeffs, weights, nv, r, order, zero, one, add, sub, mul)
            want_folded, _ = VF.fold_round(tables, terms, coeffs, nv, r, order, zero, one, add, sub, mul)
            assert all(_same(a, b) for a, b in zip(folded, want_folded))
            assert _same(msg, W.wround_evals(folded, terms, coeffs, weights, nv - 1, order, zero, one, add, sub, mul))


def test_the_pinned_vectors_regenerate_byte_for_byte():
    path = os.path.join(ROOT, "tests", "golden", "wsumcheck_kats.json")
    text = open(path).read()
    assert text == W.dump_kats(), "tests/golden/wsumcheck_kats.json is not what tools/model_wsumcheck.py writes"
    cases = json.loads(text)["cases"]
    assert {(c["ring"], c["structure"]) for c in cases} == {(r, "R1CS") for r in W.RINGS}
    assert all(set(c) >= {"leading", "trailing"} and ("weights_fold" in c) == (c["form"] == "standard") for c in cases)
    assert os.path.getsize(path) < 48 << 10
