"""CPU checks of the fused fold-and-round entry points (include/stark_rings_hip.h: sr_mle_round_fold_plan,
sr_mle_round_fold_evals[_dev]): the exports, the plan arithmetic for every ring, the refusals that need no context (the others need one
and live in tests/test_sumcheck_fold_gpu.py), and the pure-Python restatement (tools/model_sumcheck_fold.py, the oracle of the GPU
tests) against model_mle.fold, model_sumcheck.round_evals, the sum-check identities and the pinned vectors of
tests/golden/sumcheck_fold_kats.json."""
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

NEW = ("sr_mle_round_fold_plan", "sr_mle_round_fold_evals_dev", "sr_mle_round_fold_evals")
LEADING, TRAILING = 0, 1
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "sumcheck_fold_kats.json")))
# points the fused launch takes for d = 1 .. 4 (csrc/sumcheck_fold.hpp: fused_points_of) and points per launch of the round kernels that
# take the remaining ones (csrc/sumcheck.hpp: points_of), per ring id
FUSED = {0: (2, 3, 4, 5), 1: (2, 3, 4, 5), 2: (2, 3, 3, 2), 3: (2, 3, 2, 2), 4: (2, 2, 1, 1), 5: (2, 1, 1, 1)}
PER_LAUNCH = {0: (2, 3, 4, 5), 1: (2, 3, 4, 5), 2: (2, 3, 4, 2), 3: (2, 3, 2, 3), 4: (2, 3, 2, 2), 5: (2, 2, 2, 1)}


def _header():
    return open(os.path.join(ROOT, "include", "stark_rings_hip.h")).read()


def test_header_library_and_ctypes_table_carry_the_new_names():
    lib = _lib.load()
    declared = set(re.findall(r"\b(sr_[a-z0-9_]+)\s*\(", _header()))
    for name in NEW:
        assert name in declared, "%s is not declared in the header" % name
        assert name in _lib.SYMBOLS, "%s is missing from _lib.SYMBOLS" % name
        assert hasattr(lib, name), "the library does not export %s" % name


def _plan(ring, k, nv, nt, order):
    lib = _lib.load()
    work, launches = ctypes.c_size_t(1 << 60), ctypes.c_int(-1)
    rc = lib.sr_mle_round_fold_plan(ring, k, nv, nt, order, ctypes.byref(work), ctypes.byref(launches))
    return rc, work.value, launches.value


@pytest.mark.parametrize("ring,k", [(0, 0), (0, 6), (0, 10), (0, 16), (1, 5), (1, 16), (2, 4), (2, 12), (3, 0), (4, 0), (5, 0)])
def test_plan_bounds_for_every_ring_size_table_count_and_order(ring, k):
    max_groups = int(re.search(r"#define\s+SR_MLE_ROUND_MAX_GROUPS\s+(\d+)", _header()).group(1))
    split = single = 0
    for order in (LEADING, TRAILING):
        for nv in range(2, 25):
            for nt in (1, 2, 3, 4):
                rc, work, launches = _plan(ring, k, nv, nt, order)
                where = "ring %d k %d nv %d tables %d order %d: work %d launches %d" % (ring, k, nv, nt, order, work, launches)
                assert rc == 0, where
                assert launches >= 1, where
                assert (work == 0) == (launches == 1), where
                assert work <= max_groups * (nt + 1), where
                assert work % (nt + 1) == 0, where
                fused, per = FUSED[ring][nt - 1], PER_LAUNCH[ring][nt - 1]
                rest = -(-(nt + 1 - fused) // per)  # launches of the remaining points
                assert launches in (1 + rest, 2 + rest), where
                if ring <= 1:  # the one-limb fields: the fused launch takes every point, then at most the sum over the records
                    assert fused == nt + 1 and launches <= 2, where
                if rest:
                    assert work > 0, where  # several launches meet in the workspace
                # the records are those of the round in num_vars - 1 variables
                rwork, rlaunches = ctypes.c_size_t(), ctypes.c_int()
                assert _lib.load().sr_mle_round_plan(ring, k, nv - 1, nt, order, ctypes.byref(rwork), ctypes.byref(rlaunches)) == 0
                assert work == rwork.value or (rest and rwork.value == 0 and work == 2 * (nt + 1)), where
                split += work > 0
                single += work == 0
    assert split and single


def test_plan_depends_on_the_shape_only_and_needs_no_device():
    assert _plan(0, 10, 20, 2, LEADING) == _plan(0, 10, 20, 2, LEADING)
    assert _plan(0, 10, 20, 2, LEADING) == _plan(0, 10, 20, 2, TRAILING)
    rc, work, launches = _plan(0, 10, 20, 2, LEADING)
    assert (rc, launches) == (0, 2) and work % 3 == 0 and work > 0
    assert _plan(0, 16, 4, 3, LEADING) == (0, 0, 1)


def test_plan_refuses_bad_arguments_and_names_the_reason():
    lib = _lib.load()
    work, launches = ctypes.c_size_t(), ctypes.c_int()
    for args, msg in (((0, 10, 0, 2, LEADING), "num_vars >= 2"), ((0, 10, 1, 2, TRAILING), "num_vars >= 2"),
                      ((0, 10, 48, 2, LEADING), "num_vars must be below 48"),
                      ((0, 10, 4, 0, LEADING), "n_tables must be 1 .. 4"), ((0, 10, 4, 5, LEADING), "n_tables must be 1 .. 4"),
                      ((0, 10, 4, 2, 2), "unknown order"), ((0, 10, 4, 2, -1), "unknown order"),
                      ((6, 0, 4, 2, LEADING), "unknown ring"), ((-1, 0, 4, 2, LEADING), "unknown ring"), ((0, 25, 4, 2, LEADING), "log2_degree")):
        assert lib.sr_mle_round_fold_plan(*args, ctypes.byref(work), ctypes.byref(launches)) == 1, args
        assert msg in _lib.last_error(), (args, _lib.last_error())
    assert lib.sr_mle_round_fold_plan(0, 10, 4, 2, LEADING, None, ctypes.byref(launches)) == 1 and "null" in _lib.last_error()
    assert lib.sr_mle_round_fold_plan(0, 10, 4, 2, LEADING, ctypes.byref(work), None) == 1 and "null" in _lib.last_error()
    assert lib.sr_mle_round_fold_plan(0, 10, 2, 2, LEADING, ctypes.byref(work), ctypes.byref(launches)) == 0


def test_entry_points_refuse_a_null_context_before_anything_else():
    lib = _lib.load()
    assert lib.sr_mle_round_fold_evals(None, None, None, None, None, None, 9, 99, None, 7) == 1 and "null context" in _lib.last_error()
    assert lib.sr_mle_round_fold_evals_dev(None, None, None, None, None, None, 9, 99, None, 7, None, 0, None) == 1
    assert "null context" in _lib.last_error()


# ---- the restatement the GPU tests use as their oracle ---------------------------------------------------------------------------------
def _int_ops(p):
    return (lambda a, b: (a + b) % p), (lambda a, b: (a - b) % p), (lambda r, a: r * a % p)


def test_model_reproduces_the_pinned_vectors():
    assert KATS == SF.make_kats(), "tests/golden/sumcheck_fold_kats.json is not what tools/model_sumcheck_fold.py writes"
    seen = set()
    for case in KATS["cases"]:
        p = SC.PRIMES[case["ring"]]
        add, sub, mul = SC.vec_ops(p)
        dr = 1 << case["log2_degree"]
        zero, one = (0,) * dr, (1,) * dr
        tables = [[tuple(e) for e in f] for f in case["tables"]]
        assert [len(f) for f in tables] == case["n_evals"]
        nv = case["num_vars"]
        for key, order in (("leading", LEADING), ("trailing", TRAILING)):
            folded, msg = SF.fold_round(tables, nv, tuple(case["r"]), order, zero, one, add, sub, mul)
            assert [[list(e) for e in g] for g in folded] == case[key]["folded"]
            assert [list(e) for e in msg] == case[key]["message"]
            assert [len(g) for g in folded] == [SF.folded_len(n, nv, order) for n in case["n_evals"]]
        seen.add((case["ring"], len(tables), min(case["n_evals"]) < 1 << nv))
    assert seen == {(r, d, True) for r in ("goldilocks", "babybear", "stark") for d in (1, 2, 3, 4)}


@pytest.mark.parametrize("field", ["goldilocks", "babybear", "stark"])
@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_model_folds_like_model_mle_and_continues_the_sum_check(field, d):
    p = SC.PRIMES[field]
    add, sub, mul = _int_ops(p)
    rng = random.Random("fold %s %d" % (field, d))
    for nv in (2, 3, 5):
        full = 1 << nv
        tables = [[rng.choice((0, 1, p - 1, rng.randrange(p))) for _ in range(rng.choice((full, full, full - 1, full // 2 + 1, 1)))] for _ in range(d)]
        for order in (LEADING, TRAILING):
            prev = SC.round_evals(tables, nv, order, 0, 1, add, sub, mul)
            r = rng.randrange(p)
            folded, msg = SF.fold_round(tables, nv, r, order, 0, 1, add, sub, mul)
            for f, g in zip(tables, folded):
                whole = M.fold(M.pad(f, nv, 0), nv, [r], order, add, sub, mul)
                assert g == whole[:len(g)] and not any(whole[len(g):])
                assert len(g) == SF.folded_len(len(f), nv, order)
            assert msg == SC.round_evals(folded, nv - 1, order, 0, 1, add, sub, mul)
            assert len(msg) == d + 1
            assert (msg[0] + msg[1]) % p == SC.lagrange_at(prev, r, p)


@pytest.mark.parametrize("order", [LEADING, TRAILING])
def test_model_whole_prover_ends_at_the_product_of_the_evaluations(order):
    p = SC.PRIMES["goldilocks"]
    add, sub, mul = _int_ops(p)
    rng = random.Random(order)
    nv, d = 5, 3
    orig = [[rng.randrange(p) for _ in range(n)] for n in (32, 29, 17)]
    tables = orig
    claim = SC.product_sum([M.pad(f, nv, 0) for f in tables], 0, add, mul)
    msg = SC.round_evals(tables, nv, order, 0, 1, add, sub, mul)  # round 0
    point = []
    for left in range(nv, 1, -1):  # rounds 1 .. nv - 1 through the fused step
        assert (msg[0] + msg[1]) % p == claim
        r = rng.randrange(p)
        point.append(r)
        claim = SC.lagrange_at(msg, r, p)
        tables, msg = SF.fold_round(tables, left, r, order, 0, 1, add, sub, mul)
    assert (msg[0] + msg[1]) % p == claim
    r = rng.randrange(p)
    point.append(r)
    claim = SC.lagrange_at(msg, r, p)
    finals = [M.fold(M.pad(f, 1, 0), 1, [r], order, add, sub, mul)[0] for f in tables]
    prod = 1
    for v in finals:
        prod = prod * v % p
    assert prod == claim
    full_point = point if order == LEADING else point[::-1]
    assert finals == [M.fix_variables(M.pad(f, nv, 0), nv, full_point, add, sub, mul)[0] for f in orig]
