"""CPU checks of the range-check rounds (include/stark_rings_hip.h: sr_range_wround_plan, sr_range_wround_evals[_dev]): the exports, the
plan arithmetic for every ring against the points-per-launch table, the refusals that need no device, and the pure-Python restatement
(tools/model_range.py, the oracle of the GPU tests) against the pinned vectors of tests/golden/range_kats.json, against closed forms in
plain integers and, at bound 2, against model_wsumcheck on the tables (f, f - 1, f + 1)."""
import ctypes
import json
import math
import os
import random
import re
import sys

import pytest

import stark_rings_amd
from stark_rings_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tools"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
import model_range as R  # noqa: E402
import model_sumcheck as SC  # noqa: E402
import model_wsumcheck as W  # noqa: E402

NEW = ("sr_range_wround_plan", "sr_range_wround_evals_dev", "sr_range_wround_evals")
LEADING, TRAILING = 0, 1
# points per launch per ring id (csrc/range_check.hpp: points_of; tests/test_range_isa.py holds the register counts behind them)
PER_LAUNCH = {0: 7, 1: 8, 2: 3, 3: 2, 4: 2, 5: 2}
SHAPES = [(0, 0), (0, 6), (0, 10), (0, 16), (1, 5), (1, 16), (2, 4), (2, 12), (3, 0), (4, 0), (5, 0)]


def _header():
    return open(os.path.join(ROOT, "include", "stark_rings_hip.h")).read()


def test_header_library_ctypes_table_and_package_carry_the_new_names():
    lib = _lib.load()
    declared = set(re.findall(r"\b(sr_[a-z0-9_]+)\s*\(", _header()))
    for name in NEW:
        assert name in declared, "%s is not declared in the header" % name
        assert name in _lib.SYMBOLS, "%s is missing from _lib.SYMBOLS" % name
        assert hasattr(lib, name), "the library does not export %s" % name
    assert int(re.search(r"#define\s+SR_RANGE_MAX_TABLES\s+(\d+)", _header()).group(1)) == 8
    assert int(re.search(r"#define\s+SR_RANGE_MAX_BOUND\s+(\d+)", _header()).group(1)) == 8
    for name in ("range_wround_plan", "range_wround_evals_dev", "range_wround_evals", "RangePolynomial"):
        assert hasattr(stark_rings_amd, name), name
    assert not any(n.startswith("range_") for n in dir(stark_rings_amd.CyclotomicRing))  # functions of the module, not methods
    src = open(os.path.join(ROOT, "stark_rings_amd", "csrc", "range_check.hpp")).read()
    for text in ("return 7;", "return 8;", "return 3;", "return 2;"):
        assert text in src, text
    assert "Goldilocks 7, BabyBear 8, Stark 3, goldilocks24 2, babybear72 2, frog16 2" in _header()


def _plan(ring, k, nv, nt, bound, order):
    work, launches = ctypes.c_size_t(1 << 60), ctypes.c_int(-1)
    rc = _lib.load().sr_range_wround_plan(ring, k, nv, nt, bound, order, ctypes.byref(work), ctypes.byref(launches))
    return rc, work.value, launches.value


@pytest.mark.parametrize("ring,k", SHAPES)
def test_plan_for_every_ring_table_count_bound_and_order(ring, k):
    max_groups = int(re.search(r"#define\s+SR_MLE_ROUND_MAX_GROUPS\s+(\d+)", _header()).group(1))
    lib = _lib.load()
    for order in (LEADING, TRAILING):
        for nv in range(1, 25):
            for bound in range(2, 9):
                n = 2 * bound
                rc, work, launches = _plan(ring, k, nv, 1, bound, order)
                where = "ring %d k %d nv %d bound %d order %d: work %d launches %d" % (ring, k, nv, bound, order, work, launches)
                assert rc == 0, where
                assert (work == 0) == (launches == 1), where
                assert work <= max_groups * n and work % n == 0, where
                points = -(-n // min(PER_LAUNCH[ring], n))  # launches of the points
                assert launches in (points, points + 1), where
                if points > 1:
                    assert work > 0 and launches == points + 1, where
                for nt in (3, 8):  # the plan does not depend on the number of tables
                    assert _plan(ring, k, nv, nt, bound, order) == (rc, work, launches), where
                # the records are those of the unweighted round (at least two where the points go in several launches)
                uw, ul = ctypes.c_size_t(), ctypes.c_int()
                assert lib.sr_vpoly_round_plan(ring, k, nv, 1, 1, 1, order, ctypes.byref(uw), ctypes.byref(ul)) == 0
                assert work // n == uw.value // 2 or (work // n, uw.value // 2) == (2, 0), where


def test_plans_of_known_shapes():
    assert _plan(0, 16, 4, 8, 2, LEADING) == (0, 0, 1)        # Goldilocks, bound 2: four points in one launch, one record
    assert _plan(0, 16, 4, 8, 3, LEADING) == (0, 0, 1)        # six points still fit
    assert _plan(0, 16, 4, 8, 8, LEADING) == (0, 2 * 16, 4)   # 7 + 7 + 2 points, then the records
    assert _plan(1, 16, 4, 1, 8, TRAILING) == (0, 2 * 16, 3)  # BabyBear: 8 + 8
    assert _plan(2, 4, 3, 4, 2, LEADING) == (0, 2 * 4, 3)     # Stark: 3 + 1
    assert _plan(3, 0, 3, 4, 2, LEADING) == (0, 2 * 4, 3)     # goldilocks24: 2 + 2
    assert _plan(4, 0, 3, 4, 8, LEADING) == (0, 2 * 16, 9)
    assert _plan(5, 0, 3, 4, 3, LEADING) == (0, 2 * 6, 4)


def test_device_free_refusals_name_their_reason():
    lib = _lib.load()
    work, launches = ctypes.c_size_t(), ctypes.c_int()
    by = ctypes.byref
    for order in (2, 3, -1):
        assert lib.sr_range_wround_plan(0, 10, 4, 2, 2, order, by(work), by(launches)) == 1
        assert _lib.last_error() == "range_wround: unknown order"
    for ring in range(6):
        k = 4 if ring < 3 else 0
        assert lib.sr_range_wround_plan(ring, k, 0, 4, 2, LEADING, by(work), by(launches)) == 1
        assert "num_vars >= 1" in _lib.last_error() and _lib.last_error().startswith("range_wround: ")
        assert lib.sr_range_wround_plan(ring, k, 1, 4, 2, LEADING, by(work), by(launches)) == 0
        assert lib.sr_range_wround_plan(ring, k, 47, 8, 8, TRAILING, by(work), by(launches)) == 0
        assert lib.sr_range_wround_plan(ring, k, 48, 4, 2, LEADING, by(work), by(launches)) == 1
        assert "num_vars must be below 48" in _lib.last_error()
    for args, msg in (((0, 10, 4, 0, 2, LEADING), "n_tables must be 1 .. 8"), ((0, 10, 4, 9, 2, LEADING), "n_tables must be 1 .. 8"),
                      ((0, 10, 4, 2, 1, LEADING), "bound must be 2 .. 8"), ((0, 10, 4, 2, 9, LEADING), "bound must be 2 .. 8"),
                      ((6, 0, 4, 2, 2, LEADING), "unknown ring"), ((0, 25, 4, 2, 2, LEADING), "log2_degree")):
        assert lib.sr_range_wround_plan(*args, by(work), by(launches)) == 1 and msg in _lib.last_error(), (args, _lib.last_error())
    assert lib.sr_range_wround_plan(0, 10, 4, 2, 2, LEADING, None, by(launches)) == 1 and "null" in _lib.last_error()
    # null weights are refused before anything else, a null context next
    one = ctypes.c_uint64(0)
    wp = ctypes.cast(by(one), ctypes.c_void_p)
    assert lib.sr_range_wround_evals_dev(None, None, None, None, None, 9, 99, None, 99, 7, None, 0, None) == 1
    assert _lib.last_error() == "range_wround: null pointer (d_weights)"
    assert lib.sr_range_wround_evals(None, None, None, None, None, 9, 99, None, 99, 7) == 1
    assert _lib.last_error() == "range_wround: null pointer (d_weights)"
    assert lib.sr_range_wround_evals_dev(None, None, wp, None, None, 9, 99, None, 99, 7, None, 0, None) == 1
    assert "null context" in _lib.last_error()
    assert lib.sr_range_wround_evals(None, None, wp, None, None, 9, 99, None, 99, 7) == 1
    assert "null context" in _lib.last_error()


# ---- the restatement the GPU tests use as their oracle ---------------------------------------------------------------------------------
def _same(a, b):
    import numpy as np

    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def test_the_pinned_vectors_regenerate_byte_for_byte():
    path = os.path.join(ROOT, "tests", "golden", "range_kats.json")
    text = open(path).read()
    assert text == R.dump_kats(), "tests/golden/range_kats.json is not what tools/model_range.py writes"
    cases = json.loads(text)["cases"]
    assert [c["ring"] for c in cases] == R.RINGS
    assert all(set(c) >= {"leading", "trailing"} and len(c["leading"]) == 2 * c["bound"] and ("weights" in c) == (c["form"] == "standard")
               for c in cases)
    assert os.path.getsize(path) < 48 << 10


PRIMES = {"goldilocks": SC.PRIMES["goldilocks"], "babybear": SC.PRIMES["babybear"]}


def _int_ops(p):
    return 0, 1, (lambda a, b: (a + b) % p), (lambda a, b: (a - b) % p), (lambda a, b: (a * b) % p)


@pytest.mark.parametrize("bound", range(2, 9))
@pytest.mark.parametrize("field", sorted(PRIMES))
def test_the_model_against_closed_forms_in_plain_integers(field, bound):
    p = PRIMES[field]
    zero, one, add, sub, mul = _int_ops(p)
    rng = random.Random("range closed %s %d" % (field, bound))
    nv = 3
    half = 1 << (nv - 1)
    weights = [rng.randrange(p) for _ in range(half)]
    # every pair (0, 1): the line through them is t, so h(t) = (sum_b w[b]) P_B(t): 0 for t < B, (t + B - 1)! / (t - B)! from B on
    for order, table in ((LEADING, [0, 1] * half), (TRAILING, [0] * half + [1] * half)):
        h = R.wround_evals([table], bound, None, weights, nv, order, zero, one, add, sub, mul)
        for t, ht in enumerate(h):
            want = 0 if t < bound else math.factorial(t + bound - 1) // math.factorial(t - bound)
            assert ht == sum(weights) * want % p, (field, bound, order, t)
    # in-range constants with the value B planted at one first-of-pair position, weights one(): h(0) = R::from((2 B - 1)!), h(1) = 0
    fact = math.factorial(2 * bound - 1) % p
    assert fact != 0
    if bound == 8:
        assert fact == (1064785271 if field == "babybear" else math.factorial(15))
    for order in (LEADING, TRAILING):
        table = [rng.randrange(-(bound - 1), bound) % p for _ in range(1 << nv)]
        h = R.wround_evals([table], bound, None, [1] * half, nv, order, zero, one, add, sub, mul)
        assert h[0] == 0 and h[1] == 0, (field, bound, order)  # an honest instance
        table[2 if order == LEADING else 1] = bound
        h = R.wround_evals([table], bound, None, [1] * half, nv, order, zero, one, add, sub, mul)
        assert h[0] == fact and h[1] == 0, (field, bound, order)


@pytest.mark.parametrize("ring", R.RINGS)
def test_bound_two_is_the_weighted_round_of_three_shifted_tables(ring):
    """model_wsumcheck on (f, f - 1, f + 1) with one term of three factors per table; full tables, since a shifted table is full"""
    zero, one, add, sub, mul, draw, _, _ = R.ring_ops(ring)
    rng = random.Random("range b2 " + ring)
    for nv, nt in ((1, 1), (2, 2)):
        full = 1 << nv
        tables = [draw(rng, full) for _ in range(nt)]
        coeffs, weights = draw(rng, nt), draw(rng, full // 2)
        shifted = [g for f in tables for g in (f, [sub(x, one) for x in f], [add(x, one) for x in f])]
        terms = [[3 * i, 3 * i + 1, 3 * i + 2] for i in range(nt)]
        for order in (LEADING, TRAILING):
            for cf in (coeffs, None):
                got = R.wround_evals(tables, 2, cf, weights, nv, order, zero, one, add, sub, mul)
                assert _same(got, W.wround_evals(shifted, terms, cf, weights, nv, order, zero, one, add, sub, mul)), (ring, nv, order)


@pytest.mark.parametrize("ring", ["goldilocks", "frog16"])
def test_the_norm_check_model_keeps_the_round_identity(ring):
    """s_1(0) + s_1(1) is the claim of round 1: zero for an honest witness; the final values and eq(z, r) give eq(z, r) g(r)"""
    zero, one, add, sub, mul, draw, _, _ = R.ring_ops(ring)
    rng = random.Random("range eq " + ring)
    nv, bound = 2, 2
    consts = [R.from_int(j, zero, one, add, sub) for j in (-1, 0, 1)]
    tables = [[consts[rng.randrange(3)] for _ in range(1 << nv)] for _ in range(2)]
    z, rs, coeffs = draw(rng, nv), draw(rng, nv), draw(rng, 2)
    for order in (LEADING, TRAILING):
        msgs, finals, eq_r = R.eq_sumcheck(tables, bound, coeffs, z, rs, order, zero, one, add, sub, mul)
        assert len(msgs) == nv and all(len(m) == 2 * bound + 1 for m in msgs)
        assert _same([add(msgs[0][0], msgs[0][1])], [zero])
        g = zero
        for c, f in zip(coeffs, finals):
            g = add(g, mul(c, R.range_poly(f, bound, zero, one, add, sub, mul)))
        # the final values are those of the tables at the challenges: a round over constant lines with the weight eq(z, r) restates
        # eq(z, r) g(r)
        last = R.wround_evals([[f] * 2 for f in finals], bound, coeffs, [eq_r], 1, order, zero, one, add, sub, mul)
        assert _same([last[0]], [mul(eq_r, g)])
