"""CPU checks of the sum-check round entry points (include/stark_rings_hip.h: sr_mle_round_plan, sr_mle_round_evals[_dev]): the
exports, the plan arithmetic for every ring, the refusals that need no context (the others need one and live in
tests/test_sumcheck_gpu.py), the absence of a CPU fallback, and the pure-Python restatement (tools/model_sumcheck.py, the oracle of
the GPU tests) against the sum-check identities and the pinned vectors of tests/golden/sumcheck_kats.json."""
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

NEW = ("sr_mle_round_plan", "sr_mle_round_evals_dev", "sr_mle_round_evals")
LEADING, TRAILING, ROUND_SUM = 0, 1, 2
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "sumcheck_kats.json")))


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
    assert re.search(r"SR_MLE_ROUND_SUM\s*=\s*2", header)
    assert re.search(r"#define\s+SR_MLE_ROUND_MAX_TABLES\s+4\b", header)
    import stark_rings_amd

    assert stark_rings_amd.MLE_ROUND_SUM == 2


def _plan(ring, k, nv, nt, mode):
    lib = _lib.load()
    work, launches = ctypes.c_size_t(1 << 60), ctypes.c_int(-1)
    rc = lib.sr_mle_round_plan(ring, k, nv, nt, mode, ctypes.byref(work), ctypes.byref(launches))
    return rc, work.value, launches.value


@pytest.mark.parametrize("ring,k", [(0, 0), (0, 6), (0, 10), (0, 16), (1, 5), (1, 16), (2, 4), (2, 12), (3, 0), (4, 0), (5, 0)])
def test_plan_bounds_for_every_ring_size_table_count_and_mode(ring, k):
    max_groups = int(re.search(r"#define\s+SR_MLE_ROUND_MAX_GROUPS\s+(\d+)", _header()).group(1))
    split = single = 0
    for mode in (LEADING, TRAILING, ROUND_SUM):
        for nv in range(25):
            for nt in (1, 2, 3, 4):
                rc, work, launches = _plan(ring, k, nv, nt, mode)
                where = "ring %d k %d nv %d tables %d mode %d: work %d launches %d" % (ring, k, nv, nt, mode, work, launches)
                if nv == 0 and mode != ROUND_SUM:
                    assert rc == 1 and "num_vars >= 1" in _lib.last_error(), where
                    continue
                assert rc == 0, where
                assert launches >= 1, where
                assert (work == 0) == (launches == 1), where
                assert work <= max_groups * (nt + 1), where
                if mode == ROUND_SUM:
                    assert launches <= 2 and work <= max_groups, where
                if ring <= 1:  # the one-limb fields read every table once: one pass over the tables, then the sum of the partial elements
                    assert launches <= 2, where
                split += work > 0
                single += work == 0
    assert split and single


def test_plan_depends_on_the_shape_only_and_needs_no_device():
    """pure host arithmetic: the same answer every time, with no context anywhere in sight"""
    assert _plan(0, 10, 20, 2, LEADING) == _plan(0, 10, 20, 2, LEADING)
    assert _plan(0, 10, 20, 2, LEADING) == _plan(0, 10, 20, 2, TRAILING)
    rc, work, launches = _plan(0, 10, 20, 2, LEADING)
    assert (rc, launches) == (0, 2) and work % 3 == 0 and work > 0
    assert _plan(0, 16, 4, 3, LEADING) == (0, 0, 1)


def test_plan_refuses_bad_arguments_and_names_the_reason():
    lib = _lib.load()
    work, launches = ctypes.c_size_t(), ctypes.c_int()
    for args, msg in (((0, 10, 4, 0, LEADING), "n_tables must be 1 .. 4"), ((0, 10, 4, 5, LEADING), "n_tables must be 1 .. 4"),
                      ((0, 10, 4, 2, 3), "unknown mode"), ((0, 10, 4, 2, -1), "unknown mode"),
                      ((0, 10, 48, 2, LEADING), "num_vars must be below 48"), ((0, 10, 0, 2, LEADING), "num_vars >= 1"),
                      ((0, 10, 0, 2, TRAILING), "num_vars >= 1"), ((6, 0, 4, 2, LEADING), "unknown ring"),
                      ((0, 25, 4, 2, LEADING), "log2_degree")):
        assert lib.sr_mle_round_plan(*args, ctypes.byref(work), ctypes.byref(launches)) == 1, args
        assert msg in _lib.last_error(), (args, _lib.last_error())
    assert lib.sr_mle_round_plan(0, 10, 4, 2, LEADING, None, ctypes.byref(launches)) == 1 and "null" in _lib.last_error()
    assert lib.sr_mle_round_plan(0, 10, 4, 2, LEADING, ctypes.byref(work), None) == 1 and "null" in _lib.last_error()
    assert lib.sr_mle_round_plan(0, 10, 0, 2, ROUND_SUM, ctypes.byref(work), ctypes.byref(launches)) == 0


def test_entry_points_refuse_a_null_context_before_anything_else():
    lib = _lib.load()
    buf = np.zeros(16, dtype=np.uint64)
    # every other argument is bad as well: the context is looked at first
    assert lib.sr_mle_round_evals(None, None, None, None, 9, 99, 7) == 1 and "null context" in _lib.last_error()
    assert lib.sr_mle_round_evals_dev(None, None, None, None, 9, 99, 7, None, 0, None) == 1 and "null context" in _lib.last_error()
    ptrs, sizes = (ctypes.c_void_p * 1)(buf.ctypes.data), (ctypes.c_size_t * 1)(1)
    assert lib.sr_mle_round_evals(None, buf.ctypes.data_as(_lib.u64p), ptrs, sizes, 1, 1, LEADING) == 1 and "null context" in _lib.last_error()


def test_no_cpu_fallback_for_the_round_calls():
    """Without a HIP device there is no context, hence no message: the host-pointer call cannot quietly compute on the CPU."""
    try:
        import torch

        if torch.cuda.is_available():
            pytest.skip("a HIP device is present")
    except ImportError:
        pass
    from stark_rings_amd import CyclotomicRing, RingError

    with pytest.raises(RingError, match="no HIP device|no CPU fallback"):
        ring = CyclotomicRing("goldilocks", 6)
        ring.mle_round_evals([np.zeros(4 << 6, dtype=np.uint64)] * 2, 2)


# ---- the restatement the GPU tests use as their oracle, pinned by the sum-check identities on Python integers -------------------------
def _int_ops(p):
    return (lambda a, b: (a + b) % p), (lambda a, b: (a - b) % p), (lambda r, a: r * a % p)


@pytest.mark.parametrize("field", ["goldilocks", "babybear", "stark"])
@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_model_round_messages_satisfy_the_sum_check_identities(field, d):
    p = SC.PRIMES[field]
    add, sub, mul = _int_ops(p)
    rng = random.Random("%s %d" % (field, d))
    for nv in (1, 2, 4):
        full = 1 << nv
        tables = [[rng.choice((0, 1, p - 1, rng.randrange(p))) for _ in range(rng.choice((full, full, full - 1, 1)))] for _ in range(d)]
        padded = [M.pad(f, nv, 0) for f in tables]
        claim = SC.product_sum(padded, 0, add, mul)
        for order in (LEADING, TRAILING):
            msg = SC.round_evals(tables, nv, order, 0, 1, add, sub, mul)
            assert len(msg) == d + 1
            assert (msg[0] + msg[1]) % p == claim
            r = rng.randrange(p)
            folded = [M.fold(f, nv, [r], order, add, sub, mul) for f in padded]
            assert SC.lagrange_at(msg, r, p) == SC.product_sum(folded, 0, add, mul)
            for t in range(d + 1):  # the points themselves
                assert SC.lagrange_at(msg, t, p) == msg[t]


def test_model_p0_plus_p1_is_the_sum_on_slot_products_too():
    """the identity that needs no interpolation, on a ring whose product is not slot-wise: Z_p[X] / (X^2 - 3)"""
    p = 97
    add = lambda a, b: ((a[0] + b[0]) % p, (a[1] + b[1]) % p)  # noqa: E731
    sub = lambda a, b: ((a[0] - b[0]) % p, (a[1] - b[1]) % p)  # noqa: E731
    mul = lambda r, a: ((r[0] * a[0] + 3 * r[1] * a[1]) % p, (r[0] * a[1] + r[1] * a[0]) % p)  # noqa: E731
    rng = random.Random(5)
    for d in (1, 2, 3, 4):
        tables = [[(rng.randrange(p), rng.randrange(p)) for _ in range(8)] for _ in range(d)]
        claim = SC.product_sum(tables, (0, 0), add, mul)
        for order in (LEADING, TRAILING):
            msg = SC.round_evals(tables, 3, order, (0, 0), (1, 0), add, sub, mul)
            assert add(msg[0], msg[1]) == claim


def test_model_reproduces_the_pinned_vectors():
    assert KATS == SC.make_kats(), "tests/golden/sumcheck_kats.json is not what tools/model_sumcheck.py writes"
    seen = set()
    for case in KATS["cases"]:
        p = SC.PRIMES[case["ring"]]
        add, sub, mul = SC.vec_ops(p)
        dr = 1 << case["log2_degree"]
        zero, one = (0,) * dr, (1,) * dr
        tables = [[tuple(e) for e in f] for f in case["tables"]]
        assert [len(f) for f in tables] == case["n_evals"]
        nv = case["num_vars"]
        assert [list(e) for e in SC.round_evals(tables, nv, LEADING, zero, one, add, sub, mul)] == case["leading"]
        assert [list(e) for e in SC.round_evals(tables, nv, TRAILING, zero, one, add, sub, mul)] == case["trailing"]
        assert list(SC.product_sum([M.pad(f, nv, zero) for f in tables], zero, add, mul)) == case["sum"]
        seen.add((case["ring"], len(tables), min(case["n_evals"]) < 1 << nv))
    assert seen == {(r, d, True) for r in ("goldilocks", "babybear", "stark") for d in (1, 2, 3, 4)}
