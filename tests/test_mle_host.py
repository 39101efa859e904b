"""CPU checks of the dense multilinear-extension entry points (include/stark_rings_hip.h: sr_mle_plan, sr_mle_fix_variables*,
sr_mul_elem_add_batch*): the exports, the plan arithmetic for every ring, the argument checks, the absence of a CPU fallback, and
the pure-Python restatement of both fold orders (tools/model_mle.py, the oracle of tests/test_mle_gpu.py) against the closed form."""
import ctypes
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

NEW = ("sr_mle_plan", "sr_mle_fix_variables_dev", "sr_mle_fix_variables", "sr_mul_elem_add_batch_dev", "sr_mul_elem_add_batch")
LEADING, TRAILING = 0, 1


def test_header_library_and_ctypes_table_carry_the_new_names():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "stark_rings_hip.h")).read()
    declared = set(re.findall(r"\b(sr_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared, "%s is not declared in the header" % name
        assert name in _lib.SYMBOLS, "%s is missing from _lib.SYMBOLS" % name
        assert hasattr(lib, name), "the library does not export %s" % name
    assert re.search(r"SR_MLE_LEADING\s*=\s*0", header) and re.search(r"SR_MLE_TRAILING\s*=\s*1", header)


def _plan(ring, k, nv, nf, order):
    lib = _lib.load()
    work, launches = ctypes.c_size_t(1 << 60), ctypes.c_int(-1)
    rc = lib.sr_mle_plan(ring, k, nv, nf, order, ctypes.byref(work), ctypes.byref(launches))
    return rc, work.value, launches.value


@pytest.mark.parametrize("ring,k", [(0, 10), (1, 16), (2, 12), (3, 0), (4, 0), (5, 0)])
def test_plan_bounds_for_every_ring_size_and_order(ring, k):
    for order in (LEADING, TRAILING):
        for nv in range(25):
            for nf in range(nv + 1):
                rc, work, launches = _plan(ring, k, nv, nf, order)
                where = "ring %d nv %d n_fixed %d order %d: work %d launches %d" % (ring, nv, nf, order, work, launches)
                assert rc == 0, where
                assert 4 * work <= 3 * (1 << nv), where
                if launches <= 1:
                    assert work == 0, where
                if order == TRAILING:
                    assert 2 * work <= 1 << nv, where
                assert launches >= -(-nf // 3), where
                if nf > 0:
                    assert 1 <= launches <= nf, where


def test_plan_refuses_bad_arguments():
    lib = _lib.load()
    work, launches = ctypes.c_size_t(), ctypes.c_int()
    for args, msg in (((0, 10, 4, 5, LEADING), "n_fixed exceeds num_vars"), ((0, 10, 4, 2, 2), "unknown order"),
                      ((0, 10, 48, 2, LEADING), "num_vars must be below 48"), ((6, 0, 4, 2, LEADING), "unknown ring"),
                      ((0, 25, 4, 2, LEADING), "log2_degree")):
        assert lib.sr_mle_plan(*args, ctypes.byref(work), ctypes.byref(launches)) == 1, args
        assert msg in _lib.last_error(), (args, _lib.last_error())
    assert lib.sr_mle_plan(0, 10, 4, 2, LEADING, None, ctypes.byref(launches)) == 1
    assert "null" in _lib.last_error()


def test_entry_points_refuse_a_null_context_before_anything_else():
    lib = _lib.load()
    buf = np.zeros(16, dtype=np.uint64)
    p = buf.ctypes.data_as(_lib.u64p)
    assert lib.sr_mle_fix_variables(None, p, p, 1, 1, p, 1, LEADING) == 1 and "null context" in _lib.last_error()
    assert lib.sr_mle_fix_variables_dev(None, buf.ctypes.data, buf.ctypes.data, 1, 1, buf.ctypes.data, 1, LEADING, None, 0, None) == 1
    assert "null context" in _lib.last_error()
    assert lib.sr_mul_elem_add_batch(None, p, p, p, 1) == 1 and "null context" in _lib.last_error()
    assert lib.sr_mul_elem_add_batch_dev(None, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, 1, None) == 1
    assert "null context" in _lib.last_error()


def test_no_cpu_fallback_for_the_mle_calls():
    """Without a HIP device there is no context, hence no fold: the host-pointer call cannot quietly compute on the CPU."""
    try:
        import torch

        if torch.cuda.is_available():
            pytest.skip("a HIP device is present")
    except ImportError:
        pass
    from stark_rings_amd import CyclotomicRing, RingError

    with pytest.raises(RingError, match="no HIP device|no CPU fallback"):
        ring = CyclotomicRing("goldilocks", 6)
        ring.mle_fix_variables(np.zeros(4 << 6, dtype=np.uint64), 2, np.zeros(2 << 6, dtype=np.uint64))


# ---- the restatement the GPU tests use as their oracle, pinned on a small prime field ---------------------------------------------
P = 2013265921


def _ops():
    return (lambda a, b: (a + b) % P), (lambda a, b: (a - b) % P), (lambda r, a: r * a % P)


@pytest.mark.parametrize("nv", [0, 1, 2, 3, 5])
def test_python_restatement_of_both_orders_agrees_with_the_closed_form(nv):
    rng = random.Random(1000 + nv)
    add, sub, mul = _ops()
    for n_evals in sorted({0, 1, (1 << nv) - 1 if nv else 1, 1 << nv}):
        table = M.pad([rng.randrange(P) for _ in range(n_evals)], nv, 0)
        for nf in range(nv + 1):
            point = [rng.choice((0, 1, P - 1, rng.randrange(P))) for _ in range(nf)]
            assert M.fold(table, nv, point, M.LEADING, add, sub, mul) == M.eq_closed_form(table, nv, point, 0, P)
            assert M.fold(table, nv, point, M.TRAILING, add, sub, mul) == M.eq_closed_form(table, nv, point, nv - nf, P)


def test_python_restatement_splits_and_boolean_points():
    rng = random.Random(7)
    add, sub, mul = _ops()
    nv = 6
    table = [rng.randrange(P) for _ in range(1 << nv)]
    point = [rng.randrange(P) for _ in range(nv)]
    whole = M.fold(table, nv, point, M.LEADING, add, sub, mul)
    for j in range(nv + 1):
        first = M.fold(table, nv, point[:j], M.LEADING, add, sub, mul)
        assert M.fold(first, nv - j, point[j:], M.LEADING, add, sub, mul) == whole
        last = M.fold(table, nv, point[j:], M.TRAILING, add, sub, mul)
        assert M.fold(last, j, point[:j], M.TRAILING, add, sub, mul) == whole
    for index in (0, 1, 37, (1 << nv) - 1):
        bits = [(index >> i) & 1 for i in range(nv)]
        assert M.fold(table, nv, bits, M.LEADING, add, sub, mul) == [table[index]]
        assert M.fold(table, nv, bits, M.TRAILING, add, sub, mul) == [table[index]]
