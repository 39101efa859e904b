"""Host-only checks of the weighted sum-check rounds with integer columns (sr_vpoly_iwround_*): the plain-integer model
tools/model_isumcheck.py against tools/model_wsumcheck.py over tables expanded in the model, the pinned vectors, the plan
(sr_vpoly_iwround_plan is host arithmetic and needs no context) with its refusals, and the argument checks of the Python layer.  No GPU.
"""
import ctypes
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
import model_isumcheck as IS  # noqa: E402
import model_wsumcheck as W  # noqa: E402

NEW = ("sr_vpoly_iwround_plan", "sr_vpoly_iwround_evals_dev", "sr_vpoly_iwround_evals", "sr_vpoly_iwround_fold_evals_dev",
       "sr_vpoly_iwround_fold_evals")
LEADING, TRAILING, ROUND_SUM = 0, 1, 2
SHAPES = [(0, 0), (0, 6), (0, 16), (1, 5), (2, 4), (2, 12), (3, 0), (4, 0), (5, 0)]
U64 = 1 << 64


def test_header_library_and_ctypes_table_carry_the_new_names():
    lib = _lib.load()
    declared = set(re.findall(r"\b(sr_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "include", "stark_rings_hip.h")).read()))
    for name in NEW:
        assert name in declared, "%s is not declared in the header" % name
        assert name in _lib.SYMBOLS, "%s is missing from _lib.SYMBOLS" % name
        assert hasattr(lib, name), "the library does not export %s" % name


# ---- the model ------------------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    import numpy as np

    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _columns(rng, p, nv, J, shared):
    """J columns of every kind in turn: 0/1, stored and truncated with the values around p, the two progressions, uniform"""
    full, half = 1 << nv, 1 << (nv - 1)
    edge = [x % U64 for x in (p - 1, p, p + 1)] + [U64 - 1]
    kinds = [lambda: [rng.randrange(2) for _ in range(full)], lambda: (edge * full)[:full - 1], lambda: IS.Progression(U64 - full),
             lambda: [rng.randrange(U64) for _ in range(half + 1)], lambda: IS.Progression(0), lambda: [rng.randrange(U64) for _ in range(half)],
             lambda: [rng.randrange(U64)], lambda: []]
    rng.shuffle(kinds)
    cols = [kinds[j % len(kinds)]() for j in range(J)]
    if shared:
        cols[1] = cols[0]
    return cols


@pytest.mark.parametrize("order", [LEADING, TRAILING])
@pytest.mark.parametrize("sname", sorted(IS.STRUCTURES))
@pytest.mark.parametrize("ring", W.RINGS)
def test_the_model_is_the_weighted_model_over_expanded_tables(ring, sname, order):
    zero, one, add, sub, mul, draw, out, form = W.ring_ops(ring)
    base = W.SLOT_RINGS[ring][1] if ring in W.SLOT_RINGS else ring
    p = W.SLOT_PRIMES[base] if ring in W.SLOT_RINGS else W.SC.PRIMES[ring]
    K, J, terms = IS.STRUCTURES[sname]
    rng = random.Random("isumcheck host %s %s" % (ring, sname))
    for nv in (2, 3):
        full = 1 << nv
        tables = [draw(rng, n) for n in ([full, full - 1, full // 2 + 1][:K])]
        columns = _columns(rng, p, nv, J, sname == "SHARED")
        coeffs = None if sname == "MIXED" else draw(rng, len(terms))
        if sname == "PLONK":
            coeffs[3] = sub(zero, one)
        w_round, w_fold, r = draw(rng, full // 2), draw(rng, full // 4), draw(rng, 1)[0]
        dense = tables + IS.expand(columns, nv, zero, one, add)
        got = IS.iwround_evals(tables, columns, terms, coeffs, w_round, nv, order, zero, one, add, sub, mul)
        assert _same(got, W.wround_evals(dense, terms, coeffs, w_round, nv, order, zero, one, add, sub, mul)), (ring, sname, nv)
        folded, msg = IS.iwfold_round(tables, columns, terms, coeffs, w_fold, nv, r, order, zero, one, add, sub, mul)
        want_folded, want_msg = W.wfold_round(dense, terms, coeffs, w_fold, nv, r, order, zero, one, add, sub, mul)
        assert _same(msg, want_msg) and len(folded) == K + J, (ring, sname, nv)
        assert all(_same(a, b) for a, b in zip(folded, want_folded)), (ring, sname, nv)


def test_the_embedding_is_the_reference_from_u64():
    """R::from(x) is x one(): doubling-and-adding agrees with x additions, and values >= p wrap"""
    import model_lincomb_index as LI

    zero, one, add, sub, mul, draw, out, form = W.ring_ops("babybear")
    p = W.SC.PRIMES["babybear"]
    for x in (0, 1, 2, 77):
        assert LI.from_u64(x, one, zero, add) == LI.from_u64_repeated(x, one, zero, add)
    assert LI.from_u64(p, one, zero, add) == zero and LI.from_u64(p + 1, one, zero, add) == one
    assert IS.expand([[p - 1, p, p + 1], IS.Progression(3)], 2, zero, one, add)[0][1] == zero


def test_the_pinned_vectors_regenerate_byte_for_byte():
    path = os.path.join(ROOT, "tests", "golden", "isumcheck_kats.json")
    assert open(path).read() == IS.dump_kats()
    assert os.path.getsize(path) < 256 * 1024


# ---- the plan -------------------------------------------------------------------------------------------------------------------------------
def _plan(ring, k, nv, K, J, n_terms, degree, order, fold):
    work, launches = ctypes.c_size_t(1 << 60), ctypes.c_int(-1)
    rc = _lib.load().sr_vpoly_iwround_plan(ring, k, nv, K, J, n_terms, degree, order, fold, ctypes.byref(work), ctypes.byref(launches))
    return rc, work.value, launches.value


def _wplan(fn, ring, k, nv, nt, n_terms, degree, order):
    work, launches = ctypes.c_size_t(1 << 60), ctypes.c_int(-1)
    rc = getattr(_lib.load(), fn)(ring, k, nv, nt, n_terms, degree, order, ctypes.byref(work), ctypes.byref(launches))
    return rc, work.value, launches.value


@pytest.mark.parametrize("ring,k", SHAPES)
def test_the_plan_is_the_weighted_plan_at_k_plus_j_slots(ring, k):
    """the records and the points per launch of sr_vpoly_wround[_fold]_plan: every kernel of csrc/sumcheck_index.hpp holds the points of
    its weighted sibling (tests/test_isumcheck_isa.py)"""
    for order in (LEADING, TRAILING):
        for nv in (1, 2, 3, 9, 14, 20, 24):
            for K, J in ((0, 1), (0, 2), (3, 1), (1, 3), (3, 5), (0, 8), (7, 1), (4, 0), (8, 0)):
                for degree in (1, 2, 3, 4):
                    assert _plan(ring, k, nv, K, J, 3, degree, order, 0) == _wplan("sr_vpoly_wround_plan", ring, k, nv, K + J, 3, degree, order)
                    if nv >= 2:
                        assert _plan(ring, k, nv, K, J, 3, degree, order, 1) == \
                            _wplan("sr_vpoly_wround_fold_plan", ring, k, nv, K + J, 3, degree, order)


def test_plan_refusals_name_their_reason():
    lib = _lib.load()
    work, launches = ctypes.c_size_t(), ctypes.c_int()
    by = ctypes.byref

    def refused(args, prefix, text):
        assert lib.sr_vpoly_iwround_plan(*args, by(work), by(launches)) == 1, args
        assert _lib.last_error().startswith(prefix) and text in _lib.last_error(), (args, _lib.last_error())

    #        ring k  nv  K  J  terms degree order fold
    refused((0, 10, 4, 2, -1, 2, 3, LEADING, 0), "vpoly_iwround: ", "n_index must be 0 .. 8")
    refused((0, 10, 4, 0, 9, 2, 3, LEADING, 1), "vpoly_iwround_fold: ", "n_index must be 0 .. 8")
    refused((0, 10, 4, 8, 1, 2, 3, LEADING, 0), "vpoly_iwround: ", "n_tables + n_index must be 1 .. 8")
    refused((0, 10, 4, -1, 2, 2, 3, LEADING, 0), "vpoly_iwround: ", "n_tables + n_index must be 1 .. 8")
    refused((0, 10, 4, 1, 8, 2, 3, LEADING, 1), "vpoly_iwround_fold: ", "n_tables + n_index must be 1 .. 8")
    refused((0, 10, 4, 2, 2, 2, 3, LEADING, 2), "vpoly_iwround: ", "fold must be 0 or 1")
    refused((0, 10, 4, 2, 2, 0, 3, LEADING, 0), "vpoly_iwround: ", "n_terms must be 1 .. 8")
    refused((0, 10, 4, 2, 2, 2, 5, LEADING, 0), "vpoly_iwround: ", "degree")
    refused((0, 10, 4, 2, 2, 2, 3, ROUND_SUM, 0), "vpoly_iwround: ", "SR_MLE_ROUND_SUM")
    refused((0, 10, 4, 2, 2, 2, 3, ROUND_SUM, 1), "vpoly_iwround_fold: ", "unknown order")
    refused((0, 10, 4, 2, 2, 2, 3, 3, 0), "vpoly_iwround: ", "unknown order")
    refused((0, 10, 0, 2, 2, 2, 3, LEADING, 0), "vpoly_iwround: ", "num_vars >= 1")
    refused((0, 10, 1, 2, 2, 2, 3, LEADING, 1), "vpoly_iwround_fold: ", "num_vars >= 2")
    refused((0, 10, 48, 2, 2, 2, 3, LEADING, 0), "vpoly_iwround: ", "num_vars must be below 48")
    refused((6, 0, 4, 2, 2, 2, 3, LEADING, 0), "", "unknown ring")
    refused((0, 25, 4, 2, 2, 2, 3, LEADING, 0), "", "log2_degree")
    # without columns the call is the weighted call, refusals included
    refused((0, 10, 4, 0, 0, 2, 3, LEADING, 0), "vpoly_wround: ", "n_tables must be 1 .. 8")
    refused((0, 10, 4, 9, 0, 2, 3, LEADING, 1), "vpoly_wround_fold: ", "n_tables must be 1 .. 8")
    assert lib.sr_vpoly_iwround_plan(0, 10, 4, 2, 2, 2, 3, LEADING, 0, None, by(launches)) == 1 and "null" in _lib.last_error()
    for ring in range(6):
        k = 4 if ring < 3 else 0
        assert lib.sr_vpoly_iwround_plan(ring, k, 1, 0, 1, 1, 1, LEADING, 0, by(work), by(launches)) == 0
        assert lib.sr_vpoly_iwround_plan(ring, k, 47, 3, 5, 5, 3, TRAILING, 1, by(work), by(launches)) == 0


def test_context_free_refusals_of_the_calls():
    """what is decided before the context is read: the counts, the null column array, the weights"""
    lib = _lib.load()
    one = ctypes.c_uint64(0)
    wp = ctypes.cast(ctypes.byref(one), ctypes.c_void_p)
    assert lib.sr_vpoly_iwround_evals_dev(None, None, None, None, None, 1, None, 9, None, 2, None, 4, 0, None, 0, None) == 1
    assert _lib.last_error() == "vpoly_iwround: n_index must be 0 .. 8"
    assert lib.sr_vpoly_iwround_evals_dev(None, None, None, None, None, 7, None, 2, None, 2, None, 4, 0, None, 0, None) == 1
    assert _lib.last_error() == "vpoly_iwround: n_tables + n_index must be 1 .. 8"
    assert lib.sr_vpoly_iwround_evals(None, None, None, None, None, 0, None, 2, None, 2, None, 4, 0) == 1
    assert _lib.last_error() == "vpoly_iwround: null pointer (columns)"
    assert lib.sr_vpoly_iwround_fold_evals_dev(None, None, None, None, None, None, None, 0, None, 2, None, 2, None, 4, None, 0, None, 0, None) == 1
    assert _lib.last_error() == "vpoly_iwround_fold: null pointer (columns)"
    from stark_rings_amd.index_columns import sr_index_column

    cols = (sr_index_column * 2)(sr_index_column(None, 0, 0), sr_index_column(None, 0, 5))
    assert lib.sr_vpoly_iwround_evals_dev(None, None, None, None, None, 0, cols, 2, None, 2, None, 4, 0, None, 0, None) == 1
    assert _lib.last_error() == "vpoly_iwround: null pointer (d_weights)"
    assert lib.sr_vpoly_iwround_fold_evals(None, None, None, None, None, None, None, 0, cols, 2, None, 2, None, 4, None, 0) == 1
    assert _lib.last_error() == "vpoly_iwround_fold: null pointer (weights)"
    assert lib.sr_vpoly_iwround_evals_dev(None, None, wp, None, None, 0, cols, 2, None, 2, None, 4, 0, None, 0, None) == 1
    assert "null context" in _lib.last_error()
    bad = (sr_index_column * 2)(sr_index_column(wp, 1, 3), sr_index_column(None, 0, 5))
    assert lib.sr_vpoly_iwround_evals_dev(None, None, wp, None, None, 0, bad, 2, None, 2, None, 4, 0, None, 0, None) == 1
    assert _lib.last_error() == "vpoly_iwround: a stored column with a non-zero start"
    bad = (sr_index_column * 2)(sr_index_column(wp, 17, 0), sr_index_column(None, 0, 5))
    assert lib.sr_vpoly_iwround_evals_dev(None, None, wp, None, None, 0, bad, 2, None, 2, None, 4, 0, None, 0, None) == 1
    assert _lib.last_error() == "vpoly_iwround: a column's n_evals exceeds 2^num_vars"
    bad = (sr_index_column * 2)(sr_index_column(None, 0, U64 - 15), sr_index_column(None, 0, 5))
    assert lib.sr_vpoly_iwround_evals_dev(None, None, wp, None, None, 0, bad, 2, None, 2, None, 4, 0, None, 0, None) == 1
    assert _lib.last_error() == "vpoly_iwround: a progression wraps past 2^64 - 1"
    ok = (sr_index_column * 2)(sr_index_column(None, 0, U64 - 16), sr_index_column(None, 0, 5))
    assert lib.sr_vpoly_iwround_evals_dev(None, None, wp, None, None, 0, ok, 2, None, 2, None, 4, 0, None, 0, None) == 1
    assert "null context" in _lib.last_error()
    # without columns: the weighted call's own words
    assert lib.sr_vpoly_iwround_evals_dev(None, None, None, None, None, 9, None, 0, None, 9, None, 99, 7, None, 0, None) == 1
    assert _lib.last_error() == "vpoly_wround: null pointer (d_weights)"


# ---- the Python layer -------------------------------------------------------------------------------------------------------------------------
def test_index_multilinear_extension_checks_its_arguments():
    import numpy as np

    from stark_rings_amd import IndexColumn, IndexMultilinearExtension, RingError

    class Ring:  # the constructor reads no context
        device = 0

    ring = Ring()
    f = IndexMultilinearExtension(ring, 5, IndexColumn(start=7))
    assert f.num_vars == 5 and len(f) == 32 and f.key() == ("progression", 7)
    assert len(IndexMultilinearExtension(ring, 0, IndexColumn(start=U64 - 1))) == 1
    with pytest.raises(RingError, match="wraps past"):
        IndexMultilinearExtension(ring, 5, IndexColumn(start=U64 - 31))
    IndexMultilinearExtension(ring, 5, IndexColumn(start=U64 - 32))
    with pytest.raises(RingError, match="num_vars"):
        IndexMultilinearExtension(ring, 48, IndexColumn(start=0))
    with pytest.raises(RingError, match="CUDA tensor"):
        IndexMultilinearExtension(ring, 5, IndexColumn(np.arange(8, dtype=np.uint64)))
    with pytest.raises(RingError, match="CUDA tensor"):
        IndexMultilinearExtension(ring, 5, np.arange(8, dtype=np.uint64))


def test_the_wrappers_check_counts_and_columns_before_the_library():
    from stark_rings_amd import IndexColumn, RingError, wsumcheck

    with pytest.raises(RingError, match="wraps past"):
        wsumcheck._iw_columns("vpoly_iwround_evals", None, [IndexColumn(start=U64 - 3)], 2, None, 0)
    with pytest.raises(RingError, match="num_vars must be below 48"):
        wsumcheck._iw_columns("vpoly_iwround_evals", None, [IndexColumn(start=0)], 48, None, 0)
    with pytest.raises(RingError, match="at most 8"):
        wsumcheck._iw_columns("vpoly_iwround_evals", None, [IndexColumn(start=j) for j in range(9)], 3, None, 0)
    cols, arr, sizes = wsumcheck._iw_columns("vpoly_iwround_evals", None, [IndexColumn(start=U64 - 4), IndexColumn(start=1)], 2, None, 0)
    assert sizes == [4, 4] and arr[0].values is None and arr[0].start == U64 - 4 and arr[1].start == 1
    with pytest.raises(RingError, match="1 .. 8 tables and columns"):
        wsumcheck._iw_slots("vpoly_iwround_evals", 5, 4)
    with pytest.raises(RingError, match="1 .. 8 tables and columns"):
        wsumcheck._iw_slots("vpoly_iwround_evals", 0, 0)
    wsumcheck._iw_slots("vpoly_iwround_evals", 0, 8)
