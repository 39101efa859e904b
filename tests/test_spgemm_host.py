"""CPU checks of the sparse-matrix entry points (include/stark_rings_hip.h: sr_sparse_transpose_pattern, sr_spgemm_pattern,
sr_spgemm_plan and the device calls' exports): the pattern routines against the pure-Python restatement
(tools/model_sparse_matrix.py, the oracle of tests/test_spgemm_gpu.py), every SR_E_INVALID case of the host routines, the plan
arithmetic for every ring, and the model itself against dense products over BabyBear integers."""
import ctypes
import os
import random
import re
import sys

import numpy as np
import pytest

from stark_rings_amd import _lib, rings
from stark_rings_amd.rings import RingError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import model_sparse_matrix as M  # noqa: E402

NEW = ("sr_sparse_transpose_pattern", "sr_spgemm_pattern", "sr_spgemm_plan", "sr_gather_batch_dev", "sr_transpose_dev", "sr_spgemm_ntt_dev",
       "sr_spgemm_dead_count", "sr_sparse_transpose", "sr_transpose", "sr_spgemm_ntt")
RINGS = [(0, 10), (0, 0), (0, 16), (1, 5), (2, 4), (3, 0), (4, 0), (5, 0)]
P = 2013265921
ADD, MUL, IS_ZERO = (lambda a, b: (a + b) % P), (lambda a, b: a * b % P), (lambda a: a == 0)


def test_header_library_and_ctypes_table_carry_the_new_names():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "stark_rings_hip.h")).read()
    declared = set(re.findall(r"\b(sr_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared, "%s is not declared in the header" % name
        assert name in _lib.SYMBOLS, "%s is missing from _lib.SYMBOLS" % name
        assert hasattr(lib, name), "the library does not export %s" % name
    import stark_rings_amd

    assert hasattr(stark_rings_amd, "SparseMatrixNTT")
    for name in ("sparse_transpose_pattern", "gather_dev", "transpose_dev", "transpose", "spgemm_pattern", "spgemm_plan", "spgemm_ntt_dev",
                 "spgemm_dead_count", "spgemm_ntt"):
        assert hasattr(stark_rings_amd.CyclotomicRing, name), name


def _pattern(rng, nrows, ncols, density, sort=True):
    cols, row_ptr = [], [0]
    for _ in range(nrows):
        row = [c for c in range(ncols) if rng.random() < density]
        if not sort:
            rng.shuffle(row)
        cols += row
        row_ptr.append(len(cols))
    return cols, row_ptr


def _lists(arrays):
    return tuple([int(x) for x in a] for a in arrays)


def test_transpose_pattern_matches_the_model():
    rng = random.Random(1)
    for nrows, ncols, density, sort in ((5, 7, 0.4, True), (9, 2, 0.5, True), (1, 1, 1.0, True), (4, 0, 0.0, True), (0, 3, 0.0, True),
                                        (6, 6, 0.0, True), (8, 5, 0.6, False), (30, 30, 0.1, False), (3, 9, 1.0, False)):
        cols, row_ptr = _pattern(rng, nrows, ncols, density, sort)
        got = _lists(rings.sparse_transpose_pattern(cols, row_ptr, nrows, ncols))
        assert got == M.transpose_pattern(cols, row_ptr, nrows, ncols), (nrows, ncols, density, sort)
        t_row_ptr, t_cols, perm = got
        # stable: within a row of the transpose the original rows ascend, and ties (none in a valid matrix) keep input order
        for c in range(ncols):
            seg = t_cols[t_row_ptr[c]:t_row_ptr[c + 1]]
            assert seg == sorted(seg)
        assert sorted(perm) == list(range(len(cols)))
    # empty rows and empty columns, explicitly
    cols, row_ptr = [2, 0, 2], [0, 1, 1, 3, 3]
    assert _lists(rings.sparse_transpose_pattern(cols, row_ptr, 4, 4)) == ([0, 1, 1, 3, 3], [2, 0, 2], [1, 0, 2])


def test_transposing_twice_returns_a_sorted_input():
    rng = random.Random(2)
    for nrows, ncols in ((5, 7), (9, 9), (1, 4), (6, 1)):
        cols, row_ptr = _pattern(rng, nrows, ncols, 0.4)
        t_row_ptr, t_cols, perm = rings.sparse_transpose_pattern(cols, row_ptr, nrows, ncols)
        back = _lists(rings.sparse_transpose_pattern(t_cols, t_row_ptr, ncols, nrows))
        assert back[0] == row_ptr and back[1] == cols
        assert [int(perm[q]) for q in back[2]] == list(range(len(cols)))


def _raw_transpose(cols, row_ptr, nrows, ncols, null=None):
    c, r = np.array(cols + [0], dtype=np.uint32), np.array(row_ptr, dtype=np.uint64)
    out = [np.zeros(ncols + 2, dtype=np.uint64), np.zeros(len(cols) + 1, dtype=np.uint32), np.zeros(len(cols) + 1, dtype=np.uint32)]
    args = [c.ctypes.data, r.ctypes.data, nrows, ncols] + [o.ctypes.data for o in out]
    if null is not None:
        args[null] = None
    return _lib.load().sr_sparse_transpose_pattern(*args)


def test_transpose_pattern_refuses_bad_input():
    assert _raw_transpose([0, 1], [0, 1, 2], 2, 2) == 0
    assert _raw_transpose([0, 2], [0, 1, 2], 2, 2) == 1 and "out of range" in _lib.last_error()      # the reference panics there
    assert _raw_transpose([0], [0, 1], 1, 0) == 1                                                     # any column with ncols == 0
    assert _raw_transpose([0, 1], [0, 2, 1], 2, 2) == 1 and "monotone" in _lib.last_error()
    assert _raw_transpose([0, 1], [1, 1, 2], 2, 2) == 1
    for null in (0, 1, 4, 5, 6):
        assert _raw_transpose([0, 1], [0, 1, 2], 2, 2, null=null) == 1 and "null" in _lib.last_error(), null
    assert _raw_transpose([], [0, 1 << 32], 1, 2) == 1 and "2^32" in _lib.last_error()              # refused before anything is read
    with pytest.raises(RingError):
        rings.sparse_transpose_pattern([0], [0, 1, 1], 1, 1)                                          # row_ptr length


CASES = [(5, 9, 5, 0.3, 0.3), (9, 5, 9, 0.5, 0.2), (1, 2, 1, 1.0, 1.0), (2, 9, 2, 0.1, 0.1), (5, 5, 5, 0.0, 0.5), (5, 5, 5, 0.5, 0.0),
         (1, 300, 1, 1.0, 1.0), (9, 1, 9, 0.5, 0.5), (0, 3, 2, 0.0, 0.5), (3, 0, 2, 0.0, 0.0), (3, 2, 0, 0.5, 0.0), (40, 30, 50, 0.1, 0.1)]


@pytest.mark.parametrize("n,m,p,da,db", CASES)
def test_spgemm_pattern_matches_the_model_and_its_own_count(n, m, p, da, db):
    rng = random.Random(n * 1000 + m * 10 + p)
    a_cols, a_ptr = _pattern(rng, n, m, da)
    b_cols, b_ptr = _pattern(rng, m, p, db)
    want = M.structural_product(a_cols, a_ptr, n, m, b_cols, b_ptr, p)
    got = _lists(rings.spgemm_pattern(a_cols, a_ptr, n, m, b_cols, b_ptr, p))
    assert got == want
    assert rings.spgemm_pattern(a_cols, a_ptr, n, m, b_cols, b_ptr, p, count_only=True) == (len(want[1]), len(want[3]))
    out_row_ptr, out_cols, pair_ptr, pair_a, pair_b = got
    assert all(pair_ptr[e + 1] > pair_ptr[e] for e in range(len(out_cols)))           # empty intersections produce no entry
    for i in range(n):
        seg = out_cols[out_row_ptr[i]:out_row_ptr[i + 1]]
        assert seg == sorted(set(seg))
    for e in range(len(out_cols)):                                                     # pairs ascend in k and meet in it
        ks = [a_cols[t] for t in pair_a[pair_ptr[e]:pair_ptr[e + 1]]]
        assert ks == sorted(set(ks))
        for ta, tb in zip(pair_a[pair_ptr[e]:pair_ptr[e + 1]], pair_b[pair_ptr[e]:pair_ptr[e + 1]]):
            assert b_ptr[a_cols[ta]] <= tb < b_ptr[a_cols[ta] + 1] and b_cols[tb] == out_cols[e]


def test_spgemm_pattern_of_disjoint_index_lists_is_empty():
    # A uses k = 0, 1; B stores nothing in rows 0, 1
    got = _lists(rings.spgemm_pattern([0, 1, 1], [0, 2, 3], 2, 4, [0, 1, 0], [0, 0, 0, 2, 3], 2))
    assert got == ([0, 0, 0], [], [0], [], [])


def test_spgemm_pattern_refuses_bad_input():
    ok = ([0, 1], [0, 2], 1, 2, [0, 0], [0, 1, 2], 1)
    assert _lists(rings.spgemm_pattern(*ok)) == ([0, 1], [0], [0, 2], [0, 1], [0, 1])
    for bad, word in ((([1, 0], [0, 2], 1, 2, [0, 0], [0, 1, 2], 1), "ascend"),        # A unsorted
                      (([1, 1], [0, 2], 1, 2, [0, 0], [0, 1, 2], 1), "ascend"),        # A duplicate
                      (([0, 1], [0, 2], 1, 2, [1, 0], [0, 2, 2], 2), "ascend"),        # B unsorted
                      (([0, 1], [0, 2], 1, 2, [1, 1], [0, 2, 2], 2), "ascend"),        # B duplicate
                      (([0, 2], [0, 2], 1, 2, [0, 0], [0, 1, 2], 1), "out of range"),  # a column of A >= m
                      (([0, 1], [0, 2], 1, 2, [0, 1], [0, 1, 2], 1), "out of range"),  # a column of B >= p
                      (([0, 1], [2, 2], 1, 2, [0, 0], [0, 1, 2], 1), "row_ptr"),
                      (([0, 1], [0, 2], 1, 2, [0, 0], [0, 2, 1], 1), "row_ptr")):
        with pytest.raises(RingError, match=word):
            rings.spgemm_pattern(*bad)
    with pytest.raises(RingError):                                                     # the shape mismatch is the caller's: B has m rows
        rings.spgemm_pattern([0, 1], [0, 2], 1, 2, [0], [0, 1], 1)
    # some output arrays but not all
    lib, z = _lib.load(), np.zeros(8, dtype=np.uint64)
    a_c, a_p = np.array([0, 1], dtype=np.uint32), np.array([0, 2], dtype=np.uint64)
    b_c, b_p = np.array([0, 0], dtype=np.uint32), np.array([0, 1, 2], dtype=np.uint64)
    no, npairs = ctypes.c_size_t(), ctypes.c_size_t()
    head = (a_c.ctypes.data, a_p.ctypes.data, 1, 2, b_c.ctypes.data, b_p.ctypes.data, 1)
    assert lib.sr_spgemm_pattern(*head, z.ctypes.data, None, None, None, None, ctypes.byref(no), ctypes.byref(npairs)) == 1
    assert lib.sr_spgemm_pattern(*head, z.ctypes.data, None, z.ctypes.data, None, None, ctypes.byref(no), ctypes.byref(npairs)) == 1
    assert lib.sr_spgemm_pattern(*head, None, None, None, None, None, None, ctypes.byref(npairs)) == 1


@pytest.mark.parametrize("ring,k", RINGS)
def test_spgemm_plan_arithmetic(ring, k):
    """no span split: never a workspace; two launches (numeric kernel, dead count) whenever there is an entry; the grid of one launch
    is n_out workgroups per 256 slots (power-of-two rings) or per element (slot rings)"""
    chunks = max(1, (1 << k) // 256) if ring <= 2 else 1
    for n_out, n_pairs in ((0, 0), (1, 1), (1, 300), (1000, 5000), (0xFFFFFF // chunks, 1 << 30)):
        assert rings.spgemm_plan(ring, k, n_out, n_pairs) == (0, 2 if n_out else 0)
    with pytest.raises(RingError, match="grid"):
        rings.spgemm_plan(ring, k, 0xFFFFFF // chunks + 1, 1)


def test_spgemm_plan_refuses_bad_arguments():
    f, w, l = _lib.load().sr_spgemm_plan, ctypes.c_size_t(), ctypes.c_int()
    assert f(-1, 4, 2, 2, ctypes.byref(w), ctypes.byref(l)) == 1
    assert f(6, 4, 2, 2, ctypes.byref(w), ctypes.byref(l)) == 1
    assert f(0, 25, 2, 2, ctypes.byref(w), ctypes.byref(l)) == 1
    assert f(3, 25, 2, 2, ctypes.byref(w), ctypes.byref(l)) == 0
    assert f(0, 4, 2, 2, None, ctypes.byref(l)) == 1
    assert f(0, 4, 2, 2, ctypes.byref(w), None) == 1


# ---- the model itself, over BabyBear integers ------------------------------------------------------------------------------------
def _matrix(rng, nrows, ncols, density, values):
    return M.SparseMatrix(nrows, ncols, [[(rng.choice(values), c) for c in range(ncols) if rng.random() < density] for _ in range(nrows)])


def _dense_mul(a, b, n, m, p):
    return [[sum(a[i][k] * b[k][j] for k in range(m)) % P for j in range(p)] for i in range(n)]


def test_model_product_agrees_with_the_dense_product_and_stores_exactly_the_live_entries():
    rng = random.Random(7)
    # stored zeros make products zero; 1 and P - 1 make sums of non-zero products zero
    values = [0, 1, P - 1, 1, P - 1, 5]
    seen_zero_product = seen_zero_sum = False
    for n, m, p in ((5, 9, 5), (2, 2, 2), (9, 5, 1), (1, 9, 9)):
        for _ in range(20):
            a, b = _matrix(rng, n, m, 0.6, values), _matrix(rng, m, p, 0.6, values)
            c = a.checked_mul_mat(b, ADD, MUL, IS_ZERO)
            assert c.to_dense(0) == _dense_mul(a.to_dense(0), b.to_dense(0), n, m, p)
            da, db = {(i, k): v for i, r in enumerate(a.coeffs) for v, k in r}, {(k, j): v for k, r in enumerate(b.coeffs) for v, j in r}
            for i in range(n):
                stored = {j: v for v, j in c.coeffs[i]}
                for j in range(p):
                    prods = [da[i, k] * db[k, j] % P for k in range(m) if (i, k) in da and (k, j) in db]
                    assert (j in stored) == any(prods), (i, j)
                    seen_zero_product |= 0 in prods
                    seen_zero_sum |= j in stored and stored[j] == 0
                assert [j for _, j in c.coeffs[i]] == sorted(stored)
            # the structural pattern plus the live flags is the same matrix
            av, ac, ap = a.csr()
            bv, bc, bp = b.csr()
            pat = M.structural_product(ac, ap, n, m, bc, bp, p)
            vals, live = M.product_by_pairs(pat, av, bv, ADD, MUL, IS_ZERO, 0)
            kept = [[(vals[e], pat[1][e]) for e in range(pat[0][i], pat[0][i + 1]) if live[e]] for i in range(n)]
            assert kept == c.coeffs
    assert seen_zero_product and seen_zero_sum
    assert M.SparseMatrix(2, 3, [[], []]).checked_mul_mat(M.SparseMatrix(2, 2, [[], []]), ADD, MUL, IS_ZERO) is None


def test_model_transpose_from_dense_and_to_dense():
    rng = random.Random(8)
    a = _matrix(rng, 5, 7, 0.5, [1, 2, 3])
    d = a.to_dense(0)
    assert a.transpose().to_dense(0) == [[d[i][j] for i in range(5)] for j in range(7)] == M.transpose_dense(d, 0)
    assert M.SparseMatrix.from_dense(d, IS_ZERO).coeffs == a.coeffs
    assert a.transpose().transpose().coeffs == a.coeffs
    assert M.transpose_dense([[1, 2, 3], [4]], 0) == [[1, 4], [2, 0], [3, 0]]
