"""CPU checks of the symmetric-matrix entry points (include/stark_rings_hip.h: sr_gram_plan, sr_gram_ntt*, sr_symm_recompose_plan,
sr_symm_recompose*): the exports, the plan arithmetic for every ring, every SR_E_INVALID case of the two plan functions, the packed
index and the from_rows assertion of the Python mirror, and the pure-Python restatement (tools/model_symmetric.py, the oracle of
tests/test_symm_gpu.py) against closed forms built from full dense matrices."""
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
import model_symmetric as M  # noqa: E402

NEW = ("sr_gram_plan", "sr_gram_ntt_dev", "sr_gram_ntt", "sr_symm_recompose_plan", "sr_symm_recompose_dev", "sr_symm_recompose")
RINGS = [(0, 10), (0, 0), (0, 16), (1, 5), (2, 4), (3, 0), (4, 0), (5, 0)]
SIZE_MAX = (1 << 64) - 1
P = 2013265921
ADD, MUL = (lambda a, b: (a + b) % P), (lambda a, b: a * b % P)


def test_header_library_and_ctypes_table_carry_the_new_names():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "stark_rings_hip.h")).read()
    declared = set(re.findall(r"\b(sr_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared, "%s is not declared in the header" % name
        assert name in _lib.SYMBOLS, "%s is missing from _lib.SYMBOLS" % name
        assert hasattr(lib, name), "the library does not export %s" % name


def _plan(fn, ring, k, n, x):
    work, launches = ctypes.c_size_t(1 << 60), ctypes.c_int(-1)
    rc = getattr(_lib.load(), fn)(ring, k, n, x, ctypes.byref(work), ctypes.byref(launches))
    return rc, work.value, launches.value


@pytest.mark.parametrize("ring,k", RINGS)
def test_gram_plan_arithmetic(ring, k):
    """no workspace exactly where one launch suffices; a split plan asks for nsplit whole packed matrices, nsplit <= 64; n == 0
    launches nothing"""
    for n in (0, 1, 2, 3, 8, 9, 64, 65, 1000):
        packed = n * (n + 1) // 2
        for m in (0, 1, 3, 31, 32, 63, 64, 127, 128, 4096, 65536, 1 << 20):
            rc, work, launches = _plan("sr_gram_plan", ring, k, n, m)
            where = "ring %d k %d n %d m %d: work %d launches %d" % (ring, k, n, m, work, launches)
            assert rc == 0, where
            if n == 0:
                assert (work, launches) == (0, 0), where
                continue
            assert launches in (1, 2), where
            assert (work == 0) == (launches == 1), where
            if launches == 2:
                assert work % packed == 0 and 2 <= work // packed <= 64, where
                assert m // (work // packed) >= 16, where   # a span never shrinks to a handful of terms
            if m < 64:
                assert launches == 1, where
    # enough tiles to fill the chip: never split, however long the rows
    assert _plan("sr_gram_plan", ring, k, 256, 1 << 20) == (0, 0, 1)


@pytest.mark.parametrize("ring", [3, 4, 5])
def test_gram_plan_splits_two_rows_of_a_slot_ring_within_4096_columns(ring):
    found = [m for m in (1 << e for e in range(13)) if _plan("sr_gram_plan", ring, 0, 2, m)[2] == 2]
    assert found, "sr_gram_plan never splits n = 2"
    assert _plan("sr_gram_plan", ring, 0, 2, found[0] // 2)[2] == 1


@pytest.mark.parametrize("ring,k", RINGS)
def test_recompose_plan_arithmetic(ring, k):
    for n in (0, 1, 2, 5, 100):
        for d in (1, 2, 3, 8, 17):
            rc, work, launches = _plan("sr_symm_recompose_plan", ring, k, n, d)
            assert rc == 0
            assert (work, launches) == ((d * d, 2) if n else (0, 0)), (ring, k, n, d, work, launches)
            assert (work == 0) == (launches != 2)


def test_plan_functions_refuse_bad_arguments():
    lib = _lib.load()
    w, l = ctypes.c_size_t(), ctypes.c_int()
    for fn in ("sr_gram_plan", "sr_symm_recompose_plan"):
        f = getattr(lib, fn)
        assert f(-1, 4, 2, 2, ctypes.byref(w), ctypes.byref(l)) == 1, fn            # unknown ring ids
        assert f(6, 4, 2, 2, ctypes.byref(w), ctypes.byref(l)) == 1, fn
        assert f(0, -1, 2, 2, ctypes.byref(w), ctypes.byref(l)) == 1, fn            # log2_degree out of range (power-of-two rings only)
        assert f(0, 25, 2, 2, ctypes.byref(w), ctypes.byref(l)) == 1, fn
        assert f(3, 25, 2, 2, ctypes.byref(w), ctypes.byref(l)) == 0, fn
        assert f(0, 4, 2, 2, None, ctypes.byref(l)) == 1, fn                         # null result pointers
        assert f(0, 4, 2, 2, ctypes.byref(w), None) == 1, fn
        assert "null" in _lib.last_error()
    # n (n + 1) / 2 overflowing size_t
    for n in (SIZE_MAX, SIZE_MAX - 1, 1 << 33):
        assert _plan("sr_gram_plan", 3, 0, n, 1)[0] == 1, n
    # a grid past one launch's limit: n (n + 1) / 2 fits, the tiles of one launch do not
    assert _plan("sr_gram_plan", 3, 0, 1 << 20, 1)[0] == 1
    assert _plan("sr_gram_plan", 0, 16, 1 << 12, 1)[0] == 1
    # recompose: d == 0 is the reference's division by zero, whatever n
    for n in (0, 1, 7):
        assert _plan("sr_symm_recompose_plan", 0, 4, n, 0)[0] == 1
        assert "d == 0" in _lib.last_error()
    # n * d and (n d)(n d + 1) / 2 overflowing
    assert _plan("sr_symm_recompose_plan", 0, 4, 1 << 40, 1 << 40)[0] == 1
    assert _plan("sr_symm_recompose_plan", 0, 4, 1 << 20, 1 << 14)[0] == 1
    assert _plan("sr_symm_recompose_plan", 0, 4, SIZE_MAX, 1)[0] == 1
    assert _plan("sr_symm_recompose_plan", 0, 4, 1, 1 << 33)[0] == 1                 # d^2 and the packed size overflow
    assert _plan("sr_symm_recompose_plan", 3, 0, 1 << 16, 1)[0] == 1                 # one workgroup per output element: grid limit


def test_python_plan_wrappers_need_no_context():
    from stark_rings_amd import rings

    assert rings.gram_plan("goldilocks24", 0, 5, 3) == (0, 1)
    assert rings.symm_recompose_plan("stark", 4, 3, 2) == (4, 2)
    with pytest.raises(rings.RingError):
        rings.symm_recompose_plan("stark", 4, 3, 0)
    with pytest.raises(rings.RingError):
        rings.gram_plan(0, 4, -1, 3)


# ---- the Python mirror without a device: the packed index and the assertion of From<Vec<Vec<F>>> ----------------------------------
class _HostRing:
    """what SymmetricMatrixNTT needs of a ring when nothing is computed"""
    words_per_elem = 3
    device = 0

    def _batch_of(self, n):
        assert n % self.words_per_elem == 0
        return n // self.words_per_elem


def test_packed_index_at_diag_rows_and_from_rows():
    from stark_rings_amd import RingError, SymmetricMatrixNTT
    from stark_rings_amd.symmetric import packed_index

    ring, n = _HostRing(), 5
    seen = [packed_index(i, j) for i in range(n) for j in range(i + 1)]
    assert seen == list(range(n * (n + 1) // 2)), "row i holds (i, 0) .. (i, i), rows in order"
    assert all(packed_index(i, j) == packed_index(j, i) for i in range(n) for j in range(n))
    words = np.arange(n * (n + 1) // 2 * 3, dtype=np.uint64)
    mat = SymmetricMatrixNTT(ring, n, words)
    model = M.SymmetricMatrix.from_packed(n, [words[e * 3:(e + 1) * 3] for e in range(n * (n + 1) // 2)])
    assert mat.size() == n == model.size()
    for i in range(n):
        for j in range(n):
            assert np.array_equal(mat.at(i, j), model.at(i, j)) and np.array_equal(mat.at(i, j), mat.at(j, i))
    assert all(np.array_equal(a, b) for a, b in zip(mat.diag(), model.diag()))
    assert [r.size for r in mat.rows()] == [3 * (i + 1) for i in range(n)]
    assert np.array_equal(np.concatenate(mat.rows()), words)
    again = SymmetricMatrixNTT.from_rows(ring, mat.rows())
    assert again.size() == n and np.array_equal(again.words, words)
    lists = SymmetricMatrixNTT.from_rows(ring, [[words[(i * (i + 1) // 2 + j) * 3:][:3] for j in range(i + 1)] for i in range(n)])
    assert np.array_equal(lists.words, words)
    assert SymmetricMatrixNTT.from_rows(ring, []).size() == 0
    z = SymmetricMatrixNTT.zero(ring, 4)
    assert z.size() == 4 and z.words.size == 30 and not z.words.any()
    for bad in ([words[:6]], [words[:3], words[:3]], [words[:3], words[:9]], [words[:3], words[:6], words[:6]]):
        with pytest.raises(RingError, match="wrong number of entries"):
            SymmetricMatrixNTT.from_rows(ring, bad)
        with pytest.raises(AssertionError):
            M.SymmetricMatrix([list(range(r.size // 3)) for r in bad])
    with pytest.raises(RingError):
        SymmetricMatrixNTT(ring, 3, words)
    with pytest.raises(RingError):
        mat.at(0, n)
    with pytest.raises(RingError, match="must divide"):
        mat.recompose_left_right(np.zeros(6, dtype=np.uint64))      # 2 does not divide 5: the reference's assert_eq!(and % d, 0)
    with pytest.raises(RingError, match="must divide"):
        mat.recompose_left_right(np.zeros(0, dtype=np.uint64))      # d == 0


# ---- the restatement, pinned on a small prime field ------------------------------------------------------------------------------------
def _full(mat):
    n = mat.size()
    return [[mat.at(i, j) for j in range(n)] for i in range(n)]


def _matmul(a, b):
    return [[sum(a[i][t] * b[t][j] for t in range(len(b))) % P for j in range(len(b[0]))] for i in range(len(a))]


@pytest.mark.parametrize("n,d", [(1, 1), (3, 2), (2, 3), (4, 1), (1, 4)])
def test_recompose_restatement_agrees_with_the_dense_gadget_product(n, d):
    """G = I_n (x) powers (n d x n), G^T full(M) G computed on full dense matrices"""
    rng = random.Random(100 * n + d)
    nd = n * d
    mat = M.SymmetricMatrix.from_fn(nd, lambda i, j: rng.choice((0, 1, P - 1, rng.randrange(P))))
    powers = [rng.randrange(P) for _ in range(d)]
    g = [[powers[r % d] if r // d == c else 0 for c in range(n)] for r in range(nd)]
    gt = [list(col) for col in zip(*g)]
    want = _matmul(_matmul(gt, _full(mat)), g)
    got = M.recompose_left_right_symmetric_matrix(mat, powers, ADD, MUL, 0)
    assert got.size() == n
    assert _full(got) == want
    assert all(want[i][j] == want[j][i] for i in range(n) for j in range(n))


def test_recompose_restatement_asserts_like_the_reference():
    mat = M.SymmetricMatrix.zero(5, 0)
    with pytest.raises(AssertionError):
        M.recompose_left_right_symmetric_matrix(mat, [1, 2], ADD, MUL, 0)
    with pytest.raises(ZeroDivisionError):
        M.recompose_left_right_symmetric_matrix(mat, [], ADD, MUL, 0)


@pytest.mark.parametrize("n,m", [(1, 1), (2, 3), (5, 17), (9, 1), (3, 0), (0, 4)])
def test_gram_restatement_agrees_with_a_times_its_transpose(n, m):
    rng = random.Random(10 * n + m)
    a = [rng.randrange(P) for _ in range(n * m)]
    got = M.gram(a, n, m, ADD, MUL, 0)
    rows = [a[i * m:(i + 1) * m] for i in range(n)]
    want = _matmul(rows, [list(c) for c in zip(*rows)]) if n and m else [[0] * n for _ in range(n)]
    assert got.size() == n and _full(got) == want
    assert got.packed() == [want[i][j] for i in range(n) for j in range(i + 1)]


def test_the_two_restatements_are_tied_by_the_gadget_identity():
    """recompose(gram(A), powers) == gram(B) with B[i] = sum_a powers[a] A[i d + a]: the identity tests/test_symm_gpu.py runs on the
    device"""
    rng = random.Random(5)
    n, d, m = 3, 2, 4
    a = [rng.randrange(P) for _ in range(n * d * m)]
    powers = [rng.randrange(P) for _ in range(d)]
    b = [sum(powers[q] * a[(i * d + q) * m + t] for q in range(d)) % P for i in range(n) for t in range(m)]
    lhs = M.recompose_left_right_symmetric_matrix(M.gram(a, n * d, m, ADD, MUL, 0), powers, ADD, MUL, 0)
    assert lhs.packed() == M.gram(b, n, m, ADD, MUL, 0).packed()


def test_wire_framing_round_trip_on_the_model():
    """u64 row count, then per row a u64 length and the elements; a row of the wrong length survives the round trip (the reference's
    deserialize does not run the From assertion)"""
    enc, dec = (lambda e: int(e).to_bytes(4, "little")), (lambda b: int.from_bytes(b, "little"))
    rng = random.Random(9)
    mat = M.SymmetricMatrix.from_fn(4, lambda i, j: rng.randrange(P))
    data = M.wire_frame(mat.rows(), enc)
    assert len(data) == 8 + 4 * 8 + 10 * 4
    assert data[:8] == (4).to_bytes(8, "little") and data[8:16] == (1).to_bytes(8, "little")
    assert M.wire_unframe(data, 4, dec) == mat.rows()
    assert M.SymmetricMatrix(M.wire_unframe(data, 4, dec)).packed() == mat.packed()
    ragged = [[1], [2, 3, 4], []]
    back = M.wire_unframe(M.wire_frame(ragged, enc), 4, dec)
    assert back == ragged
    assert M.SymmetricMatrix(back, checked=False).rows() == ragged
    with pytest.raises(AssertionError):
        M.SymmetricMatrix(back)
    assert M.wire_unframe(M.wire_frame([], enc), 4, dec) == []
