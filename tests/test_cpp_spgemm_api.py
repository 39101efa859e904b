"""Builds and runs tests/cpp/test_spgemm_api.cpp: SparseMatrixNTT::transpose / checked_mul_mat / try_mul_mat and MatrixNTT::transpose of
include/stark_rings.hpp (the C++ mirror of crates/linear_algebra's SparseMatrix product and of Transpose over the C ABI) against
vectors the Python restatement (tools/model_sparse_matrix.py) writes."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build_tmp", "test_spgemm_api")
VECTORS = os.path.join(ROOT, "build_tmp", "spgemm_api_vectors.bin")
sys.path.insert(0, os.path.join(ROOT, "tools"))
# (ring id, log2 D, base field of the oracle, slot product of the oracle or None, words per element, words per slot, modulus)
GL, BB, FROG = 2**64 - 2**32 + 1, 2013265921, 15912092521325583641
CASES = [(0, 6, "goldilocks", None, 64, 1, GL), (1, 5, "babybear", None, 32, 1, BB), (2, 4, "stark", None, 64, 4, 2**251 + 17 * 2**192 + 1),
         (3, 0, "goldilocks", "sro_g24_ntt_mul", 24, 3, GL), (4, 0, "babybear", "sro_bb72_ntt_mul", 72, 9, BB),
         (5, 0, "frog", "sro_frog16_ntt_mul", 16, 4, FROG)]


def _build():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "test_spgemm_api.cpp")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-o", BIN, src,
           "-L" + os.path.join(ROOT, "stark_rings_amd"), "-lstarkrings_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "stark_rings_amd"),
           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-lpthread"]
    subprocess.check_call(cmd, cwd=ROOT)


def _write_vectors():
    """the model on standard-form integers (power-of-two rings) or on the oracle's slot products (the reference's own rings).  Per ring
    two products: the value-dependent pattern (stored zeros, complementary zero slots, a b + (-a) b, dead entries) and a random 5 x 9
    times 9 x 5 with empty rows; then a matrix with unsorted rows for the transpose alone."""
    import model_sparse_matrix as M
    import oracle_lib as O

    out = [np.array([len(CASES)], dtype=np.uint64)]
    for ring, k, base, slot_mul, w, slot_w, p in CASES:
        F = O.FIELD_ID[base]
        coeffs = w // O.LIMBS[F]
        if slot_mul is None:
            elem = lambda x: np.array(O.from_mont(F, x), dtype=object)  # noqa: E731
            words = lambda e: O.to_mont(F, [int(v) for v in e])  # noqa: E731
            add, mul = (lambda x, y: (x + y) % p), (lambda x, y: (x * y) % p)
        else:
            elem = lambda x: x.copy()  # noqa: E731
            words = lambda e: np.asarray(e, dtype=np.uint64)  # noqa: E731
            add = lambda x, y: ((x.astype(object) + y.astype(object)) % p).astype(np.uint64)  # noqa: E731
            mul = lambda x, y: O.small(slot_mul, x, y).reshape(-1)  # noqa: E731
        is_zero = lambda e: not e.any()  # noqa: E731
        pool = O.fill_uniform(F, 0x8000 + ring, 0, 100 * coeffs).reshape(100, w)

        def put(m):
            vals, cols, row_ptr = m.csr()
            out.extend([np.array([m.nrows, m.ncols, len(cols)] + row_ptr + cols, dtype=np.uint64)] + [words(v) for v in vals])

        def matrix(nrows, ncols, rows):
            return M.SparseMatrix(nrows, ncols, [[(elem(v), c) for v, c in row] for row in rows])

        a, b = pool[0], pool[1]
        neg_a = words((p - elem(a)) % p) if slot_mul is None else ((p - a.astype(object)) % p).astype(np.uint64)
        lo, hi = pool[2].copy(), pool[2].copy()
        lo[w // 2:] = 0
        hi[:w // 2] = 0
        assert w // 2 % slot_w == 0 and lo.any() and hi.any()
        zero = np.zeros(w, dtype=np.uint64)
        rng = random.Random(ring)
        pick = lambda nrows, ncols, base_, d: [[(pool[base_ + i * ncols + c], c) for c in range(ncols) if rng.random() < d] for i in range(nrows)]  # noqa: E731
        products = [(matrix(3, 2, [[(a, 0), (neg_a, 1)], [(lo, 0)], [(zero, 0), (lo, 1)]]), matrix(2, 2, [[(b, 0), (hi, 1)], [(b, 0), (hi, 1)]])),
                    (matrix(5, 9, pick(5, 9, 3, 0.4)), matrix(9, 5, pick(9, 5, 50, 0.4)))]
        out.append(np.array([ring, k, w, len(products)], dtype=np.uint64))
        for x, y in products:
            xy = x.checked_mul_mat(y, add, mul, is_zero)
            for m in (x, y, xy, x.transpose()):
                put(m)
        assert [[j for _, j in row] for row in products[0][0].checked_mul_mat(products[0][1], add, mul, is_zero).coeffs] == [[0, 1], [0], [0]]
        u = matrix(3, 4, [[(pool[3], 3), (pool[4], 0), (pool[5], 2)], [], [(pool[6], 2), (pool[7], 1), (pool[8], 3)]])
        put(u)
        put(u.transpose())
    np.concatenate(out).tofile(VECTORS)


def test_cpp_spgemm_mirror_compiles():
    """CPU: the mirror methods and their test compile and link against the C ABI."""
    _build()
    assert os.path.exists(BIN)


@pytest.mark.gpu
def test_cpp_spgemm_mirror_parity():
    _build()
    _write_vectors()
    r = subprocess.run([BIN, VECTORS], cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all ok" in r.stdout
