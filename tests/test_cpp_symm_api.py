"""Builds and runs tests/cpp/test_symm_api.cpp: SymmetricMatrixNTT of include/stark_rings.hpp (the C++ mirror of
crates/linear_algebra's SymmetricMatrix and of recompose_left_right_symmetric_matrix over the C ABI) against vectors the Python
restatement (tools/model_symmetric.py) writes."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build_tmp", "test_symm_api")
VECTORS = os.path.join(ROOT, "build_tmp", "symm_api_vectors.bin")
sys.path.insert(0, os.path.join(ROOT, "tools"))
# (ring id, log2 D, base field of the oracle, slot product of the oracle or None, words per element, modulus)
GL, BB, FROG = 2**64 - 2**32 + 1, 2013265921, 15912092521325583641
CASES = [(0, 6, "goldilocks", None, 64, GL), (1, 5, "babybear", None, 32, BB), (2, 4, "stark", None, 64, 2**251 + 17 * 2**192 + 1),
         (3, 0, "goldilocks", "sro_g24_ntt_mul", 24, GL), (4, 0, "babybear", "sro_bb72_ntt_mul", 72, BB), (5, 0, "frog", "sro_frog16_ntt_mul", 16, FROG)]
N, D, M_COLS = 2, 2, 3


def _build():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "test_symm_api.cpp")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-o", BIN, src,
           "-L" + os.path.join(ROOT, "stark_rings_amd"), "-lstarkrings_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "stark_rings_amd"),
           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-lpthread"]
    subprocess.check_call(cmd, cwd=ROOT)


def _write_vectors():
    """the model on standard-form integers (power-of-two rings) or on the oracle's slot products (the reference's own rings)"""
    import model_symmetric as M
    import oracle_lib as O

    out = [np.array([len(CASES)], dtype=np.uint64)]
    for ring, k, base, slot_mul, w, p in CASES:
        F = O.FIELD_ID[base]
        limbs = O.LIMBS[F]
        coeffs = w // limbs
        a = O.fill_uniform(F, 0x7000 + ring, 0, N * D * M_COLS * coeffs)
        powers = O.fill_uniform(F, 0x7100 + ring, 0, D * coeffs)
        if slot_mul is None:
            to_elems = lambda x: [np.array(O.from_mont(F, x), dtype=object)[i * coeffs:(i + 1) * coeffs] for i in range(x.size // w)]  # noqa: E731
            to_words = lambda es: O.to_mont(F, [int(v) for e in es for v in e])  # noqa: E731
            add, mul, zero = (lambda x, y: (x + y) % p), (lambda x, y: (x * y) % p), np.array([0] * coeffs, dtype=object)
        else:
            to_elems = lambda x: [x[i * w:(i + 1) * w].copy() for i in range(x.size // w)]  # noqa: E731
            to_words = np.concatenate
            add = lambda x, y: ((x.astype(object) + y.astype(object)) % p).astype(np.uint64)  # noqa: E731
            mul = lambda x, y: O.small(slot_mul, x, y)  # noqa: E731
            zero = np.zeros(w, dtype=np.uint64)
        g = M.gram(to_elems(a), N * D, M_COLS, add, mul, zero)
        small = M.recompose_left_right_symmetric_matrix(g, to_elems(powers), add, mul, zero)
        out += [np.array([ring, k, N, D, M_COLS, w], dtype=np.uint64), a, powers, to_words(g.packed()), to_words(small.packed())]
    np.concatenate(out).tofile(VECTORS)


def test_cpp_symm_mirror_compiles():
    """CPU: the mirror class and its test compile and link against the C ABI."""
    _build()
    assert os.path.exists(BIN)


@pytest.mark.gpu
def test_cpp_symm_mirror_parity():
    _build()
    _write_vectors()
    r = subprocess.run([BIN, VECTORS], cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all ok" in r.stdout
