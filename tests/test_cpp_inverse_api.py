"""Builds and runs tests/cpp/test_inverse_api.cpp: RqNTTVec::inverse / divide / inverse_zero_count and the DenseMultilinearExtension
mirrors of include/stark_rings.hpp (Field::inverse / ark_ff::batch_inversion over the C ABI's host-pointer call) on a small vector with
planted zero slots, against Python integers for the power-of-two rings; the empty vector; the count."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build_tmp", "test_inverse_api")
VECTORS = os.path.join(ROOT, "build_tmp", "inverse_api_vectors.bin")
GL, BB, FROG = 2**64 - 2**32 + 1, 2013265921, 15912092521325583641
# (ring id, log2 D, base field of the oracle, words per element, words per slot, modulus, zero slots to plant)
CASES = [(0, 6, "goldilocks", 64, 1, GL, 3), (0, 6, "goldilocks", 64, 1, GL, 0), (1, 5, "babybear", 32, 1, BB, 2),
         (2, 4, "stark", 64, 4, 2**251 + 17 * 2**192 + 1, 1), (3, 0, "goldilocks", 24, 3, GL, 2), (4, 0, "babybear", 72, 9, BB, 0),
         (5, 0, "frog", 16, 4, FROG, 1)]
N = 13


def _build():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "test_inverse_api.cpp")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-o", BIN, src,
           "-L" + os.path.join(ROOT, "stark_rings_amd"), "-lstarkrings_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "stark_rings_amd"),
           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-lpthread"]
    subprocess.check_call(cmd, cwd=ROOT)


def _write_vectors():
    import oracle_lib as O

    out = [np.array([len(CASES)], dtype=np.uint64)]
    for ring, k, base, w, slot_w, p, zeros in CASES:
        F = O.FIELD_ID[base]
        coeffs = w // O.LIMBS[F]
        den = O.fill_uniform(F, 0x9100 + ring, 0, N * coeffs)
        num = O.fill_uniform(F, 0x9200 + ring, 0, N * coeffs)
        slots = den.reshape(-1, slot_w)
        slots[~slots.any(axis=1), 0] = 1
        for z in range(zeros):
            slots[(4 * z + 1) * (w // slot_w) + z] = 0         # element 4 z + 1, slot z
        pow2 = ring <= 2
        out.append(np.array([ring, k, w, N, zeros, int(pow2)], dtype=np.uint64))
        out += [den, num]
        if pow2:
            xs, ns = O.from_mont(F, den), O.from_mont(F, num)
            inv = [0 if x == 0 else pow(x, -1, p) for x in xs]
            out += [O.to_mont(F, inv), O.to_mont(F, [i * n % p for i, n in zip(inv, ns)])]
    np.concatenate(out).tofile(VECTORS)


def test_cpp_inverse_mirror_compiles():
    """CPU: the mirror methods and their test compile and link against the C ABI."""
    _build()
    assert os.path.exists(BIN)


@pytest.mark.gpu
def test_cpp_inverse_mirror_parity():
    _build()
    _write_vectors()
    r = subprocess.run([BIN, VECTORS], cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all ok" in r.stdout
