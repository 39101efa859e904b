"""Builds and runs tests/cpp/test_isumcheck_api.cpp: IndexMultilinearExtension, VirtualPolynomial::add_product and the mul_by_mle overload
that take it, round_evals_weighted / fold_round_evals_weighted over column slots (sr_vpoly_iwround_evals, sr_vpoly_iwround_fold_evals),
the expanding slow paths, EqSumCheck over the PLONK and ALLCOL claims and the CyclotomicConfig::vpoly_iwround_plan wrapper of
include/stark_rings.hpp (the C++ mirror over the C ABI), against the same claims over to_dense() tables through the weighted calls."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build_tmp", "test_isumcheck_api")


def _build():
    import oracle_lib

    oracle_lib.build()
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "test_isumcheck_api.cpp")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-o", BIN, src,
           "-L" + os.path.join(ROOT, "stark_rings_amd"), "-lstarkrings_hip",
           "-L" + os.path.join(ROOT, "oracle"), "-lsr_oracle",
           "-Wl,-rpath," + os.path.join(ROOT, "stark_rings_amd"), "-Wl,-rpath," + os.path.join(ROOT, "oracle"),
           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-lpthread"]
    subprocess.check_call(cmd, cwd=ROOT)


def test_cpp_isumcheck_mirror_compiles():
    """CPU: the mirror classes and their test compile and link against the C ABI."""
    _build()
    assert os.path.exists(BIN)


@pytest.mark.gpu
def test_cpp_isumcheck_mirror_parity():
    _build()
    r = subprocess.run([BIN], cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all ok" in r.stdout
