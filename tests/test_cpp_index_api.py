"""Builds and runs tests/cpp/test_index_api.cpp: IndexColumn, lincomb_index, lincomb_index_plan, from_u64, index_count,
DenseMultilinearExtension::linear_combination_indexed, identity_permutation[_mles], permutation_leaves_indexed and
LookupCheck::from_indices of include/stark_rings.hpp (the C++ mirror of the integer columns over the C ABI) against a term-at-a-time
restatement whose products come from libsr_oracle and whose R::from(x) is x one() by doubling and adding."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build_tmp", "test_index_api")


def _build():
    import oracle_lib

    oracle_lib.build()
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "test_index_api.cpp")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-o", BIN, src,
           "-L" + os.path.join(ROOT, "stark_rings_amd"), "-lstarkrings_hip",
           "-L" + os.path.join(ROOT, "oracle"), "-lsr_oracle",
           "-Wl,-rpath," + os.path.join(ROOT, "stark_rings_amd"), "-Wl,-rpath," + os.path.join(ROOT, "oracle"),
           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-lpthread"]
    subprocess.check_call(cmd, cwd=ROOT)


def test_cpp_index_mirror_compiles():
    """CPU: the mirror functions and classes and their test compile and link against the C ABI."""
    _build()
    assert os.path.exists(BIN)


@pytest.mark.gpu
def test_cpp_index_mirror_parity():
    _build()
    r = subprocess.run([BIN], cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all ok" in r.stdout
