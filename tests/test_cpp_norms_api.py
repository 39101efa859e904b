"""Builds and runs tests/cpp/test_norms_api.cpp: RqPolyVec::linf_norm / l2_norm_squared (whole slice and per element) of
include/stark_rings.hpp over the C ABI, against the definition computed in the test itself (the standard form from libsr_oracle)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build_tmp", "test_norms_api")


def _build():
    import oracle_lib

    oracle_lib.build()
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "test_norms_api.cpp")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-o", BIN, src,
           "-L" + os.path.join(ROOT, "stark_rings_amd"), "-lstarkrings_hip",
           "-L" + os.path.join(ROOT, "oracle"), "-lsr_oracle",
           "-Wl,-rpath," + os.path.join(ROOT, "stark_rings_amd"), "-Wl,-rpath," + os.path.join(ROOT, "oracle"),
           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-lpthread"]
    subprocess.check_call(cmd, cwd=ROOT)


def test_cpp_norms_mirror_compiles():
    """CPU: the mirror class and its test compile and link against the C ABI."""
    _build()
    assert os.path.exists(BIN)


@pytest.mark.gpu
def test_cpp_norms_mirror_parity():
    _build()
    r = subprocess.run([BIN], cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all ok" in r.stdout
