"""The invariant-checking build (VERDICT r3 #1a).  The lazy butterflies of the tuned Goldilocks path leave 64-bit representatives
that differ from the canonical value with probability 2^-32 per value on uniform data: a kernel that feeds such a representative to
a butterfly that assumes canonical inputs is wrong, and no uniform-data parity test can see it (round 3 shipped one for 31 minutes).
libstarkrings_hip_check.so is the product's own source compiled with -DSR_GL_CHECK_REPS: every canonical butterfly counts a
non-canonical input, every lazy butterfly a second wrap or borrow, every result store a word >= p, while the real kernels run.
The GPU test drives it, in a process of its own (SR_LIB_PATH), over uniform, edge, structured and crafted operands of every tuned
plan and requires all counters to stay zero -- and a raw operand word >= p to be counted.  The same build counts the bound
violations of the lazy nine-limb Stark arithmetic (limb sums leaving int32, products that could overflow a column accumulator) and
records the largest limb seen: a second test drives every Stark kernel family over max-limb operands."""
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_SO = os.path.join(ROOT, "stark_rings_amd", "libstarkrings_hip_check.so")


def test_checking_build_exports_the_whole_abi_and_the_product_carries_no_checks():
    from stark_rings_amd import _lib

    assert os.path.exists(CHECK_SO), "build() did not produce the checking build"
    syms = subprocess.run(["nm", "-D", "--defined-only", CHECK_SO], check=True, stdout=subprocess.PIPE).stdout.decode()
    for name in _lib.SYMBOLS:
        assert " T %s\n" % name in syms, "checking build lacks %s" % name
    buf = (ctypes.c_uint64 * 8)()
    rc = _lib.load().sr_selftest_rep_counters(buf, 0)   # the product library: no counters, no checks, and it says so
    assert rc == 5 and "SR_GL_CHECK_REPS" in _lib.last_error()
    src = open(os.path.join(ROOT, "stark_rings_amd", "csrc", "fields.hpp")).read()
    assert "SR_GL_CHECK_REPS" in src and "atomicAdd(&g_counters" in src


def _worker(which):
    env = dict(os.environ)
    env["SR_LIB_PATH"] = CHECK_SO
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rep_invariants_worker.py"), which], env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1500)
    out = r.stdout.decode()
    assert r.returncode == 0 and "rep_invariants: OK" in out, out[-4000:]
    return out


@pytest.mark.gpu
def test_every_tuned_goldilocks_plan_keeps_its_representative_invariants():
    out = _worker("goldilocks")
    assert out.count(" clean") >= 11 and "negative control" in out, out[-4000:]


@pytest.mark.gpu
def test_every_stark_plan_keeps_its_limb_bounds():
    """The nine-limb lazy Stark arithmetic (csrc/stark_lazy.hpp) postpones carries and reductions; its invariants are bounds (no limb sum
    leaves int32, no product overflows its 64-bit column accumulator) that the kernels keep by reducing weakly every few stages -- and
    that uniform data never approaches.  The checking build counts violations and records the largest |limb| any add / sub produced,
    over memory images with every limb at its maximum, through every Stark kernel family and the lazily summed matrix products."""
    out = _worker("stark")
    assert out.count(" clean") >= 15 and "Stark limb high-water mark" in out, out[-4000:]


@pytest.mark.gpu
def test_the_polynomial_kernels_keep_their_representative_invariants():
    """The dense folds, the three round kernels, the sums of products and the sparse multilinear extensions (csrc/mle.hpp, sumcheck*.hpp,
    sparse_mle.hpp) are built from Goldilocks::add / sub and the lazy sums, whose preconditions no parity test on uniform data can see.
    tests/crafted_poly_operands.py puts their INTERMEDIATE words on the borders; the worker runs those and the family tests' edge
    tables through the checking build for the seven shapes at which both launch paths are reached: five groups per ring, all counters
    zero after each, every output compared with the integer models, and raw words >= p counted where add / sub touch them first."""
    out = _worker("poly")
    assert out.count(" clean") == 7 * 5 and out.count("negative control") >= 4, out[-4000:]
    assert "launch paths: the single launch and the split path were taken" in out, out[-4000:]


@pytest.mark.gpu
def test_the_matrix_kernels_keep_their_invariants_on_max_limb_operands():
    """Gram, G^T M G, sparse x sparse, gather and transpose on crafted operands (three groups for each of six rings), then every
    polynomial and matrix call on Stark rings of degree 2^4 and 2^12 with every operand a max-limb image (eight groups each): the
    limb-bound counters stay zero and the largest |limb| is reported per family."""
    out = _worker("linalg")
    assert out.count(" clean") == 6 * 3 + 2 * 8 and "negative control" in out, out[-4000:]
    assert out.count("largest |limb| in any add / sub") == 2 * 8 and out.count("Stark limb high-water mark") == 2, out[-4000:]
