"""The fused fold-and-round call of a sum of products (sr_vpoly_round_fold_evals_dev) under the invariant-checking build, as
tests/test_rep_invariants.py does for the older calls: a child process of its own loads libstarkrings_hip_check.so through SR_LIB_PATH
(the product sources compiled with -DSR_GL_CHECK_REPS), drives the call with the crafted operands of tests/crafted_poly_operands.py --
craft_vpoly's tables as the FOLDED tables of a crafted challenge, and the all-(p - 1) tables with r = p - 1 and every coefficient p - 1
through R1CS and an eight-term structure -- and reads every counter as zero after each group.  A second child runs the same calls on
the product library; both compare every output with the integer models."""
import os
import subprocess
import sys

import pytest

import crafted_poly_operands as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_SO = os.path.join(ROOT, "stark_rings_amd", "libstarkrings_hip_check.so")
pytestmark = pytest.mark.gpu


def _worker(mode):
    env = dict(os.environ)
    env.pop("SR_LIB_PATH", None)
    if mode == "check":
        assert os.path.exists(CHECK_SO), "build() did not produce the checking build"
        env["SR_LIB_PATH"] = CHECK_SO
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "vpoly_fold_invariants_worker.py"), mode], env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    out = r.stdout.decode()
    assert r.returncode == 0 and "vpoly_fold_invariants: OK" in out, out[-4000:]
    return out


def test_the_fused_sum_of_products_round_keeps_its_representative_invariants():
    out = _worker("check")
    assert out.count(" clean") == len(C.POLY_CASES), out[-4000:]


def test_the_same_calls_on_the_product_library_agree_with_the_model():
    out = _worker("product")
    assert out.count("agrees with the model") == len(C.POLY_CASES), out[-4000:]
