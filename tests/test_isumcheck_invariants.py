"""The weighted rounds with integer columns (sr_vpoly_iwround_evals_dev, sr_vpoly_iwround_fold_evals_dev) under the
invariant-checking build, as tests/test_index_invariants.py does for sr_lincomb_index_dev: a child process of its own loads
libstarkrings_hip_check.so through SR_LIB_PATH (the product sources compiled with -DSR_GL_CHECK_REPS), drives both calls with the edge
inputs -- all p - 1 tables, weights and coefficients, every column value >= p where a u64 can be, a truncated column -- and reads every
counter as zero after each ring.  A second child runs the same calls on the product library; both compare every output with
tools/model_isumcheck.py."""
import os
import subprocess
import sys

import pytest

import isumcheck_invariants_worker as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_SO = os.path.join(ROOT, "stark_rings_amd", "libstarkrings_hip_check.so")
pytestmark = pytest.mark.gpu


def _worker(mode):
    env = dict(os.environ)
    env.pop("SR_LIB_PATH", None)
    if mode == "check":
        assert os.path.exists(CHECK_SO), "build() did not produce the checking build"
        env["SR_LIB_PATH"] = CHECK_SO
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "isumcheck_invariants_worker.py"), mode], env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode()
    assert r.returncode == 0 and "isumcheck_invariants: OK" in out, out[-4000:]
    return out


def test_the_weighted_rounds_with_integer_columns_keep_the_representative_invariants():
    out = _worker("check")
    assert out.count(" clean") == len(W.RINGS), out[-4000:]


def test_the_same_calls_on_the_product_library_agree_with_the_model():
    out = _worker("product")
    assert out.count("agrees with the model") == len(W.RINGS), out[-4000:]
