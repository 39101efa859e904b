"""The crafted operands of tests/crafted_poly_operands.py -- intermediate words on the borders of the number formats, partial sums that
hover around 0 mod p, messages solved onto the border values -- through the PRODUCT library, for every ring, bit for bit against the
integer models.  tests/test_rep_invariants.py runs the same calls on the invariant-checking build and reads its counters; here a wrong
word shows up without that build too."""
import pytest

import crafted_poly_operands as C

pytestmark = pytest.mark.gpu
LINALG = [("goldilocks", 6), ("goldilocks24", 0), ("frog16", 0), ("babybear", 5), ("babybear72", 0), ("stark", 4)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


GROUPS = ("dense", "rounds", "fused", "vpoly", "sparse")


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("name,k,nv", C.POLY_CASES, ids=["%s-%d-nv%d" % c for c in C.POLY_CASES])
def test_crafted_operands_through_the_polynomial_calls_match_the_models(torch_cuda, name, k, nv, group):
    from crafted_poly_driver import Run

    run = Run(torch_cuda, name, k)
    getattr(run, group)(nv)
    assert len(run.paths) == 1


@pytest.mark.parametrize("name,k", LINALG, ids=["%s-%d" % c for c in LINALG])
def test_crafted_operands_through_the_matrix_calls_match_the_models(torch_cuda, name, k):
    from crafted_poly_driver import Run

    Run(torch_cuda, name, k).linalg()
