"""Edge words through the D = 2^16 Goldilocks kernels whose representatives changed: the column passes take their W
layer on the register side of the exchange (lazy words cross it, one leg per block takes no product), the DFT_16 networks run a lazy
slot-0 chain, the rows256 inverse no longer canonicalises the value that skips its table product, and the shift products 2^32 .. 2^63
fold without a borrow chain.  Operands that put those paths on their borders:
  * every coefficient p - 1;
  * a single coefficient 1 (at 0, D / 16 or D - 1) in a ring element of zeros: whole butterflies see 0 and +-1, sums land on p;
  * the crafted vectors of tests/crafted_poly_operands.py (acc + r x on the values {0, 1, 2^32 - 2, 2^32 - 1, p - 1}).
mul_dev, mul_ntt_rhs_dev, elementwise_crt_dev and elementwise_icrt_dev on the lane plan with the keep column kernels and with the plain
ones, and at batch 16 on one stream: every output canonical, keep == plain bit for bit, sampled elements equal to the oracle.  On one
stream both plans run the plain column kernels (only lane plans take the keep kernels), so the keep == plain comparison says nothing
for that shape: there the canonicity and oracle checks carry the case."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import crafted_poly_operands as C
import oracle_lib as O
from test_cols_keep_prologue_gpu import D, K, PLAIN_COLS, _plan, _run_four, _words

P = C.P_GL
MAX_BATCH = 72
# (batch, chunk_polys, lanes): the shapes of tests/test_cols_keep_prologue_gpu.py, and batch 16 on one stream
SHAPES = [(48, 16, 2), (72, 24, 2), (16, 0, 1)]
KINDS = ("p-1", "one-hot", "crafted")
SAMPLE = (0, 1, 2, 15)   # one-hot: positions 0, D / 16, D - 1 and 0 again; present at every batch


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@functools.lru_cache(maxsize=None)
def _operands(kind):
    """(a, b): MAX_BATCH ring elements each, flat uint64 words; element e is the same at every batch"""
    a = np.zeros((MAX_BATCH, D), dtype=np.uint64)
    b = np.zeros((MAX_BATCH, D), dtype=np.uint64)
    if kind == "p-1":
        a[:], b[:] = P - 1, P - 1
    elif kind == "one-hot":
        pos = (0, D // 16, D - 1)
        for e in range(MAX_BATCH):
            a[e, pos[e % 3]] = 1
            b[e, pos[(e // 3) % 3]] = 1
    else:
        o = C.Ops("goldilocks", K)
        acc, xs, _ = C.craft_mul_elem_add(o, MAX_BATCH)
        a[:] = o.words(xs).reshape(MAX_BATCH, D)
        b[:] = o.words(acc).reshape(MAX_BATCH, D)
    return a.reshape(-1), b.reshape(-1)


@functools.lru_cache(maxsize=None)
def _reference(kind):
    """oracle results for the sampled elements: (product, forward transform of a)"""
    a, b = _operands(kind)
    ea = np.concatenate([a[e * D:(e + 1) * D] for e in SAMPLE])
    eb = np.concatenate([b[e * D:(e + 1) * D] for e in SAMPLE])
    F = O.GOLDILOCKS
    return O.pow2_ring_mul(F, ea, eb, K, len(SAMPLE), 4), O.pow2_fwd(F, ea, K, len(SAMPLE), 4)


@pytest.mark.parametrize("batch,chunk,lanes", SHAPES)
def test_edge_words_leave_canonical_equal_between_plans_and_match_the_oracle(torch_cuda, batch, chunk, lanes):
    torch = torch_cuda
    from stark_rings_amd import CyclotomicRing

    rings = [CyclotomicRing("goldilocks", K, device=0, plan=_plan(flags, lanes, chunk)) for flags in (0, PLAIN_COLS)]
    try:
        for kind in KINDS:
            a, b = _operands(kind)
            ta = torch.from_numpy(a[:batch * D].view(np.int64)).cuda()
            tb = torch.from_numpy(b[:batch * D].view(np.int64)).cuda()
            res = [_run_four(torch, ring, ta, tb) for ring in rings]   # asserts count_noncanonical_dev == 0 on all four outputs
            names = ("mul_dev", "mul_ntt_rhs_dev", "elementwise_crt_dev", "elementwise_icrt_dev")
            for name, keep, plain in zip(names, res[0], res[1]):
                assert torch.equal(keep, plain), "%s, %s: keep and plain column passes differ" % (kind, name)
            out, out2, fa, back = res[0]
            assert torch.equal(back, ta), (kind, "elementwise_icrt_dev")
            want, wf = _reference(kind)
            for i, e in enumerate(SAMPLE):
                s = slice(i * D, (i + 1) * D)
                assert np.array_equal(_words(out, e), want[s]), (kind, "mul_dev", e)
                assert np.array_equal(_words(out2, e), want[s]), (kind, "mul_ntt_rhs_dev", e)
                assert np.array_equal(_words(fa, e), wf[s]), (kind, "elementwise_crt_dev", e)
    finally:
        for ring in rings:
            ring.close()
