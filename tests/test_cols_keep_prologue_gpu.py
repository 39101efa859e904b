"""The lane column pass (cols256_keep_kernel, Goldilocks D = 2^16) issues its first ring element's loads ahead of the table prologue
and keeps its "tile free" barrier in front of the next iteration's exchange writes.  What can go wrong is the hand-over between
iterations (a sibling wave still reading the exchange tile, the W table not yet in LDS in iteration 0) and the scalar-side
addressing of the 32 accesses per element; both would show as wrong words, so everything is compared bit for bit with the plan that
runs the plain one-tile-per-workgroup kernel (SR_PLAN_GL_PLAIN_COLS), and sampled elements with the oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle_lib as O

K = 16
D = 1 << K
PLAIN_COLS = 128  # SR_PLAN_GL_PLAIN_COLS
# batch, chunk_polys: iterations per workgroup in a lane launch = chunk / 8 (one operand), chunk / 4 (the forward pair)
CASES = [
    (48, 16),  # two and four iterations: the smallest launch the keep kernel accepts
    (72, 24),  # three and six: an odd count crosses the moved barrier with the other parity
    (56, 24),  # ragged last chunk of 8, which falls back to the plain kernel
]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _plan(flags, lanes, chunk_polys):
    from stark_rings_amd import _lib

    p = _lib.Plan()
    p.flags, p.lanes, p.chunk_polys = flags, lanes, chunk_polys
    return p


def _run_four(torch, ring, ta, tb):
    """mul_dev, mul_ntt_rhs_dev, elementwise_crt_dev, elementwise_icrt_dev -> (product, product through NTT-form b, crt(a), icrt(crt(a)))"""
    out = torch.empty_like(ta)
    ring.mul_dev(out, ta, tb)
    fb = tb.clone()
    ring.elementwise_crt_dev(fb)
    out2 = torch.empty_like(ta)
    ring.mul_ntt_rhs_dev(out2, ta, fb)
    fa = ta.clone()
    ring.elementwise_crt_dev(fa)
    back = fa.clone()
    ring.elementwise_icrt_dev(back)
    torch.cuda.synchronize()
    for t in (out, out2, fa, back):
        assert ring.count_noncanonical_dev(t) == 0
    return out, out2, fa, back


def _both_plans(torch, batch, chunk, fill):
    from stark_rings_amd import CyclotomicRing

    n = batch * D
    ta = torch.empty(n, dtype=torch.int64, device="cuda")
    tb = torch.empty(n, dtype=torch.int64, device="cuda")
    res = []
    for flags in (0, PLAIN_COLS):
        ring = CyclotomicRing("goldilocks", K, device=0, plan=_plan(flags, 2, chunk))
        fill(ring, ta, tb)
        res.append(_run_four(torch, ring, ta, tb))
        ring.close()
    names = ("mul_dev", "mul_ntt_rhs_dev", "elementwise_crt_dev", "elementwise_icrt_dev")
    for name, keep, plain in zip(names, res[0], res[1]):
        assert torch.equal(keep, plain), "%s: keep and plain column passes differ" % name
    return ta, res[0]


def _words(t, e):
    return t[e * D:(e + 1) * D].cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("batch,chunk", CASES)
def test_keep_kernel_equals_plain_kernel_and_oracle(torch_cuda, batch, chunk):
    torch = torch_cuda

    def fill(ring, ta, tb):
        ring.fill_uniform_dev(ta, 0xC7, 0)
        ring.fill_uniform_dev(tb, 0xC8, 0)

    ta, (out, out2, fa, back) = _both_plans(torch, batch, chunk, fill)
    F = O.GOLDILOCKS
    sample = [0, 7, 8, batch - 9, batch - 1]
    ea = np.concatenate([O.fill_uniform(F, 0xC7, e * D, D) for e in sample])
    eb = np.concatenate([O.fill_uniform(F, 0xC8, e * D, D) for e in sample])
    want = O.pow2_ring_mul(F, ea, eb, K, len(sample), 4)
    wf = O.pow2_fwd(F, ea, K, len(sample), 4)
    for i, e in enumerate(sample):
        s = slice(i * D, (i + 1) * D)
        assert np.array_equal(_words(out, e), want[s]), ("mul_dev", e)
        assert np.array_equal(_words(out2, e), want[s]), ("mul_ntt_rhs_dev", e)
        assert np.array_equal(_words(fa, e), wf[s]), ("elementwise_crt_dev", e)
        assert np.array_equal(_words(back, e), ea[s]), ("elementwise_icrt_dev", e)
    assert torch.equal(back, ta)


def test_keep_kernel_with_all_operands_at_p_minus_one(torch_cuda):
    """Every word p - 1: the largest canonical words through every lazy butterfly.  Words are Montgomery images (R = 2^64, and
    R^-1 = -2^32 since 2^96 = -1), so the product of two elements with all words w = p - 1 is known in closed form: the negacyclic
    square of (1 ... 1) has coefficient (i + 1) - (D - 1 - i) = 2 i + 2 - D, times w^2 R^-1 = -2^32."""
    torch = torch_cuda
    batch, chunk = CASES[0]
    p = (1 << 64) - (1 << 32) + 1

    def fill(ring, ta, tb):
        ta.fill_(p - 1 - (1 << 64))  # the word p - 1 as int64
        tb.fill_(p - 1 - (1 << 64))

    ta, (out, out2, fa, back) = _both_plans(torch, batch, chunk, fill)
    F = O.GOLDILOCKS
    ea = np.full(D, p - 1, dtype=np.uint64)
    want = O.pow2_ring_mul(F, ea, ea.copy(), K, 1, 4)
    closed = np.array([(2 * i + 2 - D) * (p - (1 << 32)) % p for i in range(D)], dtype=np.uint64)
    assert np.array_equal(want, closed)
    wf = O.pow2_fwd(F, ea, K, 1, 4)
    for e in (0, 7, 8, batch - 9, batch - 1):
        assert np.array_equal(_words(out, e), want), ("mul_dev", e)
        assert np.array_equal(_words(out2, e), want), ("mul_ntt_rhs_dev", e)
        assert np.array_equal(_words(fa, e), wf), ("elementwise_crt_dev", e)
    assert torch.equal(back, ta)
