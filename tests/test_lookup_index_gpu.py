"""A lookup and a permutation check run from integers (LookupCheck.from_indices, permutation_leaves_indexed) on goldilocks D = 2^6
and babybear72: the multiplicities are counted on the device from the u64 indices that gathered the witness, sigma stays a u64
column up to the leaves, and neither is ever a table of ring elements before that."""
import numpy as np
import pytest

from test_mle_gpu import dev, host, model_for

pytestmark = pytest.mark.gpu
CHECKS = [("goldilocks", 6), ("babybear72", 0)]
IDS = [c[0] for c in CHECKS]
# sigma on 32 rows as a product of cycles; every row not named is a fixed point
CYCLES = [(0, 3, 7), (1, 2), (4, 9, 12, 20), (6, 31, 8), (10, 11, 13, 17, 19, 23, 29), (14, 30), (15, 16, 18, 21, 22)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.mark.parametrize("name,k", CHECKS, ids=IDS)
def test_a_lookup_from_indices(torch_cuda, name, k):
    """a table of 11 stored rows of 2^4 -- one column of ring elements, one of small integers -- and a witness of 37 stored rows of
    2^6 gathered from it by u64 indices; the denominators beta - (c_0 + gamma R::from(c_1)) come from fingerprint_indexed"""
    torch = torch_cuda
    from stark_rings_amd import LookupCheck, fingerprint_indexed

    md = model_for(name, k)
    ring, w = md.ring, md.w
    n_t, n_w = 11, 37
    rng = np.random.RandomState(0x1D0)
    col = md.uniform(0xE000, n_t).reshape(n_t, w)
    ints = (np.arange(n_t, dtype=np.uint64) * np.uint64(3) + np.uint64(1 << 33))
    picks = rng.randint(0, n_t, n_w).astype(np.uint64)
    picks[:n_t] = np.arange(n_t, dtype=np.uint64)   # every row is used at least once
    zero, one = md.zero(), md.elems(md.one())[0]
    gamma = md.elems(md.uniform(0xE010, 1))[0]
    coeffs = dev(torch, md.words([md.sub(zero, one), md.sub(zero, gamma)]))
    beta = dev(torch, md.uniform(0xE020, 1))
    q_t = fingerprint_indexed(ring, [dev(torch, col.reshape(-1))], [dev(torch, ints)], coeffs, beta)
    idx = dev(torch, picks)

    def check(w_ints):
        q_w = fingerprint_indexed(ring, [dev(torch, col[picks.astype(np.int64)].reshape(-1))], [dev(torch, w_ints)], coeffs, beta)
        return LookupCheck.from_indices(ring, q_w, q_t, idx, 6, 4, n_w=n_w, n_t=n_t)

    lc = check(ints[picks.astype(np.int64)])
    assert lc.holds()
    assert ring.spmv_bad_index_count() == 0
    # the numerators of the table side are R::from of the counts
    mults = np.bincount(picks.astype(np.int64), minlength=n_t)
    want = np.concatenate([((md.one().astype(object) * int(c)) % md.p).astype(np.uint64) if not md.pow2 else
                           md.words([np.array([int(c) % md.p] * ring.degree, dtype=object)]) for c in mults])
    assert np.array_equal(host(lc.table.p_leaves), want)
    off = ints[picks.astype(np.int64)].copy()
    off[20] = np.uint64(999)   # a witness row that is not in the table
    assert not check(off).holds()


@pytest.mark.parametrize("name,k", CHECKS, ids=IDS)
def test_a_permutation_check_from_a_u64_sigma(torch_cuda, name, k):
    """num_vars = 5: f is constant on the cycles of sigma, so f[sigma(e)] = f[e] and the two grand products agree; not after two
    entries of f on different cycles are swapped"""
    torch = torch_cuda
    from stark_rings_amd import PermutationCheck, permutation_leaves_indexed

    md = model_for(name, k)
    ring, w = md.ring, md.w
    nv, n = 5, 32
    sigma = np.arange(n, dtype=np.uint64)
    cycle_of = np.arange(n) + len(CYCLES)
    for c, cyc in enumerate(CYCLES):
        for a, b in zip(cyc, cyc[1:] + cyc[:1]):
            sigma[a] = b
            cycle_of[a] = c
    assert (np.sort(sigma) == np.arange(n)).all()
    values = md.uniform(0xE100, n + len(CYCLES)).reshape(-1, w)
    f = values[cycle_of]
    assert all(np.array_equal(f[int(sigma[e])], f[e]) for e in range(n))
    beta, gamma = dev(torch, md.uniform(0xE101, 1)), dev(torch, md.uniform(0xE102, 1))

    def check(f):
        num, den = permutation_leaves_indexed(ring, dev(torch, f.reshape(-1)), dev(torch, sigma), beta, gamma)
        return PermutationCheck(ring, num, den, nv)

    assert check(f).holds()
    bad = f.copy()
    bad[[3, 9]] = bad[[9, 3]]   # rows of the cycles (0 3 7) and (4 9 12 20)
    assert not np.array_equal(bad, f) and not check(bad).holds()
