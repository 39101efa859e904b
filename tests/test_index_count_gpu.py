"""GPU parity of the multiplicities (sr_index_count_dev, sr_index_count; csrc/lincomb_index.hpp): counts[t] = #{ i : idx[i] == t }
against numpy.bincount.  Bins up to kLdsBins = 4096 are counted in LDS per workgroup, more with global atomics: both sides of that
bound, one bin, one bin hit from several workgroups, no index at all, indices out of range (skipped and counted in the context's
bad-index counter), an odd 8-byte pointer, and stale contents of the counts before the call."""
import numpy as np
import pytest

from test_mle_gpu import dev, host, model_for

pytestmark = pytest.mark.gpu
N = 70000
LDS_BINS = 4096


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def ring(torch_cuda):
    return model_for("goldilocks", 6).ring


def count(torch, ring, idx, n_bins, shift=0):
    """one call on fresh buffers: idx and counts `shift` words past a 16-byte boundary, stale non-zero counts, a guard behind them"""
    from stark_rings_amd import index_count_dev

    ibuf = torch.full((idx.size + 2,), -1, dtype=torch.int64, device="cuda")
    if idx.size:
        ibuf[shift:shift + idx.size] = dev(torch, idx)
    cbuf = torch.full((n_bins + 3,), 0x5A5A, dtype=torch.int64, device="cuda")
    assert ibuf.data_ptr() % 16 == 0 and cbuf.data_ptr() % 16 == 0
    out = index_count_dev(ring, ibuf[shift:shift + idx.size], n_bins, out=cbuf[shift:shift + n_bins])
    torch.cuda.synchronize()
    got = host(cbuf)
    assert (got[:shift] == 0x5A5A).all() and (got[shift + n_bins:] == 0x5A5A).all(), "guard overwritten"
    assert out.data_ptr() == cbuf[shift:].data_ptr()
    return got[shift:shift + n_bins]


@pytest.mark.parametrize("n_bins", [1, LDS_BINS - 1, LDS_BINS, LDS_BINS + 1, 3 * LDS_BINS + 5])
def test_uniform_indices_on_both_sides_of_the_lds_bound(torch_cuda, ring, n_bins):
    rng = np.random.RandomState(n_bins)
    idx = rng.randint(0, n_bins, N).astype(np.uint64)
    want = np.bincount(idx.astype(np.int64), minlength=n_bins).astype(np.uint64)
    assert np.array_equal(count(torch_cuda, ring, idx, n_bins), want)
    assert ring.spmv_bad_index_count() == 0


def test_one_bin_across_several_workgroups(torch_cuda, ring):
    idx = np.full(N, 3, dtype=np.uint64)
    assert np.array_equal(count(torch_cuda, ring, idx, 5), np.array([0, 0, 0, N, 0], dtype=np.uint64))


def test_no_index_clears_the_counts(torch_cuda, ring):
    assert not count(torch_cuda, ring, np.zeros(0, dtype=np.uint64), 7).any()
    assert not count(torch_cuda, ring, np.zeros(0, dtype=np.uint64), LDS_BINS + 9).any()


@pytest.mark.parametrize("n_bins", [11, LDS_BINS + 11])
def test_three_indices_out_of_range_are_skipped_and_counted(torch_cuda, ring, n_bins):
    rng = np.random.RandomState(n_bins + 1)
    idx = rng.randint(0, n_bins, 5000).astype(np.uint64)
    idx[[7, 2500, 4999]] = np.array([n_bins, 1 << 40, (1 << 64) - 1], dtype=np.uint64)
    rest = np.delete(idx, [7, 2500, 4999])
    want = np.bincount(rest.astype(np.int64), minlength=n_bins).astype(np.uint64)
    assert ring.spmv_bad_index_count() == 0
    assert np.array_equal(count(torch_cuda, ring, idx, n_bins), want)
    assert ring.spmv_bad_index_count() == 3
    assert ring.spmv_bad_index_count() == 0   # read and cleared


@pytest.mark.parametrize("n_bins", [100, LDS_BINS + 100])
def test_an_odd_eight_byte_pointer(torch_cuda, ring, n_bins):
    rng = np.random.RandomState(n_bins + 2)
    idx = rng.randint(0, n_bins, 3001).astype(np.uint64)
    want = np.bincount(idx.astype(np.int64), minlength=n_bins).astype(np.uint64)
    assert np.array_equal(count(torch_cuda, ring, idx, n_bins, shift=1), want)


def test_the_host_form_counts_and_refuses_an_index_out_of_range(torch_cuda, ring):
    from stark_rings_amd import RingError, index_count

    rng = np.random.RandomState(5)
    for n_bins in (13, LDS_BINS + 13):
        idx = rng.randint(0, n_bins, 4000).astype(np.uint64)
        assert np.array_equal(index_count(ring, idx, n_bins), np.bincount(idx.astype(np.int64), minlength=n_bins).astype(np.uint64))
        idx[1234] = n_bins
        with pytest.raises(RingError, match="not below n_bins"):
            index_count(ring, idx, n_bins)
    assert not index_count(ring, np.zeros(0, dtype=np.uint64), 4).any()
    assert ring.spmv_bad_index_count() == 0
