"""SymmetricMatrix<F> (crates/linear_algebra/src/symmetric_matrix.rs:14-92) over ring elements in CRT/NTT form, packed.

The reference stores a Vec<Vec<F>> whose row i has the i + 1 entries (i, 0) .. (i, i).  Here the rows are flattened into one buffer of
n (n + 1) / 2 ring elements in the flat layout of every other call: entry (i, j) with j <= i is element i (i + 1) / 2 + j.  The
buffer is a numpy uint64 array (the host-pointer calls run) or a torch CUDA tensor of 8-byte integers (the device calls run on the
stream given, with caller-visible workspaces, so they can be captured).

  SymmetricMatrix::from_par_fn(n, |i, j| <s_i, s_j>)   symmetric_matrix.rs:76-90    -> SymmetricMatrixNTT.gram (sr_gram_ntt[_dev]);
                                                                                       the inner-product closure is the caller's
  recompose_left_right_symmetric_matrix                balanced_decomposition/mod.rs:354-386 -> recompose_left_right
                                                                                       (sr_symm_recompose[_dev])
`rand` and `map` with an arbitrary closure have no device counterpart.
"""
import numpy as np

from .rings import RingError


def packed_index(i, j):
    """position of entry (i, j) in the packed buffer: the symmetric lookup of symmetric_matrix.rs:37-44"""
    return i * (i + 1) // 2 + j if j <= i else j * (j + 1) // 2 + i


def _is_host(words):
    return isinstance(words, np.ndarray)


class SymmetricMatrixNTT:
    def __init__(self, ring, n, words):
        """ring: a CyclotomicRing; words: n (n + 1) / 2 ring elements, packed (kept, not copied)."""
        size = words.size if _is_host(words) else words.numel()
        if n < 0 or size != n * (n + 1) // 2 * ring.words_per_elem:
            raise RingError("SymmetricMatrixNTT: the buffer does not hold n (n + 1) / 2 ring elements")
        self.ring, self._n, self.words = ring, int(n), words

    # -- constructors ------------------------------------------------------------------------------------------------------------
    @classmethod
    def zero(cls, ring, n, device=False):
        """symmetric_matrix.rs:24-28: every entry F::zero()."""
        count = n * (n + 1) // 2 * ring.words_per_elem
        if device:
            import torch

            return cls(ring, n, torch.zeros(count, dtype=torch.int64, device="cuda:%d" % ring.device))
        return cls(ring, n, np.zeros(count, dtype=np.uint64))

    @classmethod
    def from_rows(cls, ring, rows):
        """From<Vec<Vec<F>>> (symmetric_matrix.rs:17-22): rows[i] holds i + 1 ring elements (a flat uint64 array, or a list of
        element arrays); anything else raises where the reference asserts."""
        w = ring.words_per_elem
        flat = []
        for i, row in enumerate(rows):
            r = np.concatenate([np.asarray(e, dtype=np.uint64).reshape(-1) for e in row]) if isinstance(row, (list, tuple)) \
                else np.asarray(row, dtype=np.uint64).reshape(-1)
            if r.size != (i + 1) * w:
                raise RingError("cannot convert rows to SymmetricMatrixNTT, row has wrong number of entries")
            flat.append(r)
        return cls(ring, len(flat), np.concatenate(flat) if flat else np.zeros(0, dtype=np.uint64))

    @classmethod
    def gram(cls, ring, a, n, m, work=None, stream=None):
        """out(i, j) = sum_{t < m} a[i][t] * a[j][t] for the dense row-major n x m matrix a: from_par_fn with the inner-product
        closure.  a numpy: the host-pointer call; a CUDA tensor: sr_gram_ntt_dev on `stream`, with `work` (at least
        ring.gram_plan(n, m)[0] elements) or a workspace allocated here."""
        if _is_host(a):
            return cls(ring, n, ring.gram_ntt(a, n, m))
        import torch

        w = ring.words_per_elem
        out = torch.empty(n * (n + 1) // 2 * w, dtype=a.dtype, device=a.device)
        need = ring.gram_plan(n, m)[0]
        if work is None and need:
            work = torch.empty(need * w, dtype=a.dtype, device=a.device)
        ring.gram_ntt_dev(out, a, n, m, work, stream)
        return cls(ring, n, out)

    # -- the reference's accessors -----------------------------------------------------------------------------------------------
    def size(self):
        return self._n

    def at(self, i, j):
        """symmetric_matrix.rs:36-44: the element at (i, j), read from (j, i) when j > i (a view of the buffer)."""
        if not (0 <= i < self._n and 0 <= j < self._n):
            raise RingError("SymmetricMatrixNTT.at: index out of range")
        w, e = self.ring.words_per_elem, packed_index(i, j)
        return self.words[e * w:(e + 1) * w]

    def diag(self):
        """symmetric_matrix.rs:56-58: the n diagonal elements, in order."""
        return [self.at(i, i) for i in range(self._n)]

    def rows(self):
        """symmetric_matrix.rs:60-62: row i as a view of its i + 1 elements."""
        w = self.ring.words_per_elem
        return [self.words[i * (i + 1) // 2 * w:(i + 1) * (i + 2) // 2 * w] for i in range(self._n)]

    # -- recompose_left_right_symmetric_matrix ---------------------------------------------------------------------------------------
    def recompose_left_right(self, powers, work=None, stream=None):
        """balanced_decomposition/mod.rs:354-386: G^T self G for G = I_n (x) powers, `powers` holding d ring elements; the result
        has size self.size() / d.  Raises where the reference asserts (d does not divide the size) or divides by zero (d == 0)."""
        ring, w = self.ring, self.ring.words_per_elem
        d = ring._batch_of(powers.size if _is_host(powers) else powers.numel())
        if d == 0 or self._n % d:
            raise RingError("recompose_left_right: the number of powers must divide the matrix size")
        n = self._n // d
        if _is_host(self.words):
            return SymmetricMatrixNTT(ring, n, ring.symm_recompose(self.words, n, d, powers))
        import torch

        out = torch.empty(n * (n + 1) // 2 * w, dtype=self.words.dtype, device=self.words.device)
        need = ring.symm_recompose_plan(n, d)[0]
        if work is None and need:
            work = torch.empty(need * w, dtype=self.words.dtype, device=self.words.device)
        ring.symm_recompose_dev(out, self.words, n, d, powers, work, stream)
        return SymmetricMatrixNTT(ring, n, out)


def recompose_left_right_symmetric_matrix(mat, powers_of_basis, work=None, stream=None):
    """the reference's free function over SymmetricMatrixNTT"""
    return mat.recompose_left_right(powers_of_basis, work, stream)
