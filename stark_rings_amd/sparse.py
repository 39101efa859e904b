"""SparseMatrix<R> (crates/linear_algebra/src/sparse_matrix.rs) over ring elements in CRT/NTT form with the values on the device.

The reference stores rows of (value, column).  Here the rows are flattened into the CSR triple every sparse call of the library
shares (sr_spmv_ntt_dev, wire.py, SparseMultilinearExtension.from_matrix): `vals` is a CUDA tensor of nnz ring elements, the
pattern (`cols`, `row_ptr`) is kept on the host, where the index work runs, and on the device, where the kernels read it.

  SparseMatrix::transpose        ops.rs:46-62                -> transpose (sr_sparse_transpose_pattern + sr_gather_batch_dev)
  SparseMatrix::checked_mul_mat  sparse_matrix.rs:219-275    -> matmul (sr_spgemm_pattern + sr_spgemm_ntt_dev; the entries none of
                                                                whose products is non-zero are dropped with the live flags)
  SparseMatrix::checked_mul_vec  sparse_matrix.rs:201-211    -> mul_vec (sr_spmv_ntt_dev)
  SparseMatrix::to_dense         sparse_matrix.rs:129-137    -> to_dense
`rand`, `hconcat` and the padding helpers build patterns and stay with the caller.
"""
import numpy as np

from .rings import RingError, sparse_transpose_pattern, spgemm_pattern


class SparseMatrixNTT:
    def __init__(self, ring, nrows, ncols, vals, cols, row_ptr):
        """ring: a CyclotomicRing; vals: a CUDA tensor of nnz ring elements (kept, not copied); cols (nnz) and row_ptr (nrows + 1):
        host index arrays."""
        import torch

        self.ring, self.nrows, self.ncols = ring, int(nrows), int(ncols)
        self.cols = np.ascontiguousarray(cols, dtype=np.uint32)
        self.row_ptr = np.ascontiguousarray(row_ptr, dtype=np.uint64)
        if nrows < 0 or ncols < 0 or self.row_ptr.size != nrows + 1 or self.cols.size != int(self.row_ptr[-1]):
            raise RingError("SparseMatrixNTT: row_ptr needs nrows + 1 entries and cols row_ptr[nrows]")
        if vals.numel() != self.cols.size * ring.words_per_elem:
            raise RingError("SparseMatrixNTT: vals does not hold one ring element per stored entry")
        self.vals = vals
        dev = "cuda:%d" % ring.device
        self.d_cols = torch.from_numpy(self.cols.view(np.int32)).to(dev)
        self.d_row_ptr = torch.from_numpy(self.row_ptr.view(np.int64)).to(dev)

    @classmethod
    def from_rows(cls, ring, rows, ncols):
        """rows: the reference's SparseMatrix.coeffs, as CyclotomicRing.spmv_ntt takes them"""
        import torch

        vals, cols, row_ptr, nnz = ring._flatten_rows(rows)
        d_vals = torch.from_numpy(vals[:nnz * ring.words_per_elem].view(np.int64)).to("cuda:%d" % ring.device)
        return cls(ring, len(rows), ncols, d_vals, cols[:nnz], row_ptr)

    def nnz(self):
        return self.cols.size

    def rows(self):
        """SparseMatrix.coeffs with the values copied to the host"""
        return self.ring._rows_of(self.vals.cpu().numpy().view(np.uint64), self.cols, self.row_ptr)

    def transpose(self, stream=None):
        """ops.rs:46-62: row c of the result lists (value, original row) in ascending original row; the rows of self need not be sorted"""
        import torch

        t_row_ptr, t_cols, perm = sparse_transpose_pattern(self.cols, self.row_ptr, self.nrows, self.ncols)
        out = torch.empty_like(self.vals)
        d_perm = torch.from_numpy(perm.view(np.int32)).to(self.vals.device)
        self.ring.gather_dev(out, self.vals, d_perm, stream)
        return SparseMatrixNTT(self.ring, self.ncols, self.nrows, out, t_cols, t_row_ptr)

    def matmul(self, other, stream=None):
        """sparse_matrix.rs:219-275; None where the reference returns None (self.ncols != other.nrows).  Both operands need strictly
        ascending rows (RingError otherwise).  The dead entries are found from the live flags; the context counter is neither read nor
        cleared here, so it gains this product's dead entries like after any spgemm_ntt_dev call and keeps the counts of earlier ones."""
        import torch

        if self.ncols != other.nrows:
            return None
        ring, w, dev = self.ring, self.ring.words_per_elem, self.vals.device
        out_row_ptr, out_cols, pair_ptr, pair_a, pair_b = spgemm_pattern(self.cols, self.row_ptr, self.nrows, self.ncols, other.cols, other.row_ptr,
                                                                         other.ncols)
        n_out = out_cols.size
        out = torch.empty(n_out * w, dtype=self.vals.dtype, device=dev)
        live = torch.empty(n_out, dtype=torch.int32, device=dev)
        d = [torch.from_numpy(x.view(t)).to(dev) for x, t in ((pair_ptr, np.int64), (pair_a, np.int32), (pair_b, np.int32))]
        ring.spgemm_ntt_dev(out, live, self.vals, other.vals, d[0], d[1], d[2], None, stream)
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(dev)):
            keep = live.cpu().numpy().astype(bool)  # ordered behind the kernels on their stream: the one synchronisation of a product
            keep_dev = torch.from_numpy(keep).to(dev)
        if not keep.all():
            # the reference stores an entry iff one of its products is non-zero: drop the others
            with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(dev)):
                out = out.view(n_out, w)[keep_dev].reshape(-1).contiguous()
            kept_before = np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(keep, dtype=np.uint64)])
            out_row_ptr = kept_before[out_row_ptr.astype(np.int64)]
            out_cols = out_cols[keep]
        return SparseMatrixNTT(ring, self.nrows, other.ncols, out, out_cols, out_row_ptr)

    def mul_vec(self, v, stream=None):
        """sparse_matrix.rs:201-211: y = self v for a CUDA tensor of ncols ring elements"""
        import torch

        y = torch.empty(self.nrows * self.ring.words_per_elem, dtype=v.dtype, device=v.device)
        return self.ring.spmv_ntt_dev(y, self.vals, self.d_cols, self.d_row_ptr, v, self.nrows, self.ncols, stream)

    def to_dense(self):
        """sparse_matrix.rs:129-137: the row-major nrows x ncols matrix as a CUDA tensor, zero() where nothing is stored (a later
        duplicate of a position overwrites an earlier one, as in the reference)"""
        import torch

        w = self.ring.words_per_elem
        out = torch.zeros(self.nrows * self.ncols, w, dtype=self.vals.dtype, device=self.vals.device)
        if self.nnz():
            rows = np.repeat(np.arange(self.nrows, dtype=np.int64), np.diff(self.row_ptr.astype(np.int64)))
            flat = rows * self.ncols + self.cols.astype(np.int64)
            last = np.full(self.nrows * self.ncols, -1, dtype=np.int64)
            last[flat] = np.arange(flat.size)          # numpy keeps the last assignment of a repeated index
            hit = np.nonzero(last >= 0)[0]
            out[torch.from_numpy(hit).to(out.device)] = self.vals.view(-1, w)[torch.from_numpy(last[hit]).to(out.device)]
        return out.reshape(-1)
