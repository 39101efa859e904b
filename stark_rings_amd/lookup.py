"""Permutation and lookup checks end to end on device-resident tables: the leaves (sr_lincomb_dev, lincomb.py; from integer columns
sr_lincomb_index_dev, index_columns.py), the multiplicities of a lookup (sr_index_count_dev), the layered circuits
(ProductTree, FractionTree) and their layer claims (EqSumCheck).  Thin builders over those calls; nothing here computes on the host
except the comparison of two root elements.

  permutation / multiset equality   prod_e (beta + f[e] + gamma id[e]) == prod_e (beta + f[e] + gamma sigma[e]), one pair of leaf
                                    tables per wire column, all columns in one tree per side
  logUp lookup                      sum_i 1 / (beta - w_i) == sum_j m_j / (beta - t_j) with w_i, t_j fingerprints of the witness and
                                    table rows; cross-multiplied, P_w Q_t == P_t Q_w, a polynomial identity in beta that needs no inverse
"""
from .frac_tree import FractionTree
from .grand_product import ProductTree
from .index_columns import IndexColumn, _column, _one, from_u64_dev, index_count_dev, lincomb_index_dev
from .lincomb import lincomb_dev
from .rings import MLE_TRAILING, RingError


def fingerprint(ring, columns, coeffs, const=None, stream=None, out=None):
    """One table sum_k coeffs[k] * columns[k] (+ const) from 1 .. 16 column tables of equal length, in one pass.  coeffs: a tensor of
    len(columns) ring elements; const: one ring element or None.  Returns the new table (or `out`)."""
    import torch

    w, K = ring.words_per_elem, len(columns)
    n = ring._batch_of(columns[0].numel())
    if any(c.numel() != n * w for c in columns):
        raise RingError("fingerprint: the columns differ in length")
    if coeffs.numel() != K * w or (const is not None and const.numel() != w):
        raise RingError("fingerprint: one coefficient per column, and a constant of one ring element")
    rows = torch.cat([coeffs.reshape(-1), const.reshape(-1) if const is not None else coeffs.new_zeros(w)])
    if out is None:
        out = torch.empty(n * w, dtype=columns[0].dtype, device=columns[0].device)
    if stream is not None:
        rows.record_stream(stream)
        out.record_stream(stream)
    mask = (1 << K) - 1 | (1 << K if const is not None else 0)
    lincomb_dev(ring, [out], list(columns), rows, [mask], n, None, stream)
    return out


def permutation_leaves(ring, f, ident, sigma, beta, gamma, stream=None, num=None, den=None):
    """(num, den) = (beta + f + gamma id, beta + f + gamma sigma) from ONE call over the three tables (K = 3, M = 2): the mask of each
    row leaves out the table it does not use.  beta, gamma: one ring element each.  num / den: where to write (slices of two leaf
    tensors when called per wire column), default new tensors."""
    import torch

    w = ring.words_per_elem
    n = ring._batch_of(f.numel())
    if ident.numel() != n * w or sigma.numel() != n * w:
        raise RingError("permutation_leaves: the tables differ in length")
    if beta.numel() != w or gamma.numel() != w:
        raise RingError("permutation_leaves: beta and gamma are one ring element each")
    one = _one(ring, f)
    g, b = gamma.reshape(-1), beta.reshape(-1)
    rows = torch.cat([one, g, g, b, one, g, g, b])   # rows (f, id, sigma, const); the entry a mask drops is never read
    if num is None:
        num = torch.empty_like(f)
    if den is None:
        den = torch.empty_like(f)
    if stream is not None:
        for t in (rows, num, den):
            t.record_stream(stream)
    lincomb_dev(ring, [num, den], [f, ident, sigma], rows, [0b1011, 0b1101], n, None, stream)
    return num, den


def fingerprint_indexed(ring, tables, columns, coeffs, const=None, n=None, stream=None, out=None):
    """fingerprint() with integer columns beside the tables: sum_k coeffs[k] * tables[k] + sum_j coeffs[K + j] * R::from(columns[j])
    (+ const) in one pass (sr_lincomb_index_dev).  columns: IndexColumn or u64 tensors; n: the rows, needed when there is no table
    and no stored column to take it from."""
    import torch

    w, K = ring.words_per_elem, len(tables)
    cols = [_column(c) for c in columns]
    if n is None:
        n = ring._batch_of(tables[0].numel()) if tables else max([c.n_evals for c in cols if not c.is_progression], default=None)
    if n is None:
        raise RingError("fingerprint_indexed: n is needed when every input is a progression")
    if any(t.numel() != n * w for t in tables):
        raise RingError("fingerprint_indexed: the tables differ in length")
    T = K + len(cols)
    if coeffs.numel() != T * w or (const is not None and const.numel() != w):
        raise RingError("fingerprint_indexed: one coefficient per table and column, and a constant of one ring element")
    rows = torch.cat([coeffs.reshape(-1), const.reshape(-1) if const is not None else coeffs.new_zeros(w)])
    if out is None:
        out = torch.empty(n * w, dtype=coeffs.dtype, device=coeffs.device)
    if stream is not None:
        rows.record_stream(stream)
        out.record_stream(stream)
    mask = (1 << T) - 1 | (1 << T if const is not None else 0)
    lincomb_index_dev(ring, [out], list(tables), cols, rows, [mask], n, None, stream)
    return out


def permutation_leaves_indexed(ring, f, sigma_idx, beta, gamma, id_start=0, stream=None, num=None, den=None):
    """permutation_leaves() with id and sigma as integers: (num, den) = (beta + f + gamma R::from(id_start + e), beta + f + gamma
    R::from(sigma_idx[e])) from ONE call with K = 1, J = 2, M = 2.  id is a progression and reads nothing; sigma_idx is a tensor of n
    u64.  Per wire column c of 2^v rows, id_start = c 2^v."""
    import torch

    w = ring.words_per_elem
    n = ring._batch_of(f.numel())
    if sigma_idx.numel() != n:
        raise RingError("permutation_leaves_indexed: sigma_idx holds one integer per row of f")
    if beta.numel() != w or gamma.numel() != w:
        raise RingError("permutation_leaves_indexed: beta and gamma are one ring element each")
    one = _one(ring, f)
    g, b = gamma.reshape(-1), beta.reshape(-1)
    rows = torch.cat([one, g, g, b, one, g, g, b])   # rows (f, id, sigma, const); the entry a mask drops is never read
    if num is None:
        num = torch.empty_like(f)
    if den is None:
        den = torch.empty_like(f)
    if stream is not None:
        for t in (rows, num, den):
            t.record_stream(stream)
    lincomb_index_dev(ring, [num, den], [f], [IndexColumn(start=id_start), IndexColumn(sigma_idx)], rows, [0b1011, 0b1101], n, None, stream)
    return num, den


def _same(a, b):
    import torch

    return bool(torch.equal(a, b))


class PermutationCheck:
    def __init__(self, ring, num_leaves, den_leaves, num_vars, n_leaves=None, stream=None):
        """Two ProductTrees in trailing order over the numerator and denominator leaves (CUDA tensors, the first n_leaves stored,
        the rest one())."""
        self.ring = ring
        self.num = ProductTree(ring, num_leaves, num_vars, n_leaves, MLE_TRAILING, stream)
        self.den = ProductTree(ring, den_leaves, num_vars, n_leaves, MLE_TRAILING, stream)

    def roots(self):
        """(prod num, prod den): one ring element each (views)"""
        return self.num.root(), self.den.root()

    def holds(self):
        """the two grand products agree (compared on the host; synchronises)"""
        a, b = self.roots()
        return _same(a, b)

    def layer_claim(self, side, k, z, lam=None, stream=None):
        """ProductTree.layer_claim of one side: side 0 / "num" or 1 / "den" """
        tree = self.num if side in (0, "num") else self.den
        return tree.layer_claim(k, z, lam, stream)


class LookupCheck:
    def __init__(self, ring, witness_q, table_q, multiplicities, num_vars_w, num_vars_t, n_w=None, n_t=None, stream=None):
        """Two FractionTrees in trailing order: the witness side sums 1 / witness_q[i] (no stored numerators), the table side sums
        multiplicities[j] / table_q[j].  The multiplicities are ring elements supplied by the caller: counting them is index work."""
        self.ring = ring
        self.stream = stream
        self.witness = FractionTree(ring, None, witness_q, num_vars_w, n_w, MLE_TRAILING, stream)
        self.table = FractionTree(ring, multiplicities, table_q, num_vars_t, n_t, MLE_TRAILING, stream)

    @classmethod
    def from_indices(cls, ring, witness_q, table_q, indices, num_vars_w, num_vars_t, n_w=None, n_t=None, stream=None):
        """The check with its multiplicities counted on the device: indices[i] (u64, one per stored witness row) is the table row that
        witness row i was taken from; the numerators of the table side are R::from(count[j]) (sr_index_count_dev, then
        from_u64_dev).  An index at or beyond the table's stored rows is skipped and counted (ring.spmv_bad_index_count)."""
        rows_t = ring._batch_of(table_q.numel()) if n_t is None else int(n_t)
        counts = index_count_dev(ring, indices, rows_t, stream=stream)
        mult = from_u64_dev(ring, counts, rows_t, stream=stream)
        return cls(ring, witness_q, table_q, mult, num_vars_w, num_vars_t, n_w, n_t, stream)

    def roots(self):
        """((P_w, Q_w), (P_t, Q_t))"""
        return self.witness.root(), self.table.root()

    def holds(self):
        """P_w Q_t == P_t Q_w, two single-element products on the device: a polynomial identity in beta that holds for every beta
        when the multisets match, zero denominators included -- no inverse, no excluded challenge.  Synchronises."""
        import torch

        (pw, qw), (pt, qt) = self.roots()
        w = self.ring.words_per_elem
        lhs, rhs = torch.empty_like(pw[:w]), torch.empty_like(pw[:w])
        self.ring.product_dev(lhs, torch.cat([pw[:w], qt[:w]]), self.stream)
        self.ring.product_dev(rhs, torch.cat([pt[:w], qw[:w]]), self.stream)
        return _same(lhs, rhs)

    def layer_claim(self, side, k, z, lam=None, stream=None):
        """FractionTree.layer_claim of one side: side 0 / "witness" or 1 / "table" """
        tree = self.witness if side in (0, "witness") else self.table
        return tree.layer_claim(k, z, lam, stream)
