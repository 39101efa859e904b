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


class LookupHelperColumns:
    """logUp in its helper-column form: instead of two fraction trees (one sum-check per layer and side) the prover holds the inverse
    columns h_w = 1 / witness_q and h_t = multiplicities / table_q themselves (two sr_inverse_batch_dev calls), shows
    sum_b eq(z, b) (h q - num)(b) = 0 with ONE zero-check per side (zero_claim, EqSumCheck) and compares sum h_w with sum h_t.

    Unlike LookupCheck.holds -- a polynomial identity in beta that needs no inverse and excludes no challenge -- this form DOES exclude
    the challenges that hit a denominator: a zero slot of witness_q or table_q has no inverse, its helper slot is zero, and holds() is
    false whatever the sums say (zero_slots counts them).

    The zero slots are read from the context's counter (sr_inverse_zero_count), which the constructor reads twice: once before its two
    calls, so that zero_slots and holds() speak of this lookup alone, and once after them.  The first read clears what earlier inverse
    calls on the same context left unread; that number is not lost but kept in zero_slots_before for the caller who still wanted it.

    Both sides must be stored in full, n_w == 2^num_vars_w and n_t == 2^num_vars_t: a truncated side is refused.  The fraction trees
    count a missing row as the fraction 0 / 1, with q = one().  A caller with fewer rows writes the padding out and passes the full
    form.  On the table side q = one() and m = zero() give h = 0: the claim h q - m holds there and the sum is unchanged.  On the
    witness side q = one() gives h = 1 and the claim h q - 1 holds there, but every padded row adds one() to sum h_w, which the fraction
    tree does not count: the caller subtracts the number of padded rows from sum h_w, or pads the witness with copies of a row that is
    in the table and counts them in the multiplicities, after which holds() is the check as it stands."""

    def __init__(self, ring, witness_q, table_q, multiplicities, num_vars_w, num_vars_t, n_w=None, n_t=None, stream=None):
        import torch

        from .inverse import inverse_dev, inverse_zero_count
        from .mle import DenseMultilinearExtension

        w = ring.words_per_elem
        rows_w = ring._batch_of(witness_q.numel()) if n_w is None else int(n_w)
        rows_t = ring._batch_of(table_q.numel()) if n_t is None else int(n_t)
        if rows_w != 1 << num_vars_w or rows_t != 1 << num_vars_t:
            raise RingError("LookupHelperColumns: a truncated side is refused: store all 2^num_vars rows (pad q with one(), the "
                            "multiplicities with zero())")
        if witness_q.numel() < rows_w * w or table_q.numel() < rows_t * w or multiplicities.numel() < rows_t * w:
            raise RingError("LookupHelperColumns: a column holds fewer rows than its side")
        self.ring, self.stream = ring, stream
        self.num_vars_w, self.num_vars_t = int(num_vars_w), int(num_vars_t)
        self.witness_q, self.table_q = witness_q[:rows_w * w], table_q[:rows_t * w]
        self.multiplicities = multiplicities[:rows_t * w]
        self.h_w, self.h_t = torch.empty_like(self.witness_q), torch.empty_like(self.table_q)
        one = _one(ring, witness_q)
        self.minus_one = one.clone()
        ring.neg_dev(self.minus_one, stream)
        self.ones = one.repeat(rows_w)      # the numerators of the witness side, as a table: the claim h q - 1 needs it as an MLE
        if stream is not None:
            for t in (self.h_w, self.h_t, self.minus_one, self.ones):
                t.record_stream(stream)
        # a count an earlier call on this context left unread is not this lookup's: it is taken out first and kept for the caller
        self.zero_slots_before = inverse_zero_count(ring, stream)
        inverse_dev(ring, self.h_w, self.witness_q, None, rows_w, stream=stream)
        inverse_dev(ring, self.h_t, self.table_q, self.multiplicities, rows_t, stream=stream)
        self.zero_slots = inverse_zero_count(ring, stream)   # the zero slots of witness_q and table_q
        self._mle = lambda t, nv: DenseMultilinearExtension(ring, nv, t)

    @classmethod
    def from_indices(cls, ring, witness_q, table_q, indices, num_vars_w, num_vars_t, n_w=None, n_t=None, stream=None):
        """As LookupCheck.from_indices: the multiplicities are counted on the device from indices[i], the table row of witness row i."""
        rows_t = ring._batch_of(table_q.numel()) if n_t is None else int(n_t)
        counts = index_count_dev(ring, indices, rows_t, stream=stream)
        mult = from_u64_dev(ring, counts, rows_t, stream=stream)
        return cls(ring, witness_q, table_q, mult, num_vars_w, num_vars_t, n_w, n_t, stream)

    def sums(self):
        """(sum_i h_w[i], sum_j h_t[j]): one ring element each (sr_sum_batch_dev)"""
        import torch

        w = self.ring.words_per_elem
        a, b = torch.empty_like(self.h_w[:w]), torch.empty_like(self.h_w[:w])
        self.ring.sum_dev(a, self.h_w, self.stream)
        self.ring.sum_dev(b, self.h_t, self.stream)
        return a, b

    def holds(self):
        """the two sums agree and no denominator had a zero slot (compared on the host; synchronises)"""
        a, b = self.sums()
        return _same(a, b) and self.zero_slots == 0

    def zero_claim(self, side):
        """The VirtualPolynomial h q - 1 (side 0 / "witness") or h q - m (side 1 / "table"): it vanishes on the whole cube exactly when
        h is the inverse column, so EqSumCheck(zero_claim(side), z) with a random z proves it with a claimed sum of zero."""
        from .mle import VirtualPolynomial

        if side in (0, "witness"):
            nv, h, q, num = self.num_vars_w, self.h_w, self.witness_q, self.ones
        else:
            nv, h, q, num = self.num_vars_t, self.h_t, self.table_q, self.multiplicities
        g = VirtualPolynomial(self.ring, nv)
        g.add_mle_list([self._mle(h, nv), self._mle(q, nv)]).add_mle_list([self._mle(num, nv)], self.minus_one)
        return g
