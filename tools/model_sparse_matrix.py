"""Pure-Python restatement of SparseMatrix (crates/linear_algebra/src/sparse_matrix.rs: to_dense 129-137, from_dense 139-156,
checked_mul_mat 219-275) and of Transpose (ops.rs:9-62), line by line and generic over the element type: the caller supplies add,
mul, is_zero and zero, so the same code runs on Python integers modulo a prime (tests/test_spgemm_host.py pins it against dense
products) and on ring elements held as numpy arrays (the expected values of tests/test_spgemm_gpu.py).  structural_product
restates what sr_spgemm_pattern writes: the value-independent pattern with its pair lists.  No kernel, no library call.
"""


class SparseMatrix:
    """sparse_matrix.rs:17-22: coeffs[i] is the list of (value, column) of row i"""

    def __init__(self, nrows, ncols, coeffs):
        self.nrows, self.ncols, self.coeffs = nrows, ncols, [list(r) for r in coeffs]
        assert len(self.coeffs) == nrows

    def to_dense(self, zero):  # :129-137 (a later duplicate overwrites an earlier one)
        s = [[zero for _ in range(self.ncols)] for _ in range(self.nrows)]
        for i, row in enumerate(self.coeffs):
            for value, col in row:
                s[i][col] = value
        return s

    @classmethod
    def from_dense(cls, rows, is_zero):  # :139-156
        ncols = len(rows[0]) if rows else 0
        return cls(len(rows), ncols, [[(v, c) for c, v in enumerate(row) if not is_zero(v)] for row in rows])

    def transpose(self):  # ops.rs:46-62
        res = [[] for _ in range(self.ncols)]
        for row_idx, row in enumerate(self.coeffs):
            for value, col_idx in row:
                res[col_idx].append((value, row_idx))   # col_idx >= ncols: the reference panics, here IndexError
        return SparseMatrix(self.ncols, self.nrows, res)

    def checked_mul_mat(self, m, add, mul, is_zero):  # :219-275
        if self.ncols != m.nrows:
            return None
        m_cols = [[] for _ in range(m.ncols)]
        for row_idx, row in enumerate(m.coeffs):
            for val, col_idx in row:
                m_cols[col_idx].append((val, row_idx))
        coeffs = []
        for row in self.coeffs:
            res_row = []
            for j, col in enumerate(m_cols):
                total, a, b = None, 0, 0
                while a < len(row) and b < len(col):
                    (r_val, r_idx), (c_val, c_idx) = row[a], col[b]
                    if r_idx < c_idx:
                        a += 1
                    elif r_idx > c_idx:
                        b += 1
                    else:
                        product = mul(r_val, c_val)
                        if not is_zero(product):
                            total = product if total is None else add(total, product)
                        a += 1
                        b += 1
                if total is not None:
                    res_row.append((total, j))
            coeffs.append(res_row)
        return SparseMatrix(self.nrows, m.ncols, coeffs)

    # -- the flattened (CSR) form the C ABI takes -------------------------------------------------------------------------------------
    def csr(self):
        """(vals, cols, row_ptr): the rows flattened, row_ptr[i] .. row_ptr[i + 1] the entries of row i"""
        vals, cols, row_ptr = [], [], [0]
        for row in self.coeffs:
            for v, c in row:
                vals.append(v)
                cols.append(c)
            row_ptr.append(len(vals))
        return vals, cols, row_ptr

    @classmethod
    def from_csr(cls, nrows, ncols, vals, cols, row_ptr):
        return cls(nrows, ncols, [[(vals[t], cols[t]) for t in range(row_ptr[i], row_ptr[i + 1])] for i in range(nrows)])


def transpose_dense(rows, zero):
    """Transpose for Vec<Vec<R>> (ops.rs:13-33): short rows padded with zero.  Matrix::transpose (:36-44) wraps it and copies
    nrows / ncols UNSWAPPED; the data is the ncols x nrows matrix returned here."""
    ncols = max((len(r) for r in rows), default=0)
    res = [[] for _ in range(ncols)]
    for row in rows:
        for c, value in enumerate(row):
            res[c].append(value)
        for c in range(len(row), ncols):
            res[c].append(zero)
    return res


def transpose_pattern(cols, row_ptr, nrows, ncols):
    """what sr_sparse_transpose_pattern writes: (t_row_ptr, t_cols, perm) with t_vals[t] = vals[perm[t]] -- SparseMatrix::transpose on
    (position, column) pairs"""
    m = SparseMatrix.from_csr(nrows, ncols, list(range(len(cols))), cols, row_ptr).transpose()
    perm, t_cols, t_row_ptr = m.csr()
    return t_row_ptr, t_cols, perm


def structural_product(a_cols, a_row_ptr, n, m, b_cols, b_row_ptr, p):
    """what sr_spgemm_pattern writes for operands whose rows ascend strictly: (out_row_ptr, out_cols, pair_ptr, pair_a, pair_b) -- the
    merge-join of checked_mul_mat on positions instead of values, an entry stored iff the index lists intersect"""
    b_colsT = [[] for _ in range(p)]
    for k in range(m):
        for t in range(b_row_ptr[k], b_row_ptr[k + 1]):
            b_colsT[b_cols[t]].append((t, k))
    out_row_ptr, out_cols, pair_ptr, pair_a, pair_b = [0], [], [0], [], []
    for i in range(n):
        row = [(t, a_cols[t]) for t in range(a_row_ptr[i], a_row_ptr[i + 1])]
        for j, col in enumerate(b_colsT):
            x, y, found = 0, 0, False
            while x < len(row) and y < len(col):
                if row[x][1] < col[y][1]:
                    x += 1
                elif row[x][1] > col[y][1]:
                    y += 1
                else:
                    pair_a.append(row[x][0])
                    pair_b.append(col[y][0])
                    found = True
                    x += 1
                    y += 1
            if found:
                out_cols.append(j)
                pair_ptr.append(len(pair_a))
        out_row_ptr.append(len(out_cols))
    return out_row_ptr, out_cols, pair_ptr, pair_a, pair_b


def product_by_pairs(pattern, a_vals, b_vals, add, mul, is_zero, zero):
    """the numeric phase on a structural pattern: (values, live) per entry -- value = the sum of ALL products (zero ones change
    nothing), live = some product is non-zero"""
    _, _, pair_ptr, pair_a, pair_b = pattern
    vals, live = [], []
    for e in range(len(pair_ptr) - 1):
        acc, alive = zero, False
        for t in range(pair_ptr[e], pair_ptr[e + 1]):
            prod = mul(a_vals[pair_a[t]], b_vals[pair_b[t]])
            alive = alive or not is_zero(prod)
            acc = add(acc, prod)
        vals.append(acc)
        live.append(1 if alive else 0)
    return vals, live
