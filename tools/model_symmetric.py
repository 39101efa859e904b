"""Pure-Python restatement of SymmetricMatrix (crates/linear_algebra/src/symmetric_matrix.rs:17-62, from_par_fn 76-90) and of
recompose_left_right_symmetric_matrix (crates/ring/src/balanced_decomposition/mod.rs:358-386), line by line and generic over the
element type: the caller supplies add, mul and zero, so the same code runs on Python integers modulo a prime
(tests/test_symm_host.py pins it against full dense matrices) and on ring elements held as numpy arrays (the expected values of
tests/test_symm_gpu.py).  No kernel, no library call.
"""


class SymmetricMatrix:
    """symmetric_matrix.rs:14-15: rows[i] holds the i + 1 entries (i, 0) .. (i, i)"""

    def __init__(self, rows, checked=True):
        rows = [list(r) for r in rows]
        if checked:  # From<Vec<Vec<F>>>, symmetric_matrix.rs:17-22
            assert all(len(r) == i + 1 for i, r in enumerate(rows)), \
                "cannot convert value: Vec<Vec<F>> to SymmetricMatrix<F>, row has wrong number of entries"
        self._rows = rows

    @classmethod
    def zero(cls, n, zero):  # symmetric_matrix.rs:24-28
        return cls([[zero for _ in range(i + 1)] for i in range(n)])

    def size(self):  # :31-34
        return len(self._rows)

    def at(self, i, j):  # :36-44
        assert i < len(self._rows) and j < len(self._rows)
        return self._rows[i][j] if j <= i else self._rows[j][i]

    def diag(self):  # :56-58
        return [self.at(i, i) for i in range(self.size())]

    def rows(self):  # :60-62
        return self._rows

    @classmethod
    def from_fn(cls, size, func):  # from_par_fn, :76-90: row i is func(i, 0) .. func(i, i)
        return cls([[func(i, j) for j in range(i + 1)] for i in range(size)])

    def packed(self):
        """the rows flattened: entry (i, j), j <= i, at position i (i + 1) / 2 + j"""
        return [e for row in self._rows for e in row]

    @classmethod
    def from_packed(cls, n, elems):
        assert len(elems) == n * (n + 1) // 2
        return cls([elems[i * (i + 1) // 2:(i + 1) * (i + 2) // 2] for i in range(n)])


def total(terms, add, zero):
    """Iterator::sum: zero() + t_0 + t_1 + ..."""
    acc = zero
    for t in terms:
        acc = add(acc, t)
    return acc


def gram(a, n, m, add, mul, zero):
    """from_par_fn(n, |i, j| <a_i, a_j>) for the n rows of m elements of `a` (a flat list of n * m elements, row-major)"""
    assert len(a) == n * m
    return SymmetricMatrix.from_fn(n, lambda i, j: total((mul(a[i * m + t], a[j * m + t]) for t in range(m)), add, zero))


def recompose_left_right_symmetric_matrix(mat, powers_of_basis, add, mul, zero):
    """balanced_decomposition/mod.rs:358-386"""
    andd, d = mat.size(), len(powers_of_basis)
    assert andd % d == 0                      # :365 (d == 0: the remainder panics)
    n = andd // d
    rows = []
    for i in range(n):                        # :368
        row = []
        for j in range(i + 1):                # :370
            terms = []
            for k in (k for k in range(andd) if k // d == i):          # :373
                for l in (l for l in range(andd) if l // d == j):      # :375
                    terms.append(mul(mat.at(k, l), mul(powers_of_basis[k % d], powers_of_basis[l % d])))  # :376
            row.append(total(terms, add, zero))                        # :379
        rows.append(row)
    return SymmetricMatrix(rows)              # .into(), :383-384


def wire_frame(rows, elem_bytes):
    """the derived Vec<Vec<F>> framing of symmetric_matrix.rs:116-132: u64 row count, per row a u64 length and the elements'
    bytes (elem_bytes(e) -> bytes)"""
    out = len(rows).to_bytes(8, "little")
    for row in rows:
        out += len(row).to_bytes(8, "little") + b"".join(elem_bytes(e) for e in row)
    return out


def wire_unframe(data, elem_size, elem_from):
    """-> rows; no row-length check, as symmetric_matrix.rs:142-154 (`.map(Self)`)"""
    nrows, pos, rows = int.from_bytes(data[:8], "little"), 8, []
    for _ in range(nrows):
        n, pos = int.from_bytes(data[pos:pos + 8], "little"), pos + 8
        rows.append([elem_from(data[pos + e * elem_size:pos + (e + 1) * elem_size]) for e in range(n)])
        pos += n * elem_size
    assert pos == len(data)
    return rows
