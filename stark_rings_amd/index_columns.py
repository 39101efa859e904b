"""Integer columns as inputs of a linear combination, and multiplicities counted from indices (sr_lincomb_index_dev,
sr_index_count_dev, include/stark_rings_hip.h; csrc/lincomb_index.hpp):

    out_m[e] = [bit K+J of uses[m]] coef[m][K+J]  +  sum_{k < K, bit k} coef[m][k] * T_k[e]
             + sum_{j < J, bit K+j} coef[m][K+j] * R::from(col_j[e])                                   e < n

A column is one u64 per row (an 8-byte-integer CUDA tensor, or a numpy uint64 array in the host form) or a progression start + e that
occupies no memory.  R::from(x) is the reference's From<u64>: x mod p in every coefficient of a power-of-two ring, in component 0 of
every slot of the reference's own rings.  identity_permutation[_mles] are the reference's fixtures of that name (crates/poly
polynomials/multilinear_polynomial.rs:79-133) from progressions; a permutation sigma stays a u64 column all the way to the leaves
(lookup.permutation_leaves_indexed).
"""
import ctypes

import numpy as np

from .lincomb import MAX_OUTPUTS, MAX_TABLES
from .rings import STARK_POW2, RingError, _np_ptr

MAX_INDEX_COLUMNS = 8
LDS_BINS = 4096   # csrc/lincomb_index.hpp kLdsBins: up to this many bins are counted in LDS


class sr_index_column(ctypes.Structure):
    _fields_ = [("values", ctypes.c_void_p), ("n_evals", ctypes.c_size_t), ("start", ctypes.c_uint64)]


class IndexColumn:
    """values: the stored integers (None: the progression start, start + 1, ..); n_evals: how many of them count (default all), the
    rest of the column is 0.  A stored column has start 0."""

    def __init__(self, values=None, start=0, n_evals=None):
        start = int(start)
        if not 0 <= start < 1 << 64:
            raise RingError("IndexColumn: start is not a u64")
        if values is not None and start != 0:
            raise RingError("IndexColumn: a stored column with a non-zero start")
        if values is None and n_evals is not None:
            raise RingError("IndexColumn: n_evals belongs to a stored column")
        self.values, self.start = values, start
        have = None if values is None else (values.size if isinstance(values, np.ndarray) else values.numel())
        self.n_evals = have if n_evals is None else int(n_evals)
        if values is not None and not 0 <= self.n_evals <= have:
            raise RingError("IndexColumn: the column holds fewer than n_evals values")

    @property
    def is_progression(self):
        return self.values is None


def _column(c):
    return c if isinstance(c, IndexColumn) else IndexColumn(c)


def lincomb_index_plan(ring, n_tables, n_index, n_outputs):
    """sr_lincomb_index_plan: (launches, outputs_per_launch) -- host arithmetic only."""
    launches, per = ctypes.c_int(), ctypes.c_int()
    k = ring.degree.bit_length() - 1 if ring.ring <= STARK_POW2 else 0
    ring._check(ring._lib.sr_lincomb_index_plan(ring.ring, k, int(n_tables), int(n_index), int(n_outputs), ctypes.byref(launches),
                                                ctypes.byref(per)))
    return launches.value, per.value


def _masks(K, J, M, uses):
    """the argument checks that need no buffer; uses None: every output uses everything and the constant"""
    if not 0 <= K <= MAX_TABLES or not 0 <= J <= MAX_INDEX_COLUMNS or not 1 <= K + J <= MAX_TABLES:
        raise RingError("lincomb_index: 0 .. 16 tables, 0 .. 8 index columns, 1 .. 16 of both together")
    if not 1 <= M <= MAX_OUTPUTS:
        raise RingError("lincomb_index: 1 .. 4 outputs")
    T = K + J
    if uses is None:
        uses = [(2 << T) - 1] * M
    uses = [int(u) for u in uses]
    if len(uses) != M:
        raise RingError("lincomb_index: one mask per output")
    seen = 0
    for u in uses:
        if u <= 0:
            raise RingError("lincomb_index: an output with an empty mask")
        if u >> (T + 1):
            raise RingError("lincomb_index: a mask bit above the number of tables and columns")
        seen |= u
    if seen & ((1 << K) - 1) != (1 << K) - 1:
        raise RingError("lincomb_index: a table that no output uses")
    if (seen >> K) & ((1 << J) - 1) != (1 << J) - 1:
        raise RingError("lincomb_index: a column that no output uses")
    return (ctypes.c_uint32 * M)(*uses)


def _evals(K, n, n_evals, stored):
    if n_evals is None:
        n_evals = [n] * K
    if len(n_evals) != K:
        raise RingError("lincomb_index: one n_evals entry per table")
    for k, (ne, have) in enumerate(zip(n_evals, stored)):
        if ne < 0 or ne > n:
            raise RingError("lincomb_index: n_evals[%d] exceeds n" % k)
        if ne > have:
            raise RingError("lincomb_index: table %d holds fewer than n_evals[%d] elements" % (k, k))
    return (ctypes.c_size_t * max(K, 1))(*[int(x) for x in n_evals])


def _columns(cols, n, pointer, spare):
    """the sr_index_column array; pointer(values) -> address; spare: any valid address, for a column that stores nothing"""
    arr = (sr_index_column * max(len(cols), 1))()
    for j, c in enumerate(cols):
        if c.is_progression:
            if n and c.start + (n - 1) >= 1 << 64:
                raise RingError("lincomb_index: a progression wraps past 2^64 - 1")
            arr[j] = sr_index_column(None, 0, c.start)
        else:
            if c.n_evals > n:
                raise RingError("lincomb_index: column %d: n_evals exceeds n" % j)
            arr[j] = sr_index_column(pointer(c.values) if c.n_evals else spare, c.n_evals, 0)
    return arr


def lincomb_index_dev(ring, outs, tables, columns, coef, uses, n, n_evals=None, stream=None):
    """sr_lincomb_index_dev.  outs: 1 .. 4 CUDA tensors of at least n elements; tables: 0 .. 16 CUDA tensors as in lincomb_dev; columns:
    0 .. 8 IndexColumn (or 8-byte-integer CUDA tensors, taken whole); coef: len(outs) x (len(tables) + len(columns) + 1) elements,
    row-major -- tables, columns, the constant; uses: one bit mask per output in that order (None: everything).  Allocates nothing."""
    w = ring.words_per_elem
    cols = [_column(c) for c in columns]
    K, J, M = len(tables), len(cols), len(outs)
    masks = _masks(K, J, M, uses)
    n = int(n)
    if n < 0:
        raise RingError("lincomb_index: negative n")
    sizes = _evals(K, n, n_evals, [t.numel() // w for t in tables])
    pc, nc = ring._dev(coef)
    if nc != M * (K + J + 1) * w:
        raise RingError("lincomb_index: coef must hold len(outs) x (len(tables) + len(columns) + 1) elements")
    po, pt = (ctypes.c_void_p * M)(), (ctypes.c_void_p * max(K, 1))()
    for m, o in enumerate(outs):
        if o.numel() < n * w:
            raise RingError("lincomb_index: output %d holds fewer than n elements" % m)
        po[m] = ring._dev(o)[0]
    for k, t in enumerate(tables):
        pt[k] = ring._dev(t)[0] if t.numel() else pc.value   # a table that stores nothing is never read: any non-null pointer
    arr = _columns(cols, n, lambda v: ring._dev(v)[0].value, pc.value)
    ring._check(ring._lib.sr_lincomb_index_dev(ring._ctx, po, M, pt, sizes, K, arr, J, pc, masks, n, ring._stream(stream)))
    return outs


def lincomb_index(ring, tables, columns, coef, uses, n, n_outputs=None, n_evals=None):
    """Host buffers: sr_lincomb_index (see lincomb_index_dev).  tables, column values: numpy uint64 arrays; returns the list of
    n_outputs arrays of n elements (n_outputs defaults to len(uses))."""
    w = ring.words_per_elem
    tables = [np.ascontiguousarray(t, dtype=np.uint64).reshape(-1) for t in tables]
    cols = []
    for c in (_column(c) for c in columns):   # contiguous uint64 copies of the stored values: the caller's objects stay as they are
        cols.append(c if c.is_progression else IndexColumn(np.ascontiguousarray(c.values, dtype=np.uint64).reshape(-1), n_evals=c.n_evals))
    coef = np.ascontiguousarray(coef, dtype=np.uint64).reshape(-1)
    K, J = len(tables), len(cols)
    M = int(n_outputs) if n_outputs is not None else (len(uses) if uses is not None else 1)
    masks = _masks(K, J, M, uses)
    n = int(n)
    if n < 0:
        raise RingError("lincomb_index: negative n")
    sizes = _evals(K, n, n_evals, [t.size // w for t in tables])
    if coef.size != M * (K + J + 1) * w:
        raise RingError("lincomb_index: coef must hold n_outputs x (len(tables) + len(columns) + 1) elements")
    outs = [np.empty(max(n * w, 1), dtype=np.uint64) for _ in range(M)]
    z = np.zeros(1, dtype=np.uint64)
    po, pt = (ctypes.c_void_p * M)(), (ctypes.c_void_p * max(K, 1))()
    for m, o in enumerate(outs):
        po[m] = o.ctypes.data
    for k, t in enumerate(tables):
        pt[k] = t.ctypes.data if t.size else z.ctypes.data
    arr = _columns(cols, n, lambda v: v.ctypes.data, z.ctypes.data)
    ring._check(ring._lib.sr_lincomb_index(ring._ctx, po, M, pt, sizes, K, arr, J, _np_ptr(coef), masks, n))
    return [o[:n * w] for o in outs]


def _one(ring, like):
    """the ring's one in CRT/NTT form on the device of `like`: what sr_product_batch returns for no element"""
    import torch

    out = torch.empty(ring.words_per_elem, dtype=torch.int64, device=like.device)
    ring.product_dev(out, out[:0])
    return out


def from_u64_dev(ring, column, n, out=None, stream=None, like=None):
    """The table R::from(col[e]), e < n: one call with no table, one column and the coefficient one().  like: a CUDA tensor that names
    the device when neither the column nor `out` does."""
    import torch

    col = _column(column)
    where = out if out is not None else (col.values if col.values is not None else like)
    if where is None:
        raise RingError("from_u64_dev: a progression needs `out` or `like` to name the device")
    one = _one(ring, where)
    if out is None:
        out = torch.empty(int(n) * ring.words_per_elem, dtype=torch.int64, device=where.device)
    rows = torch.cat([one, one])   # the constant's entry is never read
    if stream is not None:
        for t in (one, rows, out):
            t.record_stream(stream)
    lincomb_index_dev(ring, [out], [], [col], rows, [0b01], n, None, stream)
    return out


def identity_permutation(ring, num_vars, num_chunks, like):
    """The reference's identity_permutation: the table R::from(0), R::from(1), .., R::from(num_chunks 2^num_vars - 1)."""
    return from_u64_dev(ring, IndexColumn(start=0), int(num_chunks) << int(num_vars), like=like)


def identity_permutation_mles(ring, num_vars, num_chunks, like):
    """The reference's identity_permutation_mles: num_chunks DenseMultilinearExtensions of num_vars variables, chunk i holding
    R::from(i 2^num_vars + e)."""
    from .mle import DenseMultilinearExtension

    size = 1 << int(num_vars)
    return [DenseMultilinearExtension(ring, int(num_vars), from_u64_dev(ring, IndexColumn(start=i * size), size, like=like))
            for i in range(int(num_chunks))]


class IndexMultilinearExtension:
    """A multilinear extension in num_vars variables whose evaluations are an IndexColumn: evaluation e is R::from(col[e]), a stored
    column's beyond n_evals are zero.  A factor of a VirtualPolynomial (mle.py): the weighted sum-check rounds read it as one u64 per
    row (sr_vpoly_iwround_*), everything else expands it with to_dense() first.  A stored column's values are a CUDA tensor of
    8-byte integers."""

    def __init__(self, ring, num_vars, column):
        self.ring, self._num_vars = ring, int(num_vars)
        if not 0 <= self._num_vars < 48:
            raise RingError("IndexMultilinearExtension: num_vars must be below 48")
        self.column = col = _column(column)
        full = 1 << self._num_vars
        if col.is_progression:
            if col.start + (full - 1) >= 1 << 64:
                raise RingError("IndexMultilinearExtension: a progression wraps past 2^64 - 1")
        else:
            if isinstance(col.values, np.ndarray) or not (col.values.is_cuda and col.values.is_contiguous() and col.values.element_size() == 8):
                raise RingError("IndexMultilinearExtension: the values are a contiguous CUDA tensor of 8-byte integers")
            if col.n_evals > full:
                raise RingError("IndexMultilinearExtension: n_evals exceeds 2^num_vars")

    @property
    def num_vars(self):
        return self._num_vars

    def __len__(self):
        """the stored evaluations: n_evals, or 2^num_vars of a progression"""
        return (1 << self._num_vars) if self.column.is_progression else self.column.n_evals

    def key(self):
        """what tells two columns apart as slots of a VirtualPolynomial"""
        c = self.column
        if c.is_progression:
            return ("progression", c.start)
        return ("column", c.values.data_ptr(), c.n_evals) if c.n_evals else ("empty", id(self))

    def to_dense(self, stream=None):
        """The DenseMultilinearExtension of the same evaluations: from_u64_dev over the stored part, D words per integer."""
        import torch

        from .mle import DenseMultilinearExtension

        n = len(self)
        out = torch.empty(n * self.ring.words_per_elem, dtype=torch.int64, device=torch.device("cuda", self.ring.device))
        if stream is not None:
            out.record_stream(stream)
        if n:
            from_u64_dev(self.ring, self.column, n, out=out, stream=stream)
        return DenseMultilinearExtension(self.ring, self._num_vars, out)


def index_count_dev(ring, idx, n_bins, out=None, stream=None):
    """sr_index_count_dev: counts[t] = #{ i : idx[i] == t } for t < n_bins as an int64 CUDA tensor (`out`, or a new one).  idx: a CUDA
    tensor of 8-byte integers read as u64.  An index >= n_bins is skipped and counted (ring.spmv_bad_index_count)."""
    import torch

    n_bins = int(n_bins)
    pi, n = ring._dev(idx)
    if out is None:
        out = torch.empty(n_bins, dtype=torch.int64, device=idx.device)
        if stream is not None:
            out.record_stream(stream)
    po, have = ring._dev(out)
    if have < n_bins:
        raise RingError("index_count: out holds fewer than n_bins counts")
    ring._check(ring._lib.sr_index_count_dev(ring._ctx, po if n_bins else None, pi if n else None, n, n_bins, ring._stream(stream)))
    return out


def index_count(ring, idx, n_bins):
    """Host buffers: sr_index_count.  An index >= n_bins is an error here."""
    idx = np.ascontiguousarray(idx, dtype=np.uint64).reshape(-1)
    counts = np.zeros(max(int(n_bins), 1), dtype=np.uint64)
    ring._check(ring._lib.sr_index_count(ring._ctx, _np_ptr(counts), _np_ptr(idx), idx.size, int(n_bins)))
    return counts[:int(n_bins)]
