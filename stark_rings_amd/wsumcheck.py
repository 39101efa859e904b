"""The device-pointer forms of the weighted sum-check rounds (sr_vpoly_wround_evals_dev, sr_vpoly_wround_fold_evals_dev;
include/stark_rings_hip.h) as functions of this module: the eq(z, .) factor of a zero-check as one ring element per pair that is constant
in the round's variable, not as one more table.  The plans and the host-pointer forms are methods of CyclotomicRing
(vpoly_wround_plan, vpoly_wround_evals, vpoly_wround_fold_plan, vpoly_wround_fold_evals); VirtualPolynomial.round_evals_weighted /
fold_round_evals_weighted and EqSumCheck (mle.py) are built on the two functions below.  They are functions, not methods, because
tests/test_dev_boundaries_host.py keeps a closed table of the *_dev methods of CyclotomicRing; the odd-8-byte-pointer placements of
these two calls are in tests/test_wsumcheck_gpu.py.
"""
from .rings import MLE_LEADING


def vpoly_wround_evals_dev(ring, out, weights, tables, terms, coeffs, num_vars, order=MLE_LEADING, work=None, stream=None):
    """out[t] = sum_{b < half} weights[b] * sum_k c_k prod_s (lo_s[b] + t (hi_s[b] - lo_s[b])), t = 0 .. d (d the longest term; the weight
    is not a factor).  weights: a CUDA tensor of 2^(num_vars - 1) ring elements, one per pair, never written; tables, terms, coeffs as
    in CyclotomicRing.vpoly_round_evals_dev; order: MLE_LEADING or MLE_TRAILING; work: at least ring.vpoly_wround_plan()[0] elements.
    Allocates nothing."""
    return ring._vpoly_wround_evals_dev(out, weights, tables, terms, coeffs, num_vars, order, work, stream)


def vpoly_wround_fold_evals_dev(ring, out, out_tables, weights, tables, terms, coeffs, num_vars, r, order=MLE_LEADING, work=None, stream=None):
    """CyclotomicRing.vpoly_round_fold_evals_dev with a per-pair weight on the message: the tables are folded at `r` into out_tables
    exactly as there, and out[t], t = 0 .. d, is vpoly_wround_evals_dev on the folded tables at num_vars - 1 with the same `weights`
    (2^(num_vars - 2) ring elements).  Returns the list of elements written per table.  work: at least
    ring.vpoly_wround_fold_plan()[0] elements.  Allocates nothing."""
    return ring._vpoly_wround_fold_evals_dev(out, out_tables, weights, tables, terms, coeffs, num_vars, r, order, work, stream)


# ---- integer columns as factors (sr_vpoly_iwround_*; csrc/sumcheck_index.hpp) ---------------------------------------------------------
# A slot of the sum of products is a ring table or an IndexColumn that stands for the table R::from(col[e]): terms index the tables
# first, then the columns.  The calls equal from_u64_dev followed by the weighted calls above, word for word; the first message and
# the first fold read 8 bytes per row and column, and the folded slots are ring tables.
MAX_SLOTS = 8


def _iw_columns(what, ring, columns, num_vars, pointer, spare):
    """the sr_index_column array and the stored length of every column; pointer(values) -> address; spare: any valid address, for
    an empty array"""
    from .index_columns import MAX_INDEX_COLUMNS, _column, sr_index_column
    from .rings import RingError

    cols = [_column(c) for c in columns]
    if len(cols) > MAX_INDEX_COLUMNS:
        raise RingError(what + ": at most 8 index columns")
    if not 0 <= int(num_vars) < 48:
        raise RingError(what + ": num_vars must be below 48")
    full = 1 << int(num_vars)
    arr = (sr_index_column * max(len(cols), 1))()
    sizes = []
    for j, c in enumerate(cols):
        if c.is_progression:
            if c.start + (full - 1) >= 1 << 64:
                raise RingError(what + ": a progression wraps past 2^64 - 1")
            arr[j] = sr_index_column(None, 0, c.start)
            sizes.append(full)
        else:
            if c.n_evals > full:
                raise RingError(what + ": column %d: n_evals exceeds 2^num_vars" % j)
            # a column that counts no value is never read; its own array keeps `values` non-null (not a progression), `spare` only
            # where it has none
            own = pointer(c.values) if (c.values.size if hasattr(c.values, "ctypes") else c.values.numel()) else 0
            arr[j] = sr_index_column(own or spare, c.n_evals, 0)
            sizes.append(c.n_evals)
    return cols, arr, sizes


def _iw_slots(what, n_tables, n_index):
    from .rings import RingError

    if not 1 <= n_tables + n_index <= MAX_SLOTS:
        raise RingError(what + ": 1 .. 8 tables and columns together")


def vpoly_iwround_plan(ring, num_vars, n_tables, n_index, n_terms, degree, order=MLE_LEADING, fold=False):
    """sr_vpoly_iwround_plan: (work_elems, launches) of vpoly_iwround_evals_dev (fold False) or vpoly_iwround_fold_evals_dev (fold
    True) over n_tables ring tables and n_index integer columns -- host arithmetic only."""
    return ring._plan_of(ring._lib.sr_vpoly_iwround_plan, num_vars, n_tables, n_index, n_terms, degree, order, 1 if fold else 0)


def vpoly_iwround_evals_dev(ring, out, weights, tables, columns, terms, coeffs, num_vars, order=MLE_LEADING, work=None, stream=None):
    """vpoly_wround_evals_dev over len(tables) ring tables and len(columns) integer columns (IndexColumn, or 8-byte-integer CUDA tensors
    taken whole): slot s < len(tables) of a term is tables[s], the others columns[s - len(tables)], each standing for the table
    R::from(col[e]) that from_u64_dev would write.  work: at least vpoly_iwround_plan()[0] elements.  Allocates nothing."""
    what = "vpoly_iwround_evals"
    arr, n_terms, d = ring._vpoly_terms(terms)
    po, ptrs, sizes, n, pc, pwt, pw, nw = ring._round_dev_args(what, out, d + 1, "d + 1 elements, d the longest term", tables, work, coeffs,
                                                               n_terms, "term", weights, num_vars - 1)
    cols, carr, _ = _iw_columns(what, ring, columns, num_vars, lambda v: ring._dev(v)[0].value, po.value)
    _iw_slots(what, n, len(cols))
    ring._check(ring._lib.sr_vpoly_iwround_evals_dev(ring._ctx, po, pwt, ptrs, sizes, n, carr, len(cols), arr, n_terms, pc, int(num_vars),
                                                     int(order), pw, nw, ring._stream(stream)))
    return out


def vpoly_iwround_fold_evals_dev(ring, out, out_tables, weights, tables, columns, terms, coeffs, num_vars, r, order=MLE_LEADING, work=None,
                                 stream=None):
    """vpoly_wround_fold_evals_dev over ring tables and integer columns: every slot -- table or column -- is folded at `r` into
    out_tables[s] (len(tables) + len(columns) CUDA tensors; a column's folded slot is a ring table of (n_evals + 1) // 2 elements in
    leading order, min(n_evals, 2^(num_vars-1)) in trailing order, in a buffer of its own), and out[t] is the weighted message over
    the folded tables.  Returns the list of elements written per slot.  work: at least vpoly_iwround_plan(fold=True)[0] elements."""
    from .rings import RingError

    what = "vpoly_iwround_fold_evals"
    arr, n_terms, d = ring._vpoly_terms(terms)
    po, ptrs, sizes, n, pc, pwt, pw, nw = ring._round_dev_args(what, out, d + 1, "d + 1 elements, d the longest term", tables, work, coeffs,
                                                               n_terms, "term", weights, num_vars - 2)
    cols, carr, csizes = _iw_columns(what, ring, columns, num_vars, lambda v: ring._dev(v)[0].value, po.value)
    _iw_slots(what, n, len(cols))
    slots = n + len(cols)
    if len(out_tables) != slots:
        raise RingError(what + ": one output table per table and column")
    all_sizes = [int(sizes[j]) for j in range(n)] + csizes
    optrs, osizes, pr = ring._fold_dev_args(what, out_tables, all_sizes, slots, num_vars, r, order)
    ring._check(ring._lib.sr_vpoly_iwround_fold_evals_dev(ring._ctx, po, optrs, osizes, pwt, ptrs, sizes, n, carr, len(cols), arr, n_terms, pc,
                                                          int(num_vars), pr, int(order), pw, nw, ring._stream(stream)))
    return [int(osizes[j]) for j in range(slots)]


def _iw_host_columns(what, ring, columns, num_vars):
    import numpy as np

    from .index_columns import IndexColumn, _column

    cols = []
    for c in (_column(c) for c in columns):   # contiguous uint64 copies of the stored values: the caller's objects stay as they are
        cols.append(c if c.is_progression else IndexColumn(np.ascontiguousarray(c.values, dtype=np.uint64).reshape(-1), n_evals=c.n_evals))
    z = np.zeros(1, dtype=np.uint64)
    cols, carr, csizes = _iw_columns(what, ring, cols, num_vars, lambda v: v.ctypes.data, z.ctypes.data)
    return cols, carr, csizes, z


def vpoly_iwround_evals(ring, weights, tables, columns, terms, coeffs, num_vars, order=MLE_LEADING):
    """Host buffers: sr_vpoly_iwround_evals (see vpoly_iwround_evals_dev); column values are numpy uint64 arrays.  Returns the d + 1
    elements."""
    from .rings import RingError, _np_ptr

    what = "vpoly_iwround_evals"
    arr, n_terms, d = ring._vpoly_terms(terms)
    tables, weights, coeffs, out, ptrs, sizes, n = ring._round_host_args(what, max(d, 1) + 1, tables, coeffs, n_terms, "term", weights)
    cols, carr, _, keep = _iw_host_columns(what, ring, columns, num_vars)
    _iw_slots(what, n, len(cols))
    if weights is not None and 1 <= num_vars < 48 and weights.size != ring.words_per_elem << (num_vars - 1):
        raise RingError(what + ": weights must hold one element per pair")
    ring._check(ring._lib.sr_vpoly_iwround_evals(ring._ctx, _np_ptr(out), None if weights is None else weights.ctypes.data, ptrs, sizes, n, carr,
                                                 len(cols), arr, n_terms, None if coeffs is None else coeffs.ctypes.data, int(num_vars),
                                                 int(order)))
    return out


def vpoly_iwround_fold_evals(ring, weights, tables, columns, terms, coeffs, num_vars, r, order=MLE_LEADING):
    """Host buffers: sr_vpoly_iwround_fold_evals (see vpoly_iwround_fold_evals_dev); returns (message, list of the folded slots)."""
    import ctypes

    import numpy as np

    from .rings import RingError, _np_ptr

    what, w = "vpoly_iwround_fold_evals", ring.words_per_elem
    arr, n_terms, d = ring._vpoly_terms(terms)
    tables, weights, coeffs, out, ptrs, sizes, n = ring._round_host_args(what, max(d, 1) + 1, tables, coeffs, n_terms, "term", weights)
    cols, carr, csizes, keep = _iw_host_columns(what, ring, columns, num_vars)
    _iw_slots(what, n, len(cols))
    if weights is not None and 2 <= num_vars < 48 and weights.size != w << (num_vars - 2):
        raise RingError(what + ": weights must hold one element per pair of the folded tables")
    r = np.ascontiguousarray(r, dtype=np.uint64)
    if r.size != w:
        raise RingError(what + ": r is not one ring element")
    slots = n + len(cols)
    stored = [int(sizes[j]) for j in range(n)] + csizes
    folded = [np.empty(max(s * w, 1), dtype=np.uint64) for s in stored]   # never shorter than the folded slot
    optrs = (ctypes.c_void_p * slots)(*[f.ctypes.data for f in folded])
    osizes = (ctypes.c_size_t * slots)()
    ring._check(ring._lib.sr_vpoly_iwround_fold_evals(ring._ctx, _np_ptr(out), optrs, osizes, None if weights is None else weights.ctypes.data,
                                                      ptrs, sizes, n, carr, len(cols), arr, n_terms,
                                                      None if coeffs is None else coeffs.ctypes.data, int(num_vars), _np_ptr(r), int(order)))
    return out, [f[:int(osizes[j]) * w] for j, f in enumerate(folded)]
