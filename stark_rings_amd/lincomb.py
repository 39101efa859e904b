"""Linear combinations of tables of ring elements in CRT/NTT form with ring-element coefficients, several outputs from one pass over
the tables (sr_lincomb_dev, include/stark_rings_hip.h):

    out_m[e] = [bit K of uses[m]] coef[m][K]  +  sum_{k < K, bit k of uses[m]} coef[m][k] * T_k[e]        e < n

the composition of DenseMultilinearExtension's AddAssign<(R, &Self)>, MulAssign<R> and Add<R> (crates/poly mle/dense.rs:288-317,
370-374, 386-395).  The leaves of a permutation argument and of a logUp lookup, the fold of many instances into one and the batching of
many MLEs into one are all of this form (lookup.py builds the first two).
"""
import ctypes

import numpy as np

from .rings import STARK_POW2, RingError, _np_ptr

MAX_TABLES, MAX_OUTPUTS = 16, 4


def lincomb_plan(ring, n_tables, n_outputs):
    """sr_lincomb_plan: (launches, outputs_per_launch) of a call on this ring -- host arithmetic only."""
    launches, per = ctypes.c_int(), ctypes.c_int()
    k = ring.degree.bit_length() - 1 if ring.ring <= STARK_POW2 else 0
    ring._check(ring._lib.sr_lincomb_plan(ring.ring, k, int(n_tables), int(n_outputs), ctypes.byref(launches), ctypes.byref(per)))
    return launches.value, per.value


def _masks(n_tables, n_outputs, uses):
    """the argument checks that need no buffer; uses None: every output uses every table and the constant"""
    if not 1 <= n_tables <= MAX_TABLES:
        raise RingError("lincomb: 1 .. 16 tables")
    if not 1 <= n_outputs <= MAX_OUTPUTS:
        raise RingError("lincomb: 1 .. 4 outputs")
    if uses is None:
        uses = [(2 << n_tables) - 1] * n_outputs
    uses = [int(u) for u in uses]
    if len(uses) != n_outputs:
        raise RingError("lincomb: one mask per output")
    seen = 0
    for u in uses:
        if u <= 0:
            raise RingError("lincomb: an output with an empty mask")
        if u >> (n_tables + 1):
            raise RingError("lincomb: a mask bit above the number of tables")
        seen |= u
    if seen & ((1 << n_tables) - 1) != (1 << n_tables) - 1:
        raise RingError("lincomb: a table that no output uses")
    return (ctypes.c_uint32 * n_outputs)(*uses)


def _evals(n_tables, n, n_evals, stored):
    """n_evals as a size_t array; stored[k]: the elements table k holds"""
    if n_evals is None:
        n_evals = [n] * n_tables
    if len(n_evals) != n_tables:
        raise RingError("lincomb: one n_evals entry per table")
    for k, (ne, have) in enumerate(zip(n_evals, stored)):
        if ne < 0 or ne > n:
            raise RingError("lincomb: n_evals[%d] exceeds n" % k)
        if ne > have:
            raise RingError("lincomb: table %d holds fewer than n_evals[%d] elements" % (k, k))
    return (ctypes.c_size_t * n_tables)(*[int(x) for x in n_evals])


def lincomb_dev(ring, outs, tables, coef, uses, n, n_evals=None, stream=None):
    """sr_lincomb_dev.  outs: 1 .. 4 CUDA tensors of at least n elements, written in full; tables: 1 .. 16 CUDA tensors, table k of at
    least n_evals[k] <= n elements (default n), the rest of it zero and never read; coef: a CUDA tensor of len(outs) x (len(tables) + 1)
    elements, row-major, the last of a row the additive constant; uses: one bit mask per output (None: everything), a coefficient whose
    bit is clear is never read.  An output may be a table only when there is one output.  Allocates nothing."""
    w = ring.words_per_elem
    K, M = len(tables), len(outs)
    masks = _masks(K, M, uses)
    n = int(n)
    if n < 0:
        raise RingError("lincomb: negative n")
    sizes = _evals(K, n, n_evals, [t.numel() // w for t in tables])
    pc, nc = ring._dev(coef)
    if nc != M * (K + 1) * w:
        raise RingError("lincomb: coef must hold len(outs) x (len(tables) + 1) elements")
    po, pt = (ctypes.c_void_p * M)(), (ctypes.c_void_p * K)()
    for m, o in enumerate(outs):
        if o.numel() < n * w:
            raise RingError("lincomb: output %d holds fewer than n elements" % m)
        po[m] = ring._dev(o)[0]
    for k, t in enumerate(tables):
        pt[k] = ring._dev(t)[0] if t.numel() else po[0]   # a table that stores nothing is never read: any non-null pointer
    ring._check(ring._lib.sr_lincomb_dev(ring._ctx, po, M, pt, sizes, K, pc, masks, n, ring._stream(stream)))
    return outs


def lincomb(ring, tables, coef, uses, n, n_outputs=None, n_evals=None):
    """Host buffers: sr_lincomb (see lincomb_dev).  tables: numpy arrays; coef: n_outputs x (len(tables) + 1) elements; returns the list
    of n_outputs arrays of n elements (n_outputs defaults to len(uses))."""
    w = ring.words_per_elem
    tables = [np.ascontiguousarray(t, dtype=np.uint64).reshape(-1) for t in tables]
    coef = np.ascontiguousarray(coef, dtype=np.uint64).reshape(-1)
    K = len(tables)
    M = int(n_outputs) if n_outputs is not None else (len(uses) if uses is not None else 1)
    masks = _masks(K, M, uses)
    n = int(n)
    if n < 0:
        raise RingError("lincomb: negative n")
    sizes = _evals(K, n, n_evals, [t.size // w for t in tables])
    if coef.size != M * (K + 1) * w:
        raise RingError("lincomb: coef must hold n_outputs x (len(tables) + 1) elements")
    outs = [np.empty(max(n * w, 1), dtype=np.uint64) for _ in range(M)]
    z = np.zeros(1, dtype=np.uint64)
    po, pt = (ctypes.c_void_p * M)(), (ctypes.c_void_p * K)()
    for m, o in enumerate(outs):
        po[m] = o.ctypes.data
    for k, t in enumerate(tables):
        pt[k] = t.ctypes.data if t.size else z.ctypes.data
    ring._check(ring._lib.sr_lincomb(ring._ctx, po, M, pt, sizes, K, _np_ptr(coef), masks, n))
    return [o[:n * w] for o in outs]
