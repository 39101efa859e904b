"""Batch inversion of tables of ring elements in CRT/NTT form, slot by slot (sr_inverse_batch_dev, include/stark_rings_hip.h):

    out[e] = num[e] * den[e]^-1        e < n        (num None: one())

Field::inverse / ark_ff::batch_inversion(&mut [F]) of the reference on every slot: the base field of a power-of-two ring, the Fq3 / Fq9 /
Fq4 slots of goldilocks24 / babybear72 / frog16.  A zero slot comes back as zero and is counted (inverse_zero_count); a ring element is
invertible exactly when none of its slots is zero, so a count of 0 is the `Some` of Field::inverse for the whole table.  The helper columns
of a logUp lookup (lookup.LookupHelperColumns), the value P/Q of a fraction tree (FractionTree.root_value) and quotient tables of MLEs
(DenseMultilinearExtension.inverse / .divide) are calls of this.
"""
import ctypes

import numpy as np

from .rings import STARK_POW2, RingError, _np_ptr


def inverse_plan(ring, n, has_num=False):
    """sr_inverse_plan: (work_elems, launches, chunk_elems) of a call over n elements on this ring -- host arithmetic only.  chunk_elems:
    the consecutive elements one lane inverts together with one field inversion."""
    work, launches, chunk = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_size_t()
    k = ring.degree.bit_length() - 1 if ring.ring <= STARK_POW2 else 0
    ring._check(ring._lib.sr_inverse_plan(ring.ring, k, int(n), int(bool(has_num)), ctypes.byref(work), ctypes.byref(launches),
                                          ctypes.byref(chunk)))
    return work.value, launches.value, chunk.value


def inverse_dev(ring, out, den, num=None, n=None, work=None, stream=None):
    """sr_inverse_batch_dev.  out, den, num: CUDA tensors of at least n elements (n defaults to what den holds); out may be den or num
    (the same tensor: in place).  work: a tensor of at least inverse_plan()[0] elements, None where the plan needs none (every ring
    today).  Allocates nothing; capturable."""
    w = ring.words_per_elem
    po, no = ring._dev(out)
    pd, nd = ring._dev(den)
    n = nd // w if n is None else int(n)
    if n < 0:
        raise RingError("inverse: negative n")
    if nd < n * w or no < n * w:
        raise RingError("inverse: a buffer holds fewer than n elements")
    pn = ctypes.c_void_p(0)
    if num is not None:
        pn, nn = ring._dev(num)
        if nn < n * w:
            raise RingError("inverse: num holds fewer than n elements")
    pw, nw = ring._dev_or_null(work)
    ring._check(ring._lib.sr_inverse_batch_dev(ring._ctx, po, pn, pd, n, pw, nw // w, ring._stream(stream)))
    return out


def inverse(ring, den, num=None):
    """Host buffers: sr_inverse_batch (see inverse_dev); returns num / den (1 / den without num) as a new array."""
    w = ring.words_per_elem
    den = np.ascontiguousarray(den, dtype=np.uint64).reshape(-1)
    if den.size % w:
        raise RingError("inverse: not a whole number of ring elements")
    n = den.size // w
    pn = ctypes.c_void_p(0)
    if num is not None:
        num = np.ascontiguousarray(num, dtype=np.uint64).reshape(-1)
        if num.size != den.size:
            raise RingError("inverse: num and den differ in length")
        pn = num.ctypes.data_as(ctypes.c_void_p) if n else ctypes.c_void_p(0)
    out = np.empty(max(den.size, 1), dtype=np.uint64)
    src = den if n else np.zeros(1, dtype=np.uint64)
    ring._check(ring._lib.sr_inverse_batch(ring._ctx, _np_ptr(out), pn, _np_ptr(src), n))
    return out[:den.size]


def inverse_zero_count(ring, stream=None):
    """sr_inverse_zero_count: the zero slots the inverse calls of this context met since the last read; clears the count."""
    n = ctypes.c_ulonglong(0)
    ring._check(ring._lib.sr_inverse_zero_count(ring._ctx, ctypes.byref(n), ring._stream(stream)))
    return int(n.value)
