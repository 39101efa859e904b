"""FractionTree: every layer of the binary tree that sums fractions p_i / q_i over device-resident tables of ring elements in CRT/NTT
form without dividing (sr_frac_tree_dev, include/stark_rings_hip.h) -- the circuit of the layered (GKR) fractional sum-check of
LogUp-GKR (Papini, Habock) behind lookup and range arguments.

A node is a pair (p, q); layer 0 is the 2^num_vars leaves, layer k has 2^(num_vars - k) nodes and the root is layer num_vars.  A node
combines its children (l, r) as p = p_l q_r + p_r q_l, q = q_l q_r; the children are (i, i + half) in trailing order, so the four
operands of a layer are contiguous halves of the two layers below and the claim
    P_k(z) + lambda Q_k(z) = sum_b eq(z, b) (p_lo(b) q_hi(b) + p_hi(b) q_lo(b) + lambda q_lo(b) q_hi(b))
runs on VirtualPolynomial over views of the layers, nothing copied; in leading order the children are (2i, 2i + 1).  The root (P, Q)
is P = sum_i p_i prod_{j != i} q_j and Q = prod_j q_j.
"""
import ctypes

import numpy as np

from .mle import DenseMultilinearExtension, EqSumCheck, VirtualPolynomial
from .rings import MLE_LEADING, MLE_TRAILING, STARK_POW2, RingError, _np_ptr


def frac_tree_plan(ring, num_vars, order=MLE_TRAILING):
    """sr_frac_tree_plan: (layer_elems per output, launches) of the fraction tree over 2^num_vars leaves on this ring -- host
    arithmetic only."""
    elems = ctypes.c_size_t()
    launches = ctypes.c_int()
    k = ring.degree.bit_length() - 1 if ring.ring <= STARK_POW2 else 0
    ring._check(ring._lib.sr_frac_tree_plan(ring.ring, k, int(num_vars), int(order), ctypes.byref(elems), ctypes.byref(launches)))
    return elems.value, launches.value


def _sizes(ring, p_words, q_words, num_vars, p_layer_words, q_layer_words):
    n_leaves = ring._batch_of(q_words)
    if num_vars < 0 or num_vars >= 48:
        raise RingError("frac_tree: num_vars must be in [0, 48)")
    if n_leaves > 1 << num_vars:
        raise RingError("frac_tree: more leaves than 2^num_vars")
    if p_words is not None and p_words != q_words:
        raise RingError("frac_tree: p_leaves and q_leaves must hold the same number of elements")
    want = ring.words_per_elem * ((1 << num_vars) - 1)
    if p_layer_words != want or q_layer_words != want:
        raise RingError("frac_tree: p_layers and q_layers must hold 2^num_vars - 1 elements each")
    return n_leaves


def frac_tree_dev(ring, p_layers, q_layers, p_leaves, q_leaves, num_vars, order=MLE_TRAILING, stream=None):
    """sr_frac_tree_dev: every layer of the fraction tree over the leaves (p_i, q_i) (n_leaves <= 2^num_vars elements in CRT/NTT form
    each, the rest (zero(), one()) and never read; p_leaves None: every stored numerator is one()) into p_layers and q_layers
    (2^num_vars - 1 elements each: layer k at element offset 2^num_vars - 2^(num_vars - k + 1), the root last).  Allocates nothing."""
    null = ctypes.c_void_p(0)
    q_words = q_leaves.numel() if q_leaves is not None else 0
    p_words = p_leaves.numel() if p_leaves is not None else None
    n_leaves = _sizes(ring, p_words, q_words, num_vars, p_layers.numel(), q_layers.numel())
    pp = ring._dev(p_layers)[0] if p_layers.numel() else null
    pq = ring._dev(q_layers)[0] if q_layers.numel() else null
    lp = ring._dev(p_leaves)[0] if p_words else null
    lq = ring._dev(q_leaves)[0] if q_words else null
    ring._check(ring._lib.sr_frac_tree_dev(ring._ctx, pp, pq, lp, lq, n_leaves, int(num_vars), int(order), ring._stream(stream)))
    return p_layers, q_layers


def frac_tree(ring, p_leaves, q_leaves, num_vars, order=MLE_TRAILING):
    """Host buffers: sr_frac_tree (see frac_tree_dev); returns (p_layers, q_layers), 2^num_vars - 1 elements each."""
    q_leaves = np.ascontiguousarray(q_leaves, dtype=np.uint64)
    if p_leaves is not None:
        p_leaves = np.ascontiguousarray(p_leaves, dtype=np.uint64)
    n_out = ring.words_per_elem * ((1 << num_vars) - 1) if 0 <= num_vars < 48 else 0
    n_leaves = _sizes(ring, None if p_leaves is None else p_leaves.size, q_leaves.size, num_vars, n_out, n_out)
    p_out = np.empty(max(n_out, 1), dtype=np.uint64)
    q_out = np.empty(max(n_out, 1), dtype=np.uint64)
    z = np.zeros(1, dtype=np.uint64)
    lp = None if p_leaves is None else _np_ptr(p_leaves if n_leaves else z)
    ring._check(ring._lib.sr_frac_tree(ring._ctx, _np_ptr(p_out), _np_ptr(q_out), lp, _np_ptr(q_leaves if n_leaves else z), n_leaves,
                                       int(num_vars), int(order)))
    return p_out[:n_out], q_out[:n_out]


class FractionTree:
    def __init__(self, ring, p_leaves, q_leaves, num_vars, n_leaves=None, order=MLE_TRAILING, stream=None):
        """ring: a CyclotomicRing; q_leaves (and p_leaves, unless None: every stored numerator is one()): CUDA tensors of ring
        elements in CRT/NTT form (kept, not copied, never written) of which the first n_leaves <= 2^num_vars are the stored leaves
        (default: all of q_leaves); the leaves beyond them are (zero(), one()) and are never read.  The layers are computed on
        `stream` into two tensors of 2^num_vars - 1 elements."""
        import torch

        if order not in (MLE_LEADING, MLE_TRAILING):
            raise RingError("FractionTree: unknown order")
        if num_vars < 0 or num_vars >= 48:
            raise RingError("FractionTree: num_vars must be in [0, 48)")
        w = ring.words_per_elem
        have = ring._batch_of(q_leaves.numel())
        if p_leaves is not None:
            have = min(have, ring._batch_of(p_leaves.numel()))
        n = have if n_leaves is None else int(n_leaves)
        if n < 0 or n > have or n > 1 << num_vars:
            raise RingError("FractionTree: n_leaves exceeds the stored leaves or 2^num_vars")
        self.ring = ring
        self.order = order
        self._num_vars = int(num_vars)
        self.n_leaves = n
        self.q_leaves = q_leaves[:n * w]
        self.p_leaves = None if p_leaves is None else p_leaves[:n * w]
        self.p_layers = torch.empty(((1 << num_vars) - 1) * w, dtype=q_leaves.dtype, device=q_leaves.device)
        self.q_layers = torch.empty_like(self.p_layers)
        if stream is not None:
            self.p_layers.record_stream(stream)
            self.q_layers.record_stream(stream)
        frac_tree_dev(ring, self.p_layers, self.q_layers, self.p_leaves, self.q_leaves, num_vars, order, stream)

    @property
    def num_vars(self):
        return self._num_vars

    def layer_offset(self, k):
        """element offset of layer k (1 <= k <= num_vars) in `p_layers` and `q_layers`: layer 1 first, the root last"""
        if not 1 <= k <= self._num_vars:
            raise RingError("FractionTree: layer index out of range")
        return (1 << self._num_vars) - (1 << (self._num_vars - k + 1))

    def _tables(self, k):
        """(p, q) of layer k as views (no copy); layer 0 needs every leaf and its numerator stored"""
        w = self.ring.words_per_elem
        if k == 0:
            if self.n_leaves != 1 << self._num_vars:
                raise RingError("FractionTree: layer 0 of a truncated tree is not a table (its missing leaves are (zero(), one()))")
            if self.p_leaves is None:
                raise RingError("FractionTree: layer 0 of a tree without stored numerators is not a table (they are one())")
            return self.p_leaves, self.q_leaves
        off = self.layer_offset(k)
        span = slice(off * w, (off + (1 << (self._num_vars - k))) * w)
        return self.p_layers[span], self.q_layers[span]

    def layer(self, k):
        """(P_k, Q_k): layer k as two DenseMultilinearExtensions in num_vars - k variables over views; k = 0 gives the leaves"""
        if not 0 <= k <= self._num_vars:
            raise RingError("FractionTree: layer index out of range")
        p, q = self._tables(k)
        nv = self._num_vars - k
        return DenseMultilinearExtension(self.ring, nv, p), DenseMultilinearExtension(self.ring, nv, q)

    def root(self):
        """(P, Q): the numerator and denominator of the sum of all fractions, one ring element each (views; the only leaf where
        num_vars = 0)"""
        if self._num_vars == 0:
            if self.n_leaves == 0 or self.p_leaves is None:
                raise RingError("FractionTree: a tree of no variables holds its root only as a stored leaf with a stored numerator")
            return self.p_leaves, self.q_leaves
        return self._tables(self._num_vars)

    def root_value(self, stream=None):
        """P / Q: the value of the sum of all fractions as one ring element (a new tensor), slot by slot (sr_inverse_batch_dev on the
        root).  Raises RingError when Q has a zero slot -- some denominator was no unit of the ring.  Q is copied to the host and its
        slots are tested there before the device call, so the call meets no zero and a count of inverse_zero_count the caller has not
        read yet stays as it is.  Blocks on `stream`."""
        import torch

        from .inverse import inverse_dev

        ring = self.ring
        p, q = self.root()
        if stream is not None:
            stream.synchronize()
        words = q.cpu().numpy().view(np.uint64)
        slot = ring.limbs if ring.ring <= STARK_POW2 else {3: 3, 4: 9, 5: 4}[ring.ring]   # words of a slot: Fq, Fq3, Fq9, Fq4
        if not words.reshape(-1, slot).any(axis=1).all():
            raise RingError("FractionTree.root_value: Q has a zero slot, the sum of the fractions has no value")
        out = torch.empty_like(q)
        if stream is not None:
            out.record_stream(stream)
        inverse_dev(ring, out, q, p, 1, stream=stream)
        return out

    def halves(self, k):
        """(p_lo, p_hi, q_lo, q_hi): the lower and upper halves of layer k - 1 as MLEs in num_vars - k variables, with
        P_k = p_lo q_hi + p_hi q_lo and Q_k = q_lo q_hi element by element.  Trailing order only."""
        if self.order != MLE_TRAILING:
            raise RingError("FractionTree.halves: only a trailing-order tree has contiguous operands")
        if not 1 <= k <= self._num_vars:
            raise RingError("FractionTree: layer index out of range")
        p, q = self._tables(k - 1)
        half = q.numel() // 2
        nv = self._num_vars - k
        return tuple(DenseMultilinearExtension(self.ring, nv, t) for t in (p[:half], p[half:], q[:half], q[half:]))

    def layer_claim(self, k, z, lam=None, stream=None):
        """The sum-check of the layer claim P_k(z) + lam Q_k(z) = sum_b eq(z, b) (p_lo q_hi + p_hi q_lo + lam q_lo q_hi)(b) over
        halves(k), as an EqSumCheck in trailing order: four tables and no eq table, where the explicit claim has five.  z:
        num_vars - k ring elements, k < num_vars; lam: one ring element, or None for one().  The claimed sum message()[0] +
        message()[1] is P_k(z) + lam Q_k(z) from evaluate of layer(k)."""
        p_lo, p_hi, q_lo, q_hi = self.halves(k)
        if q_lo.num_vars < 1:
            raise RingError("FractionTree.layer_claim: the root's claim has no variable")
        g = VirtualPolynomial(self.ring, q_lo.num_vars)
        g.add_mle_list([p_lo, q_hi]).add_mle_list([p_hi, q_lo]).add_mle_list([q_lo, q_hi], lam)
        return EqSumCheck(g, z, MLE_TRAILING, stream)
