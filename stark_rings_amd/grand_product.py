"""ProductTree: every layer of the binary product tree over a device-resident table of ring elements in CRT/NTT form
(sr_prod_tree_dev, include/stark_rings_hip.h) -- the circuit of the division-free, layered grand-product argument (Thaler's GKR
circuit, as used by Quarks and Lasso) behind product, permutation and multiset-equality checks.

Layer 0 is the 2^num_vars leaves, layer k has 2^(num_vars - k) elements and the root is layer num_vars.  In trailing order
L_k[i] = L_{k-1}[i] * L_{k-1}[i + half]: the two operands of a layer are the contiguous lower and upper halves of the layer below,
so the claim L_k(z) = sum_b eq(z, b) lo(b) hi(b) runs on VirtualPolynomial over views of the layers, nothing copied.  In leading
order L_k[i] = L_{k-1}[2i] * L_{k-1}[2i+1].
"""
from .mle import DenseMultilinearExtension, EqSumCheck, VirtualPolynomial
from .rings import MLE_LEADING, MLE_TRAILING, RingError


class ProductTree:
    def __init__(self, ring, leaves, num_vars, n_leaves=None, order=MLE_TRAILING, stream=None):
        """ring: a CyclotomicRing; leaves: a CUDA tensor of ring elements in CRT/NTT form (kept, not copied, never written) of which
        the first n_leaves <= 2^num_vars are the stored leaves (default: all of the tensor); the leaves beyond them are one() and
        are never read.  The layers are computed on `stream` into one tensor of 2^num_vars - 1 elements."""
        import torch

        if order not in (MLE_LEADING, MLE_TRAILING):
            raise RingError("ProductTree: unknown order")
        if num_vars < 0 or num_vars >= 48:
            raise RingError("ProductTree: num_vars must be in [0, 48)")
        w = ring.words_per_elem
        have = ring._batch_of(leaves.numel())
        n = have if n_leaves is None else int(n_leaves)
        if n < 0 or n > have or n > 1 << num_vars:
            raise RingError("ProductTree: n_leaves exceeds the stored leaves or 2^num_vars")
        self.ring = ring
        self.order = order
        self._num_vars = int(num_vars)
        self.n_leaves = n
        self.leaves = leaves[:n * w]
        self.layers = torch.empty(((1 << num_vars) - 1) * w, dtype=leaves.dtype, device=leaves.device)
        if stream is not None:
            self.layers.record_stream(stream)
        ring.prod_tree_dev(self.layers, self.leaves, num_vars, order, stream)

    @property
    def num_vars(self):
        return self._num_vars

    def layer_offset(self, k):
        """element offset of layer k (1 <= k <= num_vars) in `layers`: layer 1 first, the root last"""
        if not 1 <= k <= self._num_vars:
            raise RingError("ProductTree: layer index out of range")
        return (1 << self._num_vars) - (1 << (self._num_vars - k + 1))

    def _table(self, k):
        """layer k as a view (no copy); layer 0 needs every leaf stored (an MLE's missing tail is zero, a tree's is one)"""
        w = self.ring.words_per_elem
        if k == 0:
            if self.n_leaves != 1 << self._num_vars:
                raise RingError("ProductTree: layer 0 of a truncated tree is not a table (its missing leaves are one(), an MLE's are zero)")
            return self.leaves
        off = self.layer_offset(k)
        return self.layers[off * w:(off + (1 << (self._num_vars - k))) * w]

    def layer(self, k):
        """layer k as a DenseMultilinearExtension in num_vars - k variables over a view of the layer; k = 0 gives the leaves"""
        return DenseMultilinearExtension(self.ring, self._num_vars - k, self._table(k))

    def root(self):
        """the product of all leaves: one ring element (a view of the last element of `layers`; the only leaf where num_vars = 0)"""
        if self._num_vars == 0:
            if self.n_leaves == 0:
                raise RingError("ProductTree: a tree of no variables and no stored leaf holds no element (its root is one())")
            return self.leaves
        return self._table(self._num_vars)

    def halves(self, k):
        """(lo, hi): the lower and upper halves of layer k - 1 as two MLEs in num_vars - k variables, with layer(k) = lo * hi
        element by element.  Trailing order only: in leading order the operands are the even and the odd elements."""
        if self.order != MLE_TRAILING:
            raise RingError("ProductTree.halves: only a trailing-order tree has contiguous operands")
        if not 1 <= k <= self._num_vars:
            raise RingError("ProductTree: layer index out of range")
        below = self._table(k - 1)
        half = below.numel() // 2
        nv = self._num_vars - k
        return DenseMultilinearExtension(self.ring, nv, below[:half]), DenseMultilinearExtension(self.ring, nv, below[half:])

    def layer_claim(self, k, z, lam=None, stream=None):
        """The sum-check of the layer claim L_k(z) = sum_b eq(z, b) lo(b) hi(b) over halves(k), as an EqSumCheck in trailing order:
        eq(z, .) is held as per-pair weights, not as a table.  z: num_vars - k ring elements, k < num_vars; the claimed sum
        message()[0] + message()[1] is layer(k).evaluate(z).  lam is unused (the fraction tree's claim takes one)."""
        lo, hi = self.halves(k)
        if lo.num_vars < 1:
            raise RingError("ProductTree.layer_claim: the root's claim has no variable (it is lo * hi)")
        g = VirtualPolynomial(self.ring, lo.num_vars).add_mle_list([lo, hi])
        return EqSumCheck(g, z, MLE_TRAILING, stream)
