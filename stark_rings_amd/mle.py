"""DenseMultilinearExtension of crates/poly (src/mle/dense.rs) over a device-resident table of ring elements in CRT/NTT form.

The evaluations live in one torch CUDA tensor of 8-byte integers in the flat layout of every other call (element-major, D
coefficients per element, N u64 limbs each, Montgomery residues).  Like the reference's constructor (dense.rs:35-54) the object may
hold fewer than 2^num_vars elements: the missing tail is zero and is never read.  Folds run through sr_mle_fix_variables_dev
(include/stark_rings_hip.h); `r * a` is the slot product of the ring.
"""
from .rings import MLE_LEADING, MLE_TRAILING, RingError


class DenseMultilinearExtension:
    def __init__(self, ring, num_vars, evaluations):
        """ring: a CyclotomicRing; evaluations: a CUDA tensor of n <= 2^num_vars ring elements (kept, not copied)."""
        n = ring._batch_of(evaluations.numel())
        if num_vars < 0 or n > 1 << num_vars:
            raise RingError("DenseMultilinearExtension: more evaluations than 2^num_vars")
        if n:
            ring._dev(evaluations)  # a contiguous 8-byte CUDA tensor on the ring's device
        self.ring = ring
        self._num_vars = int(num_vars)
        self.evaluations = evaluations
        self._work = None

    @classmethod
    def from_evaluations_vec_padded(cls, ring, num_vars, evaluations):
        """dense.rs:79-89 `from_evaluations_vec_padded`: a vector shorter than 2^num_vars is padded with zeros -- here the padding
        stays implicit (the zero tail is never stored or read); to_evaluations writes it out."""
        return cls(ring, num_vars, evaluations)

    @property
    def num_vars(self):
        return self._num_vars

    def __len__(self):
        return self.ring._batch_of(self.evaluations.numel())

    def _workspace(self, elems):
        """one workspace per object, sized for its first (largest) fold and reused by the later, smaller ones"""
        import torch

        if elems and (self._work is None or self._work.numel() < elems * self.ring.words_per_elem):
            self._work = torch.empty(elems * self.ring.words_per_elem, dtype=self.evaluations.dtype, device=self.evaluations.device)
        return self._work if elems else None

    def _fold(self, point, order, stream):
        import torch

        n_fixed = self.ring._batch_of(point.numel())
        if n_fixed > self._num_vars:
            raise RingError("fix_variables: the point has more entries than the polynomial has variables")  # dense.rs:172-175 asserts
        out = torch.empty(self.ring.words_per_elem << (self._num_vars - n_fixed), dtype=self.evaluations.dtype, device=self.evaluations.device)
        work = self._workspace(self.ring.mle_plan(self._num_vars, n_fixed, order)[0])
        self.ring.mle_fix_variables_dev(out, self.evaluations, self._num_vars, point, order, work, stream)
        return out, self._num_vars - n_fixed

    def fix_variables(self, partial_point, stream=None):
        """dense.rs:171-199: fixes variables 0 .. len(partial_point) - 1 (least significant index bit first) and rebinds this
        object to the folded table of num_vars - len(partial_point) variables."""
        self.evaluations, self._num_vars = self._fold(partial_point, MLE_LEADING, stream)
        return self

    def fixed_variables(self, partial_point, stream=None):
        """dense.rs:201-205: the same as a new object; this one is unchanged."""
        out, nv = self._fold(partial_point, MLE_LEADING, stream)
        return DenseMultilinearExtension(self.ring, nv, out)

    def fix_last_variables(self, partial_point, stream=None):
        """polynomials/multilinear_polynomial.rs:227-286: fixes the LAST len(partial_point) variables, partial_point[j] being
        variable num_vars - len + j; returns a new object."""
        out, nv = self._fold(partial_point, MLE_TRAILING, stream)
        return DenseMultilinearExtension(self.ring, nv, out)

    def evaluate(self, point, stream=None):
        """dense.rs:107-113: the value at `point` as one ring element (a tensor), or None when the point has the wrong length."""
        if point.numel() != self._num_vars * self.ring.words_per_elem:
            return None
        return self._fold(point, MLE_LEADING, stream)[0]

    def add_assign_scaled(self, r, other, stream=None):
        """dense.rs:288-317 `AddAssign<(R, &Self)>`: self += r * other, r one ring element (a tensor)."""
        if other.num_vars != self._num_vars or len(other) != len(self):
            # the reference asserts equal num_vars; both operands must store the same number of evaluations here
            raise RingError("add_assign_scaled: the operands differ in num_vars or stored length (see to_evaluations)")
        self.ring.mul_elem_add_dev(self.evaluations, other.evaluations, r, stream)
        return self

    def to_evaluations(self):
        """dense.rs `to_evaluations`: all 2^num_vars elements as one tensor, the zero tail written out."""
        import torch

        full = self.ring.words_per_elem << self._num_vars
        if self.evaluations.numel() == full:
            return self.evaluations.clone()
        out = torch.zeros(full, dtype=self.evaluations.dtype, device=self.evaluations.device)
        out[:self.evaluations.numel()] = self.evaluations
        return out
