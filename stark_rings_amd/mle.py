"""DenseMultilinearExtension (src/mle/dense.rs), VirtualPolynomial (a sum of products of dense MLEs, after HyperPlonk's) and, at the
end of the file, SparseMultilinearExtension (src/mle/sparse.rs) of crates/poly.  The dense class: DenseMultilinearExtension (src/mle/dense.rs) over a device-resident table of ring elements in CRT/NTT form.

The evaluations live in one torch CUDA tensor of 8-byte integers in the flat layout of every other call (element-major, D
coefficients per element, N u64 limbs each, Montgomery residues).  Like the reference's constructor (dense.rs:35-54) the object may
hold fewer than 2^num_vars elements: the missing tail is zero and is never read.  Folds run through sr_mle_fix_variables_dev
(include/stark_rings_hip.h); `r * a` is the slot product of the ring.
"""
import numpy as np

from .rings import MLE_LEADING, MLE_ROUND_SUM, MLE_TRAILING, RingError, smle_fix_pattern


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

    @classmethod
    def eq(cls, ring, point, stream=None):
        """The table b -> eq(point, b) = prod_i (b_i ? point[i] : 1 - point[i]) as a dense MLE of len(point) variables
        (precompute_eq, sparse.rs:381-394): sum_b eq[b] f[b] = f(point)."""
        import torch

        n = ring._batch_of(point.numel())
        out = torch.empty(ring.words_per_elem << n, dtype=point.dtype, device=point.device)
        ring.eq_table_dev(out, point, stream)
        return cls(ring, n, out)

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

    def _quotient(self, num, stream):
        import torch

        from .inverse import inverse_dev

        out = torch.empty_like(self.evaluations)
        if stream is not None:
            out.record_stream(stream)
        if len(self):
            inverse_dev(self.ring, out, self.evaluations, num.evaluations if num is not None else None, len(self), stream=stream)
        return DenseMultilinearExtension(self.ring, self._num_vars, out)

    def inverse(self, stream=None):
        """The table of slot-wise inverses 1 / self[b] as a new MLE over the stored evaluations (sr_inverse_batch_dev:
        ark_ff::batch_inversion on every slot).  A zero slot gives zero and is counted: ring.inverse_zero_count() == 0 afterwards says
        that every stored evaluation was a unit.  The implicit zero tail of a truncated table stays implicit (zeros are left in place)."""
        return self._quotient(None, stream)

    def divide(self, other, stream=None):
        """The table of slot-wise quotients self[b] / other[b] as a new MLE; zero slots of `other` give zero and are counted.  Both
        operands store the same number of evaluations."""
        if other.ring is not self.ring or other.num_vars != self._num_vars or len(other) != len(self):
            raise RingError("divide: the operands differ in ring, num_vars or stored length")
        return other._quotient(self, stream)

    @staticmethod
    def linear_combination(mles, coeffs, const=None, out=None, stream=None):
        """sum_k coeffs[k] * mles[k] (+ const) as one MLE from 1 .. 16 in one pass over their tables (sr_lincomb_dev): the composition
        of `MulAssign<R>`, `AddAssign<(R, &Self)>` and `Add<R>` (dense.rs:370-374, 288-317, 386-395).  coeffs: one ring element (a
        tensor) per MLE, or one tensor of len(mles) elements; const: one ring element or None.  The inputs may be truncated and need
        not store the same number of evaluations.  The result stores the longest input's evaluations, or all 2^num_vars with a
        constant: the constant goes to every evaluation, whereas the reference's Add<R> touches only the stored ones.  out: an MLE
        that stores exactly that many (it may be one of the inputs: in place), default a new one."""
        import torch

        from .lincomb import lincomb_dev

        if not 1 <= len(mles) <= 16:
            raise RingError("linear_combination: 1 .. 16 MLEs")
        ring, nv = mles[0].ring, mles[0].num_vars
        if any(m.ring is not ring or m.num_vars != nv for m in mles):
            raise RingError("linear_combination: the MLEs differ in ring or num_vars")
        w, K = ring.words_per_elem, len(mles)
        parts = [coeffs] if hasattr(coeffs, "numel") else list(coeffs)
        if sum(c.numel() for c in parts) != K * w:
            raise RingError("linear_combination: one coefficient (one ring element) per MLE")
        if const is not None and const.numel() != w:
            raise RingError("linear_combination: the constant is not one ring element")
        first = mles[0].evaluations
        coef = torch.cat([c.reshape(-1) for c in parts] + [const.reshape(-1) if const is not None else torch.zeros(w, dtype=first.dtype, device=first.device)])
        n = 1 << nv if const is not None else max(len(m) for m in mles)
        if out is None:
            out = DenseMultilinearExtension(ring, nv, torch.empty(n * w, dtype=first.dtype, device=first.device))
        elif out.ring is not ring or out.num_vars != nv or len(out) != n:
            raise RingError("linear_combination: out must store %d evaluations of the same ring and num_vars" % n)
        if stream is not None:
            coef.record_stream(stream)
            out.evaluations.record_stream(stream)
        # a table that stores nothing is all zero: it takes no part (and has no buffer to point at)
        live = [k for k in range(K) if len(mles[k])]
        if not live:
            live = [0]
        rows = torch.cat([coef[k * w:(k + 1) * w] for k in live] + [coef[K * w:]]) if len(live) != K else coef
        tables = [mles[k].evaluations if len(mles[k]) else out.evaluations for k in live]
        n_evals = [len(mles[k]) for k in live]
        mask = (1 << len(live)) - 1 | (1 << len(live) if const is not None else 0)
        if n:
            lincomb_dev(ring, [out.evaluations], tables, rows, [mask], n, n_evals, stream)
        return out

    @staticmethod
    def _round(tables, mode, stream):
        import torch

        if not 1 <= len(tables) <= 4:
            raise RingError("round_evals: 1 .. 4 tables")
        first = tables[0]
        ring, nv = first.ring, first.num_vars
        if any(t.ring is not ring or t.num_vars != nv for t in tables):
            raise RingError("round_evals: the tables must share one ring and one num_vars")
        n_out = 1 if mode == MLE_ROUND_SUM else len(tables) + 1
        out = torch.empty(n_out * ring.words_per_elem, dtype=first.evaluations.dtype, device=first.evaluations.device)
        # a workspace of its own per call (a few records of d + 1 elements): the folds of tables[0] may run on another stream
        need = ring.mle_round_plan(nv, len(tables), mode)[0]
        work = torch.empty(need * ring.words_per_elem, dtype=first.evaluations.dtype, device=first.evaluations.device) if need else None
        if work is not None and stream is not None:
            work.record_stream(stream)  # not handed out again before the launches on `stream` are done
        ring.mle_round_evals_dev(out, [t.evaluations for t in tables], nv, mode, work, stream)
        return out

    @staticmethod
    def round_evals(tables, order=MLE_LEADING, stream=None):
        """The prover's message of one sum-check round over the product of `tables` (a list of 1 .. 4 MLEs of one ring and one
        num_vars >= 1; an MLE may appear twice): the d + 1 elements p(t) = sum_b prod_j f_j(t, b), t = 0 .. d, the variable being
        the one fix_variables (MLE_LEADING) or fix_last_variables (MLE_TRAILING) fixes next."""
        if order not in (MLE_LEADING, MLE_TRAILING):
            raise RingError("round_evals: unknown order")
        return DenseMultilinearExtension._round(tables, order, stream)

    @staticmethod
    def product_sum(tables, stream=None):
        """sum_b prod_j f_j[b] over the hypercube as one ring element: the claimed sum of a sum-check (the `sum` of
        random_mle_list, polynomials/multilinear_polynomial.rs:19-49)."""
        return DenseMultilinearExtension._round(tables, MLE_ROUND_SUM, stream)

    @staticmethod
    def fold_round_evals(tables, r, order=MLE_LEADING, stream=None):
        """One prover round in one pass over the tables: every MLE of `tables` (1 .. 4 of one ring and one num_vars >= 2, each
        appearing once) with the variable fix_variables (MLE_LEADING) or fix_last_variables (MLE_TRAILING) fixes next set to the ring
        element `r`, and the message of the round that follows over those folded tables.  Returns (message, folded tables): what
        fixed_variables / fix_last_variables of every table followed by round_evals returns, bit for bit, in one pass over the tables."""
        import torch

        if order not in (MLE_LEADING, MLE_TRAILING):
            raise RingError("fold_round_evals: unknown order")
        if not 1 <= len(tables) <= 4:
            raise RingError("fold_round_evals: 1 .. 4 tables")
        first = tables[0]
        ring, nv = first.ring, first.num_vars
        if any(t.ring is not ring or t.num_vars != nv for t in tables):
            raise RingError("fold_round_evals: the tables must share one ring and one num_vars")
        if nv < 2:
            raise RingError("fold_round_evals: num_vars >= 2 (the last round folds with fix_variables)")
        w, ev = ring.words_per_elem, first.evaluations
        out = torch.empty((len(tables) + 1) * w, dtype=ev.dtype, device=ev.device)
        sizes = [(len(t) + 1) // 2 if order == MLE_LEADING else min(len(t), 1 << (nv - 1)) for t in tables]
        folded = [torch.empty(n * w, dtype=ev.dtype, device=ev.device) for n in sizes]
        need = ring.mle_round_fold_plan(nv, len(tables), order)[0]
        work = torch.empty(need * w, dtype=ev.dtype, device=ev.device) if need else None
        if stream is not None:
            for t in folded + ([work] if work is not None else []):
                t.record_stream(stream)
        ring.mle_round_fold_evals_dev(out, folded, [t.evaluations for t in tables], nv, r, order, work, stream)
        return out, [DenseMultilinearExtension(ring, nv - 1, f) for f in folded]

    def to_evaluations(self):
        """dense.rs `to_evaluations`: all 2^num_vars elements as one tensor, the zero tail written out."""
        import torch

        full = self.ring.words_per_elem << self._num_vars
        if self.evaluations.numel() == full:
            return self.evaluations.clone()
        out = torch.zeros(full, dtype=self.evaluations.dtype, device=self.evaluations.device)
        out[:self.evaluations.numel()] = self.evaluations
        return out


class VirtualPolynomial:
    """A sum of products of dense MLEs with ring coefficients, g = sum_k c_k prod_s f_{k,s}, after HyperPlonk's VirtualPolynomial
    (the code crates/poly's polynomials/multilinear_polynomial.rs was adapted from): the object a sum-check is run on -- eq (a b - c),
    sum_i alpha_i eq prod_j (...).  The tables stay where they are; a table that is in several products is held, and read, once
    (sr_vpoly_round_evals_dev).  At most 8 distinct tables, 8 products, 4 factors per product.

    A factor may be an IndexMultilinearExtension (index_columns.py): a column of integers that stands for the table R::from(col[e]).
    round_evals_weighted and fold_round_evals_weighted read such a slot as u64 (sr_vpoly_iwround_*), and the polynomial that
    fold_round_evals_weighted returns holds dense tables only.  round_evals, sum, fold_round_evals and fixed_variables have no such
    kernels: they expand every column slot with to_dense() first -- the slow path, D words per integer."""

    MAX_TABLES, MAX_TERMS, MAX_FACTORS = 8, 8, 4

    def __init__(self, ring, num_vars):
        self.ring = ring
        self._num_vars = int(num_vars)
        self.tables = []   # the distinct MLEs, in the order they were first added: the table slots of the call
        self.terms = []    # per product: the list of its table slots
        self.coeffs = []   # per product: one ring element (a tensor) or None for one()
        self._slot = {}    # device pointer of a table -> its slot

    @property
    def num_vars(self):
        return self._num_vars

    @property
    def degree(self):
        """the largest number of factors of a product: a round message has degree + 1 elements"""
        return max([len(t) for t in self.terms] or [0])

    @staticmethod
    def _is_column(mle):
        from .index_columns import IndexMultilinearExtension

        return isinstance(mle, IndexMultilinearExtension)

    @classmethod
    def _key(cls, mle):
        """what deduplicates a slot: a table's device pointer; a column's array and stored length, or a progression's start"""
        if cls._is_column(mle):
            return mle.key()
        return mle.evaluations.data_ptr() if len(mle) else ("empty", id(mle))

    def _has_columns(self):
        return any(self._is_column(t) for t in self.tables)

    def _like(self):
        """(dtype, device) of what the polynomial allocates"""
        import torch

        for want in (True, False):
            for t in self.tables:
                if not self._is_column(t) and (len(t) or not want):
                    return t.evaluations.dtype, t.evaluations.device
        for t in self.tables:
            if t.column.values is not None:
                return torch.int64, t.column.values.device
        return torch.int64, torch.device("cuda", self.ring.device)

    def _dense(self, stream):
        """the same polynomial with every column slot expanded to a ring table (IndexMultilinearExtension.to_dense)"""
        return self._over([t.to_dense(stream) if self._is_column(t) else t for t in self.tables], self._num_vars)

    def _slot_of(self, mle, new):
        if mle.ring is not self.ring or mle.num_vars != self._num_vars:
            raise RingError("VirtualPolynomial: every MLE must have the polynomial's ring and num_vars")
        key = self._key(mle)
        if key in self._slot:
            return self._slot[key]
        if key in new:
            return new[key][0]
        if len(self.tables) + len(new) >= self.MAX_TABLES:
            raise RingError("VirtualPolynomial: more than %d distinct tables" % self.MAX_TABLES)
        new[key] = (len(self.tables) + len(new), mle)
        return new[key][0]

    def _commit(self, new):
        for key, (slot, mle) in sorted(new.items(), key=lambda kv: kv[1][0]):
            self._slot[key] = slot
            self.tables.append(mle)

    def add_mle_list(self, mles, coeff=None):
        """g += coeff * prod(mles): 1 .. 4 MLEs (one may appear twice), coeff one ring element (a tensor) or None for one().
        Tables are deduplicated by device pointer into table slots.  An MLE may be an IndexMultilinearExtension."""
        mles = list(mles)
        if not 1 <= len(mles) <= self.MAX_FACTORS:
            raise RingError("VirtualPolynomial: a product has 1 .. %d factors" % self.MAX_FACTORS)
        if len(self.terms) >= self.MAX_TERMS:
            raise RingError("VirtualPolynomial: more than %d products" % self.MAX_TERMS)
        if coeff is not None and coeff.numel() != self.ring.words_per_elem:
            raise RingError("VirtualPolynomial: the coefficient is not one ring element")
        new = {}
        term = [self._slot_of(m, new) for m in mles]
        self._commit(new)
        self.terms.append(term)
        self.coeffs.append(coeff)
        return self

    def mul_by_mle(self, mle):
        """g *= mle: the MLE (dense or an IndexMultilinearExtension) becomes one more factor of every product."""
        if not self.terms:
            raise RingError("VirtualPolynomial: mul_by_mle on an empty polynomial")
        if any(len(t) >= self.MAX_FACTORS for t in self.terms):
            raise RingError("VirtualPolynomial: a product has 1 .. %d factors" % self.MAX_FACTORS)
        new = {}
        slot = self._slot_of(mle, new)
        self._commit(new)
        for t in self.terms:
            t.append(slot)
        return self

    def _coeff_tensor(self, like, stream):
        """the coefficients as one tensor, or None where every product has none"""
        import torch

        if all(c is None for c in self.coeffs):
            return None
        w = self.ring.words_per_elem
        out = torch.empty(len(self.coeffs) * w, dtype=like.dtype, device=like.device)
        for k, c in enumerate(self.coeffs):
            if c is None:
                self.ring.eq_table_dev(out[k * w:(k + 1) * w], None, stream)  # the eq table of no variables is the single element one()
            else:
                out[k * w:(k + 1) * w] = c
        return out

    def _call(self, mode, stream):
        import torch

        if not self.terms:
            raise RingError("VirtualPolynomial: no product has been added")
        if self._has_columns():
            return self._dense(stream)._call(mode, stream)
        ring, nv = self.ring, self._num_vars
        like = next((t.evaluations for t in self.tables if len(t)), self.tables[0].evaluations)
        w = ring.words_per_elem
        n_out = 1 if mode == MLE_ROUND_SUM else self.degree + 1
        out = torch.empty(n_out * w, dtype=like.dtype, device=like.device)
        need = ring.vpoly_round_plan(nv, len(self.tables), len(self.terms), self.degree, mode)[0]
        work = torch.empty(need * w, dtype=like.dtype, device=like.device) if need else None
        coeffs = self._coeff_tensor(like, stream)
        if stream is not None:
            for t in (work, coeffs):
                if t is not None:
                    t.record_stream(stream)
        ring.vpoly_round_evals_dev(out, [t.evaluations for t in self.tables], self.terms, coeffs, nv, mode, work, stream)
        return out

    def round_evals(self, order=MLE_LEADING, stream=None):
        """The prover's message of one sum-check round over g: the degree + 1 elements p(t) = sum_b g(t, b), t = 0 .. degree, the
        variable being the one fix_variables (MLE_LEADING) or fix_last_variables (MLE_TRAILING) fixes next."""
        if order not in (MLE_LEADING, MLE_TRAILING):
            raise RingError("round_evals: unknown order")
        return self._call(order, stream)

    def sum(self, stream=None):
        """sum_b g(b) over the hypercube as one ring element: the claimed sum of the sum-check."""
        return self._call(MLE_ROUND_SUM, stream)

    def _over(self, tables, num_vars):
        """the same terms and coefficients over `tables`, one per table slot of this polynomial: the slots stay deduplicated"""
        g = VirtualPolynomial(self.ring, num_vars)
        g.tables = list(tables)
        g.terms = [list(t) for t in self.terms]
        g.coeffs = list(self.coeffs)
        g._slot = {self._key(t): j for j, t in enumerate(g.tables)}
        return g

    def fold_round_evals(self, r, order=MLE_LEADING, stream=None):
        """One prover round in one pass over the distinct tables (sr_vpoly_round_fold_evals_dev): every table slot with the variable
        fix_variables (MLE_LEADING) or fix_last_variables (MLE_TRAILING) fixes next set to the ring element `r`, and the message of
        the round that follows.  Returns (message, the polynomial of the same terms and coefficients over the folded tables, in
        num_vars - 1 variables): what fixed_variables(r) followed by round_evals returns, bit for bit.  num_vars >= 2; the last
        round folds with fixed_variables."""
        import torch

        if order not in (MLE_LEADING, MLE_TRAILING):
            raise RingError("fold_round_evals: unknown order")
        if not self.terms:
            raise RingError("VirtualPolynomial: no product has been added")
        ring, nv = self.ring, self._num_vars
        if nv < 2:
            raise RingError("fold_round_evals: num_vars >= 2 (the last round folds with fixed_variables)")
        if self._has_columns():
            return self._dense(stream).fold_round_evals(r, order, stream)
        like = next((t.evaluations for t in self.tables if len(t)), self.tables[0].evaluations)
        w = ring.words_per_elem
        out = torch.empty((self.degree + 1) * w, dtype=like.dtype, device=like.device)
        sizes = [(len(t) + 1) // 2 if order == MLE_LEADING else min(len(t), 1 << (nv - 1)) for t in self.tables]
        folded = [torch.empty(n * w, dtype=like.dtype, device=like.device) for n in sizes]
        need = ring.vpoly_round_fold_plan(nv, len(self.tables), len(self.terms), self.degree, order)[0]
        work = torch.empty(need * w, dtype=like.dtype, device=like.device) if need else None
        coeffs = self._coeff_tensor(like, stream)
        if stream is not None:
            for t in folded + [work, coeffs]:
                if t is not None:
                    t.record_stream(stream)
        ring.vpoly_round_fold_evals_dev(out, folded, [t.evaluations for t in self.tables], self.terms, coeffs, nv, r, order, work, stream)
        return out, self._over([DenseMultilinearExtension(ring, nv - 1, f) for f in folded], nv - 1)

    def round_evals_weighted(self, weights, order=MLE_LEADING, stream=None):
        """The round message with a per-pair weight (sr_vpoly_wround_evals_dev): the degree + 1 elements
        h(t) = sum_b weights[b] * g(t, b), t = 0 .. degree, b over the 2^(num_vars - 1) pairs of the round.  The weight is no factor:
        it is constant in the round's variable and is not counted in the degree.  weights: a CUDA tensor of 2^(num_vars - 1) ring
        elements, never written.  With eq(z_rest, .) as weights this is the eq(z, .) factor of a zero-check without a table
        (EqSumCheck below)."""
        import torch

        if order not in (MLE_LEADING, MLE_TRAILING):
            raise RingError("round_evals_weighted: unknown order")
        if not self.terms:
            raise RingError("VirtualPolynomial: no product has been added")
        ring, nv = self.ring, self._num_vars
        if self._has_columns():
            return self._round_evals_indexed(weights, order, stream)
        like = next((t.evaluations for t in self.tables if len(t)), self.tables[0].evaluations)
        w = ring.words_per_elem
        out = torch.empty((self.degree + 1) * w, dtype=like.dtype, device=like.device)
        need = ring.vpoly_wround_plan(nv, len(self.tables), len(self.terms), self.degree, order)[0]
        work = torch.empty(need * w, dtype=like.dtype, device=like.device) if need else None
        coeffs = self._coeff_tensor(like, stream)
        if stream is not None:
            for t in (work, coeffs):
                if t is not None:
                    t.record_stream(stream)
        ring._vpoly_wround_evals_dev(out, weights, [t.evaluations for t in self.tables], self.terms, coeffs, nv, order, work, stream)
        return out

    def _indexed_operands(self):
        """the operands of sr_vpoly_iwround_*: (tables, columns, terms, order) -- the dense slots first, then the column slots, the terms
        renumbered; order[i]: the polynomial's slot of operand slot i"""
        order = [j for j, t in enumerate(self.tables) if not self._is_column(t)] + [j for j, t in enumerate(self.tables) if self._is_column(t)]
        where = {j: i for i, j in enumerate(order)}
        tables = [self.tables[j].evaluations for j in order if not self._is_column(self.tables[j])]
        columns = [self.tables[j].column for j in order if self._is_column(self.tables[j])]
        return tables, columns, [[where[j] for j in t] for t in self.terms], order

    def _round_evals_indexed(self, weights, order, stream):
        import torch

        from . import wsumcheck

        ring, nv, w = self.ring, self._num_vars, self.ring.words_per_elem
        dtype, device = self._like()
        like = torch.empty(0, dtype=dtype, device=device)
        tables, columns, terms, _ = self._indexed_operands()
        out = torch.empty((self.degree + 1) * w, dtype=dtype, device=device)
        need = wsumcheck.vpoly_iwround_plan(ring, nv, len(tables), len(columns), len(terms), self.degree, order)[0]
        work = torch.empty(need * w, dtype=dtype, device=device) if need else None
        coeffs = self._coeff_tensor(like, stream)
        if stream is not None:
            for t in (work, coeffs):
                if t is not None:
                    t.record_stream(stream)
        wsumcheck.vpoly_iwround_evals_dev(ring, out, weights, tables, columns, terms, coeffs, nv, order, work, stream)
        return out

    def _fold_round_evals_indexed(self, r, next_weights, order, stream):
        import torch

        from . import wsumcheck

        ring, nv, w = self.ring, self._num_vars, self.ring.words_per_elem
        dtype, device = self._like()
        like = torch.empty(0, dtype=dtype, device=device)
        tables, columns, terms, slots = self._indexed_operands()
        out = torch.empty((self.degree + 1) * w, dtype=dtype, device=device)
        sizes = [(len(self.tables[j]) + 1) // 2 if order == MLE_LEADING else min(len(self.tables[j]), 1 << (nv - 1)) for j in slots]
        folded = [torch.empty(n * w, dtype=dtype, device=device) for n in sizes]
        need = wsumcheck.vpoly_iwround_plan(ring, nv, len(tables), len(columns), len(terms), self.degree, order, fold=True)[0]
        work = torch.empty(need * w, dtype=dtype, device=device) if need else None
        coeffs = self._coeff_tensor(like, stream)
        if stream is not None:
            for t in folded + [work, coeffs]:
                if t is not None:
                    t.record_stream(stream)
        wsumcheck.vpoly_iwround_fold_evals_dev(ring, out, folded, next_weights, tables, columns, terms, coeffs, nv, r, order, work, stream)
        dense = [None] * len(slots)
        for i, j in enumerate(slots):
            dense[j] = DenseMultilinearExtension(ring, nv - 1, folded[i])
        return out, self._over(dense, nv - 1)

    def fold_round_evals_weighted(self, r, next_weights, order=MLE_LEADING, stream=None):
        """fold_round_evals with a per-pair weight on the message (sr_vpoly_wround_fold_evals_dev): every table slot folded at `r`,
        and round_evals_weighted(next_weights) of the folded polynomial, in one pass.  next_weights: 2^(num_vars - 2) ring elements.
        Returns (message, the polynomial over the folded tables in num_vars - 1 variables).  num_vars >= 2."""
        import torch

        if order not in (MLE_LEADING, MLE_TRAILING):
            raise RingError("fold_round_evals_weighted: unknown order")
        if not self.terms:
            raise RingError("VirtualPolynomial: no product has been added")
        ring, nv = self.ring, self._num_vars
        if nv < 2:
            raise RingError("fold_round_evals_weighted: num_vars >= 2 (the last round folds with fixed_variables)")
        if self._has_columns():
            return self._fold_round_evals_indexed(r, next_weights, order, stream)
        like = next((t.evaluations for t in self.tables if len(t)), self.tables[0].evaluations)
        w = ring.words_per_elem
        out = torch.empty((self.degree + 1) * w, dtype=like.dtype, device=like.device)
        sizes = [(len(t) + 1) // 2 if order == MLE_LEADING else min(len(t), 1 << (nv - 1)) for t in self.tables]
        folded = [torch.empty(n * w, dtype=like.dtype, device=like.device) for n in sizes]
        need = ring.vpoly_wround_fold_plan(nv, len(self.tables), len(self.terms), self.degree, order)[0]
        work = torch.empty(need * w, dtype=like.dtype, device=like.device) if need else None
        coeffs = self._coeff_tensor(like, stream)
        if stream is not None:
            for t in folded + [work, coeffs]:
                if t is not None:
                    t.record_stream(stream)
        ring._vpoly_wround_fold_evals_dev(out, folded, next_weights, [t.evaluations for t in self.tables], self.terms, coeffs, nv, r, order,
                                         work, stream)
        return out, self._over([DenseMultilinearExtension(ring, nv - 1, f) for f in folded], nv - 1)

    def fixed_variables(self, point, order=MLE_LEADING, stream=None):
        """The polynomial of the same terms and coefficients with the variables of `point` fixed in every distinct table:
        fixed_variables (MLE_LEADING) or fix_last_variables (MLE_TRAILING) per table slot -- the last round of a sum-check, and
        callers that want no message."""
        if order not in (MLE_LEADING, MLE_TRAILING):
            raise RingError("fixed_variables: unknown order")
        n_fixed = self.ring._batch_of(point.numel())
        if n_fixed > self._num_vars:
            raise RingError("fixed_variables: the point has more entries than the polynomial has variables")
        if self._has_columns():
            return self._dense(stream).fixed_variables(point, order, stream)
        fold = (lambda t: t.fixed_variables(point, stream)) if order == MLE_LEADING else (lambda t: t.fix_last_variables(point, stream))
        return self._over([fold(t) for t in self.tables], self._num_vars - n_fixed)


class EqSumCheck:
    """The prover of a whole sum-check of  sum_b eq(z, b) g(b)  -- a zero-check, R1CS, the layer claim of a product or fraction tree --
    WITHOUT an eq table.  In the round that binds variable v, with the challenges r of the earlier rounds bound,
        s(t) = [prod_{i bound} eq(z_i, r_i)] * eq(z_v, t) * h(t),   h(t) = sum_b w[b] g(t, b),   w = eq(z_rest, .)
    where g is the claim without eq, folded at the challenges so far, and w the eq table of the unbound coordinates of z only: one
    element per pair, constant in t, never folded (VirtualPolynomial.round_evals_weighted / fold_round_evals_weighted).  h has one
    degree less than s; the message() is still the degree + 2 elements s(0 .. degree + 1), bit-identical to what the prover that holds
    eq(z, .) as one more table sends (all arithmetic is exact on canonical values).

    g: a VirtualPolynomial of n >= 1 variables (not modified); z: a CUDA tensor of n ring elements; order: MLE_LEADING binds variable
    0 first, MLE_TRAILING variable n - 1.  The weights of all n rounds are built here with n eq_table_dev calls into one buffer of
    2^n - 1 elements: round j = 1 .. n has 2^(n - j) elements, the eq table of z[j:] (leading) or z[:n - j] (trailing)."""

    def __init__(self, g, z, order=MLE_LEADING, stream=None):
        import torch

        if order not in (MLE_LEADING, MLE_TRAILING):
            raise RingError("EqSumCheck: unknown order")
        ring, n = g.ring, g.num_vars
        w = ring.words_per_elem
        if n < 1 or not g.terms:
            raise RingError("EqSumCheck: a polynomial of at least one variable and one product")
        if z.numel() != n * w:
            raise RingError("EqSumCheck: z must hold num_vars ring elements")
        self.ring, self.order, self.stream, self.z = ring, order, stream, z
        self._n, self._d = n, g.degree
        self.g = g
        self.round = 1
        self.challenges = []
        d = self._d
        with self._on():
            self.weights = torch.empty(((1 << n) - 1) * w, dtype=z.dtype, device=z.device)
            consts = torch.zeros((2 * d + 5) * w, dtype=z.dtype, device=z.device)
        for j in range(1, n + 1):
            point = z[j * w:] if order == MLE_LEADING else z[:(n - j) * w]
            ring.eq_table_dev(self._weights_of(j), point if point.numel() else None, stream)
        # constants, from one() by additions only: R::from(t), t = 0 .. d + 1, and the signed binomials of the finite difference
        self._one = consts[:w]
        ring.eq_table_dev(self._one, None, stream)
        self._t = consts[w:(d + 3) * w]  # zero, one, .., d + 1
        for t in range(1, d + 2):
            with self._on():
                self._t[t * w:(t + 1) * w] = self._t[(t - 1) * w:t * w]
            ring.add_dev(self._t[t * w:(t + 1) * w], self._one, stream)
        self._binom = consts[(d + 3) * w:(2 * d + 4) * w]  # (-1)^(d - i) C(d + 1, i), i = 0 .. d
        c = 1
        for i in range(d + 1):
            e = self._binom[i * w:(i + 1) * w]
            for _ in range(c):
                (ring.add_dev if (d - i) % 2 == 0 else ring.sub_dev)(e, self._one, stream)
            c = c * (d + 1 - i) // (i + 1)
        with self._on():
            self._ones = self._one.repeat(d + 2)
            self._prefix = self._one.clone()
        self._h = g.round_evals_weighted(self._weights_of(1), order, stream)

    def _on(self):
        import contextlib

        import torch

        return torch.cuda.stream(self.stream) if self.stream is not None else contextlib.nullcontext()

    def _weights_of(self, j):
        """the weights of round j = 1 .. n: a view of 2^(n - j) elements"""
        w, n = self.ring.words_per_elem, self._n
        off = (1 << n) - (1 << (n - j + 1))
        return self.weights[off * w:(off + (1 << (n - j))) * w]

    def _z_of(self, j):
        """the coordinate of z that round j binds"""
        w = self.ring.words_per_elem
        v = j - 1 if self.order == MLE_LEADING else self._n - j
        return self.z[v * w:(v + 1) * w]

    def _eq_line(self, j):
        """(e0, step): eq(z_v, t) = e0 + t step with e0 = one() - z_v, step = 2 z_v - one()"""
        with self._on():
            e0 = self._one.clone()
            step = self._z_of(j).clone()
        self.ring.sub_dev(e0, self._z_of(j), self.stream)
        self.ring.sub_dev(step, e0, self.stream)
        return e0, step

    @property
    def degree(self):
        """the degree of g; a message has degree + 2 elements"""
        return self._d

    def message(self):
        """s(0 .. degree + 1) of the current round: degree + 2 ring elements"""
        import torch

        if self.round > self._n:
            raise RingError("EqSumCheck: every variable is bound")
        ring, st, w, d = self.ring, self.stream, self.ring.words_per_elem, self._d
        with self._on():
            s = torch.empty((d + 2) * w, dtype=self._h.dtype, device=self._h.device)
            s[:(d + 1) * w] = self._h
            hb = self._h.clone()
        # h(d + 1) = sum_{i <= d} (-1)^(d - i) C(d + 1, i) h(i): the (d + 1)-th finite difference of a polynomial of degree d is zero
        ring.ntt_mul_dev(hb, self._binom, st)
        ring.sum_dev(s[(d + 1) * w:], hb, st)
        e0, step = self._eq_line(self.round)
        with self._on():
            line = self._ones.clone()
        ring.mul_elem_dev(line, e0, st)
        ring.mul_elem_add_dev(line, self._t[:(d + 2) * w], step, st)
        ring.ntt_mul_dev(s, line, st)
        ring.mul_elem_dev(s, self._prefix, st)  # the prefix product last
        return s

    def next(self, r):
        """binds the current round's variable to the challenge r (one ring element) and advances to the next round"""
        if self.round > self._n:
            raise RingError("EqSumCheck: every variable is bound")
        ring, st, j = self.ring, self.stream, self.round
        if self.g.num_vars >= 2:
            self._h, self.g = self.g.fold_round_evals_weighted(r, self._weights_of(j + 1), self.order, st)
        else:
            self._h, self.g = None, self.g.fixed_variables(r, self.order, st)
        e0, step = self._eq_line(j)
        ring.mul_elem_add_dev(e0, step, r, st)  # eq(z_v, r)
        ring.ntt_mul_dev(self._prefix, e0, st)
        self.challenges.append(r)
        self.round = j + 1
        return self

    def final(self):
        """(the values of g's table slots at the challenges, one ring element each; eq(z, r)) once every variable is bound"""
        if self.round <= self._n:
            raise RingError("EqSumCheck: %d variables are still unbound" % (self._n - self.round + 1))
        return [t.evaluations for t in self.g.tables], self._prefix


def _next_pow2(n):
    return 1 if n <= 1 else 1 << (n - 1).bit_length()


class SparseMultilinearExtension:
    """mle/sparse.rs: the evaluations that are stored, as (indices, values) in ascending index order -- the iteration order of the
    reference's BTreeMap.  indices: a host numpy uint64 array; values: one CUDA tensor of len(indices) ring elements in CRT/NTT
    form.  Stored zeros are legal and are kept, as from_evaluations and fix_variables keep them.  rand / rand_with_config, relabel,
    Add / Sub of two sparse MLEs and ark-serialize of the map are not mirrored (index-set merging and host bookkeeping)."""

    def __init__(self, ring, num_vars, indices, values):
        indices = np.ascontiguousarray(indices, dtype=np.uint64)
        if not 0 <= num_vars < 64:
            raise RingError("SparseMultilinearExtension: num_vars must be below 64")
        if ring._batch_of(values.numel()) != indices.size:
            raise RingError("SparseMultilinearExtension: one value per index")
        smle_fix_pattern(indices, num_vars, 0)  # ascending, below 2^num_vars
        if indices.size:
            ring._dev(values)
        self.ring = ring
        self._num_vars = int(num_vars)
        self.indices = indices
        self.values = values
        self._work = None

    @classmethod
    def from_evaluations(cls, ring, num_vars, indices, values):
        """sparse.rs:33-51: any order of distinct indices; the values are gathered into ascending index order only if needed."""
        import torch

        indices = np.ascontiguousarray(indices, dtype=np.uint64)
        if indices.size > 1 and not np.all(indices[1:] > indices[:-1]):
            order = np.argsort(indices, kind="stable")
            indices = indices[order]
            if np.any(indices[1:] == indices[:-1]):
                raise RingError("SparseMultilinearExtension: an index is stored twice")
            perm = torch.from_numpy(order.astype(np.int64)).to(values.device)
            values = values.view(-1, ring.words_per_elem)[perm].reshape(-1).contiguous()
        return cls(ring, num_vars, indices, values)

    from_sparse_slice = from_evaluations  # sparse.rs:117-123

    @classmethod
    def from_slice(cls, ring, num_vars, values):
        """sparse.rs:125-134: a dense slice, entry i at index i (zeros are stored too)."""
        return cls(ring, num_vars, np.arange(ring._batch_of(values.numel()), dtype=np.uint64), values)

    @staticmethod
    def matrix_indices(cols, row_ptr, nrows, ncols):
        """sparse.rs:97-115: (num_vars, index of every stored entry) of an nrows x ncols CSR matrix: row * next_pow2(ncols) + col."""
        cols, row_ptr = np.asarray(cols, dtype=np.uint64), np.asarray(row_ptr, dtype=np.uint64)
        n_rows, n_cols = _next_pow2(nrows), _next_pow2(ncols)
        rows = np.repeat(np.arange(nrows, dtype=np.uint64), np.diff(row_ptr).astype(np.int64))
        return (n_rows * n_cols).bit_length() - 1, rows * np.uint64(n_cols) + cols

    @classmethod
    def from_matrix(cls, ring, vals, cols, row_ptr, nrows, ncols):
        """from_matrix on the CSR triple of spmv_ntt_dev (vals: a CUDA tensor, used where it lies; cols, row_ptr: host arrays or
        tensors).  The values are gathered by a permutation only if the columns of some row are not ascending."""
        to_np = lambda a: a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
        num_vars, idx = cls.matrix_indices(to_np(cols), to_np(row_ptr), nrows, ncols)
        return cls.from_evaluations(ring, num_vars, idx, vals)

    @property
    def num_vars(self):
        return self._num_vars

    def __len__(self):
        return self.indices.size

    def _fold(self, point, stream):
        import torch

        ring = self.ring
        n_fixed = ring._batch_of(point.numel()) if point is not None else 0
        if n_fixed > self._num_vars:
            raise RingError("fix_variables: invalid partial point dimension")  # sparse.rs:172 asserts
        out_idx, seg = smle_fix_pattern(self.indices, self._num_vars, n_fixed)
        dev = self.values.device
        out = torch.empty(out_idx.size * ring.words_per_elem, dtype=self.values.dtype, device=dev)
        if out_idx.size:
            need = ring.smle_plan(self.indices.size, out_idx.size, n_fixed)[0]
            if need and (self._work is None or self._work.numel() < need * ring.words_per_elem):
                self._work = torch.empty(need * ring.words_per_elem, dtype=self.values.dtype, device=dev)
            d_idx = torch.from_numpy(self.indices.view(np.int64)).to(dev)
            d_seg = torch.from_numpy(seg.view(np.int64)).to(dev)
            ring.smle_fix_variables_dev(out, self.values, d_idx, d_seg, point, self._work if need else None, stream)
        return out_idx, out, self._num_vars - n_fixed

    def fix_variables(self, partial_point, stream=None):
        """sparse.rs:170-207: fixes variables 0 .. len(partial_point) - 1 and rebinds this object to the result."""
        self.indices, self.values, self._num_vars = self._fold(partial_point, stream)
        return self

    def fixed_variables(self, partial_point, stream=None):
        """sparse.rs:209-213: the same as a new object."""
        idx, vals, nv = self._fold(partial_point, stream)
        return SparseMultilinearExtension(self.ring, nv, idx, vals)

    def _zero(self):
        import torch

        return torch.zeros(self.ring.words_per_elem, dtype=self.values.dtype, device=self.values.device)

    def evaluate(self, point, stream=None):
        """sparse.rs:53-56: the value at `point` (one ring element); an MLE with no stored entry evaluates to zero()."""
        if self.ring._batch_of(point.numel()) != self._num_vars:
            raise RingError("evaluate: the point must have num_vars entries")  # sparse.rs:54 asserts
        idx, vals, _ = self._fold(point, stream)
        return vals if idx.size else self._zero()

    def __getitem__(self, index):
        """sparse.rs:346-365 `Index`: the stored evaluation at `index`, zero() where none is stored."""
        j = int(np.searchsorted(self.indices, np.uint64(index)))
        if j < self.indices.size and int(self.indices[j]) == int(index):
            w = self.ring.words_per_elem
            return self.values[j * w:(j + 1) * w]
        return self._zero()

    def neg(self, stream=None):
        """sparse.rs `Neg`: every stored value negated (sr_neg_batch_dev), as a new object."""
        vals = self.values.clone()
        if self.indices.size:
            self.ring.neg_dev(vals, stream)
        return SparseMultilinearExtension(self.ring, self._num_vars, self.indices.copy(), vals)

    def to_evaluations(self):
        """sparse.rs:136-145 `to_dense_multilinear_extension`'s table: all 2^num_vars elements, the stored ones scattered."""
        import torch

        w = self.ring.words_per_elem
        out = torch.zeros(w << self._num_vars, dtype=self.values.dtype, device=self.values.device)
        if self.indices.size:
            rows = torch.from_numpy(self.indices.view(np.int64)).to(self.values.device)
            out.view(-1, w)[rows] = self.values.view(-1, w)
        return out
