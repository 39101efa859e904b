"""Range-check (norm-check) rounds on device (sr_range_wround_plan, sr_range_wround_evals_dev, sr_range_wround_evals;
include/stark_rings_hip.h, csrc/range_check.hpp): the claim a lattice folding scheme runs in every fold and for every decomposed witness,

    sum_b eq(beta, b) * sum_i mu_i * prod_{j = -(B-1)}^{B-1} ( f_i(b) - j ) = 0,

which says that every entry of every f_i lies in (-B, B).  A round message is

    h(t) = sum_{b < half} w[b] * sum_i mu_i * P_B( lo_i[b] + t (hi_i[b] - lo_i[b]) ),  t = 0 .. 2 B - 1,   P_B(x) = prod_j (x - R::from(j))

with w the eq factor as a per-pair weight (wsumcheck.py).  A table is read once per launch whatever the bound: no shifted copies f - j
exist and none is folded.  The three calls are functions of this module, not methods, because tests/test_dev_boundaries_host.py keeps
a closed table of the *_dev methods of CyclotomicRing.  RangePolynomial is the claim without eq with exactly the members EqSumCheck
(mle.py) uses of its g, so that EqSumCheck(RangePolynomial(ring, tables, bound), z, order) runs a whole norm check.
"""
from .mle import DenseMultilinearExtension
from .rings import MLE_LEADING, MLE_TRAILING, RingError, _np_ptr

RANGE_MAX_TABLES = 8
RANGE_MAX_BOUND = 8


def range_wround_plan(ring, num_vars, n_tables, bound, order=MLE_LEADING):
    """sr_range_wround_plan: (work_elems, launches) of a range-check round message -- host arithmetic only."""
    return ring._plan_of(ring._lib.sr_range_wround_plan, num_vars, n_tables, bound, order)


def range_wround_evals_dev(ring, out, weights, tables, bound, coeffs, num_vars, order=MLE_LEADING, work=None, stream=None):
    """out[t] = sum_{b < half} weights[b] * sum_i coeffs[i] * P_bound(lo_i[b] + t (hi_i[b] - lo_i[b])), t = 0 .. 2 bound - 1.
    out: a CUDA tensor of 2 bound ring elements; weights: 2^(num_vars - 1) ring elements, one per pair, never written; tables: 1 .. 8
    CUDA tensors of n_evals <= 2^num_vars elements; coeffs: a CUDA tensor of one ring element per table, or None for one(); order:
    MLE_LEADING or MLE_TRAILING; work: at least range_wround_plan()[0] elements (None only where the plan needs none).  Allocates
    nothing."""
    po, ptrs, sizes, n, pc, pwt, pw, nw = ring._round_dev_args("range_wround_evals", out, 2 * bound if 2 <= bound <= RANGE_MAX_BOUND else None,
                                                               "2 bound elements", tables, work, coeffs, len(tables), "table", weights,
                                                               num_vars - 1)
    ring._check(ring._lib.sr_range_wround_evals_dev(ring._ctx, po, pwt, ptrs, sizes, n, int(bound), pc, int(num_vars), int(order), pw, nw,
                                                    ring._stream(stream)))
    return out


def range_wround_evals(ring, weights, tables, bound, coeffs, num_vars, order=MLE_LEADING):
    """Host buffers: sr_range_wround_evals (see range_wround_evals_dev); returns the 2 bound elements."""
    tables, weights, coeffs, out, ptrs, sizes, n = ring._round_host_args("range_wround_evals", 2 * max(int(bound), 1), tables, coeffs,
                                                                         len(tables), "table", weights)
    if weights is not None and 1 <= num_vars < 48 and weights.size != ring.words_per_elem << (num_vars - 1):
        raise RingError("range_wround_evals: weights must hold one element per pair")
    ring._check(ring._lib.sr_range_wround_evals(ring._ctx, _np_ptr(out), None if weights is None else weights.ctypes.data, ptrs, sizes, n,
                                                int(bound), None if coeffs is None else coeffs.ctypes.data, int(num_vars), int(order)))
    return out


class RangePolynomial:
    """The range-check claim without eq, g(x) = sum_i mu_i P_B(f_i(x)), over 1 .. 8 dense MLEs of one ring and num_vars: the members
    EqSumCheck uses of its g, so EqSumCheck(RangePolynomial(ring, tables, bound, coeffs), z, order) is the prover of the whole norm
    check.  tables: DenseMultilinearExtension objects (kept, not copied); coeffs: a CUDA tensor of one ring element per table, or
    None for one().  degree = 2 bound - 1."""

    def __init__(self, ring, tables, bound, coeffs=None):
        tables = list(tables)
        if not 1 <= len(tables) <= RANGE_MAX_TABLES:
            raise RingError("RangePolynomial: 1 .. %d tables" % RANGE_MAX_TABLES)
        if not 2 <= int(bound) <= RANGE_MAX_BOUND:
            raise RingError("RangePolynomial: bound must be 2 .. %d" % RANGE_MAX_BOUND)
        nv = tables[0].num_vars
        if any(t.ring is not ring or t.num_vars != nv for t in tables):
            raise RingError("RangePolynomial: every MLE must have the polynomial's ring and num_vars")
        if coeffs is not None and coeffs.numel() != len(tables) * ring.words_per_elem:
            raise RingError("RangePolynomial: one coefficient per table")
        self.ring = ring
        self.tables = tables
        self.bound = int(bound)
        self.coeffs = coeffs
        self._num_vars = nv
        self.terms = [list(range(len(tables)))]  # truthy: one claim over every table

    @property
    def num_vars(self):
        return self._num_vars

    @property
    def degree(self):
        """2 bound - 1: a round message has degree + 1 elements"""
        return 2 * self.bound - 1

    def round_evals_weighted(self, weights, order=MLE_LEADING, stream=None):
        """h(t) = sum_b weights[b] * g(t, b), t = 0 .. degree (range_wround_evals_dev)."""
        import torch

        if order not in (MLE_LEADING, MLE_TRAILING):
            raise RingError("round_evals_weighted: unknown order")
        ring, nv = self.ring, self._num_vars
        like = weights
        w = ring.words_per_elem
        out = torch.empty(2 * self.bound * w, dtype=like.dtype, device=like.device)
        need = range_wround_plan(ring, nv, len(self.tables), self.bound, order)[0]
        work = torch.empty(need * w, dtype=like.dtype, device=like.device) if need else None
        if stream is not None and work is not None:
            work.record_stream(stream)
        return range_wround_evals_dev(ring, out, weights, [t.evaluations for t in self.tables], self.bound, self.coeffs, nv, order, work, stream)

    def fixed_variables(self, point, order=MLE_LEADING, stream=None):
        """The same claim with the variables of `point` fixed in every table (sr_mle_fix_variables_dev per table)."""
        if order not in (MLE_LEADING, MLE_TRAILING):
            raise RingError("fixed_variables: unknown order")
        if self.ring._batch_of(point.numel()) > self._num_vars:
            raise RingError("fixed_variables: the point has more entries than the polynomial has variables")
        fold = (lambda t: t.fixed_variables(point, stream)) if order == MLE_LEADING else (lambda t: t.fix_last_variables(point, stream))
        return RangePolynomial(self.ring, [fold(t) for t in self.tables], self.bound, self.coeffs)

    def fold_round_evals_weighted(self, r, next_weights, order=MLE_LEADING, stream=None):
        """Every table folded at `r` (one variable, sr_mle_fix_variables_dev) and round_evals_weighted(next_weights) of the folded
        claim.  Returns (message, the claim over the folded tables in num_vars - 1 variables).  num_vars >= 2."""
        if self._num_vars < 2:
            raise RingError("fold_round_evals_weighted: num_vars >= 2 (the last round folds with fixed_variables)")
        g = self.fixed_variables(r, order, stream)
        return g.round_evals_weighted(next_weights, order, stream), g
