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
