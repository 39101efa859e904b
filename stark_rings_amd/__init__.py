"""stark_rings_amd -- MI355X (gfx950) backend for stark-rings' CRT/NTT ring-multiplication path.

Layout:
  csrc/                 hand-written HIP kernels + the C ABI (include/stark_rings_hip.h)
  _lib.py               ctypes loader of libstarkrings_hip.so
  rings.py              host-side mirror of the reference interface (CyclotomicConfig / CRT / ICRT /
                        Flatten at batch granularity) on top of the C ABI
  wire.py               ark-serialize framing of Vec / Matrix / SparseMatrix / SymmetricMatrix around the device codec
  mle.py                DenseMultilinearExtension and SparseMultilinearExtension of crates/poly over device-resident values,
                        with the round message of a sum-check over a product, or a sum of products (VirtualPolynomial), of dense MLEs,
                        and EqSumCheck: a whole sum-check of eq(z, .) g with eq as per-pair weights, not a table
  wsumcheck.py          the device-pointer forms of the weighted sum-check rounds (sr_vpoly_wround_evals_dev, sr_vpoly_wround_fold_evals_dev),
                        and the same rounds with integer columns as factors (sr_vpoly_iwround_*)
  range_check.py        range-check (norm-check) rounds: sum_i mu_i prod_j (f_i - j) over |j| < B from one read of each table, and
                        RangePolynomial, the claim EqSumCheck runs a whole norm check on
  grand_product.py      ProductTree: every layer of a table's binary product tree, the circuit of the layered grand-product argument
  frac_tree.py          FractionTree: every layer of a sum of fractions p/q, the circuit of the layered logUp (lookup, range) argument
  lincomb.py            linear combinations of up to 16 tables with ring-element coefficients, up to 4 outputs from one pass
  inverse.py            batch inversion num / den slot by slot (Montgomery's trick per lane), zero slots counted
  index_columns.py      integer columns (u64 per row, or a progression) beside the tables of a linear combination; multiplicities
  lookup.py             PermutationCheck and LookupCheck: leaves (lincomb), trees and layer claims end to end on the device
  symmetric.py          SymmetricMatrix of crates/linear_algebra, packed: Gram matrices and the G^T M G recomposition
  sparse.py             SparseMatrix of crates/linear_algebra with device-resident values: transpose, sparse x sparse product
  monomial.py           the reference's monomial helpers (monomial.rs) over the ring product
  sharding.py           batch sharding across the GPUs of one node (one process per GPU)
"""
from .rings import (  # noqa: F401
    BABYBEAR_72,
    BABYBEAR_POW2,
    GOLDILOCKS_24,
    GOLDILOCKS_POW2,
    STARK_POW2,
    MLE_LEADING,
    MLE_ROUND_SUM,
    MLE_TRAILING,
    CyclotomicRing,
    RingError,
)
from .mle import DenseMultilinearExtension, EqSumCheck, SparseMultilinearExtension, VirtualPolynomial  # noqa: F401
from .grand_product import ProductTree  # noqa: F401
from .wsumcheck import (vpoly_iwround_evals_dev, vpoly_iwround_fold_evals_dev, vpoly_iwround_plan, vpoly_wround_evals_dev,  # noqa: F401
                        vpoly_wround_fold_evals_dev)
from .range_check import RangePolynomial, range_wround_evals, range_wround_evals_dev, range_wround_plan  # noqa: F401
from .frac_tree import FractionTree, frac_tree_dev, frac_tree_plan  # noqa: F401  (the host-pointer form: frac_tree.frac_tree)
from .lincomb import lincomb_dev, lincomb_plan  # noqa: F401  (the host-pointer form: lincomb.lincomb)
from .inverse import inverse_dev, inverse_plan, inverse_zero_count  # noqa: F401  (the host-pointer form: inverse.inverse)
from .index_columns import (IndexColumn, IndexMultilinearExtension, from_u64_dev, identity_permutation, identity_permutation_mles, index_count,  # noqa: F401
                            index_count_dev, lincomb_index, lincomb_index_dev, lincomb_index_plan)
from .lookup import (LookupCheck, LookupHelperColumns, PermutationCheck, fingerprint, fingerprint_indexed, permutation_leaves,  # noqa: F401
                     permutation_leaves_indexed)
from .symmetric import SymmetricMatrixNTT, recompose_left_right_symmetric_matrix  # noqa: F401
from .sparse import SparseMatrixNTT  # noqa: F401
