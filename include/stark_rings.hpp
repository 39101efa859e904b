// stark_rings.hpp -- C++17 host-side mirror of the reference's ring interface for the CRT/NTT hot path,
// header-only, on top of the C ABI (stark_rings_hip.h).  The reference is Rust; no Rust toolchain exists in
// this image, so the host layer a crates/ring maintainer would write in Rust is restated
// here in C++ with the same names, argument meaning and error behaviour:
//
//   reference (crates/ring/src/cyclotomic_ring/)                     here
//   ---------------------------------------------------------------  ------------------------------------------
//   trait CyclotomicConfig<N>            ring_config.rs:11-35        class CyclotomicConfig  (one ring + degree)
//     reduce_in_place(&mut Vec<Fp>)      ring_config.rs:23             reduce_in_place(std::vector<Fp>&)
//     crt_in_place(&mut [Fp])            ring_config.rs:27             crt_in_place(Fp*, len)
//     icrt_in_place(&mut [Fp])           ring_config.rs:34             icrt_in_place(Fp*, len)
//     crt(Vec<Fp>) -> Vec<CRTField>      ring_config.rs:29             crt(std::vector<Fp>) (same allocation)
//     icrt(Vec<CRTField>) -> Vec<Fp>     ring_config.rs:30             icrt(std::vector<Fp>)
//     CRT_FIELD_EXTENSION_DEGREE         ring_config.rs:19             crt_field_extension_degree()
//   CyclotomicPolyRingGeneral<C,N,D>     coeff_form.rs:31-33         class RqPolyVec   (a Vec<RqPoly>, flat)
//     Mul  (poly_mul + reduce)           coeff_form.rs:54-67,250-258   operator*, operator*=
//   CyclotomicPolyRingNTTGeneral<C,N,D>  ntt_form.rs:25-27           class RqNTTVec    (a Vec<RqNTT>, flat)
//     Mul / MulAssign (slot-wise)        ntt_form.rs:159-225           operator*, operator*=
//     Add / Sub                          ntt_form.rs:227-285,588-638   operator+=, operator-=  (both forms)
//   CRT::elementwise_crt                 crt.rs:10-25                RqPolyVec::elementwise_crt() &&  (in place, same allocation)
//   ICRT::elementwise_icrt               crt.rs:34-49                RqNTTVec::elementwise_icrt() &&
//   Flatten::flatten_to_coeffs           flatten.rs:11-17            flatten_to_coeffs(Vec&&) -> std::vector<uint64_t>
//   Flatten::promote_from_coeffs         flatten.rs:19-33            promote_from_coeffs(...) -> std::optional (nullopt if len % D != 0)
//   Matrix<RqNTT> (linear_algebra)       matrix.rs:14-20             class MatrixNTT        (dense, row-major, flat)
//     checked_mul_vec / try_mul_vec      matrix.rs:168-183             checked_mul_vec -> std::optional (nullopt: DifferentLengths), try_mul_vec throws
//     checked_mul_mat                    matrix.rs:148-166             checked_mul_mat -> std::optional
//     MulAssign<&R> (Matrix, Sparse)     matrix.rs:207-211,            operator*=(const RqNTTVec &one_element): every entry times one ring element
//                                        sparse_matrix.rs:303-307
//   DenseMultilinearExtension<RqNTT>     crates/poly mle/dense.rs    class DenseMultilinearExtension: fix_variables, fixed_variables,
//     (fix_variables, evaluate, +=)                                    fix_last_variables, evaluate, add_assign_scaled, to_evaluations;
//                                                                      round_evals / product_sum: a sum-check round's message (sr_mle_round_evals)
//     AddAssign<(R, &Self)>, MulAssign<R>, dense.rs:288-317, 370-374, lincomb_plan / lincomb / lincomb_dev (sr_lincomb: the three composed, up to 16
//     Add<R>, in one pass                  386-395                     tables and 4 outputs); DenseMultilinearExtension::linear_combination;
//                                                                      fingerprint, permutation_leaves, class PermutationCheck / LookupCheck /
//                                                                      LayerClaim: leaves, trees and layer claims of both arguments
//     From<u64> beside the tables          polynomials/                IndexColumn, lincomb_index_plan / lincomb_index / lincomb_index_dev,
//     (integer columns),                   multilinear_polynomial.rs   from_u64, index_count, linear_combination_indexed,
//     identity_permutation[_mles]          :79-133                     permutation_leaves_indexed, identity_permutation[_mles],
//                                                                      LookupCheck::from_indices (sr_lincomb_index, sr_index_count)
//   a sum of products of dense MLEs      (HyperPlonk's VirtualPolynomial) class VirtualPolynomial: add_mle_list, mul_by_mle, degree, round_evals, sum
//                                                                      (sr_vpoly_round_evals: one pass, every distinct table read once),
//                                                                      fold_round_evals (sr_vpoly_round_fold_evals: fold at the challenge
//                                                                      and the next message in one pass), fixed_variables,
//                                                                      round_evals_weighted / fold_round_evals_weighted (sr_vpoly_wround_*:
//                                                                      a per-pair weight, the eq factor without a table); class EqSumCheck:
//                                                                      a whole sum-check of eq(z, .) g, message / next / final;
//                                                                      class IndexMultilinearExtension: an IndexColumn as a factor,
//                                                                      read as u64 by the weighted rounds (sr_vpoly_iwround_*), to_dense
//   the range (norm) check of a lattice  (LatticeFold's norm check)     class RangePolynomial: sum_i mu_i prod_{|j| < B} (f_i - j) over 1 .. 8
//     folding scheme                                                   MLEs, each read once (sr_range_wround_evals); RangeSumCheck: the
//                                                                      whole check; CyclotomicConfig::range_wround_plan / _evals_dev / _evals
//   SparseMultilinearExtension<RqNTT>    crates/poly mle/sparse.rs   class SparseMultilinearExtension: from_slice, from_matrix, fix_variables,
//     precompute_eq                      sparse.rs:381-394             fixed_variables, evaluate, to_evaluations; eq_table(point); device
//                                                                      pointers: CyclotomicConfig::eq_table_dev / smle_plan / smle_fix_variables_dev
//   SymmetricMatrix<RqNTT>               linear_algebra/src/         class SymmetricMatrixNTT (packed: entry (i, j), j <= i, is element i (i + 1) / 2 + j):
//     from_par_fn(n, |i, j| <s_i, s_j>)  symmetric_matrix.rs:14-92     size, at, diag, rows, zero, from_rows (throws where From asserts), gram
//   recompose_left_right_symmetric_      balanced_decomposition/     recompose_left_right_symmetric_matrix(mat, powers) / .recompose_left_right;
//     matrix                             mod.rs:354-386                sr_gram_ntt, sr_symm_recompose (device pointers: the *_dev C calls)
//   WithLinfNorm / WithL2Norm for [Fq]   crates/ring/src/traits.rs    RqPolyVec::linf_norm / l2_norm_squared (the flattened coefficients, as
//     (of flatten_to_coeffs)             :6-36                         little-endian u64 words of the integer), *_per_element; sr_norm_plan,
//                                                                      sr_norm_batch, and sr_norm_batch_dev through CyclotomicConfig::norm_dev
//   GadgetDecompose / GadgetRecompose    balanced_decomposition/     gadget_decompose(const RqPolyVec&, b, k) / gadget_recompose(...)
//     for &[R] / Vec<R>                  mod.rs:163-206                (digit j of element e = element e * k + j; throws where it panics)
//   SparseMatrix<RqNTT>                  sparse_matrix.rs:17-22      class SparseMatrixNTT  (coeffs: rows of (element, column))
//     checked_mul_vec / try_mul_vec      sparse_matrix.rs:201-216      same contract; an out-of-range column throws (the reference panics)
//   CanonicalSerialize / Deserialize     coeff_form.rs:154-189,      serialize_compressed(vec / matrix) -> bytes, deserialize_*(cfg, bytes):
//     for ring elements, Vec, Matrix,    ntt_form.rs:24,               the element bytes come from the device codec (sr_serialize_batch), the
//     SparseMatrix                       matrix.rs:111-145,            u64 length words and (R, usize) pairs are written here; InvalidData and
//                                        sparse_matrix.rs:158-200      short input throw
//   monomial / unit_monomial / psi /     crates/ring/src/            same names; BaseRing scalars are passed as their signed representative
//     exp / exp_signed / psi_range_check monomial.rs:17-93             (Zq::center and sign, ring.rs:160-181) in an int64_t
//   decompose basis `b: u128`            balanced_decomposition/     every gadget function takes `u128` (unsigned __int128); 2^127 and above
//                                        mod.rs:62,73                  is refused for decomposition (negative after the reference's `as i128`)
//   DecomposeToVec for &[R] / Vec<R>     mod.rs:119-161              decompose_to_vec(v, b, k) -> std::vector<RqPolyVec> (one Vec<R> per element)
//   GadgetDecompose / GadgetRecompose    mod.rs:208-352              class MatrixPoly / SparseMatrixPoly: gadget_decompose (n x m -> n x k m;
//     for &[(R, usize)], Matrix<R>,                                    sparse entries (e, c) -> (digit_i, c k + i), zero digits dropped),
//     SparseMatrix<R>                                                  gadget_recompose; sparse_row_gadget_decompose / _recompose for one row
//   Cyclotomic::rot / into_rot_iter /    traits.rs:54-91             rot(RqPolyVec&) (every element times X), Rotation, into_rot_iter(v)
//     Rotation
//   (one context per GPU of a node)      SURVEY 8b / 8e              class ContextGroup: sr_ctx_create_group + sr_shard_range
//   (device-resident batches)            --                          CyclotomicConfig::*_dev(device pointers, stream), reserve_scratch,
//                                                                      plan_in_use, and the packed-u32 BabyBear forms (*_packed32_dev)
//
// What is deliberately narrowed: ring elements of degree 2^16 are 512 KiB, so the per-element `Copy` value type of
// the reference (ring.rs:13-15) is not mirrored; the drop-in seam is the batch (hard part 4).
// Errors: the reference panics (assert_eq!(len, D): goldilocks/ntt.rs:136, stark_prime/ntt.rs:122; "Wrong length":
// coeff_form.rs:39); here std::length_error / std::runtime_error are thrown.
#pragma once
#include <algorithm>
#include <cstdint>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "stark_rings_hip.h"

namespace stark_rings {

class CyclotomicConfig {
public:
    // plan: the kernel plan of the context (sr_plan), nullptr = defaults; fixed for the life of the context
    CyclotomicConfig(sr_ring ring, int log2_degree = 0, int device = 0, const sr_plan *plan = nullptr) : ring_(ring) {
        sr_ctx *c = nullptr;
        check(sr_ctx_create_ex(ring, log2_degree, device, plan, &c), "sr_ctx_create_ex");
        ctx_.reset(c, [](sr_ctx *p) { sr_ctx_destroy(p); });
        check(sr_ctx_degree(c, &degree_), "sr_ctx_degree");
        check(sr_ctx_limbs(c, &limbs_), "sr_ctx_limbs");
    }
    // adopts a context created elsewhere (ContextGroup); `owned` contexts are destroyed with the last copy
    CyclotomicConfig(sr_ring ring, sr_ctx *adopt) : ring_(ring) {
        ctx_.reset(adopt, [](sr_ctx *p) { sr_ctx_destroy(p); });
        check(sr_ctx_degree(adopt, &degree_), "sr_ctx_degree");
        check(sr_ctx_limbs(adopt, &limbs_), "sr_ctx_limbs");
    }
    sr_ring ring() const { return ring_; }
    size_t dimension() const { return degree_; }            // PolyRing::dimension()
    int limbs() const { return limbs_; }                    // N
    size_t words_per_elem() const { return degree_ * (size_t)limbs_; }
    size_t wire_coeff_bytes() const { return sr_wire_coeff_bytes(raw()); }   // bytes of one serialised coefficient
    size_t wire_elem_bytes() const { return degree_ * wire_coeff_bytes(); }
    int crt_field_extension_degree() const {
        return ring_ == SR_RING_GOLDILOCKS_24 ? 3 : (ring_ == SR_RING_BABYBEAR_72 ? 9 : (ring_ == SR_RING_FROG_16 ? 4 : 1));
    }
    sr_ctx *raw() const { return ctx_.get(); }

    // coefficients: up to 2*D coefficients of N limbs each -> reduced mod Phi, resized to D
    void reduce_in_place(std::vector<uint64_t> &coefficients) const {
        if (coefficients.size() % limbs_) throw std::length_error("reduce_in_place: not whole coefficients");
        const size_t in_len = coefficients.size() / limbs_;
        std::vector<uint64_t> out(words_per_elem());
        std::vector<uint64_t> dummy(1);
        check(sr_reduce_batch(raw(), in_len ? coefficients.data() : dummy.data(), in_len, out.data(), 1), "reduce_in_place");
        coefficients.swap(out);
    }
    void crt_in_place(uint64_t *coefficients, size_t len_words) const {
        if (len_words != words_per_elem()) throw std::length_error("crt_in_place: coefficients.len() != D");
        check(sr_ntt_fwd_batch(raw(), coefficients, 1), "crt_in_place");
    }
    void icrt_in_place(uint64_t *evaluations, size_t len_words) const {
        if (len_words != words_per_elem()) throw std::length_error("icrt_in_place: evaluations.len() != D");
        check(sr_ntt_inv_batch(raw(), evaluations, 1), "icrt_in_place");
    }
    std::vector<uint64_t> crt(std::vector<uint64_t> coefficients) const {
        crt_in_place(coefficients.data(), coefficients.size());
        return coefficients;
    }
    std::vector<uint64_t> icrt(std::vector<uint64_t> evaluations) const {
        icrt_in_place(evaluations.data(), evaluations.size());
        return evaluations;
    }
    static void check(int rc, const char *what) {
        if (rc != SR_OK) throw std::runtime_error(std::string(what) + ": " + sr_last_error_string());
    }

    // ---- device-resident batches: pointers are HIP device pointers, `stream` a hipStream_t (as void *: no HIP header needed here),
    //      every call is asynchronous on that stream (include/stark_rings_hip.h, "device-resident entry points") ----
    void reserve_scratch(size_t batch) const { check(sr_ctx_reserve_scratch(raw(), batch), "reserve_scratch"); }
    // the plan the library settled on (lanes: 0 = auto and not settled yet, 1 = one stream, 2 = two lanes); probe_ms / probe_elems optional
    sr_plan plan_in_use(double probe_ms[2] = nullptr, size_t *probe_elems = nullptr) const {
        sr_plan p{};
        check(sr_ctx_plan_in_use(raw(), &p, probe_ms, probe_elems), "plan_in_use");
        return p;
    }
    void elementwise_crt_dev(uint64_t *d, size_t batch, void *stream) const { check(sr_ntt_fwd_batch_dev(raw(), d, batch, stream), "elementwise_crt_dev"); }
    void elementwise_icrt_dev(uint64_t *d, size_t batch, void *stream) const { check(sr_ntt_inv_batch_dev(raw(), d, batch, stream), "elementwise_icrt_dev"); }
    void ntt_mul_dev(uint64_t *lhs, const uint64_t *rhs, size_t batch, void *stream) const {
        check(sr_pointwise_mul_batch_dev(raw(), lhs, rhs, batch, stream), "ntt_mul_dev");
    }
    void add_dev(uint64_t *lhs, const uint64_t *rhs, size_t batch, void *stream) const { check(sr_add_batch_dev(raw(), lhs, rhs, batch, stream), "add_dev"); }
    void sub_dev(uint64_t *lhs, const uint64_t *rhs, size_t batch, void *stream) const { check(sr_sub_batch_dev(raw(), lhs, rhs, batch, stream), "sub_dev"); }
    // Neg, Mul<scalar>, Add<scalar> (coeff_form.rs:270-278, 390-408, 610-700; ntt_form.rs:191-203, 373-505); scalar: host pointer to the
    // Montgomery image of the base-field element
    void neg_dev(uint64_t *d, size_t batch, void *stream) const { check(sr_neg_batch_dev(raw(), d, batch, stream), "neg_dev"); }
    void mul_elem_dev(uint64_t *d, const uint64_t *d_elem, size_t batch, void *stream) const { check(sr_mul_elem_batch_dev(raw(), d, d_elem, batch, stream), "mul_elem_dev"); }
    // Sum / Product over a device-resident slice (coeff_form.rs:507-537, ntt_form.rs:640-670); out = one ring element outside the slice
    void sum_dev(uint64_t *out, const uint64_t *in, size_t n, void *stream) const { check(sr_sum_batch_dev(raw(), out, in, n, stream), "sum_dev"); }
    void product_dev(uint64_t *out, const uint64_t *in_ntt, size_t n, void *stream) const { check(sr_product_batch_dev(raw(), out, in_ntt, n, stream), "product_dev"); }
    void scale_dev(uint64_t *d, const uint64_t *scalar, size_t batch, void *stream) const { check(sr_scale_batch_dev(raw(), d, scalar, batch, stream), "scale_dev"); }
    void add_scalar_dev(uint64_t *d, const uint64_t *scalar, bool ntt_form, size_t batch, void *stream) const {
        check(sr_add_scalar_batch_dev(raw(), d, scalar, ntt_form ? 1 : 0, batch, stream), "add_scalar_dev");
    }
    // out = a * b (RqPoly * &RqPoly); a, b only read; out may alias a
    void mul_dev(uint64_t *out, const uint64_t *a, const uint64_t *b, size_t batch, void *stream) const {
        check(sr_ring_mul_batch_dev(raw(), out, a, b, batch, stream), "mul_dev");
    }
    void mul_ntt_rhs_dev(uint64_t *out, const uint64_t *a, const uint64_t *b_ntt, size_t batch, void *stream) const {
        check(sr_ring_mul_ntt_rhs_batch_dev(raw(), out, a, b_ntt, batch, stream), "mul_ntt_rhs_dev");
    }
    void rot_dev(uint64_t *out, const uint64_t *in, size_t batch, void *stream) const { check(sr_rot_batch_dev(raw(), out, in, batch, stream), "rot_dev"); }
    void matvec_dev(uint64_t *y, const uint64_t *m, const uint64_t *v, size_t nrows, size_t ncols, void *stream) const {
        check(sr_matvec_ntt_dev(raw(), y, m, v, nrows, ncols, stream), "matvec_dev");
    }
    void matmul_dev(uint64_t *y, const uint64_t *a, const uint64_t *b, size_t n, size_t m, size_t p, void *stream) const {
        check(sr_matmul_ntt_dev(raw(), y, a, b, n, m, p, stream), "matmul_dev");
    }
    void gadget_decompose_dev(uint64_t *out, const uint64_t *in, unsigned __int128 b, size_t padding_size, size_t batch, void *stream) const {
        check(sr_decompose_balanced_batch_wide_dev(raw(), out, in, (uint64_t)b, (uint64_t)(b >> 64), padding_size, batch, stream), "gadget_decompose_dev");
    }
    void gadget_recompose_dev(uint64_t *out, const uint64_t *in, unsigned __int128 b, size_t padding_size, size_t batch_out, void *stream) const {
        check(sr_recompose_batch_wide_dev(raw(), out, in, (uint64_t)b, (uint64_t)(b >> 64), padding_size, batch_out, stream), "gadget_recompose_dev");
    }
    // norms of n_coeffs device-resident coefficients, one record per `group` of them (include/stark_rings_hip.h, sr_norm_batch_dev);
    // norm_plan: {words per group, workspace words, launches}
    struct NormPlan {
        size_t words_per_group, work_words;
        int launches;
    };
    NormPlan norm_plan(size_t n_coeffs, size_t group, int which) const {
        NormPlan p{};
        check(sr_norm_plan(ring_, n_coeffs, group, which, &p.words_per_group, &p.work_words, &p.launches), "sr_norm_plan");
        return p;
    }
    void norm_dev(uint64_t *out, const uint64_t *coeffs, size_t n_coeffs, size_t group, int which, uint64_t *work, size_t work_words,
                  void *stream) const {
        check(sr_norm_batch_dev(raw(), out, coeffs, n_coeffs, group, which, work, work_words, stream), "norm_dev");
    }
    // sparse multilinear extensions on device pointers (include/stark_rings_hip.h: sr_eq_table_dev, sr_smle_plan, sr_smle_fix_variables_dev);
    // smle_plan: {workspace elements, stream operations}; log2_degree as given to the constructor (0 for the reference's own rings)
    void eq_table_dev(uint64_t *out, const uint64_t *point, size_t n_vars, void *stream) const {
        check(sr_eq_table_dev(raw(), out, point, n_vars, stream), "eq_table_dev");
    }
    // sum-check rounds with a per-pair weight on device pointers (include/stark_rings_hip.h: sr_vpoly_wround_plan, sr_vpoly_wround_evals_dev,
    // sr_vpoly_wround_fold_plan, sr_vpoly_wround_fold_evals_dev): {work_elems, launches} of the two plans, and the two device calls
    std::pair<size_t, int> vpoly_wround_plan(int log2_degree, size_t num_vars, int n_tables, int n_terms, int degree, int order) const {
        size_t work = 0;
        int launches = 0;
        check(sr_vpoly_wround_plan((int)ring_, log2_degree, num_vars, n_tables, n_terms, degree, order, &work, &launches), "vpoly_wround_plan");
        return {work, launches};
    }
    std::pair<size_t, int> vpoly_wround_fold_plan(int log2_degree, size_t num_vars, int n_tables, int n_terms, int degree, int order) const {
        size_t work = 0;
        int launches = 0;
        check(sr_vpoly_wround_fold_plan((int)ring_, log2_degree, num_vars, n_tables, n_terms, degree, order, &work, &launches),
              "vpoly_wround_fold_plan");
        return {work, launches};
    }
    void vpoly_wround_evals_dev(uint64_t *d_out, const uint64_t *d_weights, const uint64_t *const *d_tables, const size_t *n_evals, int n_tables,
                                const sr_vpoly_term *terms, int n_terms, const uint64_t *d_coeffs, size_t num_vars, int order, uint64_t *d_work,
                                size_t work_elems, void *stream) const {
        check(sr_vpoly_wround_evals_dev(raw(), d_out, d_weights, d_tables, n_evals, n_tables, terms, n_terms, d_coeffs, num_vars, order, d_work,
                                        work_elems, stream),
              "vpoly_wround_evals_dev");
    }
    void vpoly_wround_fold_evals_dev(uint64_t *d_out, uint64_t *const *d_out_tables, size_t *n_evals_out, const uint64_t *d_weights,
                                     const uint64_t *const *d_tables, const size_t *n_evals, int n_tables, const sr_vpoly_term *terms, int n_terms,
                                     const uint64_t *d_coeffs, size_t num_vars, const uint64_t *d_r, int order, uint64_t *d_work, size_t work_elems,
                                     void *stream) const {
        check(sr_vpoly_wround_fold_evals_dev(raw(), d_out, d_out_tables, n_evals_out, d_weights, d_tables, n_evals, n_tables, terms, n_terms,
                                             d_coeffs, num_vars, d_r, order, d_work, work_elems, stream),
              "vpoly_wround_fold_evals_dev");
    }
    // the same rounds with integer columns as factors (include/stark_rings_hip.h: sr_vpoly_iwround_plan, sr_vpoly_iwround_evals_dev,
    // sr_vpoly_iwround_fold_evals_dev): slots 0 .. n_tables - 1 of a term are the tables, the next n_index the columns; fold: the plan
    // of the fused call; d_out_tables and n_evals_out hold n_tables + n_index entries
    std::pair<size_t, int> vpoly_iwround_plan(int log2_degree, size_t num_vars, int n_tables, int n_index, int n_terms, int degree, int order,
                                              bool fold) const {
        size_t work = 0;
        int launches = 0;
        check(sr_vpoly_iwround_plan((int)ring_, log2_degree, num_vars, n_tables, n_index, n_terms, degree, order, fold ? 1 : 0, &work, &launches),
              "vpoly_iwround_plan");
        return {work, launches};
    }
    void vpoly_iwround_evals_dev(uint64_t *d_out, const uint64_t *d_weights, const uint64_t *const *d_tables, const size_t *n_evals, int n_tables,
                                 const sr_index_column *columns, int n_index, const sr_vpoly_term *terms, int n_terms, const uint64_t *d_coeffs,
                                 size_t num_vars, int order, uint64_t *d_work, size_t work_elems, void *stream) const {
        check(sr_vpoly_iwround_evals_dev(raw(), d_out, d_weights, d_tables, n_evals, n_tables, columns, n_index, terms, n_terms, d_coeffs, num_vars,
                                         order, d_work, work_elems, stream),
              "vpoly_iwround_evals_dev");
    }
    void vpoly_iwround_fold_evals_dev(uint64_t *d_out, uint64_t *const *d_out_tables, size_t *n_evals_out, const uint64_t *d_weights,
                                      const uint64_t *const *d_tables, const size_t *n_evals, int n_tables, const sr_index_column *columns,
                                      int n_index, const sr_vpoly_term *terms, int n_terms, const uint64_t *d_coeffs, size_t num_vars,
                                      const uint64_t *d_r, int order, uint64_t *d_work, size_t work_elems, void *stream) const {
        check(sr_vpoly_iwround_fold_evals_dev(raw(), d_out, d_out_tables, n_evals_out, d_weights, d_tables, n_evals, n_tables, columns, n_index,
                                              terms, n_terms, d_coeffs, num_vars, d_r, order, d_work, work_elems, stream),
              "vpoly_iwround_fold_evals_dev");
    }
    // range-check (norm-check) rounds (include/stark_rings_hip.h: sr_range_wround_plan, sr_range_wround_evals_dev, sr_range_wround_evals):
    // {work_elems, launches} of the plan, the device call and the host-pointer form (2 bound elements into `out`)
    std::pair<size_t, int> range_wround_plan(int log2_degree, size_t num_vars, int n_tables, int bound, int order) const {
        size_t work = 0;
        int launches = 0;
        check(sr_range_wround_plan((int)ring_, log2_degree, num_vars, n_tables, bound, order, &work, &launches), "range_wround_plan");
        return {work, launches};
    }
    void range_wround_evals_dev(uint64_t *d_out, const uint64_t *d_weights, const uint64_t *const *d_tables, const size_t *n_evals, int n_tables,
                                int bound, const uint64_t *d_coeffs, size_t num_vars, int order, uint64_t *d_work, size_t work_elems,
                                void *stream) const {
        check(sr_range_wround_evals_dev(raw(), d_out, d_weights, d_tables, n_evals, n_tables, bound, d_coeffs, num_vars, order, d_work, work_elems,
                                        stream),
              "range_wround_evals_dev");
    }
    void range_wround_evals(uint64_t *out, const uint64_t *weights, const uint64_t *const *tables, const size_t *n_evals, int n_tables, int bound,
                            const uint64_t *coeffs, size_t num_vars, int order) const {
        check(sr_range_wround_evals(raw(), out, weights, tables, n_evals, n_tables, bound, coeffs, num_vars, order), "range_wround_evals");
    }
    std::pair<size_t, int> smle_plan(int log2_degree, size_t nnz, size_t n_out, size_t n_fixed) const {
        size_t work = 0;
        int launches = 0;
        check(sr_smle_plan(ring_, log2_degree, nnz, n_out, n_fixed, &work, &launches), "sr_smle_plan");
        return {work, launches};
    }
    void smle_fix_variables_dev(uint64_t *out_vals, const uint64_t *vals, const uint64_t *idx, size_t nnz, const uint64_t *seg_ptr, size_t n_out,
                                const uint64_t *point, size_t n_fixed, uint64_t *work, size_t work_elems, void *stream) const {
        check(sr_smle_fix_variables_dev(raw(), out_vals, vals, idx, nnz, seg_ptr, n_out, point, n_fixed, work, work_elems, stream), "smle_fix_variables_dev");
    }
    // packed-u32 BabyBear boundary (the low half of the reference's Fp64 limb, babybear/mod.rs:18-26)
    void pack32_dev(uint32_t *out, const uint64_t *in, size_t batch, void *stream) const { check(sr_pack32_batch_dev(raw(), out, in, batch, stream), "pack32_dev"); }
    void unpack32_dev(uint64_t *out, const uint32_t *in, size_t batch, void *stream) const { check(sr_unpack32_batch_dev(raw(), out, in, batch, stream), "unpack32_dev"); }
    void elementwise_crt_packed32_dev(uint32_t *d, size_t batch, void *stream) const { check(sr_ntt_fwd_packed32_batch_dev(raw(), d, batch, stream), "crt_packed32"); }
    void elementwise_icrt_packed32_dev(uint32_t *d, size_t batch, void *stream) const { check(sr_ntt_inv_packed32_batch_dev(raw(), d, batch, stream), "icrt_packed32"); }
    void mul_packed32_dev(uint32_t *out, const uint32_t *a, const uint32_t *b, size_t batch, void *stream) const {
        check(sr_ring_mul_packed32_batch_dev(raw(), out, a, b, batch, stream), "mul_packed32_dev");
    }

private:
    sr_ring ring_;
    std::shared_ptr<sr_ctx> ctx_;
    size_t degree_ = 0;
    int limbs_ = 1;
};

class RqNTTVec;

// Vec<RqPoly>: `len` ring elements in coefficient form, flat element-major storage (flatten.rs layout)
class RqPolyVec {
public:
    RqPolyVec(CyclotomicConfig cfg, std::vector<uint64_t> words) : cfg_(std::move(cfg)), w_(std::move(words)) {
        if (w_.size() % cfg_.words_per_elem()) throw std::length_error("Wrong length");  // coeff_form.rs:39
    }
    size_t len() const { return w_.size() / cfg_.words_per_elem(); }
    const std::vector<uint64_t> &words() const { return w_; }
    const CyclotomicConfig &config() const { return cfg_; }
    uint64_t *element(size_t i) { return w_.data() + i * cfg_.words_per_elem(); }
    bool operator==(const RqPolyVec &o) const { return w_ == o.w_; }

    RqNTTVec elementwise_crt() &&;                               // crt.rs:10-25
    RqPolyVec &operator*=(const RqPolyVec &rhs) {                // coeff_form.rs:250-258 per element
        if (rhs.w_.size() != w_.size()) throw std::length_error("operand lengths differ");
        CyclotomicConfig::check(sr_ring_mul_batch(cfg_.raw(), w_.data(), w_.data(), rhs.w_.data(), len()), "RqPoly *");
        return *this;
    }
    // *this = icrt(crt(*this) (.) rhs_ntt words): the constant-operand product (rhs kept in NTT form); defined below RqNTTVec
    RqPolyVec &mul_assign_ntt_rhs(const std::vector<uint64_t> &rhs_ntt_words) {
        if (rhs_ntt_words.size() != w_.size()) throw std::length_error("operand lengths differ");
        CyclotomicConfig::check(sr_ring_mul_ntt_rhs_batch(cfg_.raw(), w_.data(), w_.data(), rhs_ntt_words.data(), len()),
                                "RqPoly * RqNTT");
        return *this;
    }
    friend RqPolyVec operator*(RqPolyVec lhs, const RqPolyVec &rhs) {
        lhs *= rhs;
        return lhs;
    }
    RqPolyVec &operator+=(const RqPolyVec &rhs) {                // coeff_form.rs Add<&Self>
        if (rhs.w_.size() != w_.size()) throw std::length_error("operand lengths differ");
        CyclotomicConfig::check(sr_add_batch(cfg_.raw(), w_.data(), rhs.w_.data(), len()), "RqPoly +=");
        return *this;
    }
    RqPolyVec &operator-=(const RqPolyVec &rhs) {
        if (rhs.w_.size() != w_.size()) throw std::length_error("operand lengths differ");
        CyclotomicConfig::check(sr_sub_batch(cfg_.raw(), w_.data(), rhs.w_.data(), len()), "RqPoly -=");
        return *this;
    }
    RqPolyVec operator-() && {                                   // coeff_form.rs:270-278
        CyclotomicConfig::check(sr_neg_batch(cfg_.raw(), w_.data(), len()), "-RqPoly");
        return std::move(*this);
    }
    // scalar: the Montgomery image of one base-field element (limbs() words) -- Mul<Fp>, Mul<u64> ... (coeff_form.rs:390-408, 610-650)
    RqPolyVec &operator*=(const std::vector<uint64_t> &scalar) {
        if (scalar.size() != (size_t)cfg_.limbs()) throw std::length_error("scalar: wrong number of limbs");
        CyclotomicConfig::check(sr_scale_batch(cfg_.raw(), w_.data(), scalar.data(), len()), "RqPoly *= scalar");
        return *this;
    }
    RqPolyVec &operator+=(const std::vector<uint64_t> &scalar) {  // coefficient 0 of every element (coeff_form.rs:652-700)
        if (scalar.size() != (size_t)cfg_.limbs()) throw std::length_error("scalar: wrong number of limbs");
        CyclotomicConfig::check(sr_add_scalar_batch(cfg_.raw(), w_.data(), scalar.data(), 0, len()), "RqPoly += scalar");
        return *this;
    }
    // impl Sum<&Self> (coeff_form.rs:507-521): `iter.fold(Self::zero(), |acc, x| acc + x)` -> a vector of ONE element (zero() when empty)
    RqPolyVec sum() const {
        std::vector<uint64_t> out(cfg_.words_per_elem());
        const uint64_t dummy = 0;
        CyclotomicConfig::check(sr_sum_batch(cfg_.raw(), out.data(), w_.empty() ? &dummy : w_.data(), len()), "RqPoly sum");
        return RqPolyVec(cfg_, std::move(out));
    }
    RqPolyVec product() const;  // impl Product<&Self> (coeff_form.rs:523-537); defined below RqNTTVec
    // WithLinfNorm / WithL2Norm of the flattened coefficients (traits.rs:6-36): the integer as little-endian u64 words -- limbs() words
    // for linf, 3 (one-limb fields) or 9 (Stark) for the squared l2 norm.  linf_norm of an empty vector throws (the reference panics).
    std::vector<uint64_t> linf_norm() const { return norm(SR_NORM_LINF, w_.size() / cfg_.limbs()); }
    std::vector<uint64_t> l2_norm_squared() const { return norm(SR_NORM_L2SQ, w_.size() / cfg_.limbs()); }
    // the same per ring element: len() records one after the other
    std::vector<uint64_t> linf_norm_per_element() const { return norm(SR_NORM_LINF, cfg_.dimension()); }
    std::vector<uint64_t> l2_norm_squared_per_element() const { return norm(SR_NORM_L2SQ, cfg_.dimension()); }
    std::vector<uint64_t> into_words() && { return std::move(w_); }

private:
    std::vector<uint64_t> norm(int which, size_t group) const {
        const size_t n = w_.size() / cfg_.limbs();
        if (group == 0) group = 1;  // the empty vector as one slice
        const CyclotomicConfig::NormPlan p = cfg_.norm_plan(n, group, which);
        std::vector<uint64_t> out((n ? n / group : 1) * p.words_per_group);
        const uint64_t dummy = 0;
        CyclotomicConfig::check(sr_norm_batch(cfg_.raw(), out.data(), w_.empty() ? &dummy : w_.data(), n, group, which), "RqPoly norm");
        return out;
    }
    CyclotomicConfig cfg_;
    std::vector<uint64_t> w_;
};

// Vec<RqNTT>: the same bytes reinterpreted as CRT slots (crt.rs:61 transmute)
class RqNTTVec {
public:
    RqNTTVec(CyclotomicConfig cfg, std::vector<uint64_t> words) : cfg_(std::move(cfg)), w_(std::move(words)) {
        if (w_.size() % cfg_.words_per_elem()) throw std::length_error("Should be of correct length");  // ntt_form.rs:703
    }
    size_t len() const { return w_.size() / cfg_.words_per_elem(); }
    const std::vector<uint64_t> &words() const { return w_; }
    const CyclotomicConfig &config() const { return cfg_; }
    bool operator==(const RqNTTVec &o) const { return w_ == o.w_; }

    RqPolyVec elementwise_icrt() && {                            // crt.rs:34-49
        CyclotomicConfig::check(sr_ntt_inv_batch(cfg_.raw(), w_.data(), len()), "elementwise_icrt");
        return RqPolyVec(cfg_, std::move(w_));
    }
    RqNTTVec &operator*=(const RqNTTVec &rhs) {                  // ntt_form.rs:213-225
        if (rhs.w_.size() != w_.size()) throw std::length_error("operand lengths differ");
        CyclotomicConfig::check(sr_pointwise_mul_batch(cfg_.raw(), w_.data(), rhs.w_.data(), len()), "RqNTT *=");
        return *this;
    }
    friend RqNTTVec operator*(RqNTTVec lhs, const RqNTTVec &rhs) {
        lhs *= rhs;
        return lhs;
    }
    RqNTTVec &operator+=(const RqNTTVec &rhs) {                  // ntt_form.rs:227-285
        if (rhs.w_.size() != w_.size()) throw std::length_error("operand lengths differ");
        CyclotomicConfig::check(sr_add_batch(cfg_.raw(), w_.data(), rhs.w_.data(), len()), "RqNTT +=");
        return *this;
    }
    RqNTTVec &operator-=(const RqNTTVec &rhs) {                  // ntt_form.rs:588-638
        if (rhs.w_.size() != w_.size()) throw std::length_error("operand lengths differ");
        CyclotomicConfig::check(sr_sub_batch(cfg_.raw(), w_.data(), rhs.w_.data(), len()), "RqNTT -=");
        return *this;
    }
    RqNTTVec operator-() && {                                    // ntt_form.rs:191-203
        CyclotomicConfig::check(sr_neg_batch(cfg_.raw(), w_.data(), len()), "-RqNTT");
        return std::move(*this);
    }
    RqNTTVec &operator*=(const std::vector<uint64_t> &scalar) {  // `*lhs *= BaseCRTField::from(rhs)` (ntt_form.rs:373-425)
        if (scalar.size() != (size_t)cfg_.limbs()) throw std::length_error("scalar: wrong number of limbs");
        CyclotomicConfig::check(sr_scale_batch(cfg_.raw(), w_.data(), scalar.data(), len()), "RqNTT *= scalar");
        return *this;
    }
    // every element of the vector times ONE ring element r (r.len() == 1), slot-wise: the loop body of `Matrix<R> *= &R`
    RqNTTVec &mul_assign_elem(const RqNTTVec &r) {
        if (r.len() != 1) throw std::length_error("mul_assign_elem: the multiplier is not one ring element");
        CyclotomicConfig::check(sr_mul_elem_batch(cfg_.raw(), w_.empty() ? dummy_word() : w_.data(), r.w_.data(), len()), "RqNTT[] *= &RqNTT");
        return *this;
    }
    RqNTTVec &operator+=(const std::vector<uint64_t> &scalar) {  // component 0 of every slot (ntt_form.rs:427-505)
        if (scalar.size() != (size_t)cfg_.limbs()) throw std::length_error("scalar: wrong number of limbs");
        CyclotomicConfig::check(sr_add_scalar_batch(cfg_.raw(), w_.data(), scalar.data(), 1, len()), "RqNTT += scalar");
        return *this;
    }
    // impl Sum<&Self> / Product<&Self> (ntt_form.rs:640-670): folds over the slice -> a vector of ONE element (zero() / one() when empty)
    RqNTTVec sum() const {
        std::vector<uint64_t> out(cfg_.words_per_elem());
        CyclotomicConfig::check(sr_sum_batch(cfg_.raw(), out.data(), w_.empty() ? dummy_word() : w_.data(), len()), "RqNTT sum");
        return RqNTTVec(cfg_, std::move(out));
    }
    RqNTTVec product() const {
        std::vector<uint64_t> out(cfg_.words_per_elem());
        CyclotomicConfig::check(sr_product_batch(cfg_.raw(), out.data(), w_.empty() ? dummy_word() : w_.data(), len()), "RqNTT product");
        return RqNTTVec(cfg_, std::move(out));
    }
    // Field::inverse / ark_ff::batch_inversion on every slot of every element (sr_inverse_batch): 1 / self[e], and self[e] / den[e].  A
    // zero slot gives zero -- batch_inversion leaves zeros in place -- and is counted: inverse_zero_count() == 0 afterwards is the
    // `Some` of Field::inverse for every element.
    RqNTTVec inverse() const { return quotient(nullptr, *this); }
    RqNTTVec divide(const RqNTTVec &den) const {
        if (den.w_.size() != w_.size()) throw std::length_error("operand lengths differ");
        return quotient(this, den);
    }
    // sr_inverse_zero_count: the zero slots the calls above met on this configuration's context since the last read; clears the count
    unsigned long long inverse_zero_count() const {
        unsigned long long n = 0;
        CyclotomicConfig::check(sr_inverse_zero_count(cfg_.raw(), &n, nullptr), "sr_inverse_zero_count");
        return n;
    }
    std::vector<uint64_t> into_words() && { return std::move(w_); }

private:
    static RqNTTVec quotient(const RqNTTVec *num, const RqNTTVec &den) {
        std::vector<uint64_t> out(den.w_.size());
        CyclotomicConfig::check(sr_inverse_batch(den.cfg_.raw(), out.empty() ? dummy_word() : out.data(), num && !num->w_.empty() ? num->w_.data() : nullptr,
                                                 den.w_.empty() ? dummy_word() : den.w_.data(), den.len()),
                                "RqNTT inverse");
        return RqNTTVec(den.cfg_, std::move(out));
    }
    static uint64_t *dummy_word() {
        static uint64_t z = 0;
        return &z;
    }
    CyclotomicConfig cfg_;
    std::vector<uint64_t> w_;
};

// sr_lincomb_plan: {kernel launches, outputs one launch produces} of a linear combination of n_tables tables into n_outputs outputs
inline std::pair<int, int> lincomb_plan(sr_ring ring, int log2_degree, int n_tables, int n_outputs) {
    int launches = 0, per = 0;
    CyclotomicConfig::check(sr_lincomb_plan(ring, log2_degree, n_tables, n_outputs, &launches, &per), "sr_lincomb_plan");
    return {launches, per};
}
// sr_lincomb_dev on device pointers: out_m[e] = [bit K of uses[m]] coef[m][K] + sum_{k < K, bit k of uses[m]} coef[m][k] * T_k[e] for
// e < n, the composition of dense.rs's AddAssign<(R, &Self)> (:288-317), MulAssign<R> (:370-374) and Add<R> (:386-395) in one pass.
// d_outs / d_tables / uses are host arrays; n_evals may be null (every table full); allocates nothing.  Throws where the C call refuses.
inline void lincomb_dev(const CyclotomicConfig &cfg, uint64_t *const *d_outs, int n_outputs, const uint64_t *const *d_tables, const size_t *n_evals,
                        int n_tables, const uint64_t *d_coef, const uint32_t *uses, size_t n, void *stream = nullptr) {
    CyclotomicConfig::check(sr_lincomb_dev(cfg.raw(), d_outs, n_outputs, d_tables, n_evals, n_tables, d_coef, uses, n, stream), "sr_lincomb_dev");
}
// sr_lincomb on host words: tables[k] holds its stored elements (at most n, the rest of the table is zero), coef the uses.size() rows of
// tables.size() + 1 elements (the constant last); returns the uses.size() outputs of n elements each
inline std::vector<std::vector<uint64_t>> lincomb(const CyclotomicConfig &cfg, const std::vector<const std::vector<uint64_t> *> &tables,
                                                  const std::vector<uint64_t> &coef, const std::vector<uint32_t> &uses, size_t n) {
    const size_t w = cfg.words_per_elem();
    if (tables.empty() || tables.size() > SR_LINCOMB_MAX_TABLES) throw std::length_error("lincomb: 1 .. 16 tables");
    if (uses.empty() || uses.size() > SR_LINCOMB_MAX_OUTPUTS) throw std::length_error("lincomb: 1 .. 4 outputs");
    if (coef.size() != uses.size() * (tables.size() + 1) * w) throw std::length_error("lincomb: coef must hold n_outputs x (n_tables + 1) elements");
    std::vector<std::vector<uint64_t>> outs(uses.size(), std::vector<uint64_t>(n * w));
    const uint64_t dummy = 0;
    uint64_t sink = 0;
    std::vector<const uint64_t *> pt;
    std::vector<size_t> sizes;
    std::vector<uint64_t *> po;
    for (const std::vector<uint64_t> *t : tables) {
        if (t->size() % w) throw std::length_error("Should be of correct length");
        pt.push_back(t->empty() ? &dummy : t->data());
        sizes.push_back(t->size() / w);
    }
    for (auto &o : outs) po.push_back(o.empty() ? &sink : o.data());
    CyclotomicConfig::check(sr_lincomb(cfg.raw(), po.data(), (int)uses.size(), pt.data(), sizes.data(), (int)tables.size(), coef.data(), uses.data(), n),
                            "sr_lincomb");
    return outs;
}

// A column of integers as an input of a linear combination (sr_index_column): stored uint64_t values -- at most n, the rest of the
// column counts as 0 -- or the progression start, start + 1, .., which occupies no memory.  It enters as coef * R::from(col[e]), the
// reference's From<u64> (from_scalar(BaseRing::from(x)) in CRT/NTT form).
struct IndexColumn {
    std::vector<uint64_t> values;
    bool is_progression = false;
    uint64_t start = 0;
    static IndexColumn stored(std::vector<uint64_t> v) {
        IndexColumn c;
        c.values = std::move(v);
        return c;
    }
    static IndexColumn progression(uint64_t first) {
        IndexColumn c;
        c.is_progression = true;
        c.start = first;
        return c;
    }
};
// sr_lincomb_index_plan: {kernel launches, outputs one launch produces}
inline std::pair<int, int> lincomb_index_plan(sr_ring ring, int log2_degree, int n_tables, int n_index, int n_outputs) {
    int launches = 0, per = 0;
    CyclotomicConfig::check(sr_lincomb_index_plan(ring, log2_degree, n_tables, n_index, n_outputs, &launches, &per), "sr_lincomb_index_plan");
    return {launches, per};
}
// sr_lincomb_index_dev on device pointers (columns: a host array whose `values` are device pointers); allocates nothing
inline void lincomb_index_dev(const CyclotomicConfig &cfg, uint64_t *const *d_outs, int n_outputs, const uint64_t *const *d_tables,
                              const size_t *n_evals, int n_tables, const sr_index_column *columns, int n_index, const uint64_t *d_coef,
                              const uint32_t *uses, size_t n, void *stream = nullptr) {
    CyclotomicConfig::check(sr_lincomb_index_dev(cfg.raw(), d_outs, n_outputs, d_tables, n_evals, n_tables, columns, n_index, d_coef, uses, n, stream),
                            "sr_lincomb_index_dev");
}
// sr_lincomb_index on host words: out_m[e] = [bit K+J] coef[m][K+J] + sum_k [bit k] coef[m][k] * T_k[e] + sum_j [bit K+j] coef[m][K+j] *
// R::from(col_j[e]); coef holds uses.size() rows of tables.size() + columns.size() + 1 elements: tables, columns, the constant
inline std::vector<std::vector<uint64_t>> lincomb_index(const CyclotomicConfig &cfg, const std::vector<const std::vector<uint64_t> *> &tables,
                                                        const std::vector<IndexColumn> &columns, const std::vector<uint64_t> &coef,
                                                        const std::vector<uint32_t> &uses, size_t n) {
    const size_t w = cfg.words_per_elem(), terms = tables.size() + columns.size();
    if (tables.size() > SR_LINCOMB_MAX_TABLES || columns.size() > SR_LINCOMB_MAX_INDEX_COLUMNS || terms < 1 || terms > SR_LINCOMB_MAX_TABLES)
        throw std::length_error("lincomb_index: 0 .. 16 tables, 0 .. 8 index columns, 1 .. 16 of both together");
    if (uses.empty() || uses.size() > SR_LINCOMB_MAX_OUTPUTS) throw std::length_error("lincomb_index: 1 .. 4 outputs");
    if (coef.size() != uses.size() * (terms + 1) * w) throw std::length_error("lincomb_index: coef must hold n_outputs x (n_tables + n_index + 1) elements");
    std::vector<std::vector<uint64_t>> outs(uses.size(), std::vector<uint64_t>(n * w));
    const uint64_t dummy = 0;
    uint64_t sink = 0;
    std::vector<const uint64_t *> pt;
    std::vector<size_t> sizes;
    std::vector<uint64_t *> po;
    std::vector<sr_index_column> pc;
    for (const std::vector<uint64_t> *t : tables) {
        if (t->size() % w) throw std::length_error("Should be of correct length");
        pt.push_back(t->empty() ? &dummy : t->data());
        sizes.push_back(t->size() / w);
    }
    for (const IndexColumn &c : columns) {
        if (c.is_progression) pc.push_back(sr_index_column{nullptr, 0, c.start});
        else pc.push_back(sr_index_column{c.values.empty() ? &dummy : c.values.data(), c.values.size(), 0});
    }
    for (auto &o : outs) po.push_back(o.empty() ? &sink : o.data());
    CyclotomicConfig::check(sr_lincomb_index(cfg.raw(), po.data(), (int)uses.size(), pt.data(), sizes.data(), (int)tables.size(), pc.data(),
                                             (int)columns.size(), coef.data(), uses.data(), n),
                            "sr_lincomb_index");
    return outs;
}
// sr_index_count on host words: counts[t] = #{ i : idx[i] == t } for t < n_bins; throws on an index that is not below n_bins
inline std::vector<uint64_t> index_count(const CyclotomicConfig &cfg, const std::vector<uint64_t> &idx, size_t n_bins) {
    std::vector<uint64_t> counts(n_bins, 0);
    uint64_t sink = 0, none = 0;
    CyclotomicConfig::check(sr_index_count(cfg.raw(), n_bins ? counts.data() : &sink, idx.empty() ? &none : idx.data(), idx.size(), n_bins),
                            "sr_index_count");
    return counts;
}
// The table R::from(col[e]), e < n, as words: one call with no table, one column and the coefficient one()
inline std::vector<uint64_t> from_u64(const CyclotomicConfig &cfg, const IndexColumn &column, size_t n, const std::vector<uint64_t> &one_words) {
    if (one_words.size() != cfg.words_per_elem()) throw std::length_error("from_u64: one is one ring element");
    std::vector<uint64_t> coef(one_words);
    coef.resize(2 * one_words.size(), 0);
    return std::move(lincomb_index(cfg, {}, {column}, coef, {0x1u}, n)[0]);
}

// DenseMultilinearExtension<RqNTT> of crates/poly (src/mle/dense.rs): a table of 2^num_vars ring elements in CRT/NTT form, of which
// only the first len() are stored -- the rest is zero (dense.rs:35-54, 397-407).  Host buffers over sr_mle_fix_variables /
// sr_mul_elem_add_batch; `r * a` is the slot product of the ring.  Throws where the reference asserts.
class DenseMultilinearExtension {
public:
    DenseMultilinearExtension(CyclotomicConfig cfg, size_t num_vars, std::vector<uint64_t> evaluation_words)
        : cfg_(std::move(cfg)), nv_(num_vars), w_(std::move(evaluation_words)) {
        if (w_.size() % cfg_.words_per_elem()) throw std::length_error("Should be of correct length");
        if (nv_ >= 48 || len() > ((size_t)1 << nv_)) throw std::length_error("more evaluations than 2^num_vars");
    }
    // dense.rs:79-89: a shorter vector is padded with zeros -- implicitly here; to_evaluations() writes the padding out
    static DenseMultilinearExtension from_evaluations_vec_padded(size_t num_vars, const RqNTTVec &evaluations) {
        return DenseMultilinearExtension(evaluations.config(), num_vars, evaluations.words());
    }
    size_t num_vars() const { return nv_; }
    size_t len() const { return w_.size() / cfg_.words_per_elem(); }  // stored evaluations
    const std::vector<uint64_t> &words() const { return w_; }
    const CyclotomicConfig &config() const { return cfg_; }

    // dense.rs:171-199: partial_point[i] fixes variable i, the least significant index bit first
    void fix_variables(const RqNTTVec &partial_point) { *this = fold(partial_point, SR_MLE_LEADING); }
    DenseMultilinearExtension fixed_variables(const RqNTTVec &partial_point) const { return fold(partial_point, SR_MLE_LEADING); }  // :201-205
    // polynomials/multilinear_polynomial.rs:227-286: the LAST len variables, partial_point[j] = variable num_vars - len + j
    DenseMultilinearExtension fix_last_variables(const RqNTTVec &partial_point) const { return fold(partial_point, SR_MLE_TRAILING); }
    // dense.rs:107-113: None on a point of the wrong length
    std::optional<RqNTTVec> evaluate(const RqNTTVec &point) const {
        if (point.len() != nv_) return std::nullopt;
        return RqNTTVec(cfg_, fold(point, SR_MLE_LEADING).w_);
    }
    // dense.rs:288-317 `AddAssign<(R, &Self)>`: *this += r * other, r one ring element
    DenseMultilinearExtension &add_assign_scaled(const RqNTTVec &r, const DenseMultilinearExtension &other) {
        if (other.nv_ != nv_) throw std::length_error("trying to add two dense MLEs with different numbers of variables");  // dense.rs:291-294
        if (r.len() != 1) throw std::length_error("add_assign_scaled: r is not one ring element");
        if (w_.size() < other.w_.size()) w_.resize(other.w_.size(), 0);  // the implicit zeros of the shorter operand, written out
        if (!other.w_.empty())
            CyclotomicConfig::check(sr_mul_elem_add_batch(cfg_.raw(), w_.data(), other.w_.data(), r.words().data(), other.len()),
                                    "DenseMultilinearExtension +=");
        return *this;
    }
    // the tables 1 / self[b] and self[b] / other[b] over the stored evaluations (RqNTTVec::inverse / divide); the implicit zero tail stays
    // implicit.  Zero slots give zero and are counted (inverse_zero_count).
    DenseMultilinearExtension inverse() const { return DenseMultilinearExtension(cfg_, nv_, RqNTTVec(cfg_, w_).inverse().into_words()); }
    DenseMultilinearExtension divide(const DenseMultilinearExtension &other) const {
        if (other.nv_ != nv_ || other.w_.size() != w_.size()) throw std::length_error("divide: the operands differ in num_vars or stored length");
        return DenseMultilinearExtension(cfg_, nv_, RqNTTVec(cfg_, w_).divide(RqNTTVec(cfg_, other.w_)).into_words());
    }
    unsigned long long inverse_zero_count() const { return RqNTTVec(cfg_, {}).inverse_zero_count(); }
    // sum_k coeffs[k] * mles[k] (+ constant) from 1 .. 16 MLEs of one ring and one num_vars in one pass (sr_lincomb): MulAssign<R>,
    // AddAssign<(R, &Self)> and Add<R> of dense.rs composed.  coeffs: one ring element per MLE; constant: one ring element or null.  The
    // inputs may be truncated; the result stores the longest input's evaluations, or all 2^num_vars with a constant (which goes to every
    // evaluation, where the reference's Add<R> touches only the stored ones).
    static DenseMultilinearExtension linear_combination(const std::vector<const DenseMultilinearExtension *> &mles, const RqNTTVec &coeffs,
                                                        const RqNTTVec *constant = nullptr) {
        if (mles.empty() || mles.size() > SR_LINCOMB_MAX_TABLES) throw std::length_error("linear_combination: 1 .. 16 MLEs");
        const DenseMultilinearExtension &first = *mles[0];
        const size_t w = first.cfg_.words_per_elem();
        if (coeffs.len() != mles.size() || (constant && constant->len() != 1))
            throw std::length_error("linear_combination: one coefficient per MLE, and a constant of one ring element");
        std::vector<const std::vector<uint64_t> *> tables;
        size_t n = 0;
        for (const DenseMultilinearExtension *m : mles) {
            if (m->cfg_.raw() != first.cfg_.raw() || m->nv_ != first.nv_) throw std::length_error("linear_combination: the MLEs differ in ring or num_vars");
            tables.push_back(&m->w_);
            n = std::max(n, m->len());
        }
        if (constant) n = (size_t)1 << first.nv_;
        std::vector<uint64_t> coef(coeffs.words());
        if (constant) coef.insert(coef.end(), constant->words().begin(), constant->words().end());
        else coef.resize(coef.size() + w, 0);
        const uint32_t mask = (((uint32_t)1 << mles.size()) - 1) | (constant ? (uint32_t)1 << mles.size() : 0);
        auto outs = lincomb(first.cfg_, tables, coef, {mask}, n);
        return DenseMultilinearExtension(first.cfg_, first.nv_, std::move(outs[0]));
    }
    // linear_combination with integer columns beside the MLEs (sr_lincomb_index): sum_k coeffs[k] * mles[k] + sum_j coeffs[K + j] *
    // R::from(columns[j]) (+ constant) over num_vars variables of the ring cfg (there may be no MLE to take them from).  The result
    // stores the longest input (a progression is as long as the table), or all 2^num_vars with a constant.
    static DenseMultilinearExtension linear_combination_indexed(const CyclotomicConfig &cfg, size_t num_vars,
                                                                const std::vector<const DenseMultilinearExtension *> &mles,
                                                                const std::vector<IndexColumn> &columns, const RqNTTVec &coeffs,
                                                                const RqNTTVec *constant = nullptr) {
        const size_t w = cfg.words_per_elem(), terms = mles.size() + columns.size();
        if (num_vars >= 48) throw std::length_error("linear_combination_indexed: num_vars must be below 48");
        if (coeffs.len() != terms || (constant && constant->len() != 1))
            throw std::length_error("linear_combination_indexed: one coefficient per MLE and column, and a constant of one ring element");
        std::vector<const std::vector<uint64_t> *> tables;
        size_t n = 0;
        for (const DenseMultilinearExtension *m : mles) {
            if (m->cfg_.raw() != cfg.raw() || m->nv_ != num_vars) throw std::length_error("linear_combination_indexed: the MLEs differ in ring or num_vars");
            tables.push_back(&m->w_);
            n = std::max(n, m->len());
        }
        for (const IndexColumn &c : columns) {
            if (!c.is_progression && c.values.size() > ((size_t)1 << num_vars)) throw std::length_error("linear_combination_indexed: more values than 2^num_vars");
            n = std::max(n, c.is_progression ? (size_t)1 << num_vars : c.values.size());
        }
        if (constant) n = (size_t)1 << num_vars;
        std::vector<uint64_t> coef(coeffs.words());
        if (constant) coef.insert(coef.end(), constant->words().begin(), constant->words().end());
        else coef.resize(coef.size() + w, 0);
        const uint32_t mask = (((uint32_t)1 << terms) - 1) | (constant ? (uint32_t)1 << terms : 0);
        auto outs = lincomb_index(cfg, tables, columns, coef, {mask}, n);
        return DenseMultilinearExtension(cfg, num_vars, std::move(outs[0]));
    }
    RqNTTVec to_evaluations() const {  // all 2^num_vars elements
        std::vector<uint64_t> all(w_);
        all.resize(cfg_.words_per_elem() << nv_, 0);
        return RqNTTVec(cfg_, std::move(all));
    }
    // The prover's message of one sum-check round over the product of `tables` (1 .. 4 MLEs of one ring and one num_vars >= 1; the
    // same MLE may appear twice): the d + 1 elements p(t) = sum_b prod_j f_j(t, b), t = 0 .. d, the variable being the one
    // fix_variables (SR_MLE_LEADING) or fix_last_variables (SR_MLE_TRAILING) fixes next.  Throws where sr_mle_round_evals refuses.
    static RqNTTVec round_evals(const std::vector<const DenseMultilinearExtension *> &tables, int order = SR_MLE_LEADING) {
        if (order != SR_MLE_LEADING && order != SR_MLE_TRAILING) throw std::invalid_argument("round_evals: unknown order");
        return round(tables, order);
    }
    // sum_b prod_j f_j[b] over the hypercube: the claimed sum of a sum-check (the `sum` of random_mle_list,
    // polynomials/multilinear_polynomial.rs:19-49), one ring element
    static RqNTTVec product_sum(const std::vector<const DenseMultilinearExtension *> &tables) { return round(tables, SR_MLE_ROUND_SUM); }
    // One prover round in one pass over the tables (sr_mle_round_fold_evals): every MLE of `tables` (1 .. 4 of one ring and one
    // num_vars >= 2) with its next variable fixed at the ring element r, and the message of the round that follows over those folded
    // tables: {message, folded tables} -- what fixed_variables / fix_last_variables of every table followed by round_evals returns.
    static std::pair<RqNTTVec, std::vector<DenseMultilinearExtension>> fold_round_evals(const std::vector<const DenseMultilinearExtension *> &tables,
                                                                                        const RqNTTVec &r, int order = SR_MLE_LEADING) {
        if (order != SR_MLE_LEADING && order != SR_MLE_TRAILING) throw std::invalid_argument("fold_round_evals: unknown order");
        if (tables.empty() || tables.size() > SR_MLE_ROUND_MAX_TABLES) throw std::length_error("fold_round_evals: 1 .. 4 tables");
        if (r.len() != 1) throw std::length_error("fold_round_evals: r is not one ring element");
        const DenseMultilinearExtension &first = *tables[0];
        if (first.nv_ < 2) throw std::length_error("fold_round_evals: num_vars >= 2");
        const size_t w = first.cfg_.words_per_elem();
        std::vector<const uint64_t *> ptrs;
        std::vector<size_t> sizes;
        std::vector<std::vector<uint64_t>> folded;
        std::vector<uint64_t *> optrs;
        for (const DenseMultilinearExtension *t : tables) {
            if (t->cfg_.raw() != first.cfg_.raw() || t->nv_ != first.nv_)
                throw std::length_error("fold_round_evals: the tables differ in ring or num_vars");
            ptrs.push_back(t->w_.empty() ? nullptr : t->w_.data());
            sizes.push_back(t->len());
            folded.emplace_back(t->w_.size());  // never shorter than the folded table
        }
        for (auto &f : folded) optrs.push_back(f.empty() ? nullptr : f.data());
        std::vector<size_t> n_out(tables.size());
        std::vector<uint64_t> out(w * (tables.size() + 1));
        CyclotomicConfig::check(sr_mle_round_fold_evals(first.cfg_.raw(), out.data(), optrs.data(), n_out.data(), ptrs.data(), sizes.data(),
                                                        (int)tables.size(), first.nv_, r.words().data(), order),
                                "sr_mle_round_fold_evals");
        std::vector<DenseMultilinearExtension> g;
        for (size_t j = 0; j < tables.size(); j++) {
            folded[j].resize(n_out[j] * w);
            g.emplace_back(first.cfg_, first.nv_ - 1, std::move(folded[j]));
        }
        return {RqNTTVec(first.cfg_, std::move(out)), std::move(g)};
    }
    // sr_mle_plan of a fold of n_fixed of this table's variables: {workspace elements, kernel launches} of the device form
    std::pair<size_t, int> plan(size_t n_fixed, int order, int log2_degree) const {
        size_t work = 0;
        int launches = 0;
        CyclotomicConfig::check(sr_mle_plan(cfg_.ring(), log2_degree, nv_, n_fixed, order, &work, &launches), "sr_mle_plan");
        return {work, launches};
    }

private:
    static RqNTTVec round(const std::vector<const DenseMultilinearExtension *> &tables, int mode) {
        if (tables.empty() || tables.size() > SR_MLE_ROUND_MAX_TABLES) throw std::length_error("round_evals: 1 .. 4 tables");
        const DenseMultilinearExtension &first = *tables[0];
        std::vector<const uint64_t *> ptrs;
        std::vector<size_t> sizes;
        for (const DenseMultilinearExtension *t : tables) {
            if (t->cfg_.raw() != first.cfg_.raw() || t->nv_ != first.nv_) throw std::length_error("round_evals: the tables differ in ring or num_vars");
            ptrs.push_back(t->w_.empty() ? nullptr : t->w_.data());
            sizes.push_back(t->len());
        }
        std::vector<uint64_t> out(first.cfg_.words_per_elem() * (mode == SR_MLE_ROUND_SUM ? 1 : tables.size() + 1));
        CyclotomicConfig::check(sr_mle_round_evals(first.cfg_.raw(), out.data(), ptrs.data(), sizes.data(), (int)tables.size(), first.nv_, mode),
                                "sr_mle_round_evals");
        return RqNTTVec(first.cfg_, std::move(out));
    }
    DenseMultilinearExtension fold(const RqNTTVec &point, int order) const {
        if (point.len() > nv_) throw std::length_error("too many partial points");  // dense.rs:172-175
        std::vector<uint64_t> out(cfg_.words_per_elem() << (nv_ - point.len()));
        const uint64_t dummy = 0;
        CyclotomicConfig::check(sr_mle_fix_variables(cfg_.raw(), out.data(), w_.empty() ? &dummy : w_.data(), len(), nv_,
                                                     point.len() ? point.words().data() : &dummy, point.len(), order),
                                "sr_mle_fix_variables");
        return DenseMultilinearExtension(cfg_, nv_ - point.len(), std::move(out));
    }
    CyclotomicConfig cfg_;
    size_t nv_;
    std::vector<uint64_t> w_;
};

// precompute_eq (crates/poly mle/sparse.rs:381-394): the 2^len eq(point, .) elements, bit 0 of the index <-> point[0]
inline RqNTTVec eq_table(const RqNTTVec &point) {
    const CyclotomicConfig &cfg = point.config();
    if (point.len() >= 48) throw std::length_error("eq_table: too many variables");
    std::vector<uint64_t> out(cfg.words_per_elem() << point.len());
    const uint64_t dummy = 0;
    CyclotomicConfig::check(sr_eq_table(cfg.raw(), out.data(), point.len() ? point.words().data() : &dummy, point.len()), "sr_eq_table");
    return RqNTTVec(cfg, std::move(out));
}

// Every layer of the binary product tree over a table of ring elements in CRT/NTT form (sr_prod_tree): the circuit of the
// division-free, layered grand-product argument.  Layer 0 is the 2^num_vars leaves (those beyond the stored ones are one()), layer k
// has 2^(num_vars - k) elements, the root is layer num_vars.  SR_MLE_TRAILING: L_k[i] = L_{k-1}[i] * L_{k-1}[i + half], so the two
// operands of a layer are the lower and upper halves of the layer below; SR_MLE_LEADING: L_k[i] = L_{k-1}[2i] * L_{k-1}[2i+1].
// Host buffers; throws where the Python class raises.
class ProductTree {
public:
    ProductTree(CyclotomicConfig cfg, std::vector<uint64_t> leaf_words, size_t num_vars, int order = SR_MLE_TRAILING)
        : cfg_(std::move(cfg)), num_vars_(num_vars), order_(order), leaves_(std::move(leaf_words)) {
        if (order != SR_MLE_LEADING && order != SR_MLE_TRAILING) throw std::invalid_argument("ProductTree: unknown order");
        if (leaves_.size() % cfg_.words_per_elem()) throw std::length_error("Should be of correct length");
        if (num_vars_ >= 48 || n_leaves() > ((size_t)1 << num_vars_)) throw std::length_error("ProductTree: more leaves than 2^num_vars");
        layers_.resize(cfg_.words_per_elem() * (((size_t)1 << num_vars_) - 1));
        const uint64_t dummy = 0;
        CyclotomicConfig::check(sr_prod_tree(cfg_.raw(), layers_.empty() ? nullptr : layers_.data(), leaves_.empty() ? &dummy : leaves_.data(),
                                             n_leaves(), num_vars_, order_),
                                "sr_prod_tree");
    }
    size_t num_vars() const { return num_vars_; }
    size_t n_leaves() const { return leaves_.size() / cfg_.words_per_elem(); }  // stored leaves
    int order() const { return order_; }
    const std::vector<uint64_t> &layer_words() const { return layers_; }  // layers 1 .. num_vars, one behind the other
    // element offset of layer k (1 <= k <= num_vars) in layer_words(): layer 1 first, the root last
    size_t layer_offset(size_t k) const {
        if (k < 1 || k > num_vars_) throw std::out_of_range("ProductTree: layer index out of range");
        return ((size_t)1 << num_vars_) - ((size_t)1 << (num_vars_ - k + 1));
    }
    // layer k as an MLE in num_vars - k variables; k = 0 gives the leaves (every leaf must be stored: an MLE's missing tail is zero)
    DenseMultilinearExtension layer(size_t k) const {
        if (k > num_vars_) throw std::out_of_range("ProductTree: layer index out of range");
        return DenseMultilinearExtension(cfg_, num_vars_ - k, table(k));
    }
    // the product of all leaves, one ring element
    RqNTTVec root() const {
        if (num_vars_ == 0 && leaves_.empty()) throw std::length_error("ProductTree: a tree of no variables and no stored leaf holds no element");
        return RqNTTVec(cfg_, num_vars_ ? table(num_vars_) : leaves_);
    }
    // {lo, hi}: the lower and upper halves of layer k - 1 as MLEs in num_vars - k variables, layer(k) = lo * hi element by element
    std::pair<DenseMultilinearExtension, DenseMultilinearExtension> halves(size_t k) const {
        if (order_ != SR_MLE_TRAILING) throw std::invalid_argument("ProductTree::halves: only a trailing-order tree has contiguous operands");
        if (k < 1 || k > num_vars_) throw std::out_of_range("ProductTree: layer index out of range");
        const std::vector<uint64_t> below = table(k - 1);
        const auto mid = below.begin() + below.size() / 2;
        return {DenseMultilinearExtension(cfg_, num_vars_ - k, std::vector<uint64_t>(below.begin(), mid)),
                DenseMultilinearExtension(cfg_, num_vars_ - k, std::vector<uint64_t>(mid, below.end()))};
    }
    // sr_prod_tree_plan: {elements of the layers, kernel launches} of the device form
    static std::pair<size_t, int> plan(sr_ring ring, int log2_degree, size_t num_vars, int order = SR_MLE_TRAILING) {
        size_t elems = 0;
        int launches = 0;
        CyclotomicConfig::check(sr_prod_tree_plan(ring, log2_degree, num_vars, order, &elems, &launches), "sr_prod_tree_plan");
        return {elems, launches};
    }

private:
    std::vector<uint64_t> table(size_t k) const {
        if (k == 0) {
            if (n_leaves() != ((size_t)1 << num_vars_))
                throw std::length_error("ProductTree: layer 0 of a truncated tree is not a table (its missing leaves are one())");
            return leaves_;
        }
        const size_t w = cfg_.words_per_elem(), off = layer_offset(k);
        return std::vector<uint64_t>(layers_.begin() + off * w, layers_.begin() + (off + ((size_t)1 << (num_vars_ - k))) * w);
    }
    CyclotomicConfig cfg_;
    size_t num_vars_;
    int order_;
    std::vector<uint64_t> leaves_, layers_;
};

// sr_frac_tree_plan: {elements of the layers per output, kernel launches} of the device form of a fraction tree
inline std::pair<size_t, int> frac_tree_plan(sr_ring ring, int log2_degree, size_t num_vars, int order = SR_MLE_TRAILING) {
    size_t elems = 0;
    int launches = 0;
    CyclotomicConfig::check(sr_frac_tree_plan(ring, log2_degree, num_vars, order, &elems, &launches), "sr_frac_tree_plan");
    return {elems, launches};
}
// sr_frac_tree_dev on device pointers (d_p_leaves may be null: every stored numerator is one()); allocates nothing
inline void frac_tree_dev(const CyclotomicConfig &cfg, uint64_t *d_p_layers, uint64_t *d_q_layers, const uint64_t *d_p_leaves,
                          const uint64_t *d_q_leaves, size_t n_leaves, size_t num_vars, int order = SR_MLE_TRAILING, void *stream = nullptr) {
    CyclotomicConfig::check(sr_frac_tree_dev(cfg.raw(), d_p_layers, d_q_layers, d_p_leaves, d_q_leaves, n_leaves, num_vars, order, stream),
                            "sr_frac_tree_dev");
}
// sr_frac_tree on host words: {p_layers, q_layers}; p_leaf_words null: every stored numerator is one()
inline std::pair<std::vector<uint64_t>, std::vector<uint64_t>> frac_tree(const CyclotomicConfig &cfg, const std::vector<uint64_t> *p_leaf_words,
                                                                         const std::vector<uint64_t> &q_leaf_words, size_t num_vars,
                                                                         int order = SR_MLE_TRAILING) {
    const size_t w = cfg.words_per_elem();
    if (q_leaf_words.size() % w || (p_leaf_words && p_leaf_words->size() != q_leaf_words.size()))
        throw std::length_error("Should be of correct length");
    const size_t n = q_leaf_words.size() / w;
    if (num_vars >= 48 || n > ((size_t)1 << num_vars)) throw std::length_error("frac_tree: more leaves than 2^num_vars");
    std::vector<uint64_t> p(w * (((size_t)1 << num_vars) - 1)), q(p.size());
    const uint64_t dummy = 0;
    CyclotomicConfig::check(sr_frac_tree(cfg.raw(), p.empty() ? nullptr : p.data(), q.empty() ? nullptr : q.data(),
                                         p_leaf_words ? (n ? p_leaf_words->data() : &dummy) : nullptr, n ? q_leaf_words.data() : &dummy, n, num_vars,
                                         order),
                            "sr_frac_tree");
    return {std::move(p), std::move(q)};
}

// Every layer of the binary tree that sums fractions p_i / q_i of ring elements in CRT/NTT form without dividing (sr_frac_tree): the
// circuit of the layered fractional sum-check behind logUp lookup and range arguments.  A node is (p, q) = (p_l q_r + p_r q_l, q_l q_r)
// with the children of ProductTree; the leaves beyond the stored ones are (zero(), one()); without stored numerators every stored
// leaf has numerator one().  Host buffers; throws where the Python class raises.
class FractionTree {
public:
    FractionTree(CyclotomicConfig cfg, std::vector<uint64_t> q_leaf_words, size_t num_vars, int order = SR_MLE_TRAILING)
        : cfg_(std::move(cfg)), num_vars_(num_vars), order_(order), has_p_(false), q_leaves_(std::move(q_leaf_words)) {
        build();
    }
    FractionTree(CyclotomicConfig cfg, std::vector<uint64_t> p_leaf_words, std::vector<uint64_t> q_leaf_words, size_t num_vars,
                 int order = SR_MLE_TRAILING)
        : cfg_(std::move(cfg)), num_vars_(num_vars), order_(order), has_p_(true), p_leaves_(std::move(p_leaf_words)),
          q_leaves_(std::move(q_leaf_words)) {
        build();
    }
    size_t num_vars() const { return num_vars_; }
    size_t n_leaves() const { return q_leaves_.size() / cfg_.words_per_elem(); }  // stored leaves
    int order() const { return order_; }
    bool has_numerators() const { return has_p_; }
    const std::vector<uint64_t> &p_layer_words() const { return p_layers_; }  // layers 1 .. num_vars, one behind the other
    const std::vector<uint64_t> &q_layer_words() const { return q_layers_; }
    // element offset of layer k (1 <= k <= num_vars) in either output: layer 1 first, the root last
    size_t layer_offset(size_t k) const {
        if (k < 1 || k > num_vars_) throw std::out_of_range("FractionTree: layer index out of range");
        return ((size_t)1 << num_vars_) - ((size_t)1 << (num_vars_ - k + 1));
    }
    // {P_k, Q_k}: layer k as two MLEs in num_vars - k variables; k = 0 gives the leaves (every leaf and numerator must be stored)
    std::pair<DenseMultilinearExtension, DenseMultilinearExtension> layer(size_t k) const {
        if (k > num_vars_) throw std::out_of_range("FractionTree: layer index out of range");
        return {DenseMultilinearExtension(cfg_, num_vars_ - k, table(true, k)), DenseMultilinearExtension(cfg_, num_vars_ - k, table(false, k))};
    }
    // {P, Q}: the numerator and the denominator of the sum of all fractions, one ring element each
    std::pair<RqNTTVec, RqNTTVec> root() const {
        if (num_vars_ == 0 && (q_leaves_.empty() || !has_p_))
            throw std::length_error("FractionTree: a tree of no variables holds its root only as a stored leaf with a stored numerator");
        return {RqNTTVec(cfg_, table(true, num_vars_)), RqNTTVec(cfg_, table(false, num_vars_))};
    }
    // {p_lo, p_hi, q_lo, q_hi}: the halves of layer k - 1 as MLEs in num_vars - k variables; P_k = p_lo q_hi + p_hi q_lo, Q_k = q_lo q_hi
    std::vector<DenseMultilinearExtension> halves(size_t k) const {
        if (order_ != SR_MLE_TRAILING) throw std::invalid_argument("FractionTree::halves: only a trailing-order tree has contiguous operands");
        if (k < 1 || k > num_vars_) throw std::out_of_range("FractionTree: layer index out of range");
        std::vector<DenseMultilinearExtension> out;
        for (bool numer : {true, false}) {
            const std::vector<uint64_t> below = table(numer, k - 1);
            const auto mid = below.begin() + below.size() / 2;
            out.emplace_back(cfg_, num_vars_ - k, std::vector<uint64_t>(below.begin(), mid));
            out.emplace_back(cfg_, num_vars_ - k, std::vector<uint64_t>(mid, below.end()));
        }
        return out;
    }
    static std::pair<size_t, int> plan(sr_ring ring, int log2_degree, size_t num_vars, int order = SR_MLE_TRAILING) {
        return frac_tree_plan(ring, log2_degree, num_vars, order);
    }

private:
    void build() {
        if (order_ != SR_MLE_LEADING && order_ != SR_MLE_TRAILING) throw std::invalid_argument("FractionTree: unknown order");
        auto both = frac_tree(cfg_, has_p_ ? &p_leaves_ : nullptr, q_leaves_, num_vars_, order_);
        p_layers_ = std::move(both.first);
        q_layers_ = std::move(both.second);
    }
    std::vector<uint64_t> table(bool numer, size_t k) const {
        if (k == 0) {
            if (n_leaves() != ((size_t)1 << num_vars_))
                throw std::length_error("FractionTree: layer 0 of a truncated tree is not a table (its missing leaves are (zero(), one()))");
            if (!has_p_) throw std::length_error("FractionTree: layer 0 of a tree without stored numerators is not a table (they are one())");
            return numer ? p_leaves_ : q_leaves_;
        }
        const std::vector<uint64_t> &src = numer ? p_layers_ : q_layers_;
        const size_t w = cfg_.words_per_elem(), off = layer_offset(k);
        return std::vector<uint64_t>(src.begin() + off * w, src.begin() + (off + ((size_t)1 << (num_vars_ - k))) * w);
    }
    CyclotomicConfig cfg_;
    size_t num_vars_;
    int order_;
    bool has_p_;
    std::vector<uint64_t> p_leaves_, q_leaves_, p_layers_, q_layers_;
};

// A multilinear extension in num_vars variables whose evaluations are an IndexColumn: evaluation e is R::from(col[e]); a stored column's
// evaluations beyond its values are zero.  A factor of a VirtualPolynomial: the weighted sum-check rounds read it as one u64 per row
// (sr_vpoly_iwround_evals / sr_vpoly_iwround_fold_evals), everything else expands it with to_dense() first.
class IndexMultilinearExtension {
public:
    IndexMultilinearExtension(CyclotomicConfig cfg, size_t num_vars, IndexColumn column) : cfg_(std::move(cfg)), nv_(num_vars), col_(std::move(column)) {
        if (nv_ >= 48) throw std::length_error("IndexMultilinearExtension: num_vars must be below 48");
        const uint64_t full = (uint64_t)1 << nv_;
        if (col_.is_progression) {
            if (!col_.values.empty()) throw std::length_error("IndexMultilinearExtension: a progression stores no values");
            if (col_.start > UINT64_MAX - (full - 1)) throw std::length_error("IndexMultilinearExtension: a progression wraps past 2^64 - 1");
        } else {
            if (col_.start != 0) throw std::length_error("IndexMultilinearExtension: a stored column with a non-zero start");
            if (col_.values.size() > full) throw std::length_error("IndexMultilinearExtension: more values than 2^num_vars");
        }
    }
    size_t num_vars() const { return nv_; }
    size_t len() const { return col_.is_progression ? (size_t)1 << nv_ : col_.values.size(); }  // stored evaluations
    const IndexColumn &column() const { return col_; }
    const CyclotomicConfig &config() const { return cfg_; }
    // the DenseMultilinearExtension of the same evaluations: from_u64 over the stored part, D words per integer
    DenseMultilinearExtension to_dense() const {
        if (len() == 0) return DenseMultilinearExtension(cfg_, nv_, std::vector<uint64_t>());
        const uint64_t dummy = 0;
        std::vector<uint64_t> one(cfg_.words_per_elem());  // the eq table of no variables is the single element one()
        CyclotomicConfig::check(sr_eq_table(cfg_.raw(), one.data(), &dummy, 0), "sr_eq_table");
        return DenseMultilinearExtension(cfg_, nv_, from_u64(cfg_, col_, len(), one));
    }

private:
    CyclotomicConfig cfg_;
    size_t nv_;
    IndexColumn col_;
};

// A sum of products of dense MLEs with ring coefficients, g = sum_k c_k prod_s f_{k,s}, after HyperPlonk's VirtualPolynomial (the code
// crates/poly's polynomials/multilinear_polynomial.rs was adapted from): the object a sum-check is run on -- eq (a b - c),
// sum_i alpha_i eq prod_j (...).  The MLEs are referred to, not copied, and must outlive the polynomial; an MLE that is in several
// products is one table slot and is read once per round (sr_vpoly_round_evals).  At most SR_VPOLY_MAX_TABLES distinct MLEs,
// SR_VPOLY_MAX_TERMS products, SR_VPOLY_MAX_FACTORS factors per product; throws std::length_error beyond, leaving the polynomial as it was.
// A factor may be an IndexMultilinearExtension, a column of integers that stands for the table R::from(col[e]): round_evals_weighted
// and fold_round_evals_weighted read such a slot as u64 (sr_vpoly_iwround_*), and the polynomial fold_round_evals_weighted returns
// holds dense tables only.  round_evals, sum, fold_round_evals and fixed_variables have no such kernels: they expand every column slot
// with to_dense() first -- the slow path, D words per integer.
class VirtualPolynomial {
public:
    VirtualPolynomial(CyclotomicConfig cfg, size_t num_vars) : cfg_(std::move(cfg)), nv_(num_vars) {}
    size_t num_vars() const { return nv_; }
    // the largest number of factors of a product: a round message has degree() + 1 elements
    size_t degree() const {
        int d = 0;
        for (const sr_vpoly_term &t : terms_) d = t.n_factors > d ? t.n_factors : d;
        return (size_t)d;
    }
    // the table slots, in order of first use; a slot that holds a column is nullptr here and set in columns()
    const std::vector<const DenseMultilinearExtension *> &tables() const { return tables_; }
    const std::vector<const IndexMultilinearExtension *> &columns() const { return columns_; }
    bool has_columns() const {
        for (const IndexMultilinearExtension *c : columns_)
            if (c) return true;
        return false;
    }
    const std::vector<sr_vpoly_term> &terms() const { return terms_; }
    // g += coeff * prod(mles): 1 .. 4 MLEs (one may appear twice), coeff one ring element or nullptr for one()
    void add_mle_list(const std::vector<const DenseMultilinearExtension *> &mles, const RqNTTVec *coeff = nullptr) {
        add_product(mles, {}, coeff);
    }
    // g += coeff * prod(mles) * prod(columns): add_mle_list with factors of both kinds, 1 .. 4 together.  Its own name, not one more
    // overload: a braced list of pointers, or {}, would otherwise have to choose between two vector types and a null coefficient.
    void add_product(const std::vector<const DenseMultilinearExtension *> &mles, const std::vector<const IndexMultilinearExtension *> &columns,
                     const RqNTTVec *coeff = nullptr) {
        if (mles.size() + columns.size() < 1 || mles.size() + columns.size() > SR_VPOLY_MAX_FACTORS)
            throw std::length_error("VirtualPolynomial: a product has 1 .. 4 factors");
        if (terms_.size() >= SR_VPOLY_MAX_TERMS) throw std::length_error("VirtualPolynomial: more than 8 products");
        if (coeff && coeff->len() != 1) throw std::length_error("VirtualPolynomial: the coefficient is not one ring element");
        std::vector<const DenseMultilinearExtension *> slots = tables_;
        std::vector<const IndexMultilinearExtension *> cslots = columns_;
        sr_vpoly_term t{};
        for (const DenseMultilinearExtension *m : mles) t.table[t.n_factors++] = slot_of(slots, cslots, m, nullptr);
        for (const IndexMultilinearExtension *c : columns) t.table[t.n_factors++] = slot_of(slots, cslots, nullptr, c);
        tables_ = std::move(slots);
        columns_ = std::move(cslots);
        terms_.push_back(t);
        has_coeff_.push_back(coeff != nullptr);
        coeffs_.push_back(coeff ? coeff->words() : std::vector<uint64_t>());
    }
    // g *= mle: the MLE becomes one more factor of every product
    void mul_by_mle(const DenseMultilinearExtension *mle) { mul_by(mle, nullptr); }
    void mul_by_mle(const IndexMultilinearExtension *mle) { mul_by(nullptr, mle); }
    // The prover's message of one sum-check round over g: the degree() + 1 elements p(t) = sum_b g(t, b), t = 0 .. degree(), the variable
    // being the one fix_variables (SR_MLE_LEADING) or fix_last_variables (SR_MLE_TRAILING) fixes next.
    RqNTTVec round_evals(int order = SR_MLE_LEADING) const {
        if (order != SR_MLE_LEADING && order != SR_MLE_TRAILING) throw std::invalid_argument("round_evals: unknown order");
        return call(order);
    }
    // sum_b g(b) over the hypercube: the claimed sum of the sum-check, one ring element
    RqNTTVec sum() const { return call(SR_MLE_ROUND_SUM); }
    // One prover round in one pass over the distinct tables (sr_vpoly_round_fold_evals): every table slot with its next variable fixed at
    // the ring element r, and the message of the round that follows: {message, the polynomial of the same terms and coefficients over
    // the folded tables in num_vars() - 1 variables} -- what fixed_variables(r) followed by round_evals returns, bit for bit.  The
    // returned polynomial owns its tables; the slots stay deduplicated.  Throws where the C call refuses (num_vars() < 2: the last round
    // folds with fixed_variables).
    std::pair<RqNTTVec, VirtualPolynomial> fold_round_evals(const RqNTTVec &r, int order = SR_MLE_LEADING) const {
        if (order != SR_MLE_LEADING && order != SR_MLE_TRAILING) throw std::invalid_argument("fold_round_evals: unknown order");
        if (terms_.empty()) throw std::length_error("VirtualPolynomial: no product has been added");
        if (has_columns()) return dense().fold_round_evals(r, order);
        if (r.len() != 1) throw std::length_error("fold_round_evals: r is not one ring element");
        if (nv_ < 2) throw std::length_error("fold_round_evals: num_vars >= 2");
        const size_t w = cfg_.words_per_elem();
        std::vector<const uint64_t *> ptrs;
        std::vector<size_t> sizes;
        std::vector<std::vector<uint64_t>> folded;
        std::vector<uint64_t *> optrs;
        for (const DenseMultilinearExtension *t : tables_) {
            ptrs.push_back(t->words().empty() ? nullptr : t->words().data());
            sizes.push_back(t->len());
            folded.emplace_back(t->words().size());  // never shorter than the folded table
        }
        for (auto &f : folded) optrs.push_back(f.empty() ? nullptr : f.data());
        std::vector<size_t> n_out(tables_.size());
        std::vector<uint64_t> out(w * (degree() + 1));
        const std::vector<uint64_t> coeffs = coeff_words();
        CyclotomicConfig::check(sr_vpoly_round_fold_evals(cfg_.raw(), out.data(), optrs.data(), n_out.data(), ptrs.data(), sizes.data(),
                                                          (int)tables_.size(), terms_.data(), (int)terms_.size(),
                                                          coeffs.empty() ? nullptr : coeffs.data(), nv_, r.words().data(), order),
                                "sr_vpoly_round_fold_evals");
        std::vector<DenseMultilinearExtension> g;
        for (size_t j = 0; j < tables_.size(); j++) {
            folded[j].resize(n_out[j] * w);
            g.emplace_back(cfg_, nv_ - 1, std::move(folded[j]));
        }
        return {RqNTTVec(cfg_, std::move(out)), over(std::move(g), nv_ - 1)};
    }
    // The polynomial of the same terms and coefficients with the variables of `point` fixed in every distinct table: fixed_variables
    // (SR_MLE_LEADING) or fix_last_variables (SR_MLE_TRAILING) per table slot -- the last round of a sum-check, and callers that want no
    // message.  The returned polynomial owns its tables.
    VirtualPolynomial fixed_variables(const RqNTTVec &point, int order = SR_MLE_LEADING) const {
        if (order != SR_MLE_LEADING && order != SR_MLE_TRAILING) throw std::invalid_argument("fixed_variables: unknown order");
        if (point.len() > nv_) throw std::length_error("too many partial points");
        if (has_columns()) return dense().fixed_variables(point, order);
        std::vector<DenseMultilinearExtension> g;
        for (const DenseMultilinearExtension *t : tables_) g.push_back(order == SR_MLE_LEADING ? t->fixed_variables(point) : t->fix_last_variables(point));
        return over(std::move(g), nv_ - point.len());
    }
    // The round message with a per-pair weight (sr_vpoly_wround_evals): the degree() + 1 elements h(t) = sum_b weights[b] g(t, b), b over
    // the 2^(num_vars() - 1) pairs of the round.  The weight is constant in the round's variable and is no factor: it is not counted in
    // degree().  With eq(z_rest, .) as weights this is the eq(z, .) factor of a zero-check without a table (EqSumCheck below).
    RqNTTVec round_evals_weighted(const RqNTTVec &weights, int order = SR_MLE_LEADING) const {
        if (order != SR_MLE_LEADING && order != SR_MLE_TRAILING) throw std::invalid_argument("round_evals_weighted: unknown order");
        if (terms_.empty()) throw std::length_error("VirtualPolynomial: no product has been added");
        if (nv_ < 1 || weights.len() != (size_t)1 << (nv_ - 1)) throw std::length_error("round_evals_weighted: one weight per pair");
        if (has_columns()) return indexed(weights, nullptr, order).first;
        std::vector<const uint64_t *> ptrs;
        std::vector<size_t> sizes;
        for (const DenseMultilinearExtension *t : tables_) {
            ptrs.push_back(t->words().empty() ? nullptr : t->words().data());
            sizes.push_back(t->len());
        }
        const std::vector<uint64_t> coeffs = coeff_words();
        std::vector<uint64_t> out(cfg_.words_per_elem() * (degree() + 1));
        CyclotomicConfig::check(sr_vpoly_wround_evals(cfg_.raw(), out.data(), weights.words().data(), ptrs.data(), sizes.data(), (int)tables_.size(),
                                                      terms_.data(), (int)terms_.size(), coeffs.empty() ? nullptr : coeffs.data(), nv_, order),
                                "sr_vpoly_wround_evals");
        return RqNTTVec(cfg_, std::move(out));
    }
    // fold_round_evals with a per-pair weight on the message (sr_vpoly_wround_fold_evals): every table slot folded at r, and
    // round_evals_weighted(next_weights) of the folded polynomial, in one pass.  next_weights: 2^(num_vars() - 2) elements.
    std::pair<RqNTTVec, VirtualPolynomial> fold_round_evals_weighted(const RqNTTVec &r, const RqNTTVec &next_weights, int order = SR_MLE_LEADING) const {
        if (order != SR_MLE_LEADING && order != SR_MLE_TRAILING) throw std::invalid_argument("fold_round_evals_weighted: unknown order");
        if (terms_.empty()) throw std::length_error("VirtualPolynomial: no product has been added");
        if (r.len() != 1) throw std::length_error("fold_round_evals_weighted: r is not one ring element");
        if (nv_ < 2) throw std::length_error("fold_round_evals_weighted: num_vars >= 2");
        if (next_weights.len() != (size_t)1 << (nv_ - 2)) throw std::length_error("fold_round_evals_weighted: one weight per pair of the folded tables");
        if (has_columns()) return indexed(next_weights, &r, order);
        const size_t w = cfg_.words_per_elem();
        std::vector<const uint64_t *> ptrs;
        std::vector<size_t> sizes;
        std::vector<std::vector<uint64_t>> folded;
        std::vector<uint64_t *> optrs;
        for (const DenseMultilinearExtension *t : tables_) {
            ptrs.push_back(t->words().empty() ? nullptr : t->words().data());
            sizes.push_back(t->len());
            folded.emplace_back(t->words().size());  // never shorter than the folded table
        }
        for (auto &f : folded) optrs.push_back(f.empty() ? nullptr : f.data());
        std::vector<size_t> n_out(tables_.size());
        std::vector<uint64_t> out(w * (degree() + 1));
        const std::vector<uint64_t> coeffs = coeff_words();
        CyclotomicConfig::check(sr_vpoly_wround_fold_evals(cfg_.raw(), out.data(), optrs.data(), n_out.data(), next_weights.words().data(), ptrs.data(),
                                                           sizes.data(), (int)tables_.size(), terms_.data(), (int)terms_.size(),
                                                           coeffs.empty() ? nullptr : coeffs.data(), nv_, r.words().data(), order),
                                "sr_vpoly_wround_fold_evals");
        std::vector<DenseMultilinearExtension> g;
        for (size_t j = 0; j < tables_.size(); j++) {
            folded[j].resize(n_out[j] * w);
            g.emplace_back(cfg_, nv_ - 1, std::move(folded[j]));
        }
        return {RqNTTVec(cfg_, std::move(out)), over(std::move(g), nv_ - 1)};
    }
    const CyclotomicConfig &config() const { return cfg_; }

private:
    // the same terms and coefficients over `tables`, one per table slot, owned by the result
    VirtualPolynomial over(std::vector<DenseMultilinearExtension> tables, size_t num_vars) const {
        VirtualPolynomial g(cfg_, num_vars);
        g.owned_ = std::make_shared<std::vector<DenseMultilinearExtension>>(std::move(tables));
        for (const DenseMultilinearExtension &t : *g.owned_) g.tables_.push_back(&t);
        g.terms_ = terms_;
        g.has_coeff_ = has_coeff_;
        g.coeffs_ = coeffs_;
        return g;
    }
    // the coefficients of a call: empty where every coefficient is one() and none is passed
    std::vector<uint64_t> coeff_words() const {
        std::vector<uint64_t> coeffs;
        bool any = false;
        for (bool h : has_coeff_) any = any || h;
        if (any) {
            const uint64_t dummy = 0;
            std::vector<uint64_t> one(cfg_.words_per_elem());  // the eq table of no variables is the single element one()
            CyclotomicConfig::check(sr_eq_table(cfg_.raw(), one.data(), &dummy, 0), "sr_eq_table");
            for (size_t k = 0; k < terms_.size(); k++) {
                const std::vector<uint64_t> &c = has_coeff_[k] ? coeffs_[k] : one;
                coeffs.insert(coeffs.end(), c.begin(), c.end());
            }
        }
        return coeffs;
    }
    // the slot of a dense MLE (m) or of a column (c): the two vectors run in parallel, one of the two entries of a slot is set
    int slot_of(std::vector<const DenseMultilinearExtension *> &slots, std::vector<const IndexMultilinearExtension *> &cslots,
                const DenseMultilinearExtension *m, const IndexMultilinearExtension *c) const {
        if ((m && (m->config().raw() != cfg_.raw() || m->num_vars() != nv_)) || (c && (c->config().raw() != cfg_.raw() || c->num_vars() != nv_)))
            throw std::length_error("VirtualPolynomial: the MLEs differ in ring or num_vars");
        cslots.resize(slots.size(), nullptr);
        for (size_t j = 0; j < slots.size(); j++)
            if (slots[j] == m && cslots[j] == c) return (int)j;
        if (slots.size() >= SR_VPOLY_MAX_TABLES) throw std::length_error("VirtualPolynomial: more than 8 distinct tables");
        slots.push_back(m);
        cslots.push_back(c);
        return (int)slots.size() - 1;
    }
    void mul_by(const DenseMultilinearExtension *m, const IndexMultilinearExtension *c) {
        if (terms_.empty()) throw std::length_error("VirtualPolynomial: mul_by_mle on an empty polynomial");
        for (const sr_vpoly_term &t : terms_)
            if (t.n_factors >= SR_VPOLY_MAX_FACTORS) throw std::length_error("VirtualPolynomial: a product has 1 .. 4 factors");
        std::vector<const DenseMultilinearExtension *> slots = tables_;
        std::vector<const IndexMultilinearExtension *> cslots = columns_;
        const int slot = slot_of(slots, cslots, m, c);
        tables_ = std::move(slots);
        columns_ = std::move(cslots);
        for (sr_vpoly_term &t : terms_) t.table[t.n_factors++] = slot;
    }
    const IndexMultilinearExtension *column_at(size_t j) const { return j < columns_.size() ? columns_[j] : nullptr; }
    // the same polynomial with every column slot expanded to a ring table
    VirtualPolynomial dense() const {
        std::vector<DenseMultilinearExtension> g;
        for (size_t j = 0; j < tables_.size(); j++) g.push_back(column_at(j) ? column_at(j)->to_dense() : *tables_[j]);
        return over(std::move(g), nv_);
    }
    // sr_vpoly_iwround_evals (r == nullptr) or sr_vpoly_iwround_fold_evals: the dense slots first, then the column slots, the terms
    // renumbered; the folded slots come back in the polynomial's own slot order
    std::pair<RqNTTVec, VirtualPolynomial> indexed(const RqNTTVec &weights, const RqNTTVec *r, int order) const {
        const size_t w = cfg_.words_per_elem(), n = tables_.size();
        const uint64_t dummy = 0;
        std::vector<size_t> slot_of_operand;
        for (size_t j = 0; j < n; j++)
            if (!column_at(j)) slot_of_operand.push_back(j);
        const size_t K = slot_of_operand.size();
        for (size_t j = 0; j < n; j++)
            if (column_at(j)) slot_of_operand.push_back(j);
        std::vector<int> operand_of_slot(n);
        for (size_t i = 0; i < n; i++) operand_of_slot[slot_of_operand[i]] = (int)i;
        std::vector<sr_vpoly_term> terms = terms_;
        for (sr_vpoly_term &t : terms)
            for (int s = 0; s < t.n_factors; s++) t.table[s] = operand_of_slot[t.table[s]];
        std::vector<const uint64_t *> ptrs;
        std::vector<size_t> sizes;
        std::vector<sr_index_column> cols;
        std::vector<std::vector<uint64_t>> folded;
        for (size_t i = 0; i < n; i++) {
            const size_t j = slot_of_operand[i];
            if (i < K) {
                ptrs.push_back(tables_[j]->words().empty() ? nullptr : tables_[j]->words().data());
                sizes.push_back(tables_[j]->len());
            } else {
                const IndexColumn &c = column_at(j)->column();
                if (c.is_progression) cols.push_back(sr_index_column{nullptr, 0, c.start});
                else cols.push_back(sr_index_column{c.values.empty() ? &dummy : c.values.data(), c.values.size(), 0});
            }
            const size_t stored = i < K ? tables_[j]->len() : column_at(j)->len();
            if (r) folded.emplace_back(stored * w);  // never shorter than the folded slot
        }
        const std::vector<uint64_t> coeffs = coeff_words();
        std::vector<uint64_t> out(w * (degree() + 1));
        if (!r) {
            CyclotomicConfig::check(sr_vpoly_iwround_evals(cfg_.raw(), out.data(), weights.words().data(), ptrs.data(), sizes.data(), (int)K, cols.data(),
                                                           (int)(n - K), terms.data(), (int)terms.size(), coeffs.empty() ? nullptr : coeffs.data(),
                                                           nv_, order),
                                    "sr_vpoly_iwround_evals");
            return {RqNTTVec(cfg_, std::move(out)), VirtualPolynomial(cfg_, nv_)};
        }
        std::vector<uint64_t *> optrs;
        uint64_t sink = 0;
        for (auto &f : folded) optrs.push_back(f.empty() ? &sink : f.data());
        std::vector<size_t> n_out(n);
        CyclotomicConfig::check(sr_vpoly_iwround_fold_evals(cfg_.raw(), out.data(), optrs.data(), n_out.data(), weights.words().data(), ptrs.data(),
                                                            sizes.data(), (int)K, cols.data(), (int)(n - K), terms.data(), (int)terms.size(),
                                                            coeffs.empty() ? nullptr : coeffs.data(), nv_, r->words().data(), order),
                                "sr_vpoly_iwround_fold_evals");
        std::vector<DenseMultilinearExtension> g;
        for (size_t j = 0; j < n; j++) {
            const size_t i = (size_t)operand_of_slot[j];
            folded[i].resize(n_out[i] * w);
            g.emplace_back(cfg_, nv_ - 1, std::move(folded[i]));
        }
        return {RqNTTVec(cfg_, std::move(out)), over(std::move(g), nv_ - 1)};
    }
    RqNTTVec call(int mode) const {
        if (terms_.empty()) throw std::length_error("VirtualPolynomial: no product has been added");
        if (has_columns()) return dense().call(mode);
        const size_t w = cfg_.words_per_elem();
        std::vector<const uint64_t *> ptrs;
        std::vector<size_t> sizes;
        for (const DenseMultilinearExtension *t : tables_) {
            ptrs.push_back(t->words().empty() ? nullptr : t->words().data());
            sizes.push_back(t->len());
        }
        const std::vector<uint64_t> coeffs = coeff_words();
        std::vector<uint64_t> out(w * (mode == SR_MLE_ROUND_SUM ? 1 : degree() + 1));
        CyclotomicConfig::check(sr_vpoly_round_evals(cfg_.raw(), out.data(), ptrs.data(), sizes.data(), (int)tables_.size(), terms_.data(),
                                                     (int)terms_.size(), coeffs.empty() ? nullptr : coeffs.data(), nv_, mode),
                                "sr_vpoly_round_evals");
        return RqNTTVec(cfg_, std::move(out));
    }
    CyclotomicConfig cfg_;
    size_t nv_;
    std::vector<const DenseMultilinearExtension *> tables_;
    std::vector<const IndexMultilinearExtension *> columns_;  // parallel to tables_ (shorter: no column behind); one of the two is set per slot
    std::vector<sr_vpoly_term> terms_;
    std::vector<bool> has_coeff_;
    std::vector<std::vector<uint64_t>> coeffs_;
    std::shared_ptr<std::vector<DenseMultilinearExtension>> owned_;  // the tables of a polynomial that fold_round_evals / fixed_variables made
};

// The range-check (norm-check) claim without eq, g(x) = sum_i mu_i P_B(f_i(x)) with P_B(x) = prod_{j = -(B-1)}^{B-1} (x - R::from(j)), over
// 1 .. 8 dense MLEs (sr_range_wround_evals): every entry of every f_i lies in (-B, B) exactly when sum_b eq(beta, b) g(b) = 0.  It has the
// members EqSumCheckOver uses of its g, so RangeSumCheck(RangePolynomial(cfg, tables, bound), z, order) is the prover of the whole norm
// check.  The tables are referred to, not copied; coeffs: one ring element per table, or nullptr for one().  degree() = 2 bound - 1.
class RangePolynomial {
public:
    RangePolynomial(CyclotomicConfig cfg, const std::vector<const DenseMultilinearExtension *> &tables, int bound, const RqNTTVec *coeffs = nullptr)
        : cfg_(std::move(cfg)), nv_(tables.empty() ? 0 : tables[0]->num_vars()), bound_(bound), tables_(tables) {
        if (tables.empty() || tables.size() > SR_RANGE_MAX_TABLES) throw std::length_error("RangePolynomial: 1 .. 8 tables");
        if (bound < 2 || bound > SR_RANGE_MAX_BOUND) throw std::length_error("RangePolynomial: bound must be 2 .. 8");
        for (const DenseMultilinearExtension *t : tables)
            if (t->config().raw() != cfg_.raw() || t->num_vars() != nv_) throw std::length_error("RangePolynomial: the MLEs differ in ring or num_vars");
        if (coeffs && coeffs->len() != tables.size()) throw std::length_error("RangePolynomial: one coefficient per table");
        if (coeffs) coeffs_ = coeffs->words();
    }
    size_t num_vars() const { return nv_; }
    size_t degree() const { return (size_t)(2 * bound_ - 1); }  // a round message has degree() + 1 elements
    int bound() const { return bound_; }
    const std::vector<const DenseMultilinearExtension *> &tables() const { return tables_; }
    const CyclotomicConfig &config() const { return cfg_; }
    // h(t) = sum_b weights[b] g(t, b), t = 0 .. degree(), b over the 2^(num_vars() - 1) pairs of the round
    RqNTTVec round_evals_weighted(const RqNTTVec &weights, int order = SR_MLE_LEADING) const {
        if (order != SR_MLE_LEADING && order != SR_MLE_TRAILING) throw std::invalid_argument("round_evals_weighted: unknown order");
        if (nv_ < 1 || weights.len() != (size_t)1 << (nv_ - 1)) throw std::length_error("round_evals_weighted: one weight per pair");
        std::vector<const uint64_t *> ptrs;
        std::vector<size_t> sizes;
        for (const DenseMultilinearExtension *t : tables_) {
            ptrs.push_back(t->words().empty() ? nullptr : t->words().data());
            sizes.push_back(t->len());
        }
        std::vector<uint64_t> out(cfg_.words_per_elem() * 2 * (size_t)bound_);
        cfg_.range_wround_evals(out.data(), weights.words().data(), ptrs.data(), sizes.data(), (int)tables_.size(), bound_,
                                coeffs_.empty() ? nullptr : coeffs_.data(), nv_, order);
        return RqNTTVec(cfg_, std::move(out));
    }
    // the same claim with the variables of `point` fixed in every table; the result owns its tables
    RangePolynomial fixed_variables(const RqNTTVec &point, int order = SR_MLE_LEADING) const {
        if (order != SR_MLE_LEADING && order != SR_MLE_TRAILING) throw std::invalid_argument("fixed_variables: unknown order");
        if (point.len() > nv_) throw std::length_error("too many partial points");
        auto owned = std::make_shared<std::vector<DenseMultilinearExtension>>();
        for (const DenseMultilinearExtension *t : tables_)
            owned->push_back(order == SR_MLE_LEADING ? t->fixed_variables(point) : t->fix_last_variables(point));
        RangePolynomial g(*this);
        g.nv_ = nv_ - point.len();
        g.tables_.clear();
        for (const DenseMultilinearExtension &t : *owned) g.tables_.push_back(&t);
        g.owned_ = std::move(owned);
        return g;
    }
    // every table folded at r (one variable, sr_mle_fix_variables) and round_evals_weighted(next_weights) of the folded claim
    std::pair<RqNTTVec, RangePolynomial> fold_round_evals_weighted(const RqNTTVec &r, const RqNTTVec &next_weights, int order = SR_MLE_LEADING) const {
        if (r.len() != 1) throw std::length_error("fold_round_evals_weighted: r is not one ring element");
        if (nv_ < 2) throw std::length_error("fold_round_evals_weighted: num_vars >= 2");
        RangePolynomial g = fixed_variables(r, order);
        RqNTTVec msg = g.round_evals_weighted(next_weights, order);
        return {std::move(msg), std::move(g)};
    }

private:
    CyclotomicConfig cfg_;
    size_t nv_;
    int bound_;
    std::vector<const DenseMultilinearExtension *> tables_;
    std::vector<uint64_t> coeffs_;
    std::shared_ptr<std::vector<DenseMultilinearExtension>> owned_;  // the tables of a claim that fixed_variables made
};

// The prover of a whole sum-check of  sum_b eq(z, b) g(b)  -- a zero-check, R1CS, the layer claim of a product or fraction tree -- WITHOUT
// an eq table.  In the round that binds variable v, with the challenges r of the earlier rounds bound,
//     s(t) = [prod_{i bound} eq(z_i, r_i)] * eq(z_v, t) * h(t),   h(t) = sum_b w[b] g(t, b),   w = eq(z_rest, .)
// with g folded at the challenges so far and w the eq table of the unbound coordinates of z only: one element per pair, never folded
// (VirtualPolynomial::round_evals_weighted / fold_round_evals_weighted).  message() is s(0 .. degree + 1), bit-identical to what the
// prover that holds eq(z, .) as one more table sends.  g is referred to, not copied, until the first next(); z: num_vars ring elements;
// SR_MLE_LEADING binds variable 0 first, SR_MLE_TRAILING variable n - 1.
// G: VirtualPolynomial (EqSumCheck) or RangePolynomial (RangeSumCheck).
template <class G>
class EqSumCheckOver {
public:
    EqSumCheckOver(const G &g, const RqNTTVec &z, int order = SR_MLE_LEADING)
        : cfg_(g.config()), g_(g), z_(z), order_(order), n_(g.num_vars()), d_(g.degree()), round_(1), prefix_(one()), h_(one()) {
        if (order != SR_MLE_LEADING && order != SR_MLE_TRAILING) throw std::invalid_argument("EqSumCheck: unknown order");
        if (n_ < 1 || d_ < 1) throw std::length_error("EqSumCheck: a polynomial of at least one variable and one product");
        if (z.len() != n_) throw std::length_error("EqSumCheck: z must hold num_vars ring elements");
        h_ = g_.round_evals_weighted(weights(1), order_);
    }
    size_t degree() const { return d_; }
    size_t round() const { return round_; }  // 1 .. num_vars; num_vars + 1 once every variable is bound
    // the weights of round j = 1 .. n: the eq table of z[j:] (leading) or z[:n - j] (trailing), 2^(n - j) elements
    RqNTTVec weights(size_t j) const { return eq_table(order_ == SR_MLE_LEADING ? slice(z_, j, n_) : slice(z_, 0, n_ - j)); }
    // s(0 .. degree + 1) of the current round: degree + 2 ring elements
    RqNTTVec message() const {
        if (round_ > n_) throw std::length_error("EqSumCheck: every variable is bound");
        // h(d + 1) = sum_{i <= d} (-1)^(d - i) C(d + 1, i) h(i): the (d + 1)-th finite difference of a polynomial of degree d is zero
        RqNTTVec next = zero();
        size_t c = 1;
        for (size_t i = 0; i <= d_; i++) {
            const RqNTTVec hi = slice(h_, i, i + 1);
            for (size_t q = 0; q < c; q++) {
                if ((d_ - i) % 2 == 0) next += hi;
                else next -= hi;
            }
            c = c * (d_ + 1 - i) / (i + 1);
        }
        const RqNTTVec zv = bound_coordinate(round_);
        RqNTTVec e = one();
        e -= zv;  // eq(z_v, 0)
        RqNTTVec step = zv;
        step -= e;  // 2 z_v - one()
        std::vector<uint64_t> out;
        for (size_t t = 0; t <= d_ + 1; t++) {
            RqNTTVec s = (t <= d_ ? slice(h_, t, t + 1) : next) * e;
            s *= prefix_;  // the prefix product last
            out.insert(out.end(), s.words().begin(), s.words().end());
            e += step;
        }
        return RqNTTVec(cfg_, std::move(out));
    }
    // binds the current round's variable to the challenge r and advances: the fused call while two variables are left, fixed_variables
    // for the last round
    void next(const RqNTTVec &r) {
        if (round_ > n_) throw std::length_error("EqSumCheck: every variable is bound");
        if (r.len() != 1) throw std::length_error("EqSumCheck: r is not one ring element");
        if (g_.num_vars() >= 2) {
            auto step = g_.fold_round_evals_weighted(r, weights(round_ + 1), order_);
            h_ = std::move(step.first);
            g_ = std::move(step.second);
        } else {
            g_ = g_.fixed_variables(r, order_);
        }
        const RqNTTVec zv = bound_coordinate(round_);
        RqNTTVec e = one();
        e -= zv;
        RqNTTVec step = zv;
        step -= e;
        step *= r;
        e += step;  // eq(z_v, r)
        prefix_ *= e;
        round_++;
    }
    // {the values of g's table slots at the challenges, one ring element each; eq(z, r)} once every variable is bound
    std::pair<std::vector<RqNTTVec>, RqNTTVec> final() const {
        if (round_ <= n_) throw std::length_error("EqSumCheck: variables are still unbound");
        std::vector<RqNTTVec> vals;
        for (const DenseMultilinearExtension *t : g_.tables()) vals.emplace_back(cfg_, t->words());
        return {vals, prefix_};
    }

private:
    RqNTTVec one() const { return eq_table(RqNTTVec(cfg_, std::vector<uint64_t>())); }
    RqNTTVec zero() const { return RqNTTVec(cfg_, std::vector<uint64_t>(cfg_.words_per_elem(), 0)); }
    RqNTTVec slice(const RqNTTVec &v, size_t from, size_t to) const {
        const size_t w = cfg_.words_per_elem();
        return RqNTTVec(cfg_, std::vector<uint64_t>(v.words().begin() + from * w, v.words().begin() + to * w));
    }
    RqNTTVec bound_coordinate(size_t j) const {
        const size_t v = order_ == SR_MLE_LEADING ? j - 1 : n_ - j;
        return slice(z_, v, v + 1);
    }
    CyclotomicConfig cfg_;
    G g_;
    RqNTTVec z_;
    int order_;
    size_t n_, d_, round_;
    RqNTTVec prefix_, h_;
};
using EqSumCheck = EqSumCheckOver<VirtualPolynomial>;
using RangeSumCheck = EqSumCheckOver<RangePolynomial>;

// The leaves of a permutation argument from ONE call over the three tables (K = 3, M = 2): {num, den} = {beta + f + gamma id,
// beta + f + gamma sigma}; the mask of each row leaves out the table it does not use.  beta, gamma, one: one ring element each.
inline std::pair<std::vector<uint64_t>, std::vector<uint64_t>> permutation_leaves(const CyclotomicConfig &cfg, const std::vector<uint64_t> &f,
                                                                                  const std::vector<uint64_t> &ident, const std::vector<uint64_t> &sigma,
                                                                                  const RqNTTVec &beta, const RqNTTVec &gamma, const RqNTTVec &one) {
    const size_t w = cfg.words_per_elem();
    if (ident.size() != f.size() || sigma.size() != f.size() || f.size() % w) throw std::length_error("permutation_leaves: the tables differ in length");
    if (beta.len() != 1 || gamma.len() != 1 || one.len() != 1) throw std::length_error("permutation_leaves: beta, gamma and one are one ring element each");
    std::vector<uint64_t> coef;
    for (int row = 0; row < 2; row++)
        for (const RqNTTVec *c : {&one, &gamma, &gamma, &beta}) coef.insert(coef.end(), c->words().begin(), c->words().end());
    auto outs = lincomb(cfg, {&f, &ident, &sigma}, coef, {0xBu, 0xDu}, f.size() / w);
    return {std::move(outs[0]), std::move(outs[1])};
}
// One table sum_k coeffs[k] * columns[k] (+ constant) from 1 .. 16 columns of equal length, in one pass
inline std::vector<uint64_t> fingerprint(const CyclotomicConfig &cfg, const std::vector<const std::vector<uint64_t> *> &columns, const RqNTTVec &coeffs,
                                         const RqNTTVec *constant = nullptr) {
    const size_t w = cfg.words_per_elem();
    if (columns.empty() || coeffs.len() != columns.size() || (constant && constant->len() != 1))
        throw std::length_error("fingerprint: one coefficient per column, and a constant of one ring element");
    for (const auto *c : columns)
        if (c->size() != columns[0]->size()) throw std::length_error("fingerprint: the columns differ in length");
    std::vector<uint64_t> coef(coeffs.words());
    if (constant) coef.insert(coef.end(), constant->words().begin(), constant->words().end());
    else coef.resize(coef.size() + w, 0);
    const uint32_t mask = (((uint32_t)1 << columns.size()) - 1) | (constant ? (uint32_t)1 << columns.size() : 0);
    return std::move(lincomb(cfg, columns, coef, {mask}, columns[0]->size() / w)[0]);
}

// permutation_leaves with id and sigma as integers: {num, den} = {beta + f + gamma R::from(id_start + e), beta + f + gamma
// R::from(sigma_idx[e])} from ONE call with K = 1, J = 2, M = 2; id is a progression, sigma_idx one uint64_t per row of f
inline std::pair<std::vector<uint64_t>, std::vector<uint64_t>> permutation_leaves_indexed(const CyclotomicConfig &cfg, const std::vector<uint64_t> &f,
                                                                                          const std::vector<uint64_t> &sigma_idx, const RqNTTVec &beta,
                                                                                          const RqNTTVec &gamma, const RqNTTVec &one,
                                                                                          uint64_t id_start = 0) {
    const size_t w = cfg.words_per_elem();
    if (f.size() % w || sigma_idx.size() != f.size() / w) throw std::length_error("permutation_leaves_indexed: sigma_idx holds one integer per row of f");
    if (beta.len() != 1 || gamma.len() != 1 || one.len() != 1)
        throw std::length_error("permutation_leaves_indexed: beta, gamma and one are one ring element each");
    std::vector<uint64_t> coef;
    for (int row = 0; row < 2; row++)
        for (const RqNTTVec *c : {&one, &gamma, &gamma, &beta}) coef.insert(coef.end(), c->words().begin(), c->words().end());
    auto outs = lincomb_index(cfg, {&f}, {IndexColumn::progression(id_start), IndexColumn::stored(sigma_idx)}, coef, {0xBu, 0xDu}, f.size() / w);
    return {std::move(outs[0]), std::move(outs[1])};
}
// The reference's identity_permutation (polynomials/multilinear_polynomial.rs:79-89): R::from(0), .., R::from(num_chunks 2^num_vars - 1)
inline std::vector<uint64_t> identity_permutation(const CyclotomicConfig &cfg, size_t num_vars, size_t num_chunks, const RqNTTVec &one) {
    return from_u64(cfg, IndexColumn::progression(0), num_chunks << num_vars, one.words());
}
// identity_permutation_mles (:91-105): chunk i holds R::from(i 2^num_vars + e)
inline std::vector<DenseMultilinearExtension> identity_permutation_mles(const CyclotomicConfig &cfg, size_t num_vars, size_t num_chunks,
                                                                        const RqNTTVec &one) {
    std::vector<DenseMultilinearExtension> out;
    for (size_t i = 0; i < num_chunks; i++)
        out.emplace_back(cfg, num_vars, from_u64(cfg, IndexColumn::progression((uint64_t)i << num_vars), (size_t)1 << num_vars, one.words()));
    return out;
}

// The layer claim of a tree as an object that owns its operands: the halves of the layer below, the polynomial over them and the
// EqSumCheck of eq(z, .) times it (VirtualPolynomial refers to its MLEs, so they live here).
class LayerClaim {
public:
    LayerClaim(const CyclotomicConfig &cfg, std::vector<DenseMultilinearExtension> halves, const RqNTTVec &z, const RqNTTVec *lam)
        : halves_(std::move(halves)), g_(cfg, halves_.at(0).num_vars()) {
        if (halves_.size() == 2) {
            g_.add_mle_list({&halves_[0], &halves_[1]});
        } else {  // {p_lo, p_hi, q_lo, q_hi}: p_lo q_hi + p_hi q_lo + lam q_lo q_hi
            g_.add_mle_list({&halves_[0], &halves_[3]});
            g_.add_mle_list({&halves_[1], &halves_[2]});
            g_.add_mle_list({&halves_[2], &halves_[3]}, lam);
        }
        check_.emplace(g_, z, SR_MLE_TRAILING);
    }
    LayerClaim(const LayerClaim &) = delete;
    LayerClaim &operator=(const LayerClaim &) = delete;
    EqSumCheck &sumcheck() { return *check_; }

private:
    std::vector<DenseMultilinearExtension> halves_;
    VirtualPolynomial g_;
    std::optional<EqSumCheck> check_;
};

// Two ProductTrees in trailing order over the numerator and denominator leaves of a permutation (multiset-equality) argument
class PermutationCheck {
public:
    PermutationCheck(CyclotomicConfig cfg, std::vector<uint64_t> num_leaf_words, std::vector<uint64_t> den_leaf_words, size_t num_vars)
        : cfg_(cfg), num_(cfg, std::move(num_leaf_words), num_vars, SR_MLE_TRAILING), den_(cfg, std::move(den_leaf_words), num_vars, SR_MLE_TRAILING) {}
    const ProductTree &num() const { return num_; }
    const ProductTree &den() const { return den_; }
    std::pair<RqNTTVec, RqNTTVec> roots() const { return {num_.root(), den_.root()}; }
    bool holds() const { return num_.root().words() == den_.root().words(); }
    // side 0: the numerators, 1: the denominators; z: num_vars - k ring elements
    std::unique_ptr<LayerClaim> layer_claim(int side, size_t k, const RqNTTVec &z) const {
        const auto h = (side == 0 ? num_ : den_).halves(k);
        return std::make_unique<LayerClaim>(cfg_, std::vector<DenseMultilinearExtension>{h.first, h.second}, z, nullptr);
    }

private:
    CyclotomicConfig cfg_;
    ProductTree num_, den_;
};

// Two FractionTrees in trailing order of a logUp lookup: the witness side sums 1 / witness_q[i] (no stored numerators), the table side
// multiplicities[j] / table_q[j]; the multiplicities are ring elements supplied by the caller.  holds(): P_w Q_t == P_t Q_w, a
// polynomial identity in the challenge that needs no inverse and excludes no challenge.
class LookupCheck {
public:
    LookupCheck(CyclotomicConfig cfg, std::vector<uint64_t> witness_q, std::vector<uint64_t> table_q, std::vector<uint64_t> multiplicities,
                size_t num_vars_w, size_t num_vars_t)
        : cfg_(cfg), witness_(cfg, std::move(witness_q), num_vars_w, SR_MLE_TRAILING),
          table_(cfg, std::move(multiplicities), std::move(table_q), num_vars_t, SR_MLE_TRAILING) {}
    // The check with its multiplicities counted from indices: indices[i] is the table row that witness row i was taken from; the
    // numerators of the table side are R::from(count[j]) (sr_index_count, then from_u64).  Throws on an index beyond the table.
    static LookupCheck from_indices(CyclotomicConfig cfg, std::vector<uint64_t> witness_q, std::vector<uint64_t> table_q,
                                    const std::vector<uint64_t> &indices, size_t num_vars_w, size_t num_vars_t, const RqNTTVec &one) {
        const size_t rows = table_q.size() / cfg.words_per_elem();
        std::vector<uint64_t> mult = from_u64(cfg, IndexColumn::stored(index_count(cfg, indices, rows)), rows, one.words());
        return LookupCheck(cfg, std::move(witness_q), std::move(table_q), std::move(mult), num_vars_w, num_vars_t);
    }
    const FractionTree &witness() const { return witness_; }
    const FractionTree &table() const { return table_; }
    bool holds() const {
        const auto rw = witness_.root(), rt = table_.root();
        return (rw.first * rt.second).words() == (rt.first * rw.second).words();
    }
    // side 0: the witness, 1: the table; z: num_vars - k ring elements; lam: one ring element
    std::unique_ptr<LayerClaim> layer_claim(int side, size_t k, const RqNTTVec &z, const RqNTTVec &lam) const {
        return std::make_unique<LayerClaim>(cfg_, (side == 0 ? witness_ : table_).halves(k), z, &lam);
    }

private:
    CyclotomicConfig cfg_;
    FractionTree witness_, table_;
};

// SparseMultilinearExtension<RqNTT> of crates/poly (src/mle/sparse.rs): the stored evaluations as ascending indices and their values
// in CRT/NTT form, the iteration order of the reference's BTreeMap.  Stored zeros are kept.  Host buffers over sr_smle_fix_variables;
// rand, relabel, Add / Sub of two sparse MLEs and ark-serialize are not mirrored.  Throws where the reference asserts.
class SparseMultilinearExtension {
public:
    SparseMultilinearExtension(CyclotomicConfig cfg, size_t num_vars, std::vector<uint64_t> indices, std::vector<uint64_t> value_words)
        : cfg_(std::move(cfg)), nv_(num_vars), idx_(std::move(indices)), w_(std::move(value_words)) {
        if (w_.size() != idx_.size() * cfg_.words_per_elem()) throw std::length_error("one value per index");
        std::vector<uint64_t> keys(idx_.size()), seg(idx_.size() + 1);
        size_t n = 0;
        CyclotomicConfig::check(sr_smle_fix_pattern(idx_.data(), idx_.size(), nv_, 0, keys.data(), seg.data(), &n), "SparseMultilinearExtension");
    }
    // sparse.rs:125-134: a dense slice, entry i at index i
    static SparseMultilinearExtension from_slice(size_t num_vars, const RqNTTVec &v) {
        std::vector<uint64_t> idx(v.len());
        for (size_t i = 0; i < idx.size(); i++) idx[i] = i;
        return SparseMultilinearExtension(v.config(), num_vars, std::move(idx), v.words());
    }
    // sparse.rs:97-115 on a CSR triple with ascending columns in every row: index = row * next_pow2(ncols) + col
    static SparseMultilinearExtension from_matrix(const RqNTTVec &vals, const std::vector<uint32_t> &cols, const std::vector<uint64_t> &row_ptr,
                                                  size_t nrows, size_t ncols) {
        auto np2 = [](size_t n) { size_t p = 1; while (p < n) p <<= 1; return p; };
        const size_t n_cols = np2(ncols);
        size_t nv = 0;
        while (((size_t)1 << nv) < np2(nrows) * n_cols) nv++;
        std::vector<uint64_t> idx;
        for (size_t r = 0; r < nrows; r++)
            for (uint64_t j = row_ptr[r]; j < row_ptr[r + 1]; j++) idx.push_back(r * n_cols + cols[j]);
        return SparseMultilinearExtension(vals.config(), nv, std::move(idx), vals.words());
    }
    size_t num_vars() const { return nv_; }
    size_t len() const { return idx_.size(); }
    const std::vector<uint64_t> &indices() const { return idx_; }
    const std::vector<uint64_t> &words() const { return w_; }

    void fix_variables(const RqNTTVec &partial_point) { *this = fixed_variables(partial_point); }  // sparse.rs:170-207
    SparseMultilinearExtension fixed_variables(const RqNTTVec &partial_point) const {               // sparse.rs:209-213
        if (partial_point.len() > nv_) throw std::length_error("invalid partial point dimension");
        std::vector<uint64_t> out(w_.size()), keys(idx_.size());
        size_t n = 0;
        const uint64_t dummy = 0;
        CyclotomicConfig::check(sr_smle_fix_variables(cfg_.raw(), out.data(), keys.data(), &n, w_.data(), idx_.data(), idx_.size(), nv_,
                                                      partial_point.len() ? partial_point.words().data() : &dummy, partial_point.len()),
                                "sr_smle_fix_variables");
        out.resize(n * cfg_.words_per_elem());
        keys.resize(n);
        return SparseMultilinearExtension(cfg_, nv_ - partial_point.len(), std::move(keys), std::move(out));
    }
    // sparse.rs:53-56; an MLE with no stored entry evaluates to zero() (sparse.rs:359-365)
    RqNTTVec evaluate(const RqNTTVec &point) const {
        if (point.len() != nv_) throw std::length_error("evaluate: the point must have num_vars entries");
        SparseMultilinearExtension f = fixed_variables(point);
        return RqNTTVec(cfg_, f.len() ? f.w_ : std::vector<uint64_t>(cfg_.words_per_elem(), 0));
    }
    RqNTTVec to_evaluations() const {  // all 2^num_vars elements, the stored ones scattered
        const size_t w = cfg_.words_per_elem();
        std::vector<uint64_t> all(w << nv_, 0);
        for (size_t j = 0; j < idx_.size(); j++) std::copy(w_.begin() + j * w, w_.begin() + (j + 1) * w, all.begin() + idx_[j] * w);
        return RqNTTVec(cfg_, std::move(all));
    }

private:
    CyclotomicConfig cfg_;
    size_t nv_;
    std::vector<uint64_t> idx_, w_;
};

// `iter.fold(Self::one(), |acc, x| acc * x)` with the ring product = icrt(product(crt(x_i))): the CRT is a ring isomorphism
inline RqPolyVec RqPolyVec::product() const {
    return RqPolyVec(*this).elementwise_crt().product().elementwise_icrt();
}
inline RqNTTVec RqPolyVec::elementwise_crt() && {
    CyclotomicConfig::check(sr_ntt_fwd_batch(cfg_.raw(), w_.data(), len()), "elementwise_crt");
    return RqNTTVec(cfg_, std::move(w_));
}

// GadgetDecompose for &[R] / Vec<R> (balanced_decomposition/mod.rs:163-175, 192-198): len * padding_size elements, digit j of
// element e at index e * padding_size + j.  The reference panics on basis 0, 1 or odd and when padding_size digits do not
// suffice; std::runtime_error here.
typedef unsigned __int128 u128;  // the reference's basis type (decompose_balanced_in_place(v, b: u128, ..), mod.rs:62)
inline RqPolyVec gadget_decompose(const RqPolyVec &v, u128 b, size_t padding_size) {
    const CyclotomicConfig &cfg = v.config();
    std::vector<uint64_t> out(v.len() * padding_size * cfg.words_per_elem());
    std::vector<uint64_t> dummy(1);
    CyclotomicConfig::check(sr_decompose_balanced_batch_wide(cfg.raw(), out.empty() ? dummy.data() : out.data(),
                                                             v.words().empty() ? dummy.data() : v.words().data(), (uint64_t)b,
                                                             (uint64_t)(b >> 64), padding_size, v.len()),
                            "gadget_decompose");
    return RqPolyVec(cfg, std::move(out));
}
// GadgetRecompose (mod.rs:177-189, 200-206): len / padding_size elements
inline RqPolyVec gadget_recompose(const RqPolyVec &digits, u128 b, size_t padding_size) {
    const CyclotomicConfig &cfg = digits.config();
    if (padding_size == 0 || digits.len() % padding_size) throw std::length_error("length is not a multiple of padding_size");
    const size_t n = digits.len() / padding_size;
    std::vector<uint64_t> out(n * cfg.words_per_elem());
    std::vector<uint64_t> dummy(1);
    CyclotomicConfig::check(sr_recompose_batch_wide(cfg.raw(), out.empty() ? dummy.data() : out.data(),
                                                    digits.words().empty() ? dummy.data() : digits.words().data(), (uint64_t)b,
                                                    (uint64_t)(b >> 64), padding_size, n),
                            "gadget_recompose");
    return RqPolyVec(cfg, std::move(out));
}
// DecomposeToVec for &[R] / Vec<R> (mod.rs:119-161): one Vec<R> of padding_size digits per element of v
inline std::vector<RqPolyVec> decompose_to_vec(const RqPolyVec &v, u128 b, size_t padding_size) {
    const CyclotomicConfig &cfg = v.config();
    const RqPolyVec all = gadget_decompose(v, b, padding_size);   // digit j of element e at e * padding_size + j
    const size_t w = cfg.words_per_elem();
    std::vector<RqPolyVec> out;
    out.reserve(v.len());
    for (size_t e = 0; e < v.len(); e++)
        out.emplace_back(cfg, std::vector<uint64_t>(all.words().begin() + e * padding_size * w, all.words().begin() + (e + 1) * padding_size * w));
    return out;
}

// Cyclotomic::rot (traits.rs:54-66): every element of the batch times X modulo the ring, in place
inline void rot(RqPolyVec &v) {
    if (v.len() == 0) return;
    CyclotomicConfig::check(sr_rot_batch(v.config().raw(), v.element(0), v.len()), "rot");
}
// Rotation / into_rot_iter (traits.rs:68-91): an endless iterator x, X x, X^2 x, ... (next() returns the current value, then rotates)
class Rotation {
public:
    explicit Rotation(RqPolyVec curr) : curr_(std::move(curr)) {}
    RqPolyVec next() {
        RqPolyVec out = curr_;
        rot(curr_);
        return out;
    }

private:
    RqPolyVec curr_;
};
inline Rotation into_rot_iter(RqPolyVec v) { return Rotation(std::move(v)); }

// GadgetDecompose / GadgetRecompose for &[(R, usize)] (mod.rs:208-275): one sparse row of (element, column) pairs
using SparseRow = std::vector<std::pair<std::vector<uint64_t>, size_t>>;
inline SparseRow sparse_row_gadget_decompose(const CyclotomicConfig &cfg, const SparseRow &row, u128 b, size_t padding_size) {
    const size_t w = cfg.words_per_elem();
    std::vector<uint64_t> flat;
    for (const auto &e : row) {
        if (e.first.size() != w) throw std::length_error("Wrong length");
        flat.insert(flat.end(), e.first.begin(), e.first.end());
    }
    const RqPolyVec digits = gadget_decompose(RqPolyVec(cfg, std::move(flat)), b, padding_size);
    SparseRow out;
    for (size_t i = 0; i < row.size(); i++)
        for (size_t j = 0; j < padding_size; j++) {
            const uint64_t *d = digits.words().data() + (i * padding_size + j) * w;
            bool zero = true;
            for (size_t q = 0; q < w && zero; q++) zero = d[q] == 0;
            if (!zero) out.emplace_back(std::vector<uint64_t>(d, d + w), row[i].second * padding_size + j);  // "Maintain full sparsity"
        }
    return out;
}
inline SparseRow sparse_row_gadget_recompose(const CyclotomicConfig &cfg, const SparseRow &row, u128 b, size_t padding_size) {
    if (padding_size == 0) throw std::length_error("padding_size is zero");
    const size_t w = cfg.words_per_elem();
    // consecutive entries with the same index / padding_size form one chunk (mod.rs:241-256); missing digits are zero
    std::vector<size_t> index;
    std::vector<uint64_t> flat;
    for (size_t i = 0; i < row.size(); i++) {
        const size_t idx = row[i].second / padding_size;
        if (i == 0 || idx != row[i - 1].second / padding_size) {
            index.push_back(idx);
            flat.resize(flat.size() + padding_size * w, 0);
        }
        if (row[i].first.size() != w) throw std::length_error("Wrong length");
        std::copy(row[i].first.begin(), row[i].first.end(), flat.end() - padding_size * w + (row[i].second % padding_size) * w);
    }
    const RqPolyVec vals = gadget_recompose(RqPolyVec(cfg, std::move(flat)), b, padding_size);
    SparseRow out;
    for (size_t i = 0; i < index.size(); i++)
        out.emplace_back(std::vector<uint64_t>(vals.words().begin() + i * w, vals.words().begin() + (i + 1) * w), index[i]);
    return out;
}

// Matrix<R> in coefficient form (the decompositions work coefficient-wise): GadgetDecompose / GadgetRecompose for Matrix<R>
// (mod.rs:276-313): n x m -> n x (k m), row by row; entry (r, c) -> (r, c k .. c k + k - 1)
class MatrixPoly {
public:
    MatrixPoly(CyclotomicConfig cfg, size_t nrows, size_t ncols, std::vector<uint64_t> words)
        : cfg_(std::move(cfg)), nrows_(nrows), ncols_(ncols), w_(std::move(words)) {
        if (w_.size() != nrows_ * ncols_ * cfg_.words_per_elem()) throw std::length_error("Wrong length");
    }
    size_t nrows() const { return nrows_; }
    size_t ncols() const { return ncols_; }
    const std::vector<uint64_t> &words() const { return w_; }
    bool operator==(const MatrixPoly &o) const { return nrows_ == o.nrows_ && ncols_ == o.ncols_ && w_ == o.w_; }
    MatrixPoly gadget_decompose(u128 b, size_t padding_size) const {   // row-major storage: the flat batch IS row after row
        RqPolyVec d = stark_rings::gadget_decompose(RqPolyVec(cfg_, w_), b, padding_size);
        return MatrixPoly(cfg_, nrows_, ncols_ * padding_size, std::move(d).into_words());
    }
    MatrixPoly gadget_recompose(u128 b, size_t padding_size) const {
        if (padding_size == 0 || ncols_ % padding_size) throw std::length_error("ncols is not a multiple of padding_size");
        RqPolyVec r = stark_rings::gadget_recompose(RqPolyVec(cfg_, w_), b, padding_size);
        return MatrixPoly(cfg_, nrows_, ncols_ / padding_size, std::move(r).into_words());
    }

private:
    CyclotomicConfig cfg_;
    size_t nrows_, ncols_;
    std::vector<uint64_t> w_;
};
// SparseMatrix<R> in coefficient form: GadgetDecompose / GadgetRecompose for SparseMatrix<R> (mod.rs:315-352)
class SparseMatrixPoly {
public:
    SparseMatrixPoly(CyclotomicConfig cfg, size_t nrows, size_t ncols, std::vector<SparseRow> coeffs)
        : cfg_(std::move(cfg)), nrows_(nrows), ncols_(ncols), coeffs_(std::move(coeffs)) {
        if (coeffs_.size() != nrows_) throw std::length_error("Wrong length");
    }
    size_t nrows() const { return nrows_; }
    size_t ncols() const { return ncols_; }
    const std::vector<SparseRow> &coeffs() const { return coeffs_; }
    SparseMatrixPoly gadget_decompose(u128 b, size_t padding_size) const {
        std::vector<SparseRow> rows;
        for (const auto &r : coeffs_) rows.push_back(sparse_row_gadget_decompose(cfg_, r, b, padding_size));
        return SparseMatrixPoly(cfg_, nrows_, ncols_ * padding_size, std::move(rows));
    }
    SparseMatrixPoly gadget_recompose(u128 b, size_t padding_size) const {
        std::vector<SparseRow> rows;
        for (const auto &r : coeffs_) rows.push_back(sparse_row_gadget_recompose(cfg_, r, b, padding_size));
        return SparseMatrixPoly(cfg_, nrows_, ncols_ / padding_size, std::move(rows));
    }

private:
    CyclotomicConfig cfg_;
    size_t nrows_, ncols_;
    std::vector<SparseRow> coeffs_;
};

// One context per GPU of a node from ONE process (what a Rust host that drives all 8 GPUs binds): sr_ctx_create_group builds the
// twiddle block on device_ids[0] and peer-copies it to the others (the only inter-GPU traffic of the path); shard_range is the
// contiguous, balanced batch partition of SURVEY 8e (the first batch % n parts get one element more).
class ContextGroup {
public:
    ContextGroup(sr_ring ring, int log2_degree, const std::vector<int> &device_ids, const sr_plan *plan = nullptr) {
        std::vector<sr_ctx *> raw(device_ids.size(), nullptr);
        CyclotomicConfig::check(sr_ctx_create_group(ring, log2_degree, device_ids.data(), (int)device_ids.size(), plan, raw.data()),
                                "sr_ctx_create_group");
        for (sr_ctx *c : raw) cfgs_.emplace_back(ring, c);
    }
    size_t size() const { return cfgs_.size(); }
    const CyclotomicConfig &operator[](size_t i) const { return cfgs_.at(i); }
    // elements [first, first + count) of a batch belong to context i
    std::pair<size_t, size_t> shard_range(size_t batch, size_t i) const {
        size_t first = 0, count = 0;
        CyclotomicConfig::check(sr_shard_range(batch, (int)cfgs_.size(), (int)i, &first, &count), "sr_shard_range");
        return {first, count};
    }

private:
    std::vector<CyclotomicConfig> cfgs_;
};

// Matrix<RqNTT> (crates/linear_algebra/src/matrix.rs): nrows x ncols ring elements in CRT/NTT form, row-major, flat
class MatrixNTT {
public:
    MatrixNTT(CyclotomicConfig cfg, size_t nrows, size_t ncols, std::vector<uint64_t> words)
        : cfg_(std::move(cfg)), nrows_(nrows), ncols_(ncols), w_(std::move(words)) {
        if (w_.size() != nrows_ * ncols_ * cfg_.words_per_elem()) throw std::length_error("Wrong length");
    }
    size_t nrows() const { return nrows_; }
    size_t ncols() const { return ncols_; }
    const std::vector<uint64_t> &words() const { return w_; }
    // matrix.rs:168-178: None when ncols != v.len()
    std::optional<RqNTTVec> checked_mul_vec(const RqNTTVec &v) const {
        if (v.len() != ncols_) return std::nullopt;
        std::vector<uint64_t> y(nrows_ * cfg_.words_per_elem());
        std::vector<uint64_t> dummy(1);
        CyclotomicConfig::check(sr_matvec_ntt(cfg_.raw(), y.empty() ? dummy.data() : y.data(), w_.empty() ? dummy.data() : w_.data(),
                                              v.words().empty() ? dummy.data() : v.words().data(), nrows_, ncols_),
                                "Matrix * vec");
        return RqNTTVec(cfg_, std::move(y));
    }
    RqNTTVec try_mul_vec(const RqNTTVec &v) const {  // matrix.rs:180-183: AlgebraError::DifferentLengths
        auto r = checked_mul_vec(v);
        if (!r) throw std::length_error("DifferentLengths");
        return std::move(*r);
    }
    std::optional<MatrixNTT> checked_mul_mat(const MatrixNTT &m) const {  // matrix.rs:148-166
        if (ncols_ != m.nrows_) return std::nullopt;
        std::vector<uint64_t> y(nrows_ * m.ncols_ * cfg_.words_per_elem());
        std::vector<uint64_t> dummy(1);
        CyclotomicConfig::check(sr_matmul_ntt(cfg_.raw(), y.empty() ? dummy.data() : y.data(), w_.empty() ? dummy.data() : w_.data(),
                                              m.w_.empty() ? dummy.data() : m.w_.data(), nrows_, ncols_, m.ncols_),
                                "Matrix * Matrix");
        return MatrixNTT(cfg_, nrows_, m.ncols_, std::move(y));
    }
    // Transpose for Matrix<R> (ops.rs:36-44).  The reference transposes vals but copies nrows and ncols UNSWAPPED; the result here
    // reports the shape of its data, ncols x nrows.
    MatrixNTT transpose() const {
        std::vector<uint64_t> y(w_.size());
        std::vector<uint64_t> dummy(1);
        CyclotomicConfig::check(sr_transpose(cfg_.raw(), y.empty() ? dummy.data() : y.data(), w_.empty() ? dummy.data() : w_.data(), nrows_, ncols_),
                                "Matrix::transpose");
        return MatrixNTT(cfg_, ncols_, nrows_, std::move(y));
    }
    MatrixNTT &operator*=(const RqNTTVec &r) {  // MulAssign<&R> for Matrix<R> (matrix.rs:207-211): every entry *= r
        if (r.len() != 1) throw std::length_error("Matrix *= &R: the multiplier is not one ring element");
        std::vector<uint64_t> dummy(1);
        CyclotomicConfig::check(sr_mul_elem_batch(cfg_.raw(), w_.empty() ? dummy.data() : w_.data(), r.words().data(), nrows_ * ncols_), "Matrix *= &R");
        return *this;
    }

private:
    CyclotomicConfig cfg_;
    size_t nrows_, ncols_;
    std::vector<uint64_t> w_;
};

// SparseMatrix<RqNTT> (crates/linear_algebra/src/sparse_matrix.rs:17-22): coeffs[r] = the stored (element, column) pairs of row r
class SparseMatrixNTT {
public:
    using Entry = std::pair<std::vector<uint64_t>, size_t>;
    SparseMatrixNTT(CyclotomicConfig cfg, size_t nrows, size_t ncols, std::vector<std::vector<Entry>> coeffs)
        : cfg_(std::move(cfg)), nrows_(nrows), ncols_(ncols) {
        if (coeffs.size() != nrows_) throw std::length_error("Wrong length");
        row_ptr_.assign(nrows_ + 1, 0);
        for (size_t r = 0; r < nrows_; r++) {
            row_ptr_[r + 1] = row_ptr_[r] + coeffs[r].size();
            for (auto &e : coeffs[r]) {
                if (e.first.size() != cfg_.words_per_elem()) throw std::length_error("Wrong length");
                vals_.insert(vals_.end(), e.first.begin(), e.first.end());
                cols_.push_back((uint32_t)e.second);
                if (e.second > 0xFFFFFFFFull) throw std::length_error("column index does not fit 32 bits");
            }
        }
    }
    size_t nrows() const { return nrows_; }
    size_t ncols() const { return ncols_; }
    std::optional<RqNTTVec> checked_mul_vec(const RqNTTVec &v) const {  // sparse_matrix.rs:201-211
        if (v.len() != ncols_) return std::nullopt;
        std::vector<uint64_t> y(nrows_ * cfg_.words_per_elem());
        std::vector<uint64_t> dummy(1);
        std::vector<uint32_t> dummy32(1);
        CyclotomicConfig::check(sr_spmv_ntt(cfg_.raw(), y.empty() ? dummy.data() : y.data(), vals_.empty() ? dummy.data() : vals_.data(),
                                            cols_.empty() ? dummy32.data() : cols_.data(), row_ptr_.data(),
                                            v.words().empty() ? dummy.data() : v.words().data(), nrows_, ncols_),
                                "SparseMatrix * vec");
        return RqNTTVec(cfg_, std::move(y));
    }
    RqNTTVec try_mul_vec(const RqNTTVec &v) const {  // sparse_matrix.rs:213-216
        auto r = checked_mul_vec(v);
        if (!r) throw std::length_error("DifferentLengths");
        return std::move(*r);
    }
    // the rows as the constructor takes them: coeffs()[r] = the stored (element, column) pairs of row r
    std::vector<std::vector<Entry>> coeffs() const {
        const size_t w = cfg_.words_per_elem();
        std::vector<std::vector<Entry>> out(nrows_);
        for (size_t r = 0; r < nrows_; r++)
            for (uint64_t t = row_ptr_[r]; t < row_ptr_[r + 1]; t++)
                out[r].emplace_back(std::vector<uint64_t>(vals_.begin() + t * w, vals_.begin() + (t + 1) * w), (size_t)cols_[t]);
        return out;
    }
    size_t nnz() const { return cols_.size(); }
    // Transpose for SparseMatrix<R> (ops.rs:46-62): row c of the result lists (value, original row) in ascending original row; the
    // rows of *this need not be sorted.  Throws where the reference panics (a column >= ncols).
    SparseMatrixNTT transpose() const {
        SparseMatrixNTT t(cfg_, ncols_, nrows_);
        t.vals_.resize(vals_.size());
        t.cols_.resize(cols_.size());
        std::vector<uint64_t> dummy(1);
        std::vector<uint32_t> dummy32(1);
        CyclotomicConfig::check(sr_sparse_transpose(cfg_.raw(), t.vals_.empty() ? dummy.data() : t.vals_.data(),
                                                    t.cols_.empty() ? dummy32.data() : t.cols_.data(), t.row_ptr_.data(),
                                                    vals_.empty() ? dummy.data() : vals_.data(), cols_.empty() ? dummy32.data() : cols_.data(),
                                                    row_ptr_.data(), nrows_, ncols_),
                                "SparseMatrix::transpose");
        return t;
    }
    // sparse_matrix.rs:219-275: None when ncols != m.nrows.  An entry is stored iff one of its products is non-zero (a stored entry may
    // itself be zero).  The reference's merge-join needs rows that ascend strictly in both operands; anything else throws.
    std::optional<SparseMatrixNTT> checked_mul_mat(const SparseMatrixNTT &m) const {
        if (ncols_ != m.nrows_) return std::nullopt;
        std::vector<uint64_t> dummy(1);
        std::vector<uint32_t> dummy32(1);
        const uint32_t *ac = cols_.empty() ? dummy32.data() : cols_.data(), *bc = m.cols_.empty() ? dummy32.data() : m.cols_.data();
        size_t n_out = 0, n_pairs = 0, kept = 0;
        CyclotomicConfig::check(sr_spgemm_pattern(ac, row_ptr_.data(), nrows_, ncols_, bc, m.row_ptr_.data(), m.ncols_, nullptr, nullptr, nullptr,
                                                  nullptr, nullptr, &n_out, &n_pairs),
                                "SparseMatrix * SparseMatrix");
        SparseMatrixNTT y(cfg_, nrows_, m.ncols_);
        y.vals_.resize(n_out * cfg_.words_per_elem());  // room for the structural entries; the dead ones are dropped by the call
        y.cols_.resize(n_out);
        CyclotomicConfig::check(sr_spgemm_ntt(cfg_.raw(), y.vals_.empty() ? dummy.data() : y.vals_.data(), y.cols_.empty() ? dummy32.data() : y.cols_.data(),
                                              y.row_ptr_.data(), &kept, vals_.empty() ? dummy.data() : vals_.data(), ac, row_ptr_.data(), nrows_, ncols_,
                                              m.vals_.empty() ? dummy.data() : m.vals_.data(), bc, m.row_ptr_.data(), m.ncols_),
                                "SparseMatrix * SparseMatrix");
        y.vals_.resize(kept * cfg_.words_per_elem());
        y.cols_.resize(kept);
        return y;
    }
    SparseMatrixNTT try_mul_mat(const SparseMatrixNTT &m) const {  // Mul<&SparseMatrix> (sparse_matrix.rs:293-301): DifferentLengths
        auto r = checked_mul_mat(m);
        if (!r) throw std::length_error("DifferentLengths");
        return std::move(*r);
    }
    SparseMatrixNTT &operator*=(const RqNTTVec &r) {  // MulAssign<&R> for SparseMatrix<R> (sparse_matrix.rs:303-307): every stored entry *= r
        if (r.len() != 1) throw std::length_error("SparseMatrix *= &R: the multiplier is not one ring element");
        std::vector<uint64_t> dummy(1);
        CyclotomicConfig::check(sr_mul_elem_batch(cfg_.raw(), vals_.empty() ? dummy.data() : vals_.data(), r.words().data(), cols_.size()),
                                "SparseMatrix *= &R");
        return *this;
    }

private:
    SparseMatrixNTT(CyclotomicConfig cfg, size_t nrows, size_t ncols) : cfg_(std::move(cfg)), nrows_(nrows), ncols_(ncols), row_ptr_(nrows + 1, 0) {}
    CyclotomicConfig cfg_;
    size_t nrows_, ncols_;
    std::vector<uint64_t> vals_, row_ptr_;
    std::vector<uint32_t> cols_;
};

// ---- CanonicalSerialize / CanonicalDeserialize (ark-serialize; Compress and Validate make no difference for these types) ----
// SymmetricMatrix<RqNTT> (crates/linear_algebra/src/symmetric_matrix.rs:14-92), packed: the reference's Vec<Vec<F>> rows (row i has
// i + 1 entries) flattened, entry (i, j) with j <= i is ring element i (i + 1) / 2 + j.  Host buffers over sr_gram_ntt /
// sr_symm_recompose; throws where the reference asserts.
class SymmetricMatrixNTT {
public:
    SymmetricMatrixNTT(CyclotomicConfig cfg, size_t n, std::vector<uint64_t> packed_words) : cfg_(std::move(cfg)), n_(n), w_(std::move(packed_words)) {
        if (w_.size() != n_ * (n_ + 1) / 2 * cfg_.words_per_elem()) throw std::length_error("SymmetricMatrixNTT: not n (n + 1) / 2 ring elements");
    }
    static SymmetricMatrixNTT zero(const CyclotomicConfig &cfg, size_t n) {  // symmetric_matrix.rs:24-28
        return SymmetricMatrixNTT(cfg, n, std::vector<uint64_t>(n * (n + 1) / 2 * cfg.words_per_elem(), 0));
    }
    // From<Vec<Vec<F>>> (symmetric_matrix.rs:17-22): row i must hold i + 1 elements
    static SymmetricMatrixNTT from_rows(const CyclotomicConfig &cfg, const std::vector<RqNTTVec> &rows) {
        std::vector<uint64_t> w;
        for (size_t i = 0; i < rows.size(); i++) {
            if (rows[i].len() != i + 1)
                throw std::length_error("cannot convert value: Vec<Vec<F>> to SymmetricMatrix<F>, row has wrong number of entries");
            w.insert(w.end(), rows[i].words().begin(), rows[i].words().end());
        }
        return SymmetricMatrixNTT(cfg, rows.size(), std::move(w));
    }
    // from_par_fn(n, |i, j| sum_t a[i][t] * a[j][t]) (symmetric_matrix.rs:76-90) for the n rows of m elements of `a` (row-major); the
    // inner-product closure is the caller's, not the reference's
    static SymmetricMatrixNTT gram(const RqNTTVec &a, size_t n, size_t m) {
        const CyclotomicConfig &cfg = a.config();
        if (a.len() != n * m) throw std::length_error("gram: the matrix does not hold n * m elements");
        std::vector<uint64_t> out(n * (n + 1) / 2 * cfg.words_per_elem());
        const uint64_t dummy = 0;
        uint64_t sink = 0;
        CyclotomicConfig::check(sr_gram_ntt(cfg.raw(), out.empty() ? &sink : out.data(), a.words().empty() ? &dummy : a.words().data(), n, m), "sr_gram_ntt");
        return SymmetricMatrixNTT(cfg, n, std::move(out));
    }
    size_t size() const { return n_; }                            // :31-34
    static size_t packed_index(size_t i, size_t j) { return j <= i ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i; }
    RqNTTVec at(size_t i, size_t j) const {                       // :36-44: (i, j) with j > i reads (j, i)
        if (i >= n_ || j >= n_) throw std::out_of_range("SymmetricMatrixNTT::at");
        const size_t w = cfg_.words_per_elem(), e = packed_index(i, j);
        return RqNTTVec(cfg_, std::vector<uint64_t>(w_.begin() + e * w, w_.begin() + (e + 1) * w));
    }
    RqNTTVec diag() const {                                       // :56-58: the n diagonal elements as one vector
        std::vector<uint64_t> d;
        for (size_t i = 0; i < n_; i++) {
            const RqNTTVec e = at(i, i);
            d.insert(d.end(), e.words().begin(), e.words().end());
        }
        return RqNTTVec(cfg_, std::move(d));
    }
    std::vector<RqNTTVec> rows() const {                          // :60-62
        std::vector<RqNTTVec> r;
        const size_t w = cfg_.words_per_elem();
        for (size_t i = 0; i < n_; i++) r.emplace_back(cfg_, std::vector<uint64_t>(w_.begin() + i * (i + 1) / 2 * w, w_.begin() + (i + 1) * (i + 2) / 2 * w));
        return r;
    }
    const std::vector<uint64_t> &words() const { return w_; }
    const CyclotomicConfig &config() const { return cfg_; }
    // balanced_decomposition/mod.rs:354-386: G^T * this * G for G = I_n (x) powers_of_basis
    SymmetricMatrixNTT recompose_left_right(const RqNTTVec &powers_of_basis) const {
        const size_t d = powers_of_basis.len();
        if (d == 0 || n_ % d) throw std::length_error("recompose_left_right_symmetric_matrix: the number of powers must divide the size");  // :365
        const size_t n = n_ / d;
        std::vector<uint64_t> out(n * (n + 1) / 2 * cfg_.words_per_elem());
        uint64_t sink = 0;
        CyclotomicConfig::check(sr_symm_recompose(cfg_.raw(), out.empty() ? &sink : out.data(), w_.empty() ? &sink : w_.data(), n, d,
                                                  powers_of_basis.words().data()),
                                "sr_symm_recompose");
        return SymmetricMatrixNTT(cfg_, n, std::move(out));
    }
    // {workspace elements, kernel launches} of the device forms (sr_gram_plan / sr_symm_recompose_plan)
    static std::pair<size_t, int> gram_plan(sr_ring ring, int log2_degree, size_t n, size_t m) {
        size_t work = 0;
        int launches = 0;
        CyclotomicConfig::check(sr_gram_plan(ring, log2_degree, n, m, &work, &launches), "sr_gram_plan");
        return {work, launches};
    }
    static std::pair<size_t, int> recompose_plan(sr_ring ring, int log2_degree, size_t n, size_t d) {
        size_t work = 0;
        int launches = 0;
        CyclotomicConfig::check(sr_symm_recompose_plan(ring, log2_degree, n, d, &work, &launches), "sr_symm_recompose_plan");
        return {work, launches};
    }

private:
    CyclotomicConfig cfg_;
    size_t n_;
    std::vector<uint64_t> w_;
};
inline SymmetricMatrixNTT recompose_left_right_symmetric_matrix(const SymmetricMatrixNTT &mat, const RqNTTVec &powers_of_basis) {
    return mat.recompose_left_right(powers_of_basis);
}

namespace wire_detail {
inline void put_u64(std::vector<uint8_t> &out, uint64_t v) {
    for (int i = 0; i < 8; i++) out.push_back((uint8_t)(v >> (8 * i)));
}
inline uint64_t get_u64(const std::vector<uint8_t> &in, size_t &pos) {
    if (pos + 8 > in.size()) throw std::runtime_error("deserialize: unexpected end of input");
    uint64_t v = 0;
    for (int i = 0; i < 8; i++) v |= (uint64_t)in[pos + i] << (8 * i);
    pos += 8;
    return v;
}
// the elements alone (what [Fp; D] / RqNTT serialise to, coeff_form.rs:157-163), appended to out
inline void put_elems(const CyclotomicConfig &cfg, std::vector<uint8_t> &out, const uint64_t *words, size_t n_elems) {
    if (!n_elems) return;
    const size_t at = out.size();
    out.resize(at + n_elems * cfg.wire_elem_bytes());
    CyclotomicConfig::check(sr_serialize_batch(cfg.raw(), out.data() + at, words, n_elems), "serialize");
}
inline std::vector<uint64_t> get_elems(const CyclotomicConfig &cfg, const uint8_t *bytes, size_t n_elems) {
    std::vector<uint64_t> w(n_elems * cfg.words_per_elem());
    if (n_elems) CyclotomicConfig::check(sr_deserialize_batch(cfg.raw(), w.data(), bytes, n_elems), "deserialize");
    return w;
}
}  // namespace wire_detail

// Vec<RqPoly> / Vec<RqNTT>: u64 length, then the elements
template <class V>
inline std::vector<uint8_t> serialize_compressed(const V &v) {
    std::vector<uint8_t> out;
    wire_detail::put_u64(out, v.len());
    wire_detail::put_elems(v.config(), out, v.words().data(), v.len());
    return out;
}
template <class V>
inline V deserialize_vec(const CyclotomicConfig &cfg, const std::vector<uint8_t> &in, size_t *pos_io = nullptr) {
    size_t pos = pos_io ? *pos_io : 0;
    const uint64_t n = wire_detail::get_u64(in, pos);
    if (n > (in.size() - pos) / cfg.wire_elem_bytes()) throw std::runtime_error("deserialize: unexpected end of input");
    V v(cfg, wire_detail::get_elems(cfg, in.data() + pos, n));
    pos += n * cfg.wire_elem_bytes();
    if (pos_io) *pos_io = pos;
    return v;
}
// Matrix<RqNTT> = Vec<Vec<RqNTT>> (matrix.rs:111-124)
inline std::vector<uint8_t> serialize_compressed(const MatrixNTT &m, const CyclotomicConfig &cfg) {
    std::vector<uint8_t> out;
    wire_detail::put_u64(out, m.nrows());
    for (size_t r = 0; r < m.nrows(); r++) {
        wire_detail::put_u64(out, m.ncols());
        wire_detail::put_elems(cfg, out, m.words().data() + r * m.ncols() * cfg.words_per_elem(), m.ncols());
    }
    return out;
}
// matrix.rs:132-144: ncols is the first row's length; ragged rows (which the reference accepts and trips over later) throw
inline MatrixNTT deserialize_matrix(const CyclotomicConfig &cfg, const std::vector<uint8_t> &in) {
    size_t pos = 0;
    const uint64_t nrows = wire_detail::get_u64(in, pos);
    uint64_t ncols = 0;
    std::vector<uint64_t> words;
    for (uint64_t r = 0; r < nrows; r++) {
        RqNTTVec row = deserialize_vec<RqNTTVec>(cfg, in, &pos);
        if (r == 0) ncols = row.len();
        if (row.len() != ncols) throw std::runtime_error("deserialize: ragged matrix rows");
        words.insert(words.end(), row.words().begin(), row.words().end());
    }
    return MatrixNTT(cfg, nrows, ncols, std::move(words));
}
// SparseMatrix<RqNTT>: nrows, ncols, Vec<Vec<(RqNTT, usize)>> (sparse_matrix.rs:158-175)
inline std::vector<uint8_t> serialize_compressed(const CyclotomicConfig &cfg, size_t nrows, size_t ncols,
                                                 const std::vector<std::vector<SparseMatrixNTT::Entry>> &coeffs) {
    std::vector<uint8_t> out;
    wire_detail::put_u64(out, nrows);
    wire_detail::put_u64(out, ncols);
    wire_detail::put_u64(out, coeffs.size());
    for (const auto &row : coeffs) {
        wire_detail::put_u64(out, row.size());
        for (const auto &e : row) {
            if (e.first.size() != cfg.words_per_elem()) throw std::length_error("Wrong length");
            wire_detail::put_elems(cfg, out, e.first.data(), 1);
            wire_detail::put_u64(out, e.second);
        }
    }
    return out;
}
struct SparseParts {
    size_t nrows, ncols;
    std::vector<std::vector<SparseMatrixNTT::Entry>> coeffs;
};
inline SparseParts deserialize_sparse(const CyclotomicConfig &cfg, const std::vector<uint8_t> &in) {  // sparse_matrix.rs:183-199
    size_t pos = 0;
    SparseParts s;
    s.nrows = wire_detail::get_u64(in, pos);
    s.ncols = wire_detail::get_u64(in, pos);
    const uint64_t nlists = wire_detail::get_u64(in, pos);
    for (uint64_t r = 0; r < nlists; r++) {
        const uint64_t n = wire_detail::get_u64(in, pos);
        std::vector<SparseMatrixNTT::Entry> row;
        for (uint64_t j = 0; j < n; j++) {
            if (pos + cfg.wire_elem_bytes() > in.size()) throw std::runtime_error("deserialize: unexpected end of input");
            std::vector<uint64_t> e = wire_detail::get_elems(cfg, in.data() + pos, 1);
            pos += cfg.wire_elem_bytes();
            const uint64_t col = wire_detail::get_u64(in, pos);
            row.emplace_back(std::move(e), (size_t)col);
        }
        s.coeffs.push_back(std::move(row));
    }
    return s;
}

// ---- monomial helpers (crates/ring/src/monomial.rs:17-93), coefficient form, one element each ----------------------------
namespace monomial_detail {
// ring element from signed small integers: each coefficient's standard form is c mod p, written as wire bytes (p - |c| needs
// the modulus: a negative coefficient is produced on the device as 0 - |c|)
inline RqPolyVec from_signed(const CyclotomicConfig &cfg, const std::vector<int64_t> &coeffs) {
    const size_t d = cfg.dimension(), w = cfg.wire_coeff_bytes();
    if (coeffs.size() != d) throw std::length_error("Wrong length");
    std::vector<uint8_t> pos_b(d * w, 0), neg_b(d * w, 0);
    for (size_t i = 0; i < d; i++) {
        const uint64_t mag = coeffs[i] < 0 ? (uint64_t)0 - (uint64_t)coeffs[i] : (uint64_t)coeffs[i];
        std::vector<uint8_t> &dst = coeffs[i] < 0 ? neg_b : pos_b;
        for (size_t b = 0; b < w && b < 8; b++) dst[i * w + b] = (uint8_t)(mag >> (8 * b));
        if (w < 8 && (mag >> (8 * w))) throw std::runtime_error("coefficient magnitude does not fit the field");
    }
    RqPolyVec pos(cfg, wire_detail::get_elems(cfg, pos_b.data(), 1));
    RqPolyVec neg(cfg, wire_detail::get_elems(cfg, neg_b.data(), 1));
    pos -= neg;
    return pos;
}
}  // namespace monomial_detail

inline RqPolyVec monomial(const CyclotomicConfig &cfg, size_t i, int64_t coeff) {   // monomial.rs:17-21; index past D panics there
    if (i >= cfg.dimension()) throw std::out_of_range("monomial: index outside the ring's dimension");
    std::vector<int64_t> c(cfg.dimension(), 0);
    c[i] = coeff;
    return monomial_detail::from_signed(cfg, c);
}
inline RqPolyVec zero_monomial(const CyclotomicConfig &cfg) { return RqPolyVec(cfg, std::vector<uint64_t>(cfg.words_per_elem(), 0)); }
inline RqPolyVec unit_monomial(const CyclotomicConfig &cfg, size_t i) { return monomial(cfg, i, 1); }
inline RqPolyVec psi(const CyclotomicConfig &cfg) {                                   // monomial.rs:36-49
    const size_t d = cfg.dimension();
    std::vector<int64_t> c(d, 0);
    for (size_t i = 1; i < d / 2; i++) {
        c[i] += (int64_t)i;
        c[d - i] -= (int64_t)i;
    }
    return monomial_detail::from_signed(cfg, c);
}
// a: the signed representative of the scalar (sign(a), center(a) = |a|)
inline RqPolyVec exp(const CyclotomicConfig &cfg, int64_t a) {                        // monomial.rs:56-66
    const uint64_t mag = a < 0 ? (uint64_t)0 - (uint64_t)a : (uint64_t)a;
    if (a >= 0) return unit_monomial(cfg, mag);
    if (mag > cfg.dimension()) throw std::out_of_range("monomial: index outside the ring's dimension");
    return unit_monomial(cfg, cfg.dimension() - mag);
}
inline RqPolyVec exp_signed(const CyclotomicConfig &cfg, int64_t a) {                 // monomial.rs:72-78
    const uint64_t mag = a < 0 ? (uint64_t)0 - (uint64_t)a : (uint64_t)a;
    return monomial(cfg, mag, a < 0 ? -1 : 1);
}
// Ok(()) -> true, MonomialError::RangeCheck -> false                                  // monomial.rs:84-93
inline bool psi_range_check(const CyclotomicConfig &cfg, int64_t a) {
    RqPolyVec prod = psi(cfg) * exp(cfg, a);
    std::vector<int64_t> want(cfg.dimension(), 0);
    want[0] = a;
    RqPolyVec a_elem = monomial_detail::from_signed(cfg, want);
    for (int l = 0; l < cfg.limbs(); l++)
        if (prod.words()[l] != a_elem.words()[l]) return false;   // ct(): coefficient 0, compared in the memory image
    return true;
}

// Flatten (flatten.rs:10-34): the flat coefficient vector IS the batch's storage; both directions are moves.
template <class V>
inline std::vector<uint64_t> flatten_to_coeffs(V &&vec) {
    return std::move(vec).into_words();
}
template <class V>
inline std::optional<V> promote_from_coeffs(const CyclotomicConfig &cfg, std::vector<uint64_t> coeffs) {
    if (coeffs.size() % cfg.words_per_elem() != 0) return std::nullopt;  // flatten.rs:22-24
    return V(cfg, std::move(coeffs));
}

}  // namespace stark_rings
