/* stark_rings_hip.h -- C ABI of the MI355X (gfx950) backend for stark-rings' CRT/NTT hot path.
 *
 * Drop-in boundary: these entry points are what a Rust `extern "C"` block in crates/ring would
 * bind to replace the CPU implementations behind `CyclotomicConfig<N>`
 * (crates/ring/src/cyclotomic_ring/ring_config.rs:11-35) at BATCH granularity, i.e. at the seam
 * the reference itself exposes through `CRT::elementwise_crt` / `ICRT::elementwise_icrt`
 * (crt.rs:10-25, 34-49), `Flatten` (flatten.rs:10-34) and `into_raw_parts` (utils.rs:3-6).
 * INTEGRATION.md shows the Rust-side shim.
 *
 * Data layout (identical to the reference's, no padding, 8-byte aligned):
 *   a batch is `batch` ring elements, element-major; each element is D coefficients (or CRT
 *   slots, same bytes); each coefficient is N little-endian u64 limbs holding the ark-ff 0.4.2
 *   Montgomery residue a * 2^(64N) mod p, canonical in [0, p).  N = 1 (Goldilocks, BabyBear --
 *   BabyBear really is an Fp64 in the reference: babybear/mod.rs:25), N = 4 (Starknet prime).
 *
 * Ownership: the caller owns every buffer; transforms are in place; the library never frees or
 * reallocates caller memory.  A context owns twiddle tables, constants and staging scratch.
 *
 * Errors: every call returns 0 on success, non-zero otherwise (SR_E_*).  The reference panics on
 * a wrong length (goldilocks/ntt.rs:136, stark_prime/ntt.rs:122, coeff_form.rs:39); the Rust shim
 * turns a non-zero status into panic! to match.  `sr_last_error_string()` gives the reason.
 *
 * Threading: a context is bound to one HIP device and serialises its own calls with a mutex;
 * use one context per thread (or per stream) for concurrency.  `*_dev` calls are asynchronous
 * on the given stream.
 *
 * There is NO CPU fallback: if no HIP device is present every compute call fails with
 * SR_E_NO_DEVICE.
 */
#ifndef STARK_RINGS_HIP_H
#define STARK_RINGS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ring identifiers */
enum sr_ring {
    /* generalised power-of-two configs  Fp[X]/(X^D+1), D = 2^log2_degree, fully split
     * (BaseCRTField = Fq, CRT_FIELD_EXTENSION_DEGREE = 1); algorithm and slot order of
     * stark_prime/ntt.rs:121-346 with psi = generator^((p-1)/2D).  SR_RING_STARK_POW2 with
     * log2_degree = 4 IS the reference's stark_prime ring (StarkRingConfig, stark_prime/mod.rs:34-68). */
    SR_RING_GOLDILOCKS_POW2 = 0,
    SR_RING_BABYBEAR_POW2 = 1,
    SR_RING_STARK_POW2 = 2,
    /* reference-native partially-splitting rings (log2_degree ignored) */
    SR_RING_GOLDILOCKS_24 = 3, /* X^24-X^12+1, 8 x Fq3: GoldilocksRingConfig, goldilocks/mod.rs:69-119 */
    SR_RING_BABYBEAR_72 = 4,   /* X^72-X^36+1, 8 x Fq9: BabyBearRingConfig,  babybear/mod.rs:81-131 */
    SR_RING_FROG_16 = 5        /* X^16+1 over p = 15912092521325583641, 4 x Fq4: FrogRingConfig, frog_ring/mod.rs:62-107
                                  ("next" row 4; crt/icrt frog_ring/ntt.rs:114-200, one u64 Montgomery limb per coefficient) */
};

enum sr_status {
    SR_OK = 0,
    SR_E_INVALID = 1,   /* null pointer, bad ring id, bad degree, bad length */
    SR_E_NO_DEVICE = 2, /* no HIP device / device index out of range */
    SR_E_HIP = 3,       /* a HIP runtime call failed */
    SR_E_ALLOC = 4,
    SR_E_UNSUPPORTED = 5 /* the entry point exists but this build does not provide it (sr_selftest_rep_counters outside the checking build) */
};

typedef struct sr_ctx sr_ctx;

/* ---- context -------------------------------------------------------------------------- */
/* Creates a context on HIP device `device` and builds its twiddle tables there.
 * Threading (the reference's types are Send + Sync): every entry point may be called from any thread; calls on one
 * context are serialised by the context (host-pointer calls run to completion, device-pointer calls enqueue and return).
 * Device-pointer calls on different streams of one context may overlap on the GPU; the context orders its own shared scratch
 * between streams with an event.  Contexts are independent of each other. */
int sr_ctx_create(int ring, int log2_degree, int device, sr_ctx **out);
/* The same with an explicit kernel plan, fixed for the life of the context (the library itself reads no environment
 * variable: a getenv racing a setenv in another thread of a Send + Sync host would be a data race).  plan == NULL or an
 * all-zero plan = the measured-fastest defaults, i.e. sr_ctx_create.  The alternative plans compute the same function bit
 * for bit and exist for differential tests and A/B measurements (tests/test_gpu_parity.py, README.md). */
enum sr_plan_flags {
    SR_PLAN_GENERIC_KERNELS = 1u << 0,  /* field-generic radix-2 LDS kernels instead of the tuned / register-tiled paths        */
    SR_PLAN_GL_NO_COLS256 = 1u << 1,    /* Goldilocks 2^16 <= D <= 2^20: strided register passes + 4096-point rows              */
    SR_PLAN_RT_NO_COLS256 = 1u << 2,    /* register-tiled path (BabyBear): 4-stage column passes + 12-stage rows                */
    SR_PLAN_GL_REGTILE = 1u << 3,       /* Goldilocks on the register-tiled path (cross-check of ntt_regtile.hpp)               */
    SR_PLAN_STARK_NO_LAZY = 1u << 4,    /* Stark transforms and sums on 8 x 32-bit limbs instead of nine 28-bit lazy limbs       */
    SR_PLAN_STARK_GENERIC_ON_LAZY = 1u << 5, /* Stark: generic LDS kernels on the lazy limbs instead of ntt_stark.hpp            */
    SR_PLAN_NO_HOST_PIN = 1u << 6,      /* accepted, no effect: host buffers are never registered (round 4 removed the pinning)  */
    SR_PLAN_GL_PLAIN_COLS = 1u << 7,    /* Goldilocks lane plans: the plain column pass instead of the workgroup-owns-its-columns
                                           one (cols256_keep_kernel, ntt_goldilocks.hpp)                                          */
    SR_PLAN_GL_SPLIT_ROWS = 1u << 8     /* Goldilocks D > 4096 ring products: the fused rows kernel as two launches (crt of b's tiles in
                                           the scratch, then the constant-operand product) -- A/B plan, measured slower */
};
typedef struct sr_plan {
    uint32_t flags;               /* OR of sr_plan_flags                                                                       */
    int32_t log_tile;             /* 0 = default; 8..12: LDS tile of the generic kernels                                       */
    int32_t stark_whole_max;      /* 0 = default (11); 9..12: largest log2 D the Stark kernels keep as one tile per element    */
    uint32_t chunk_polys;         /* fused ring products above one tile: ring elements per chunk of launches (0 = default: as many
                                     as the operand scratch holds; the tuned Goldilocks path: see lanes)                       */
    uint64_t scratch_limit_bytes; /* cap of the operand scratch (0 = default 16 GiB); larger batches run in chunks             */
    uint32_t host_chunk_mb;       /* chunk of the host-pointer pipeline in MiB (0 = default 128)                               */
    uint32_t lanes;               /* chunked products (tuned Goldilocks 2^16 <= D <= 2^20, register-tiled BabyBear): 0 = AUTO -- the
                                     library times both plans, warmed up and run as they will run, once on this process's real stream-to-hardware-
                                     queue mapping and keeps the faster.  The measurement runs ONLY inside sr_ctx_reserve_scratch
                                     (a blocking call anyway); a context whose host never reserves runs two lanes, unmeasured --
                                     no asynchronous _dev call ever probes, blocks on a measurement or breaks a stream capture;
                                     2 = two internal streams ("lanes"), chunks of chunk_polys or 64 MiB of coefficients each,
                                     intermediates in per-lane scratch so that they are re-read from the Infinity Cache;
                                     1 = one stream (eight large chunks, or chunk_polys).  sr_ctx_plan_in_use tells which.     */
} sr_plan;
int sr_ctx_create_ex(int ring, int log2_degree, int device, const sr_plan *plan, sr_ctx **out);
/* Pre-sizes the context's operand scratch for fused ring products of up to `batch` elements (capped by the plan's
 * scratch_limit_bytes).  Device entry points are asynchronous, with ONE exception: a ring product above one LDS tile whose
 * scratch has to grow first blocks (hipDeviceSynchronize + hipFree + hipMalloc) -- call this once after creating the context
 * (or accept that the first product of a new size blocks) and no _dev call blocks afterwards: the reservation covers ring
 * products AND stand-alone transforms of up to `batch` elements.  From then on the _dev calls of
 * that batch size can also be CAPTURED into a HIP graph by the caller (hipStreamBeginCapture on `stream`): they neither allocate
 * nor synchronise nor probe, and the internal lanes fork from and join to `stream` by events
 * (tests/test_gpu_parity.py: test_device_calls_can_be_captured_into_a_hip_graph).
 * LIMITS of capture -- a captured graph bakes in this context's scratch addresses and lane streams:
 *   (1) the scratch must not move while the graph is alive.  The library enforces its half: once a _dev call has arrived on a
 *       capturing stream, no _dev call grows a context buffer any more -- one that would have to returns SR_E_INVALID (also during the
 *       capture itself: reserve first).  Only sr_ctx_reserve_scratch still grows; calling it with a larger batch INVALIDATES graphs
 *       captured earlier on this context (destroy them first).
 *   (2) ordering between a replay and other work on the same context is the HOST's job: the event that orders users of the shared
 *       scratch is recorded at capture time, not at replay, so a replay is unordered against eager _dev calls of this context on
 *       other streams and against replays of a second graph -- do not overlap them (same stream, or an event / synchronisation of
 *       your own).  One graph per context at a time; use one context per concurrent graph.
 * Chunking of a batch (sr_plan.chunk_polys = 0): never below 64 MiB of coefficients per set of launches; products take the two
 * lanes from three and a half such chunks on, stand-alone transforms from eight, one set of launches on the caller's stream below. */
int sr_ctx_reserve_scratch(sr_ctx *ctx, size_t batch);
/* The plan the context runs: *plan = the sr_plan it was created with, with lanes resolved to 1 or 2 once the library has settled it
 * (lanes stays 0 while sr_plan.lanes = 0 and sr_ctx_reserve_scratch has not run: such a context runs two lanes).  probe_ms
 * (optional): what the probe measured, [0] two lanes, [1] one stream: milliseconds per call of probe_elems ring products, each plan
 * run as it will run (mean of four calls after four warm-up calls; 0 = not measured: the plan was given explicitly, the ring has no
 * chunked product, the batch reserved for is below eight chunks, or the probe's temporaries could not be allocated). */
int sr_ctx_plan_in_use(sr_ctx *ctx, sr_plan *plan, double probe_ms[2], size_t *probe_elems);
int sr_ctx_destroy(sr_ctx *ctx);
/* D, u64 limbs per coefficient, u64 words per ring element */
int sr_ctx_degree(const sr_ctx *ctx, size_t *degree);
int sr_ctx_limbs(const sr_ctx *ctx, int *limbs);
/* Twiddle block (forward + inverse tables, device memory) for sharing across the GPUs of a node:
 * rank 0 builds it, broadcasts the bytes (RCCL over xGMI), the other ranks adopt them. */
int sr_ctx_twiddle_block(sr_ctx *ctx, void **dev_ptr, size_t *bytes);
/* Tell the context its twiddle block was overwritten (e.g. by a broadcast). */
int sr_ctx_twiddles_updated(sr_ctx *ctx);
/* Single-process multi-GPU form of the above ("sr_ctx_create(.., device_ids[], n)"; what a Rust host that drives the
 * 8 GPUs of a node from one process binds): n contexts, one per device_ids[i], whose twiddle blocks are all copies of the block
 * device_ids[0] built (hipMemcpyPeer, i.e. xGMI between the GPUs of a node) -- the only inter-GPU traffic of the path.  out[]
 * receives n contexts (all destroyed again on failure).  sr_shard_range gives part i of a batch split contiguously and evenly
 * (the first batch % n parts get one element more), the partition of stark_rings_amd/sharding.py. */
int sr_ctx_create_group(int ring, int log2_degree, const int *device_ids, int n, const sr_plan *plan, sr_ctx **out);
int sr_shard_range(size_t batch, int n, int i, size_t *first, size_t *count);

/* ---- host-buffer entry points (stage through device memory; PCIe-inclusive) ------------- */
/* CRT::elementwise_crt  (crt.rs:10-25): coefficient form -> CRT/NTT form, in place.       */
int sr_ntt_fwd_batch(sr_ctx *ctx, uint64_t *data, size_t batch);
/* ICRT::elementwise_icrt (crt.rs:34-49): inverse, in place.                               */
int sr_ntt_inv_batch(sr_ctx *ctx, uint64_t *data, size_t batch);
/* RqNTT MulAssign<&Self> per element (ntt_form.rs:213-225; values of mul_unchecked :177-189) */
int sr_pointwise_mul_batch(sr_ctx *ctx, uint64_t *lhs_inout, const uint64_t *rhs, size_t batch);
/* RqNTT += / -= &RqNTT (ntt_form.rs:227-285, 588-638) and the same for RqPoly: coefficient-wise in either form. */
int sr_add_batch(sr_ctx *ctx, uint64_t *lhs_inout, const uint64_t *rhs, size_t batch);
int sr_sub_batch(sr_ctx *ctx, uint64_t *lhs_inout, const uint64_t *rhs, size_t batch);
/* The unary operators of the same element types (round 4), every ring id, word-wise in either form:
 *   sr_neg_batch          Neg: RqPoly `self.0.map(|x| -x)` (coeff_form.rs:270-278), RqNTT (ntt_form.rs:191-203).
 *   sr_scale_batch        every coefficient / every slot component times ONE base-field scalar: RqPoly Mul<Fp> (= poly_mul by
 *                         from_scalar, coeff_form.rs:390-408) and Mul / MulAssign<u128|u64|u32|u16|u8|bool> (`*lhs *= Fp::from(rhs)`,
 *                         coeff_form.rs:610-650); RqNTT Mul / MulAssign<primitive> (`*lhs *= BaseCRTField::from(rhs)`,
 *                         ntt_form.rs:373-425: a base-field element embedded in Fq3 / Fq9 / Fq4 scales every component).
 *   sr_add_scalar_batch   Add / AddAssign<primitive> (Sub: pass the negated scalar).  ntt_form = 0, RqPoly: coefficient 0 of every
 *                         element += scalar (coeff_form.rs:652-700); ntt_form != 0, RqNTT: component 0 of EVERY slot += scalar
 *                         (`*lhs += BaseCRTField::from(rhs)`, ntt_form.rs:427-505).
 * scalar: HOST pointer (also in the _dev forms) to the N-limb Montgomery memory image of the base-field element (what Fp::from(rhs)
 * holds); a word >= p is SR_E_INVALID. */
int sr_neg_batch(sr_ctx *ctx, uint64_t *data, size_t batch);
int sr_scale_batch(sr_ctx *ctx, uint64_t *data, const uint64_t *scalar, size_t batch);
int sr_add_scalar_batch(sr_ctx *ctx, uint64_t *data, const uint64_t *scalar, int ntt_form, size_t batch);
/* Every element of the batch (CRT/NTT form) times ONE ring element, slot-wise: `MulAssign<&R> for Matrix<R>`
 * (linear_algebra/src/matrix.rs:207-211) and `for SparseMatrix<R>` (sparse_matrix.rs:303-307) on the matrix's flat storage --
 * `row.iter_mut().for_each(|r_m| *r_m *= r)`.  Every ring id (Fq3 / Fq9 / Fq4 slot products for the reference's own rings).
 * elem: D coefficients; it must not lie inside the batch it multiplies (the _dev form: a DEVICE pointer). */
int sr_mul_elem_batch(sr_ctx *ctx, uint64_t *data_inout, const uint64_t *elem, size_t batch);
/* Batch reductions of the same element types (round 5): `Sum` and `Product` over a slice of ring elements --
 *   sr_sum_batch       impl Sum<Self> / Sum<&Self>: `iter.fold(Self::zero(), |acc, x| acc + x)` for RqPoly (coeff_form.rs:507-521)
 *                      and RqNTT (ntt_form.rs:640-654): n elements -> 1, word-wise, the same in either form, every ring id;
 *                      n = 0 gives zero().
 *   sr_product_batch   impl Product<Self> / Product<&Self> for RqNTT: `iter.fold(Self::one(), |acc, x| acc * x)`, slot-wise
 *                      (ntt_form.rs:656-670), every ring id (Fq3 / Fq9 / Fq4 slot products for the reference's own rings); n = 0
 *                      gives one() = every slot (1, 0, ..).  Product for RqPoly (coeff_form.rs:523-537, `acc * x` = the ring product)
 *                      is icrt(product(crt(x_i))): the mirrors compose it from sr_ntt_fwd_batch, this call and sr_ntt_inv_batch on
 *                      ONE element (include/stark_rings.hpp: product_poly; stark_rings_amd/rings.py: product_poly[_dev]).
 * out: one ring element; it must not overlap the n input elements.  The folds are associative and commutative and every partial
 * result is canonical, so the tree order the device uses gives the reference's left fold bit for bit.  Partial elements live in
 * context-owned temporaries (ordered between caller streams like the operand scratch; sized on first use or by
 * sr_ctx_reserve_scratch). */
int sr_sum_batch(sr_ctx *ctx, uint64_t *out, const uint64_t *in, size_t n);
int sr_product_batch(sr_ctx *ctx, uint64_t *out, const uint64_t *in_ntt, size_t n);
/* acc[e] += r * x[e] for e < batch, `*` the slot product (CRT/NTT form): `AddAssign<(R, &Self)>` of DenseMultilinearExtension
 * (crates/poly/src/mle/dense.rs:288-317) in one pass.  Every ring id.  r: one ring element outside acc and x; acc and x are the
 * same buffer or disjoint. */
int sr_mul_elem_add_batch(sr_ctx *ctx, uint64_t *acc_inout, const uint64_t *x, const uint64_t *r, size_t batch);
/* RqPoly * RqPoly == icrt(crt(a) * crt(b)) (coeff_form.rs:250-258; identity tested at
 * stark_prime/mod.rs:161-177).  out may alias a.                                          */
int sr_ring_mul_batch(sr_ctx *ctx, uint64_t *out, const uint64_t *a, const uint64_t *b, size_t batch);
/* CyclotomicConfig::reduce_in_place (stark_prime/mod.rs:40-47, goldilocks/mod.rs:75-98,
 * babybear/mod.rs:87-110): each element has in_len_per_elem <= 2D coefficients -> D.      */
int sr_reduce_batch(sr_ctx *ctx, const uint64_t *in, size_t in_len_per_elem, uint64_t *out, size_t batch);

/* ---- device-resident entry points (pointers are HIP device pointers; `stream` is a
 *      hipStream_t passed as void*; asynchronous) ----------------------------------------- */
int sr_ntt_fwd_batch_dev(sr_ctx *ctx, uint64_t *d_data, size_t batch, void *stream);
int sr_ntt_inv_batch_dev(sr_ctx *ctx, uint64_t *d_data, size_t batch, void *stream);
int sr_pointwise_mul_batch_dev(sr_ctx *ctx, uint64_t *d_lhs_inout, const uint64_t *d_rhs, size_t batch, void *stream);
int sr_add_batch_dev(sr_ctx *ctx, uint64_t *d_lhs_inout, const uint64_t *d_rhs, size_t batch, void *stream);
int sr_sub_batch_dev(sr_ctx *ctx, uint64_t *d_lhs_inout, const uint64_t *d_rhs, size_t batch, void *stream);
int sr_neg_batch_dev(sr_ctx *ctx, uint64_t *d_data, size_t batch, void *stream);
int sr_scale_batch_dev(sr_ctx *ctx, uint64_t *d_data, const uint64_t *host_scalar, size_t batch, void *stream);
int sr_add_scalar_batch_dev(sr_ctx *ctx, uint64_t *d_data, const uint64_t *host_scalar, int ntt_form, size_t batch, void *stream);
int sr_mul_elem_batch_dev(sr_ctx *ctx, uint64_t *d_data_inout, const uint64_t *d_elem, size_t batch, void *stream);
int sr_sum_batch_dev(sr_ctx *ctx, uint64_t *d_out, const uint64_t *d_in, size_t n, void *stream);
int sr_product_batch_dev(sr_ctx *ctx, uint64_t *d_out, const uint64_t *d_in_ntt, size_t n, void *stream);
int sr_mul_elem_add_batch_dev(sr_ctx *ctx, uint64_t *d_acc_inout, const uint64_t *d_x, const uint64_t *d_r, size_t batch, void *stream);
/* Dense multilinear extensions of crates/poly over ring elements in CRT/NTT form (a coefficient-form table goes through
 * sr_ntt_fwd_batch_dev first): a table of 2^num_vars ring elements, folded one variable at a time with the slot product of the ring.
 *   SR_MLE_LEADING   DenseMultilinearExtension::fix_variables (mle/dense.rs:171-199): point[i] fixes variable i, the least significant
 *                    index bit first -- self[b] = self[2b] + point[i] * (self[2b+1] - self[2b]).
 *   SR_MLE_TRAILING  fix_last_variables (polynomials/multilinear_polynomial.rs:227-286): point[j] fixes variable num_vars - n_fixed + j,
 *                    the last entry first -- self[b] = self[b] + r * (self[b + half] - self[b]).
 * d_evals: n_evals <= 2^num_vars elements; the elements from n_evals up to 2^num_vars are zero and are NOT read (the reference's
 * truncated storage, dense.rs:35-54, 397-407); n_evals = 0 is the zero MLE.  d_point: n_fixed <= num_vars elements.  d_out receives all
 * 2^(num_vars - n_fixed) elements, zeros included; n_fixed == num_vars is `evaluate` (dense.rs:107-113), n_fixed == 0 copies and
 * zero-pads.  Canonical inputs give canonical results.  The table and the point are never written, with one exception:
 * SR_MLE_TRAILING allows d_out == d_evals (the `&mut self` form; d_work is then ignored).  SR_MLE_LEADING cannot run in place (element b
 * is an input of another workgroup), and every other overlap between d_out, d_evals, d_point and d_work is SR_E_INVALID.
 * The library allocates nothing and touches no context scratch: intermediate tables between launches live in d_work (work_elems ring
 * elements, at least what sr_mle_plan returns), so the call can be captured into a HIP graph on any stream without a warm-up.
 * sr_mle_plan: pure host arithmetic, no device, no context -- how the library runs the fold: *launches kernel launches (a table with
 * n_evals = 0 takes one) and *work_elems <= 3 * 2^num_vars / 4 elements of workspace, 0 whenever one launch suffices; a launch folds up
 * to three variables (two for the Stark field and babybear72: registers).  num_vars < 48.
 * The host-pointer form stages like sr_sum_batch: the whole table goes to a context-owned device temporary, is folded there and the
 * result comes back; chunked staging of folds is not implemented. */
enum { SR_MLE_LEADING = 0, SR_MLE_TRAILING = 1 };
int sr_mle_plan(int ring, int log2_degree, size_t num_vars, size_t n_fixed, int order, size_t *work_elems, int *launches);
int sr_mle_fix_variables_dev(sr_ctx *ctx, uint64_t *d_out, const uint64_t *d_evals, size_t n_evals, size_t num_vars, const uint64_t *d_point,
                             size_t n_fixed, int order, uint64_t *d_work, size_t work_elems, void *stream);
int sr_mle_fix_variables(sr_ctx *ctx, uint64_t *out, const uint64_t *evals, size_t n_evals, size_t num_vars, const uint64_t *point,
                         size_t n_fixed, int order);
/* The prover's message of a sum-check round over a product of dense MLEs (csrc/sumcheck.hpp): one pass that reads every table once.
 * d_tables: a HOST array of n_tables (1 .. SR_MLE_ROUND_MAX_TABLES) device pointers, n_evals: a HOST array; both are consumed at call
 * time (they reach the kernels by value: a captured graph holds no host pointer).  Table j is an MLE in num_vars variables in CRT/NTT
 * form of which the first n_evals[j] <= 2^num_vars elements are stored; the rest are zero and are NEVER read (the truncated-storage
 * contract of sr_mle_fix_variables).  `*` is the slot product of the ring, t the ring constant R::from(t), half = 2^(num_vars - 1),
 * d = n_tables:
 *   SR_MLE_LEADING    d_out[t] = sum_{b < half} prod_j ( f_j[2b] + t * (f_j[2b+1] - f_j[2b]) ) for t = 0 .. d: d + 1 ring elements; the
 *                     summand is fix_variables with the point [R::from(t)] (mle/dense.rs:171-199)
 *   SR_MLE_TRAILING   the same with the pair (f_j[b], f_j[b + half]) (fix_last_variables, multilinear_polynomial.rs:251-286)
 *   SR_MLE_ROUND_SUM  d_out[0] = sum_{b < 2^num_vars} prod_j f_j[b]: one element, the claimed sum (the `sum` of random_mle_list,
 *                     multilinear_polynomial.rs:19-49); num_vars = 0 is allowed here, the two round modes need num_vars >= 1
 * Canonical in, canonical out.  All sums are exact modular integers on canonical values, so the result does not depend on the grid,
 * on how the plan splits the pairs, or on scheduling.  A pair or index beyond the stored part of ANY table contributes zero and is
 * skipped without a load; if any n_evals[j] == 0 every output is zero(): one launch that loads no table.
 * The call allocates nothing and touches no context scratch: partial results live in d_work (work_elems ring elements, at least what
 * sr_mle_round_plan returns) and every workspace word that is read was written by the same call, so it can be captured into a HIP graph
 * on any stream without a warm-up, as one linear chain of launches.  Tables are never written and may alias each other (f * f).
 * SR_E_INVALID: a null pointer, n_tables outside 1 .. 4, an unknown mode, num_vars >= 48, num_vars == 0 in a round mode,
 * n_evals[j] > 2^num_vars, work_elems below the plan's, d_out or d_work overlapping a table or each other.
 * sr_mle_round_plan: pure host arithmetic, no device, no context; it depends on the shape only.  *launches >= 1; *work_elems == 0
 * whenever one launch suffices, and never more than SR_MLE_ROUND_MAX_GROUPS * (n_tables + 1) elements: a shape whose degree alone
 * does not fill the device takes its pairs in up to SR_MLE_ROUND_MAX_GROUPS records -- a workgroup of 256 lanes each, whatever the
 * degree (the lane-groups of a workgroup meet in LDS), so 1024 records are four workgroups on each of 256 compute units -- and each
 * record leaves d + 1 partial elements that a last launch adds.  Some shapes take the d + 1 points in several launches (registers),
 * reading the tables once per launch: Stark at d = 4 (2 + 2 + 1 points), goldilocks24 at d = 3 (2 + 2) and d = 4 (3 + 2), babybear72
 * at d = 3 (2 + 2) and d = 4 (2 + 2 + 1), frog16 at d = 2 (2 + 1), d = 3 (2 + 2) and d = 4 (one point per launch); such a plan always
 * uses the workspace.  The one-limb fields read every table exactly once for every d <= 4.
 * The host-pointer form stages like sr_mle_fix_variables: the whole tables go to context-owned device temporaries, the message is
 * computed there and the d + 1 elements come back; chunked staging is not implemented. */
#define SR_MLE_ROUND_MAX_TABLES 4
#define SR_MLE_ROUND_MAX_GROUPS 1024
enum { SR_MLE_ROUND_SUM = 2 }; /* beside SR_MLE_LEADING = 0, SR_MLE_TRAILING = 1 */
int sr_mle_round_plan(int ring, int log2_degree, size_t num_vars, int n_tables, int mode, size_t *work_elems, int *launches);
int sr_mle_round_evals_dev(sr_ctx *ctx, uint64_t *d_out, const uint64_t *const *d_tables, const size_t *n_evals, int n_tables,
                           size_t num_vars, int mode, uint64_t *d_work, size_t work_elems, void *stream);
int sr_mle_round_evals(sr_ctx *ctx, uint64_t *out, const uint64_t *const *tables, const size_t *n_evals, int n_tables, size_t num_vars,
                       int mode);
/* A sum-check round in one pass (csrc/sumcheck_fold.hpp): fold every table at the challenge of the round that has just ended and
 * compute the message of the round that follows while the folded neighbours are still in registers -- 1.5 n elements of traffic per
 * table of n instead of the 2 n of sr_mle_fix_variables_dev followed by sr_mle_round_evals_dev on the folded tables.  order: SR_MLE_LEADING or
 * SR_MLE_TRAILING; d = n_tables in 1 .. SR_MLE_ROUND_MAX_TABLES; 2 <= num_vars < 48.
 *   d_out_tables[j]  g_j = f_j with one variable fixed at the ring element *d_r (one element in CRT/NTT form): exactly what
 *                    sr_mle_fix_variables_dev(.., n_fixed = 1, order) computes, in truncated storage: n_evals_out[j] elements are written
 *                    -- (n_evals[j] + 1) / 2 in leading order, min(n_evals[j], 2^(num_vars-1)) in trailing order -- and nothing beyond
 *                    them is touched.  Every table is folded to ITS OWN length.
 *   d_out[t]         t = 0 .. d: the message of the next round over g_0 .. g_{d-1} in num_vars - 1 variables, bit-identical to
 *                    sr_mle_round_evals_dev on the folded tables with the same order.
 * d_tables, d_out_tables and n_evals are HOST arrays consumed at call time; n_evals_out is a HOST array filled at call time by host
 * arithmetic.  Canonical in, canonical out; all arithmetic is exact, so both outputs are bit-identical to the two calls made one after
 * the other, whatever the grid or the split.  If any n_evals[j] == 0 the message is zero (no table is loaded for the product) and the
 * other tables are still folded and written; if every table is empty one launch zeroes d_out.
 * Aliasing: outputs may not overlap inputs, each other, d_r, d_out or d_work, with one exception: in SR_MLE_TRAILING
 * d_out_tables[j] == d_tables[j] folds table j in place (a lane reads its four elements before it writes two of the same positions).
 * Input tables may alias each other (f * f), but such a table cannot be folded in place: it would be folded twice.
 * The call allocates nothing and touches no context scratch; every workspace word that is read was written by the same call, and the
 * launches are one linear chain on one stream, so it can be captured without a warm-up.
 * SR_E_INVALID: a null pointer, n_tables outside 1 .. 4, num_vars < 2 or >= 48, an unknown order, n_evals[j] > 2^num_vars, work_elems
 * below the plan's, any forbidden overlap.
 * sr_mle_round_fold_plan: pure host arithmetic, no device, no context; the records are those of sr_mle_round_plan at num_vars - 1.
 * *work_elems == 0 exactly when *launches == 1; *work_elems <= SR_MLE_ROUND_MAX_GROUPS * (n_tables + 1).  The fused launch takes all
 * d + 1 points for Goldilocks and BabyBear at every d <= 4 (at most two launches).  The other families keep the fused kernel within
 * 256 registers by taking the first points there -- Stark 2, 3, 3, 2 for d = 1 .. 4, goldilocks24 2, 3, 2, 2, babybear72 2, 2, 1, 1, frog16
 * 2, 1, 1, 1 -- and the remaining ones from the round kernels of sr_mle_round_evals_dev over the FOLDED tables (half the size), into the
 * same records; such a plan always uses the workspace.
 * The host-pointer form stages like sr_mle_round_evals: whole tables go to context-owned device temporaries, the folded tables and the
 * message come back; chunked staging is not implemented. */
int sr_mle_round_fold_plan(int ring, int log2_degree, size_t num_vars, int n_tables, int order, size_t *work_elems, int *launches);
int sr_mle_round_fold_evals_dev(sr_ctx *ctx, uint64_t *d_out, uint64_t *const *d_out_tables, size_t *n_evals_out,
                                const uint64_t *const *d_tables, const size_t *n_evals, int n_tables, size_t num_vars, const uint64_t *d_r,
                                int order, uint64_t *d_work, size_t work_elems, void *stream);
int sr_mle_round_fold_evals(sr_ctx *ctx, uint64_t *out, uint64_t *const *out_tables, size_t *n_evals_out, const uint64_t *const *tables,
                            const size_t *n_evals, int n_tables, size_t num_vars, const uint64_t *r, int order);
/* The round message of a SUM OF PRODUCTS of dense MLEs with ring coefficients in one pass (csrc/sumcheck_vpoly.hpp): HyperPlonk's
 * VirtualPolynomial, the shape of the claims built on DenseMultilinearExtension -- eq (a b - c), sum_i alpha_i eq prod_j (...).
 *   g(x) = sum_k c_k prod_{s < terms[k].n_factors} f_{terms[k].table[s]}(x),   d = max_k n_factors (the plan's `degree`)
 *   SR_MLE_LEADING    d_out[t] = sum_{b < half} sum_k c_k prod_s ( f[2b] + t (f[2b+1] - f[2b]) ),  t = 0 .. d: d + 1 elements
 *   SR_MLE_TRAILING   the same with the pair (f[b], f[b + half])
 *   SR_MLE_ROUND_SUM  d_out[0] = sum_b g(b): one element; num_vars = 0 is allowed here only
 * Everything is in CRT / NTT form, `*` is the slot product of the ring, t is R::from(t); every ring id, canonical in and out.  A
 * table may occur more than once in a term and in any number of terms, and two table slots may hold the same pointer; every distinct
 * table slot is read once per launch.  d_coeffs: n_terms contiguous ring elements on the device, or NULL for one() everywhere (no
 * coefficient product is computed).  terms, d_tables and n_evals are HOST arrays, consumed at call time: a captured graph holds no
 * host pointer.
 *
 * Truncated storage, per term: an element beyond the stored part of a table is zero and is never loaded; a pair contributes to a
 * term only while its first element lies inside every table of that term, so the pass ends at the longest term.  A term with an empty
 * table contributes nothing; if every term has one, a single launch zeroes d_out and loads nothing.
 *
 * All arithmetic is exact on canonical values: the output depends on neither the grid, the split nor the association of the sums,
 * and one term with d_coeffs == NULL gives sr_mle_round_evals_dev's output bit for bit.  The call allocates nothing and touches no
 * context scratch; partial results live in d_work, every word of which is written before it is read; the launches form one chain on
 * one stream, so the call is capturable on a fresh context.  The points go in several launches where d + 1 lazy sums do not fit the
 * registers beside the tables (the plan reports them); each launch reads the tables once.
 *
 * sr_vpoly_round_plan is pure host arithmetic on the shape (no device, no context): *work_elems == 0 exactly when *launches == 1,
 * *work_elems <= SR_MLE_ROUND_MAX_GROUPS * (degree + 1); the records are those of sr_mle_round_plan.  `degree` must be the largest
 * n_factors of the call.  SR_E_INVALID (nothing launched, the reason in sr_last_error): a null pointer; n_tables outside 1 ..
 * SR_VPOLY_MAX_TABLES; n_terms outside 1 .. SR_VPOLY_MAX_TERMS; n_factors outside 1 .. SR_VPOLY_MAX_FACTORS; a table index outside
 * 0 .. n_tables - 1; a table no term uses; an unknown mode; num_vars >= 48, or 0 in a round mode; n_evals[j] > 2^num_vars; a
 * workspace below the plan's; d_out, d_work or d_coeffs overlapping a table or each other.
 * The host-pointer form stages whole tables through context-owned temporaries, as sr_mle_round_evals does. */
#define SR_VPOLY_MAX_TABLES 8
#define SR_VPOLY_MAX_TERMS 8
#define SR_VPOLY_MAX_FACTORS 4
typedef struct {
    int n_factors;
    int table[SR_VPOLY_MAX_FACTORS];
} sr_vpoly_term;
int sr_vpoly_round_plan(int ring, int log2_degree, size_t num_vars, int n_tables, int n_terms, int degree, int mode, size_t *work_elems,
                        int *launches);
int sr_vpoly_round_evals_dev(sr_ctx *ctx, uint64_t *d_out, const uint64_t *const *d_tables, const size_t *n_evals, int n_tables,
                             const sr_vpoly_term *terms, int n_terms, const uint64_t *d_coeffs, size_t num_vars, int mode, uint64_t *d_work,
                             size_t work_elems, void *stream);
int sr_vpoly_round_evals(sr_ctx *ctx, uint64_t *out, const uint64_t *const *tables, const size_t *n_evals, int n_tables,
                         const sr_vpoly_term *terms, int n_terms, const uint64_t *coeffs, size_t num_vars, int mode);
/* A sum-check round of a SUM OF PRODUCTS in one pass (csrc/sumcheck_vpoly_fold.hpp): fold every distinct table slot at the challenge
 * of the round that has just ended and compute the message of the round that follows while the folded neighbours are still in
 * registers.  The contract is the conjunction of sr_mle_round_fold_evals_dev and sr_vpoly_round_evals_dev above:
 *   d_out_tables[j]  exactly what sr_mle_fix_variables_dev(.., n_fixed = 1, order) writes for slot j at *d_r, in truncated storage:
 *                    n_evals_out[j] = (n_evals[j] + 1) / 2 elements in leading order, min(n_evals[j], 2^(num_vars-1)) in trailing
 *                    order; nothing beyond them is touched.  Every table is folded to ITS OWN length.
 *   d_out[t]         t = 0 .. degree: bit-identical to sr_vpoly_round_evals_dev on the folded tables at num_vars - 1 with the same
 *                    terms, coefficients and order.  One term with d_coeffs == NULL gives sr_mle_round_fold_evals_dev's message and
 *                    tables bit for bit.
 * order: SR_MLE_LEADING or SR_MLE_TRAILING; 2 <= num_vars < 48; the limits are SR_VPOLY_MAX_TABLES, SR_VPOLY_MAX_TERMS and
 * SR_VPOLY_MAX_FACTORS; every ring id; canonical in, canonical out.  terms, d_tables, d_out_tables and n_evals are HOST arrays consumed
 * at call time; n_evals_out is a HOST array filled at call time by host arithmetic.
 * Empty tables: a term with an empty table contributes zero and the other tables are still folded and written; if every term has one
 * the message is zero and no table is loaded for the products; if every table is empty one launch zeroes d_out.
 * Aliasing: outputs may not overlap inputs, each other, d_r, d_coeffs, d_out or d_work, with one exception: in SR_MLE_TRAILING
 * d_out_tables[j] == d_tables[j] folds slot j in place.  Two slots may hold the same input pointer; each then gets its own output and
 * neither may be folded in place.
 * The call allocates nothing and touches no context scratch; every workspace word is written before it is read; the launches are one
 * linear chain on one stream, so the call is capturable on a fresh context.
 * SR_E_INVALID (nothing launched, the reason in sr_last_error): every refusal of the two calls above, and d_coeffs overlapping a
 * folded table.
 * sr_vpoly_round_fold_plan: pure host arithmetic, no device, no context; the records are those of sr_vpoly_round_plan at
 * num_vars - 1.  *work_elems == 0 exactly when *launches == 1; *work_elems <= SR_MLE_ROUND_MAX_GROUPS * (degree + 1).  The fused launch
 * takes the first points -- over 4 / 8 table slots: Goldilocks 5 / 4, BabyBear 5 / 3, Stark 2 / 1, goldilocks24 2 / 1, babybear72 1 / 0
 * (over 8 slots the fused launch only folds), frog16 1 / 1 -- and the remaining ones come from the round kernels of
 * sr_vpoly_round_evals_dev over the FOLDED tables (half the size), into the same records; such a plan always uses the workspace.
 * The host-pointer form stages like sr_mle_round_fold_evals. */
int sr_vpoly_round_fold_plan(int ring, int log2_degree, size_t num_vars, int n_tables, int n_terms, int degree, int order,
                             size_t *work_elems, int *launches);
int sr_vpoly_round_fold_evals_dev(sr_ctx *ctx, uint64_t *d_out, uint64_t *const *d_out_tables, size_t *n_evals_out,
                                  const uint64_t *const *d_tables, const size_t *n_evals, int n_tables, const sr_vpoly_term *terms,
                                  int n_terms, const uint64_t *d_coeffs, size_t num_vars, const uint64_t *d_r, int order, uint64_t *d_work,
                                  size_t work_elems, void *stream);
int sr_vpoly_round_fold_evals(sr_ctx *ctx, uint64_t *out, uint64_t *const *out_tables, size_t *n_evals_out, const uint64_t *const *tables,
                              const size_t *n_evals, int n_tables, const sr_vpoly_term *terms, int n_terms, const uint64_t *coeffs,
                              size_t num_vars, const uint64_t *r, int order);
/* Sum-check rounds with a PER-PAIR WEIGHT (csrc/sumcheck_weighted.hpp): the eq(z, .) factor of a zero-check -- eq (a b - c), the layer
 * claims L_k(z) = sum_b eq(z, b) lo(b) hi(b) of sr_prod_tree_dev and P_k(z) + lambda Q_k(z) of sr_frac_tree_dev -- as one ring element per
 * pair that is constant in the round's variable, not as one more table.  In the round that binds variable v, with the challenges r
 * of the earlier rounds bound,
 *     s(t) = [prod_{i bound} eq(z_i, r_i)] * eq(z_v, t) * h(t),   h(t) = sum_b w[b] g(t, b),   w = eq(z_rest, .) (sr_eq_table_dev)
 * where g is the claim without eq, folded at the challenges so far: w is never folded (the next round has its own, half as long), is
 * read once per round, and h has one degree less than s.  The calls below compute h; the two factors in front are single elements.
 *
 * sr_vpoly_wround_evals_dev: the weighted sibling of sr_vpoly_round_evals_dev.
 *   d_out[t] = sum_{b < half} w[b] * sum_k c_k prod_s ( lo_s[b] + t (hi_s[b] - lo_s[b]) ),  t = 0 .. degree
 * with the pairs (lo, hi) of sr_vpoly_round_evals_dev in the same order (SR_MLE_LEADING: f[2b], f[2b+1]; SR_MLE_TRAILING: f[b],
 * f[b + half]).  `degree` is the largest n_factors: the weight is not a factor and is not counted.  d_weights holds 2^(num_vars - 1) ring
 * elements in CRT / NTT form, one per pair, indexed by the pair index b, stored in full, never written.  num_vars >= 1.
 * SR_MLE_ROUND_SUM is SR_E_INVALID: a weight of a plain sum is just a table.  Truncated tables work as in the unweighted call: the pass
 * ends at the longest term, and a weight whose pair is not visited is not read.  All arithmetic is exact on canonical values: the
 * output depends on neither the grid, the split nor the association, and with every weight one() it equals
 * sr_vpoly_round_evals_dev bit for bit.  terms, d_tables and n_evals are HOST arrays consumed at call time; nothing is allocated, no
 * context scratch is touched, every workspace word is written before it is read, the launches are one linear chain on one stream
 * (capturable on a fresh context); canonical in, canonical out; every ring id.
 *
 * sr_vpoly_wround_fold_evals_dev: the weighted sibling of sr_vpoly_round_fold_evals_dev.  d_out_tables and n_evals_out are exactly those
 * of sr_vpoly_round_fold_evals_dev; d_out is bit-identical to sr_vpoly_wround_evals_dev on the folded tables at num_vars - 1 with the
 * same d_weights, which therefore holds 2^(num_vars - 2) elements.  num_vars >= 2.  The aliasing rules are those of the unweighted fused
 * call; in addition d_weights may not overlap any output or d_work.
 *
 * SR_E_INVALID (nothing launched, the reason in sr_last_error): every refusal of the unweighted calls, a null d_weights (refused before
 * anything else), SR_MLE_ROUND_SUM, d_out or d_work overlapping d_weights, and for the fused call a folded table overlapping d_weights.
 *
 * The plans are pure host arithmetic (no device, no context): *work_elems == 0 exactly when *launches == 1, *work_elems <=
 * SR_MLE_ROUND_MAX_GROUPS * (degree + 1); the records are those of sr_vpoly_round_plan (sr_vpoly_wround_fold_plan: at num_vars - 1).
 * Points per launch over 4 / 8 table slots, the largest number that keeps a kernel without scratch within 256 registers (BabyBear 128):
 *   the weighted round kernels   Goldilocks 5 / 5, BabyBear 5 / 5, Stark 4 / 1, goldilocks24 3 / 1, babybear72 1 / 1, frog16 1 / 1
 *   the weighted fused launch    Goldilocks 5 / 4, BabyBear 5 / 3, Stark 2 / 1, goldilocks24 2 / 1, babybear72 1 / 0, frog16 1 / 1
 * (babybear72 over 8 slots: the fused launch only folds).  The remaining points of a fused call come from the weighted round kernels
 * over the FOLDED tables, into the same records; such a plan always uses the workspace.
 * The host-pointer forms stage whole tables (and the weights) through context-owned temporaries as sr_vpoly_round_evals and
 * sr_vpoly_round_fold_evals do; chunked staging is not implemented. */
int sr_vpoly_wround_plan(int ring, int log2_degree, size_t num_vars, int n_tables, int n_terms, int degree, int order, size_t *work_elems,
                         int *launches);
int sr_vpoly_wround_evals_dev(sr_ctx *ctx, uint64_t *d_out, const uint64_t *d_weights, const uint64_t *const *d_tables, const size_t *n_evals,
                              int n_tables, const sr_vpoly_term *terms, int n_terms, const uint64_t *d_coeffs, size_t num_vars, int order,
                              uint64_t *d_work, size_t work_elems, void *stream);
int sr_vpoly_wround_evals(sr_ctx *ctx, uint64_t *out, const uint64_t *weights, const uint64_t *const *tables, const size_t *n_evals,
                          int n_tables, const sr_vpoly_term *terms, int n_terms, const uint64_t *coeffs, size_t num_vars, int order);
int sr_vpoly_wround_fold_plan(int ring, int log2_degree, size_t num_vars, int n_tables, int n_terms, int degree, int order,
                              size_t *work_elems, int *launches);
int sr_vpoly_wround_fold_evals_dev(sr_ctx *ctx, uint64_t *d_out, uint64_t *const *d_out_tables, size_t *n_evals_out, const uint64_t *d_weights,
                                   const uint64_t *const *d_tables, const size_t *n_evals, int n_tables, const sr_vpoly_term *terms,
                                   int n_terms, const uint64_t *d_coeffs, size_t num_vars, const uint64_t *d_r, int order, uint64_t *d_work,
                                   size_t work_elems, void *stream);
int sr_vpoly_wround_fold_evals(sr_ctx *ctx, uint64_t *out, uint64_t *const *out_tables, size_t *n_evals_out, const uint64_t *weights,
                               const uint64_t *const *tables, const size_t *n_evals, int n_tables, const sr_vpoly_term *terms, int n_terms,
                               const uint64_t *coeffs, size_t num_vars, const uint64_t *r, int order);
/* Range-check (norm-check) rounds (csrc/range_check.hpp): the claim a lattice folding scheme runs in every fold and for every decomposed
 * witness,
 *     sum_b eq(beta, b) * sum_i mu_i * prod_{j = -(B-1)}^{B-1} ( f_i(b) - j ) = 0,
 * which says that every entry of every f_i lies in (-B, B).  With eq as a per-pair weight (see above) the round message is
 *   d_out[t] = sum_{b < half} w[b] * sum_i mu_i * P_B( lo_i[b] + t (hi_i[b] - lo_i[b]) ),   t = 0 .. 2 B - 1
 *   P_B(x)   = prod_{j = -(B-1)}^{B-1} (x - R::from(j))
 * with the pairs (lo, hi) of sr_vpoly_wround_evals_dev in the same order (SR_MLE_LEADING: f[2b], f[2b+1]; SR_MLE_TRAILING: f[b],
 * f[b + half]).  The degree is 2 bound - 1 and a message has 2 bound elements.  A table is read ONCE per launch whatever the bound: no
 * shifted copies f - j exist, none is folded, and the kernels evaluate P_B(x) = x prod_{j=1}^{B-1} (x^2 - j^2) with j^2 as base-field
 * constants.  d_weights holds 2^(num_vars - 1) ring elements, one per pair, stored in full, never written.  d_coeffs holds n_tables
 * elements (mu), or is NULL for one().  d_tables and n_evals are HOST arrays consumed at call time.  1 <= num_vars < 48,
 * 1 <= n_tables <= SR_RANGE_MAX_TABLES, 2 <= bound <= SR_RANGE_MAX_BOUND; every ring id; CRT / NTT form, canonical in, canonical out.
 * All arithmetic is exact on canonical values: the output depends on neither the grid, the split, the association nor how P_B is
 * factored.  Nothing is allocated, no context scratch is touched, every workspace word is written before it is read, the launches are one
 * linear chain on one stream (capturable on a fresh context).
 *
 * Truncated storage: a pair of table i is visited exactly while its first element is stored; an absent second element is zero and is
 * never loaded; unvisited pairs contribute nothing, which is exact since P_B(0) = 0; a weight whose pair no table visits is not read.
 * Every table empty: one launch zeroes d_out.
 *
 * SR_E_INVALID (nothing launched, the reason in sr_last_error): a null pointer (d_weights is checked first); bound, n_tables, order or
 * num_vars outside their ranges; n_evals[i] > 2^num_vars; a workspace below the plan's; d_out or d_work overlapping a table, the
 * weights, the coefficients or each other.
 *
 * sr_range_wround_plan is pure host arithmetic (no device, no context): *work_elems == 0 exactly when *launches == 1, *work_elems <=
 * SR_MLE_ROUND_MAX_GROUPS * 2 bound; the records are those of sr_vpoly_round_plan.  Points per launch, the largest number that keeps
 * the kernel without scratch within 256 registers (BabyBear 128), whatever n_tables and bound:
 *   Goldilocks 7, BabyBear 8, Stark 3, goldilocks24 2, babybear72 2, frog16 2
 * so a call takes ceil(2 bound / points) launches, each of which reads the tables and the weights once, plus the sum over the records
 * where there are several.  The host-pointer form stages whole tables (and the weights) through context-owned temporaries as
 * sr_vpoly_wround_evals does; chunked staging is not implemented. */
#define SR_RANGE_MAX_TABLES 8
#define SR_RANGE_MAX_BOUND 8
int sr_range_wround_plan(int ring, int log2_degree, size_t num_vars, int n_tables, int bound, int order, size_t *work_elems, int *launches);
int sr_range_wround_evals_dev(sr_ctx *ctx, uint64_t *d_out, const uint64_t *d_weights, const uint64_t *const *d_tables, const size_t *n_evals,
                              int n_tables, int bound, const uint64_t *d_coeffs, size_t num_vars, int order, uint64_t *d_work,
                              size_t work_elems, void *stream);
int sr_range_wround_evals(sr_ctx *ctx, uint64_t *out, const uint64_t *weights, const uint64_t *const *tables, const size_t *n_evals,
                          int n_tables, int bound, const uint64_t *coeffs, size_t num_vars, int order);
/* Sparse multilinear extensions: the arithmetic of crates/poly's SparseMultilinearExtension (mle/sparse.rs) on device-resident
 * values.  Elements are ring elements in CRT / NTT form in the usual flat layout, canonical in and canonical out, for every ring id.
 *
 * sr_eq_table: out[b] = prod_i (bit i of b ? point[i] : one() - point[i]) for b < 2^n_vars, bit 0 <-> point[0]: precompute_eq
 * (sparse.rs:381-394), bit-identical to its doubling recurrence (exact arithmetic on canonical values; the factors commute).
 * n_vars = 0 gives the single element one().  sum_b out[b] f[b] = f(point) for a dense table f.  One launch, no workspace, no
 * context scratch; d_out overlapping d_point is SR_E_INVALID.
 *
 * A sparse MLE is (num_vars < 64; idx: nnz u64 indices, strictly ascending, each < 2^num_vars -- the BTreeMap's iteration order;
 * vals: nnz ring elements in the same order).  Stored zeros are legal and are kept.  Fixing the first n_fixed variables
 * (fix_variables, sparse.rs:170-207) sends entry j to key idx[j] >> n_fixed; idx ascends, so equal keys are contiguous RUNS and
 *     out_vals[s] = sum over the entries j of run s of eq(point, idx[j] & (2^n_fixed - 1)) * vals[j],
 * one output per distinct key, in ascending key order; an output whose sum is zero stays (the reference's map keeps it too).
 *   n_fixed == num_vars is `evaluate` (sparse.rs:53-56): n_out is 1 when nnz > 0.
 *   nnz == 0 gives n_out == 0 and touches nothing (the value of an empty MLE is zero(), sparse.rs:359-365: the mirrors return it).
 *   n_fixed == 0 copies.
 * sr_smle_fix_pattern: host arithmetic, no device, no context.  Validates idx and writes the n_out distinct keys to out_idx (room for
 * nnz) and the run boundaries to seg_ptr (room for nnz + 1): run s is the entries seg_ptr[s] .. seg_ptr[s + 1] - 1,
 * seg_ptr[n_out] = nnz.  SR_E_INVALID: num_vars >= 64, n_fixed > num_vars, indices not strictly ascending or >= 2^num_vars, null
 * pointers.
 * sr_smle_plan: host arithmetic: the workspace in ring elements and the stream operations (at least 1) of a fold of nnz entries in
 * n_out runs.  The plan depends on nnz and n_out only, never on the run lengths:
 *   - the entries are cut into spans of consecutive entries, at most nnz / 2 of them; a run that crosses a span boundary leaves
 *     partial elements in the workspace (two per span at most) which a second launch adds.  n_out == nnz (every run is one entry)
 *     cannot cross one and takes no such launch;
 *   - nnz >= SR_SMLE_TABLE_MIN_NNZ with n_fixed >= 2: eq(point, x) is taken as a product over windows of SR_SMLE_WINDOW_BITS
 *     variables, whose eq tables one more launch builds in the workspace (ceil(n_fixed / window) tables of 2^window elements);
 *     below, point[i] or one() - point[i] are multiplied in on the fly and no table exists.
 *   work_elems <= nnz + SR_SMLE_MAX_TABLE_ELEMS, and work_elems == 0 whenever launches == 1.
 * sr_smle_fix_variables_dev: d_idx and d_seg_ptr are device copies of what sr_smle_fix_pattern saw and wrote; they are NOT validated
 * (corrupt arrays give wrong values, never an access outside the buffers).  SR_E_INVALID: null pointers, n_fixed >= 64, n_out > nnz,
 * work_elems below the plan, d_out_vals overlapping d_vals, d_point or d_work.  Nothing is allocated, no context scratch is touched and
 * every workspace word that is read was written by the same call: the call can sit in a captured graph (one stream, a linear chain)
 * and be replayed on changed values and points.
 * sr_smle_fix_variables (host pointers): validates, runs the pattern itself (out_idx: room for nnz keys, out_vals: room for nnz
 * elements; *n_out of each are written) and stages like sr_mle_fix_variables. */
#define SR_SMLE_WINDOW_BITS 8
#define SR_SMLE_TABLE_MIN_NNZ 1024
#define SR_SMLE_MAX_TABLE_ELEMS 2048 /* ceil(63 / SR_SMLE_WINDOW_BITS) << SR_SMLE_WINDOW_BITS */
int sr_eq_table_dev(sr_ctx *ctx, uint64_t *d_out, const uint64_t *d_point, size_t n_vars, void *stream);
int sr_eq_table(sr_ctx *ctx, uint64_t *out, const uint64_t *point, size_t n_vars);
int sr_smle_fix_pattern(const uint64_t *idx, size_t nnz, size_t num_vars, size_t n_fixed, uint64_t *out_idx, uint64_t *seg_ptr, size_t *n_out);
int sr_smle_plan(int ring, int log2_degree, size_t nnz, size_t n_out, size_t n_fixed, size_t *work_elems, int *launches);
int sr_smle_fix_variables_dev(sr_ctx *ctx, uint64_t *d_out_vals, const uint64_t *d_vals, const uint64_t *d_idx, size_t nnz,
                              const uint64_t *d_seg_ptr, size_t n_out, const uint64_t *d_point, size_t n_fixed, uint64_t *d_work,
                              size_t work_elems, void *stream);
int sr_smle_fix_variables(sr_ctx *ctx, uint64_t *out_vals, uint64_t *out_idx, size_t *n_out, const uint64_t *vals, const uint64_t *idx,
                          size_t nnz, size_t num_vars, const uint64_t *point, size_t n_fixed);
/* Grand products (csrc/prod_tree.hpp): every layer of the binary product tree over a table of 2^num_vars ring elements in CRT/NTT form,
 * the circuit of the division-free, layered product argument (each layer is proved from the one below by one sum-check of
 * eq(z, .) * lo * hi; sr_vpoly_round_fold_evals_dev runs that claim).  `*` is the slot product of the ring, as in sr_product_batch.
 * Layer 0 is the leaves; layer k (1 <= k <= num_vars) has half = 2^(num_vars - k) elements:
 *   SR_MLE_LEADING   L_k[i] = L_{k-1}[2i] * L_{k-1}[2i+1]       the pairs sr_mle_fix_variables folds in leading order
 *   SR_MLE_TRAILING  L_k[i] = L_{k-1}[i] * L_{k-1}[i + half]    the pairs it folds in trailing order: the two operands of a layer are the
 *                    contiguous lower and upper halves of the layer below, usable as MLE tables as they lie
 * d_leaves: n_leaves <= 2^num_vars elements; the leaves from n_leaves up to 2^num_vars are one() (what sr_product_batch returns for
 * n = 0) and are NOT read; a group of leaves that begins at or beyond n_leaves is written as one() without any load.
 * d_layers receives 2^num_vars - 1 elements, every layer in full, ones included: layer k at element offset
 * 2^num_vars - 2^(num_vars - k + 1), layer 1 first, the root last.  Canonical inputs give canonical results.  The leaves are never
 * written, and any overlap of d_layers and the stored leaves is SR_E_INVALID.
 * The library allocates nothing and touches no context scratch (later launches read the layer an earlier launch of the same call
 * wrote), so the call can be captured into a HIP graph on any stream without a warm-up.
 * sr_prod_tree_plan: pure host arithmetic, no device, no context -- *layer_elems = 2^num_vars - 1 and the kernel launches of the call:
 * a launch reads each group of leaves once and writes up to three levels (two for babybear72: registers), full launches first, the
 * remainder last.  num_vars < 48; num_vars = 0 is no launch and nothing written.
 * The host-pointer form stages like sr_sum_batch: leaves and layers live in context-owned device temporaries for the call. */
int sr_prod_tree_plan(int ring, int log2_degree, size_t num_vars, int order, size_t *layer_elems, int *launches);
int sr_prod_tree_dev(sr_ctx *ctx, uint64_t *d_layers, const uint64_t *d_leaves, size_t n_leaves, size_t num_vars, int order, void *stream);
int sr_prod_tree(sr_ctx *ctx, uint64_t *layers, const uint64_t *leaves, size_t n_leaves, size_t num_vars, int order);
/* Fraction trees (csrc/frac_tree.hpp): every layer of the binary tree that sums 2^num_vars fractions p_i / q_i of ring elements in
 * CRT/NTT form without dividing, the circuit of the layered (GKR) fractional sum-check behind logUp lookup and range arguments.  A node
 * is a pair (p, q); with the children (l, r) of sr_prod_tree -- (2i, 2i+1) in SR_MLE_LEADING, (i, i + half) in SR_MLE_TRAILING --
 *   p = p_l * q_r + p_r * q_l        q = q_l * q_r
 * `*` the slot product of sr_product_batch, `+` the slot sum of sr_add_batch.  The root (P, Q) is P = sum_i p_i prod_{j != i} q_j,
 * Q = prod_j q_j, so P / Q = sum_i p_i / q_i wherever the q_i are units.
 * d_p_leaves, d_q_leaves: n_leaves <= 2^num_vars elements each; the leaves beyond them are the neutral fraction (zero(), one()) and are
 * NOT read.  d_p_leaves = NULL: every stored leaf has numerator one() (sum 1 / q_i), and no numerator is read; the general formula
 * still defines every node (a stored left child with an absent right one gives (p_l, q_l)).
 * d_p_layers, d_q_layers: 2^num_vars - 1 elements each in the layout of sr_prod_tree (layer k at element offset
 * 2^num_vars - 2^(num_vars - k + 1), the root last), every layer in full, every word canonical.  d_q_layers is, word for word, what
 * sr_prod_tree_dev writes for d_q_leaves.  In trailing order the four operands of a layer (p_lo, p_hi, q_lo, q_hi) are contiguous halves
 * of the two layers below, usable as MLE tables as they lie:
 *   P_k(z) + l Q_k(z) = sum_b eq(z, b) (p_lo(b) q_hi(b) + p_hi(b) q_lo(b) + l q_lo(b) q_hi(b))
 * SR_E_INVALID, each with its own message: unknown order, num_vars >= 48, too many elements, n_leaves > 2^num_vars, a null output with
 * num_vars > 0, null d_q_leaves with n_leaves > 0, any overlap of an output with a stored input or of the two outputs (back-to-back
 * buffers and leaves that are not stored do not overlap).
 * The library allocates nothing and touches no context scratch: one chain of launches on `stream`, capturable on a fresh context.
 * sr_frac_tree_plan: pure host arithmetic -- *layer_elems = 2^num_vars - 1 (per output) and the kernel launches of the call: a launch
 * forms up to three levels on BabyBear, two on Goldilocks, Stark, goldilocks24 and frog16, one on babybear72 (registers), full launches
 * first, the remainder last.  num_vars = 0 is no launch and nothing written.
 * The host-pointer form stages like sr_prod_tree. */
int sr_frac_tree_plan(int ring, int log2_degree, size_t num_vars, int order, size_t *layer_elems, int *launches);
int sr_frac_tree_dev(sr_ctx *ctx, uint64_t *d_p_layers, uint64_t *d_q_layers, const uint64_t *d_p_leaves, const uint64_t *d_q_leaves,
                     size_t n_leaves, size_t num_vars, int order, void *stream);
int sr_frac_tree(sr_ctx *ctx, uint64_t *p_layers, uint64_t *q_layers, const uint64_t *p_leaves, const uint64_t *q_leaves, size_t n_leaves,
                 size_t num_vars, int order);
/* Linear combinations (csrc/lincomb.hpp): up to SR_LINCOMB_MAX_OUTPUTS tables from up to SR_LINCOMB_MAX_TABLES in one pass, with
 * ring-element coefficients -- the leaves of a permutation argument (beta + f + gamma id, beta + f + gamma sigma) or a logUp lookup
 * (beta - sum_k gamma^k col_k), the fold sum_i rho_i f_i of many instances into one, many MLEs batched into one.  For every ring id,
 * with elements in CRT/NTT form, `*` the slot product of sr_mul_elem_add_batch and `+` the slot sum:
 *   out_m[e] = [bit n_tables of uses[m]] coef[m][n_tables]  +  sum_{k < n_tables, bit k of uses[m]} coef[m][k] * T_k[e]      e < n
 * It is the composition of three operators of crates/poly's DenseMultilinearExtension: AddAssign<(R, &Self)> (mle/dense.rs:288-317),
 * MulAssign<R> (:370-374) and Add<R> (:386-395).  The constant goes to every one of the n output elements: that is the mathematical
 * definition, whereas the reference's Add<R> touches only the stored evaluations of a truncated MLE.
 * d_outs, d_tables: HOST arrays of n_outputs / n_tables device pointers; they reach the kernel by value, so a captured graph holds no
 * host pointer.  d_coef: n_outputs x (n_tables + 1) ring elements on the device, row-major, entry n_tables of a row the additive
 * constant.  uses: a HOST array of one bit mask per output; an entry of d_coef whose bit is clear is never read and may hold anything.
 * n_evals[k] <= n: the stored part of table k; the rest of it is zero and is never loaded.  n_evals == NULL: every table is full.
 * All n elements of every output are written.  Canonical inputs give canonical outputs.  n = 0 succeeds and launches nothing; n < 2^48.
 * Nothing is allocated and no context scratch is touched: no warm-up and no sr_ctx_reserve_scratch before a capture.
 * Tables may coincide or overlap each other.  Outputs are mutually disjoint and disjoint from d_coef.  An output may be the same
 * buffer as a table (the same base pointer: in place) only when n_outputs == 1 -- several outputs may go in several launches, and a
 * later launch would read what an earlier one wrote.  Every other overlap is SR_E_INVALID.  Also SR_E_INVALID, each with its own
 * message and before any device work: a null context (first), n_tables outside 1 .. 16, n_outputs outside 1 .. 4, a null pointer, a
 * mask of zero, a mask bit above n_tables, a table that no output uses, n_evals[k] > n.
 * sr_lincomb_plan: pure host arithmetic -- the kernel launches of a call and the outputs one launch produces.  A call of at most
 * four tables whose outputs fit one launch keeps its coefficients in registers (two outputs on Goldilocks and BabyBear, one on Stark
 * and goldilocks24, none on babybear72 and frog16); otherwise a launch produces four outputs on BabyBear, three on Goldilocks, one on
 * the other rings, and reads every table once per launch.
 * The host-pointer form stages whole tables like sr_mle_fix_variables (the chunked pipeline takes two operands, not seventeen): the
 * stored parts of the tables, the outputs and the coefficients live in context-owned device temporaries for the call. */
enum { SR_LINCOMB_MAX_TABLES = 16, SR_LINCOMB_MAX_OUTPUTS = 4 };
int sr_lincomb_plan(int ring, int log2_degree, int n_tables, int n_outputs, int *launches, int *outputs_per_launch);
int sr_lincomb_dev(sr_ctx *ctx, uint64_t *const *d_outs, int n_outputs, const uint64_t *const *d_tables, const size_t *n_evals,
                   int n_tables, const uint64_t *d_coef, const uint32_t *uses, size_t n, void *stream);
int sr_lincomb(sr_ctx *ctx, uint64_t *const *outs, int n_outputs, const uint64_t *const *tables, const size_t *n_evals, int n_tables,
               const uint64_t *coef, const uint32_t *uses, size_t n);
/* Integer columns (csrc/lincomb_index.hpp): a linear combination whose inputs are tables of ring elements AND columns of integers,
 *   out_m[e] = [bit K+J of uses[m]] coef[m][K+J]  +  sum_{k < K, bit k} coef[m][k] * T_k[e]
 *            + sum_{j < J, bit K+j} coef[m][K+j] * R::from(col_j[e])                  e < n, 0 <= K <= 16, 0 <= J <= 8, 1 <= K + J <= 16
 * -- sr_lincomb (mle/dense.rs:288-317, :370-374, :386-395) with R::from(u64) = from_scalar(BaseRing::from(x)) in CRT / NTT form as a
 * further kind of operand: x mod p in every coefficient of a power-of-two ring, in component 0 of every slot of goldilocks24 /
 * babybear72 / frog16 (what sr_add_scalar_batch adds with ntt_form != 0), so coef * R::from(x) scales every base-field component of
 * coef by x mod p (sr_scale_batch); x >= p (Goldilocks, frog16) is reduced.  A column is n_evals <= n stored uint64_t (the rest count
 * as 0 and are never read) or, with values == NULL, the progression start, start + 1, .. which reads no memory: the reference's
 * identity_permutation[_mles] / random_permutation[_mles] (crates/poly/src/polynomials/multilinear_polynomial.rs:79-133), the table
 * side of a logUp lookup over small integers and its multiplicities need no ring table.  A row of coef has K + J + 1 elements -- tables,
 * columns, the constant -- and the mask bits follow that order.  The array `columns` is a HOST array in both forms, consumed at call
 * time (its entries travel in the kernel arguments); in the _dev form `values` is a DEVICE pointer.
 * sr_lincomb_index_dev keeps sr_lincomb_dev's promises: nothing allocated, no context scratch, capturable without warm-up, canonical in
 * gives canonical out, n == 0 succeeds and launches nothing, n < 2^48, in place for one output; with n_index == 0 it is sr_lincomb_dev.
 * SR_E_INVALID, each with its own message and before any device work: a null context (first), counts outside the bounds above, a null
 * pointer where one is needed, a mask of zero, a mask bit above K + J, a table or column that no output uses, n_evals > n, values !=
 * NULL with start != 0, a progression with start + (n - 1) > 2^64 - 1, an output overlapping a column's array or d_coef, and the
 * aliasing rules of sr_lincomb_dev for tables and outputs.
 * sr_lincomb_index_plan: pure host arithmetic, as sr_lincomb_plan; K + J <= 4 keeps the coefficients in registers (two outputs on
 * Goldilocks and BabyBear, one on goldilocks24), otherwise four outputs per launch on BabyBear, three on Goldilocks, one elsewhere.
 * sr_index_count[_dev]: counts[t] = #{ i : idx[i] == t } as uint64_t for t < n_bins, n and n_bins below 2^48.  The call clears counts
 * itself, on the stream.  The _dev form skips an index >= n_bins and counts it with the out-of-range columns of spmv
 * (sr_spmv_bad_index_count); the host form validates and returns SR_E_INVALID.  Up to 4096 bins are counted in LDS per workgroup. */
enum { SR_LINCOMB_MAX_INDEX_COLUMNS = 8 };
typedef struct sr_index_column {
    const uint64_t *values; /* n_evals integers (a DEVICE pointer in the _dev form), or NULL: the progression start, start + 1, .. */
    size_t n_evals;         /* stored entries <= n, the rest count as 0; ignored for a progression */
    uint64_t start;         /* first value of a progression; 0 when values != NULL */
} sr_index_column;
int sr_lincomb_index_plan(int ring, int log2_degree, int n_tables, int n_index, int n_outputs, int *launches, int *outputs_per_launch);
int sr_lincomb_index_dev(sr_ctx *ctx, uint64_t *const *d_outs, int n_outputs, const uint64_t *const *d_tables, const size_t *n_evals,
                         int n_tables, const sr_index_column *columns, int n_index, const uint64_t *d_coef, const uint32_t *uses, size_t n,
                         void *stream);
int sr_lincomb_index(sr_ctx *ctx, uint64_t *const *outs, int n_outputs, const uint64_t *const *tables, const size_t *n_evals, int n_tables,
                     const sr_index_column *columns, int n_index, const uint64_t *coef, const uint32_t *uses, size_t n);
int sr_index_count_dev(sr_ctx *ctx, uint64_t *d_counts, const uint64_t *d_idx, size_t n, size_t n_bins, void *stream);
int sr_index_count(sr_ctx *ctx, uint64_t *counts, const uint64_t *idx, size_t n, size_t n_bins);
/* Integer columns in weighted sum-check rounds (csrc/sumcheck_index.hpp): a factor that is really a column of integers -- the selectors
 * of a Plonkish gate, a 0/1 mask, a multiplicity column out of sr_index_count_dev, sigma, id -- is read as one uint64_t per row (or not
 * at all: a progression) by the first message and the first fold, and never expanded to a ring table.
 *   slots   terms[k].table[s] in 0 .. K - 1 are the ring tables, K .. K + J - 1 the columns, in the order of the arrays;
 *           0 <= K, 0 <= J <= 8, 1 <= K + J <= SR_VPOLY_MAX_TABLES; K == 0 is a claim over columns only
 * With E_j the table R::from(col_j[e]), e < n_evals_j, as sr_lincomb_index_dev writes it (a progression: n_evals_j = 2^num_vars),
 * sr_vpoly_iwround_evals_dev writes in d_out exactly what sr_vpoly_wround_evals_dev writes over T_0 .. T_{K-1}, E_0 .. E_{J-1}, and
 * sr_vpoly_iwround_fold_evals_dev writes in d_out, d_out_tables[0 .. K+J-1] and n_evals_out[0 .. K+J-1] exactly what
 * sr_vpoly_wround_fold_evals_dev writes over those tables -- every word.  A folded column slot is a ring table of (n_evals_j + 1) / 2
 * (leading) or min(n_evals_j, 2^(num_vars-1)) (trailing) elements with a buffer of its own; nothing beyond that length is touched, a
 * stored value beyond n_evals_j counts as 0 and is never read, values >= p are reduced.  After the first fold every slot is a ring
 * table and the weighted calls carry on.  With n_index == 0 the calls ARE the weighted calls.
 * d_weights is required; order is SR_MLE_LEADING or SR_MLE_TRAILING; 1 <= num_vars (fused: 2) < 48.  The promises of the weighted
 * calls hold: nothing allocated, no context scratch, every workspace word written before it is read, one chain of launches on one
 * stream (capturable on a fresh context), canonical in gives canonical out, every ring id; terms, d_tables, d_out_tables, n_evals and
 * columns are host arrays consumed at call time; a trailing-order fold may run in place for table slots.
 * SR_E_INVALID, each with its own message and before any device work: every refusal of the weighted calls; n_index outside 0 .. 8;
 * K + J outside 1 .. 8; null columns with n_index > 0; a column no term uses; n_evals_j > 2^num_vars; values != NULL with start != 0;
 * a progression with start + 2^num_vars - 1 > 2^64 - 1; a column's array overlapping d_out, d_work or a folded table.  Column arrays
 * may overlap each other and may be the same pointer in two slots.
 * sr_vpoly_iwround_plan (fold: 0 the message, 1 the fused call) is pure host arithmetic with the records of sr_vpoly_wround[_fold]_plan
 * and the points per launch of the weighted calls at K + J slots.  The host-pointer forms stage their operands as
 * sr_vpoly_wround_evals does. */
int sr_vpoly_iwround_plan(int ring, int log2_degree, size_t num_vars, int n_tables, int n_index, int n_terms, int degree, int order, int fold,
                          size_t *work_elems, int *launches);
int sr_vpoly_iwround_evals_dev(sr_ctx *ctx, uint64_t *d_out, const uint64_t *d_weights, const uint64_t *const *d_tables, const size_t *n_evals,
                               int n_tables, const sr_index_column *columns, int n_index, const sr_vpoly_term *terms, int n_terms,
                               const uint64_t *d_coeffs, size_t num_vars, int order, uint64_t *d_work, size_t work_elems, void *stream);
int sr_vpoly_iwround_evals(sr_ctx *ctx, uint64_t *out, const uint64_t *weights, const uint64_t *const *tables, const size_t *n_evals,
                           int n_tables, const sr_index_column *columns, int n_index, const sr_vpoly_term *terms, int n_terms,
                           const uint64_t *coeffs, size_t num_vars, int order);
int sr_vpoly_iwround_fold_evals_dev(sr_ctx *ctx, uint64_t *d_out, uint64_t *const *d_out_tables, size_t *n_evals_out, const uint64_t *d_weights,
                                    const uint64_t *const *d_tables, const size_t *n_evals, int n_tables, const sr_index_column *columns,
                                    int n_index, const sr_vpoly_term *terms, int n_terms, const uint64_t *d_coeffs, size_t num_vars,
                                    const uint64_t *d_r, int order, uint64_t *d_work, size_t work_elems, void *stream);
int sr_vpoly_iwround_fold_evals(sr_ctx *ctx, uint64_t *out, uint64_t *const *out_tables, size_t *n_evals_out, const uint64_t *weights,
                                const uint64_t *const *tables, const size_t *n_evals, int n_tables, const sr_index_column *columns, int n_index,
                                const sr_vpoly_term *terms, int n_terms, const uint64_t *coeffs, size_t num_vars, const uint64_t *r, int order);
/* Batch inversion (csrc/inverse.hpp): out[e] = num[e] * den[e]^-1 for e < n, slot by slot on tables in CRT / NTT form -- Field::inverse
 * / ark_ff::batch_inversion(&mut [F]) on every slot: the base field of a power-of-two ring, the Fq3 / Fq9 / Fq4 slots of goldilocks24 /
 * babybear72 / frog16.  d_num == NULL: every numerator is one().  `*` is the slot product (sr_pointwise_mul_batch), so for a ring
 * element a none of whose slots is zero, the result is the inverse of a in the ring.
 * Montgomery's trick: a lane inverts `chunk_elems` consecutive elements of its unit with ONE field inversion x^(|F| - 2) -- three
 * products per element and unit (four with numerators) plus the inversion shared by the chunk.
 * Zeros: a zero slot of den[e] cannot be inverted.  It does not disturb its neighbours; its output slot is ZERO, with or without a
 * numerator (batch_inversion leaves zeros in place), and it is added to a context counter that sr_inverse_zero_count reads and clears
 * (ordered on `stream`, like sr_spmv_bad_index_count).  The count is in slots: base-field coefficients of a power-of-two ring, Fq3 /
 * Fq9 / Fq4 slots otherwise.  A ring element is a unit exactly when none of its slots is zero, so a count of 0 says that every element
 * was invertible -- the `Some` of Field::inverse for the whole table.
 * Canonical inputs give canonical outputs.  n == 0 writes nothing and succeeds.  d_out may be exactly d_den or exactly d_num (in place).
 * Nothing is allocated and no context scratch is touched: capturable without warm-up or sr_ctx_reserve_scratch.  Pointers that are only
 * 8-byte aligned are taken one coefficient per lane, as by the streaming calls.
 * sr_inverse_plan: pure host arithmetic.  chunk_elems: the consecutive elements one lane inverts together (it depends on the ring and
 * on has_num); launches: 1, or 0 for n == 0; work_elems: the workspace the _dev call wants, 0 on every ring today -- d_work may then be
 * NULL -- and kept so that the call has the shape of its siblings.
 * SR_E_INVALID, each with its own message and before any device work: a null context (first), a null d_out or d_den, d_out
 * overlapping d_den or d_num without being that very pointer, a workspace below the plan, an element count too large, and for the plan
 * an unknown ring id or a log2_degree out of range.
 * The host-pointer form goes through the chunked staging pipeline of the element-wise calls (SR_HOST_CHUNK_MB). */
int sr_inverse_plan(int ring, int log2_degree, size_t n, int has_num, size_t *work_elems, int *launches, size_t *chunk_elems);
int sr_inverse_batch_dev(sr_ctx *ctx, uint64_t *d_out, const uint64_t *d_num /* may be NULL */, const uint64_t *d_den, size_t n,
                         uint64_t *d_work, size_t work_elems, void *stream);
int sr_inverse_batch(sr_ctx *ctx, uint64_t *out, const uint64_t *num /* may be NULL */, const uint64_t *den, size_t n);
int sr_inverse_zero_count(sr_ctx *ctx, unsigned long long *out, void *stream);
/* Norms of a coefficient slice on the device: WithLinfNorm::linf_norm / WithL2Norm::l2_norm_squared over [Fq]
 * (crates/ring/src/traits.rs:6-36; per element balanced_decomposition/convertible_ring.rs:49-66; the signed representative of
 * fq_convertible.rs:20-34 and stark_prime/decomposition.rs:40-52).
 * d_coeffs: n_coeffs base-field coefficients in the usual memory image (Montgomery form, canonical, `limbs` u64 words each: what
 * Flatten::flatten_to_coeffs gives for a Vec of ring elements, for every ring id; the call neither knows nor uses D).  Per coefficient
 * x = the standard-form integer, s = x if x <= (p - 1) / 2, else x - p; linf = max |s|, l2sq = sum s^2, exact non-negative integers.
 * NTT-form data is accepted and meaningless, as in the reference.  Words >= p are outside the contract.
 * Groups: the slice is n_coeffs / group consecutive groups of `group` coefficients (group >= 1, a divisor of n_coeffs, any value -- not
 * only powers of two), one result each: group = n_coeffs is the reference's slice norm, group = D one norm per ring element,
 * group = ncols * D one per matrix row.
 * which: SR_NORM_LINF | SR_NORM_L2SQ; both = one pass over the data.  Output per group, standard-form (NOT Montgomery) little-endian
 * u64 words: linf `limbs` words (1 or 4), then l2sq 3 words for the one-limb fields (s^2 < 2^126, at most 2^64 coefficients: the sum
 * is below 2^190) or 9 words for Stark (|s| < 2^251, s^2 < 2^502: the sum is below 2^566).
 * Empty slice: linf_norm of the reference panics (max().unwrap()), so n_coeffs == 0 with SR_NORM_LINF is SR_E_INVALID; l2sq of an empty
 * slice is ONE record of zero words, whatever `group`.
 * sr_norm_plan: pure host arithmetic, no device, no context: the words per group, the workspace in u64 words and the launches
 * (1 or 2).  Groups below 1024 coefficients take one launch and no workspace (a fixed number of lanes per group inside a wave); wider
 * groups are cut into spans of whole workgroups whose partial records go to the workspace and are combined by a second launch -- at
 * most 2^15 partial records per call (1 MiB for a one-limb field, 3.25 MiB for Stark), none when the groups alone fill the device.
 * sr_norm_batch_dev allocates nothing, touches no context scratch, writes every workspace word it later reads (the previous contents
 * do not matter, nothing is accumulated across calls) and can be captured into a HIP graph without a warm-up and replayed on changed
 * data.  d_coeffs needs 8-byte alignment only.  SR_E_INVALID: a null pointer, `which` outside 1..3, group == 0, n_coeffs % group != 0,
 * n_coeffs == 0 with SR_NORM_LINF, work_words below the plan's, d_out overlapping d_coeffs or d_work.  The result does not depend on
 * the grid or on scheduling: integer max and integer sums only.
 * sr_norm_batch (host pointers) streams the slice through the chunked staging pipeline (sr_plan.host_chunk_mb) and combines the
 * per-chunk partial records on the host with max / add-with-carry; a group may straddle chunks. */
#define SR_NORM_LINF 1
#define SR_NORM_L2SQ 2
int sr_norm_plan(int ring, size_t n_coeffs, size_t group, int which, size_t *out_words_per_group, size_t *work_words, int *launches);
int sr_norm_batch_dev(sr_ctx *ctx, uint64_t *d_out, const uint64_t *d_coeffs, size_t n_coeffs, size_t group, int which, uint64_t *d_work,
                      size_t work_words, void *stream);
int sr_norm_batch(sr_ctx *ctx, uint64_t *out, const uint64_t *coeffs, size_t n_coeffs, size_t group, int which);
/* First "next" row: y = M * v for a dense nrows x ncols matrix of ring elements in CRT/NTT form
 * (row-major, each entry one ring element) and a vector of ncols elements -- Matrix<RqNTT>::checked_mul_vec,
 * crates/linear_algebra/src/matrix.rs:168-178 -- as one fused multiply-accumulate pass over M.  Every ring id: the fully
 * split power-of-two rings (lane = slot) and the reference's own Goldilocks-24 / BabyBear-72 / Frog-16 (Fq3 / Fq9 / Fq4 slot
 * products, csrc/small_linalg.hpp); d_y must not alias d_m or d_v. */
int sr_matvec_ntt_dev(sr_ctx *ctx, uint64_t *d_y, const uint64_t *d_m, const uint64_t *d_v, size_t nrows, size_t ncols, void *stream);
/* y = S * v for a sparse nrows x ncols matrix in CSR form: d_vals[j] one ring element (CRT/NTT form), d_cols[j] its column,
 * d_row_ptr[r] .. d_row_ptr[r+1] the stored entries of row r -- SparseMatrix<RqNTT>::checked_mul_vec,
 * crates/linear_algebra/src/sparse_matrix.rs:201-211 (its Vec<Vec<(R, usize)>> rows, flattened; an empty row gives zero).
 * An entry with column >= ncols (the reference panics on v[col]) is skipped and counted; sr_spmv_bad_index_count reads
 * and clears that count (synchronises the stream).  The host-pointer form validates the indices and returns SR_E_INVALID. */
int sr_spmv_ntt_dev(sr_ctx *ctx, uint64_t *d_y, const uint64_t *d_vals, const uint32_t *d_cols, const uint64_t *d_row_ptr,
                    const uint64_t *d_v, size_t nrows, size_t ncols, void *stream);
int sr_spmv_bad_index_count(sr_ctx *ctx, unsigned long long *out, void *stream);
/* Y (n x p) = A (n x m) * B (m x p), dense row-major, CRT/NTT form -- Matrix<RqNTT>::checked_mul_mat,
 * crates/linear_algebra/src/matrix.rs:148-166.  d_y must not alias d_a or d_b. */
int sr_matmul_ntt_dev(sr_ctx *ctx, uint64_t *d_y, const uint64_t *d_a, const uint64_t *d_b, size_t n, size_t m, size_t p, void *stream);
/* Host-pointer forms of the three linear-algebra entry points (temporaries allocated per call). */
int sr_matvec_ntt(sr_ctx *ctx, uint64_t *y, const uint64_t *m, const uint64_t *v, size_t nrows, size_t ncols);
int sr_spmv_ntt(sr_ctx *ctx, uint64_t *y, const uint64_t *vals, const uint32_t *cols, const uint64_t *row_ptr, const uint64_t *v,
                size_t nrows, size_t ncols);
int sr_matmul_ntt(sr_ctx *ctx, uint64_t *y, const uint64_t *a, const uint64_t *b, size_t n, size_t m, size_t p);
/* Symmetric matrices (csrc/symmetric.hpp): SymmetricMatrix<F>, crates/linear_algebra/src/symmetric_matrix.rs:14-92, over ring elements in
 * CRT/NTT form, every ring id, canonical in and canonical out.  A symmetric matrix of size n is PACKED: n (n + 1) / 2 ring elements,
 * entry (i, j) with j <= i is element i (i + 1) / 2 + j -- the reference's Vec<Vec<F>> rows (row i has i + 1 entries), flattened.
 * sr_gram_ntt[_dev]: d_a is a dense row-major n x m matrix, out[i (i + 1) / 2 + j] = sum_{t < m} a[i][t] * a[j][t] with `*` the slot
 * product of the ring.  This is what SymmetricMatrix::from_par_fn(n, |i, j| <s_i, s_j>) (symmetric_matrix.rs:76-90) yields for the
 * inner-product closure over n vectors of m ring elements; that closure is the caller's and is not in the reference.  m == 0 gives
 * all zero(); n == 0 writes nothing.  The sums are exact modular integers: any summation order gives the reference's bits.  Only the
 * lower triangle is computed, both operands are rows of A (no transposed copy exists), and a short, wide A (few tiles over a long
 * inner dimension) is cut into spans of the inner dimension whose partial packed matrices go to d_work and are added by a second
 * launch.
 * sr_symm_recompose[_dev]: recompose_left_right_symmetric_matrix (crates/ring/src/balanced_decomposition/mod.rs:354-386), G^T M G for
 * the gadget matrix G = I_n (x) powers.  d_mat is a packed matrix of size n * d, d_powers holds d ring elements (powers_of_basis: ring
 * elements in the reference too), out is packed of size n: out(i, j) = sum_{a, b < d} mat[(i d + a, j d + b)] * (powers[a] * powers[b]),
 * where mat[(k, l)] is the symmetric lookup (l > k reads (l, k)).  d == 0 is the reference's division by zero: SR_E_INVALID.  n == 0
 * writes nothing.  The first launch writes the d^2 weights powers[a] * powers[b] to d_work, the second streams d_mat once.
 * sr_gram_plan / sr_symm_recompose_plan: pure host arithmetic, no device, no context: the workspace in ring elements and the number
 * of launches (Gram: 1 without workspace, or 2 with nsplit * n (n + 1) / 2 elements; recompose: 2 with d^2 elements; 0 and 0 for
 * n == 0).  The Gram's split depends on the shape alone: fewer than 1024 workgroups of tiles, at least 64 inner indices per span (32
 * for Goldilocks-24 and BabyBear-72), at most 64 spans.
 * The _dev calls allocate nothing, touch no context scratch, write every workspace word they later read and can be captured into a
 * HIP graph without a warm-up.  SR_E_INVALID: a null pointer where something would be read or written, work_elems below the plan's,
 * the output overlapping an input or the workspace, n (n + 1) / 2 or n * d overflowing size_t, a grid past one launch's limit.  The
 * host-pointer forms stage whole operands in context-owned temporaries. */
int sr_gram_plan(int ring, int log2_degree, size_t n, size_t m, size_t *work_elems, int *launches);
int sr_gram_ntt_dev(sr_ctx *ctx, uint64_t *d_out, const uint64_t *d_a, size_t n, size_t m, uint64_t *d_work, size_t work_elems, void *stream);
int sr_gram_ntt(sr_ctx *ctx, uint64_t *out, const uint64_t *a, size_t n, size_t m);
int sr_symm_recompose_plan(int ring, int log2_degree, size_t n, size_t d, size_t *work_elems, int *launches);
int sr_symm_recompose_dev(sr_ctx *ctx, uint64_t *d_out, const uint64_t *d_mat, size_t n, size_t d, const uint64_t *d_powers, uint64_t *d_work,
                          size_t work_elems, void *stream);
int sr_symm_recompose(sr_ctx *ctx, uint64_t *out, const uint64_t *mat, size_t n, size_t d, const uint64_t *powers);
/* Sparse matrices (csrc/sparse_matrix.hpp): SparseMatrix::transpose and Matrix::transpose (crates/linear_algebra/src/ops.rs:9-62) and
 * SparseMatrix::checked_mul_mat (sparse_matrix.rs:219-281, the Mul<&SparseMatrix> of :293-301), over ring elements in CRT/NTT form, every
 * ring id, canonical in and canonical out.  A sparse matrix is the CSR triple of sr_spmv_ntt_dev: uint32_t columns, uint64_t row pointers
 * (row_ptr[0] == 0); positions into a value array are uint32_t, so an operand with 2^32 or more stored entries is SR_E_INVALID.  The index
 * work is host arithmetic without device or context; the device moves and multiplies whole ring elements by position.
 * sr_sparse_transpose_pattern: a stable counting sort by column.  Row c of the transpose lists the original rows (t_cols) of the entries in
 * column c, ascending, whatever the order inside the input rows; t_vals[t] = vals[perm[t]].  SR_E_INVALID: a column >= ncols (the reference
 * panics there), a non-monotone row_ptr or row_ptr[0] != 0, a null pointer, more than 2^32 - 1 rows.
 * sr_spgemm_pattern: the STRUCTURAL product of A (n x m) and B (m x p): one entry per (i, j) whose index lists intersect, rows ascending in
 * j, and per entry e the intersecting positions pair_a[t] into a_vals and pair_b[t] into b_vals for pair_ptr[e] <= t < pair_ptr[e + 1],
 * ascending in k.  With the five output arrays null it only counts (*n_out, *n_pairs), so that a caller can size them; with buffers it
 * fills them.  Both operands must have strictly ascending rows and indices in range (hconcat, from_dense, identity and rand produce such
 * rows; the reference's merge-join means nothing otherwise): SR_E_INVALID.  Cost: nnz_a + nnz_b + n_pairs + n + m + p steps.
 * sr_spgemm_ntt_dev: d_out_vals[e] = sum of d_a_vals[pair_a[t]] * d_b_vals[pair_b[t]] over the pairs of entry e, `*` the slot product;
 * d_live[e] = 1 iff some product of the entry is a non-zero ring element (NTT-form elements have zero divisors, so the reference's stored
 * pattern depends on the values), else 0.  The number of entries with d_live == 0 is added to a context counter that sr_spgemm_dead_count
 * reads and clears (synchronises the stream).  With a dead count of 0 the structural pattern is the reference's result; otherwise the
 * caller drops the dead entries.  A live entry may hold zero (a b + (-a) b).  A position >= nnz_a / nnz_b is skipped.  n_out == 0 writes
 * nothing.  SR_E_INVALID: a null pointer, d_out_vals or d_live overlapping each other, an input or the workspace, a size overflow, a grid
 * past one launch's limit.
 * sr_spgemm_plan: host arithmetic on (n_out, n_pairs) only.  Pair lists are never cut into spans: work_elems is always 0 (d_work may be
 * null) and launches is 2 -- the numeric kernel and the count of the dead entries -- or 0 for n_out == 0.
 * sr_gather_batch_dev: d_out[t] = d_in[d_perm[t]] on whole ring elements, out of place; d_perm[t] >= n_in leaves element t unwritten and
 * is counted with the out-of-range columns of spmv (sr_spmv_bad_index_count).  sr_transpose_dev: dense d_out[j][i] = d_in[i][j] for a
 * row-major nrows x ncols d_in, out of place.  (Matrix::transpose copies nrows and ncols unswapped, ops.rs:36-44; the data it returns is the
 * ncols x nrows matrix written here.)
 * The _dev calls allocate nothing, touch no context scratch, write every flag word they later read and can be captured into a HIP graph
 * without a warm-up.  The host-pointer forms stage whole operands in context-owned temporaries; sr_spgemm_ntt runs pattern, numeric phase
 * and compaction and returns exactly the reference's SparseMatrix (out_vals and out_cols need room for the structural n_out entries,
 * *nnz_out is the number kept). */
int sr_sparse_transpose_pattern(const uint32_t *cols, const uint64_t *row_ptr, size_t nrows, size_t ncols, uint64_t *t_row_ptr /* ncols + 1 */,
                                uint32_t *t_cols /* nnz */, uint32_t *perm /* nnz */);
int sr_spgemm_pattern(const uint32_t *a_cols, const uint64_t *a_row_ptr, size_t n, size_t m, const uint32_t *b_cols, const uint64_t *b_row_ptr,
                      size_t p, uint64_t *out_row_ptr /* n + 1 */, uint32_t *out_cols, uint64_t *pair_ptr /* n_out + 1 */, uint32_t *pair_a,
                      uint32_t *pair_b, size_t *n_out, size_t *n_pairs);
int sr_spgemm_plan(int ring, int log2_degree, size_t n_out, size_t n_pairs, size_t *work_elems, int *launches);
int sr_gather_batch_dev(sr_ctx *ctx, uint64_t *d_out, const uint64_t *d_in, const uint32_t *d_perm, size_t n_out, size_t n_in, void *stream);
int sr_transpose_dev(sr_ctx *ctx, uint64_t *d_out, const uint64_t *d_in, size_t nrows, size_t ncols, void *stream);
int sr_spgemm_ntt_dev(sr_ctx *ctx, uint64_t *d_out_vals, uint32_t *d_live, const uint64_t *d_a_vals, size_t nnz_a, const uint64_t *d_b_vals,
                      size_t nnz_b, const uint64_t *d_pair_ptr, const uint32_t *d_pair_a, const uint32_t *d_pair_b, size_t n_out, size_t n_pairs,
                      uint64_t *d_work, size_t work_elems, void *stream);
int sr_spgemm_dead_count(sr_ctx *ctx, unsigned long long *out, void *stream);
int sr_sparse_transpose(sr_ctx *ctx, uint64_t *t_vals, uint32_t *t_cols, uint64_t *t_row_ptr, const uint64_t *vals, const uint32_t *cols,
                        const uint64_t *row_ptr, size_t nrows, size_t ncols);
int sr_transpose(sr_ctx *ctx, uint64_t *out, const uint64_t *in, size_t nrows, size_t ncols);
int sr_spgemm_ntt(sr_ctx *ctx, uint64_t *out_vals, uint32_t *out_cols, uint64_t *out_row_ptr, size_t *nnz_out, const uint64_t *a_vals,
                  const uint32_t *a_cols, const uint64_t *a_row_ptr, size_t n, size_t m, const uint64_t *b_vals, const uint32_t *b_cols,
                  const uint64_t *b_row_ptr, size_t p);
/* Cyclotomic::rot (crates/ring/src/traits.rs:54-66): every ring element of the batch (COEFFICIENT form) times X, modulo X^D + 1
 * (stark_prime/mod.rs:87-95, frog_ring/mod.rs:126-134 and the power-of-two rings) or X^D - X^(D/2) + 1 (goldilocks/mod.rs:138-149,
 * babybear/mod.rs:150-161).  The device form is out of place (d_out must not alias d_in); the host form works in place. */
int sr_rot_batch_dev(sr_ctx *ctx, uint64_t *d_out, const uint64_t *d_in, size_t batch, void *stream);
int sr_rot_batch(sr_ctx *ctx, uint64_t *data, size_t batch);
/* Second "next" row: balanced gadget decomposition, coefficient-wise, of `batch` ring elements in COEFFICIENT
 * form: digit j of element e is ring element e * padding_size + j of d_out (batch * padding_size elements) --
 * GadgetDecompose for &[R] (crates/ring/src/balanced_decomposition/mod.rs:163-175) over Decompose for the ring
 * (cyclotomic_ring/coeff_form.rs:587-605) over decompose_balanced_in_place (mod.rs:62-117; signed representative
 * fq_convertible.rs:21-35, stark_prime/decomposition.rs:41-53).  basis: any even value in [2, 2^64) here and the reference's whole u128 range through the
 * _wide forms below (it panics on 0, 1 and odd values: SR_E_INVALID).  Every ring id; digits are field elements in the same Montgomery
 * layout.  A coefficient that needs more than padding_size digits makes the reference panic (out[i] out of bounds): the
 * device form writes the first padding_size digits and counts it (sr_decompose_overflow_count reads and clears the count,
 * synchronising the stream); the host form returns SR_E_INVALID. */
int sr_decompose_balanced_batch_dev(sr_ctx *ctx, uint64_t *d_out, const uint64_t *d_in, uint64_t basis, size_t padding_size,
                                    size_t batch, void *stream);
int sr_decompose_overflow_count(sr_ctx *ctx, unsigned long long *out, void *stream);
/* GadgetRecompose (mod.rs:177-189, recompose :119-131): d_out[e] = sum_j basis^j * d_in[e * padding_size + j], batch_out elements */
int sr_recompose_batch_dev(sr_ctx *ctx, uint64_t *d_out, const uint64_t *d_in, uint64_t basis, size_t padding_size,
                           size_t batch_out, void *stream);
int sr_decompose_balanced_batch(sr_ctx *ctx, uint64_t *out, const uint64_t *in, uint64_t basis, size_t padding_size, size_t batch);
int sr_recompose_batch(sr_ctx *ctx, uint64_t *out, const uint64_t *in, uint64_t basis, size_t padding_size, size_t batch_out);
/* The reference's full u128 basis range: basis = basis_hi * 2^64 + basis_lo (basis_hi = 0: the calls above).  With basis >= 2^64 a
 * coefficient of a one-limb field (|x| < 2^63 < basis / 2) is its own digit 0 and every other digit is zero; for the 252-bit Stark
 * prime the digits come from a 256-by-128-bit division per digit. */
int sr_decompose_balanced_batch_wide_dev(sr_ctx *ctx, uint64_t *d_out, const uint64_t *d_in, uint64_t basis_lo, uint64_t basis_hi,
                                         size_t padding_size, size_t batch, void *stream);
int sr_recompose_batch_wide_dev(sr_ctx *ctx, uint64_t *d_out, const uint64_t *d_in, uint64_t basis_lo, uint64_t basis_hi,
                                size_t padding_size, size_t batch_out, void *stream);
int sr_decompose_balanced_batch_wide(sr_ctx *ctx, uint64_t *out, const uint64_t *in, uint64_t basis_lo, uint64_t basis_hi,
                                     size_t padding_size, size_t batch);
int sr_recompose_batch_wide(sr_ctx *ctx, uint64_t *out, const uint64_t *in, uint64_t basis_lo, uint64_t basis_hi, size_t padding_size,
                            size_t batch_out);
/* Third "next" row: the ark-serialize canonical wire format of a batch of ring elements --
 * CanonicalSerialize / CanonicalDeserialize for RqPoly (crates/ring/src/cyclotomic_ring/coeff_form.rs:154-189) and RqNTT
 * (ntt_form.rs:24, derived), both the flat coefficient array: each coefficient is the standard-form integer (out of
 * Montgomery form) as sr_wire_coeff_bytes() little-endian bytes (8 Goldilocks / frog, 4 BabyBear, 32 Stark; ark-ff 0.4.2
 * Fp::serialize_with_flags with EmptyFlags, third party: the byte layout is restated from the published format and is
 * PARITY UNPINNED -- the reference holds no serialised golden bytes).  An element is D * sr_wire_coeff_bytes() bytes; no
 * length prefix (the u64 length words of Vec / Matrix / SparseMatrix, matrix.rs:111-145, sparse_matrix.rs:158-200, are
 * host-side framing: include/stark_rings.hpp, stark_rings_amd/wire.py).
 * d_offsets (optional, device, one u64 per element): byte offset of the element inside the wire buffer, multiples of 8 (4 for the
 * BabyBear rings), so the
 * caller can leave room for its framing words; NULL = densely packed.  Wire and element buffers must not overlap.
 * Deserialising a coefficient >= p is ark's SerializationError::InvalidData: the device form stores 0 for it and counts it
 * (sr_wire_invalid_count reads and clears the count, synchronising the stream; misaligned offsets are counted there too and
 * their elements skipped); the host form returns SR_E_INVALID. */
size_t sr_wire_coeff_bytes(const sr_ctx *ctx);
int sr_serialize_batch_dev(sr_ctx *ctx, uint8_t *d_wire, const uint64_t *d_in, const uint64_t *d_offsets, size_t batch, void *stream);
int sr_deserialize_batch_dev(sr_ctx *ctx, uint64_t *d_out, const uint8_t *d_wire, const uint64_t *d_offsets, size_t batch,
                             void *stream);
int sr_wire_invalid_count(sr_ctx *ctx, unsigned long long *out, void *stream);
int sr_serialize_batch(sr_ctx *ctx, uint8_t *wire, const uint64_t *in, size_t batch);
int sr_deserialize_batch(sr_ctx *ctx, uint64_t *out, const uint8_t *wire, size_t batch);
/* RqPoly * &RqPoly (coeff_form.rs:250-258): d_a and d_b are only read -- the reference never mutates an operand, so one b can
 * be multiplied into many a.  d_out may alias d_a; d_b must not alias d_out.  Above one LDS tile the intermediates go
 * through the context's operand scratch (sr_ctx_reserve_scratch).  Stream semantics: one stream-ordered operation on `stream`;
 * a batch of three and a half chunks or more (64 MiB of coefficients each by default; with sr_plan.chunk_polys set: more than one
 * chunk) is forked onto the context's two internal streams and joined back onto `stream` before the call returns (sr_plan.lanes = 1, or the library's own choice when
 * lanes = 0 and its probe found one stream faster: everything on `stream` itself). */
int sr_ring_mul_batch_dev(sr_ctx *ctx, uint64_t *d_out, const uint64_t *d_a, const uint64_t *d_b, size_t batch, void *stream);
/* The constant-operand case: d_b_ntt already holds crt(b) (sr_ntt_fwd_batch_dev), e.g. the rows of a commitment matrix that
 * stay in NTT form (matrix.rs:168-178) while fresh coefficient-form elements arrive: d_out = icrt(crt(d_a) (.) d_b_ntt),
 * one of the three transforms saved.  Every ring id (rings without a fused kernel run forward transform, slot product and
 * inverse transform one after the other on d_out).  d_out may alias d_a; d_b_ntt is only read and must not alias d_out. */
int sr_ring_mul_ntt_rhs_batch_dev(sr_ctx *ctx, uint64_t *d_out, const uint64_t *d_a, const uint64_t *d_b_ntt, size_t batch, void *stream);
/* host-pointer form (staged through device memory like sr_ring_mul_batch) */
int sr_ring_mul_ntt_rhs_batch(sr_ctx *ctx, uint64_t *out, const uint64_t *a, const uint64_t *b_ntt, size_t batch);
int sr_reduce_batch_dev(sr_ctx *ctx, const uint64_t *d_in, size_t in_len_per_elem, uint64_t *d_out, size_t batch, void *stream);
/* ---- packed-u32 boundary, SR_RING_BABYBEAR_POW2 only (opt-in; BASELINE configs[2] "packed 32-bit modmul") -------------------------
 * The reference keeps a BabyBear coefficient in an ark-ff Fp64: one u64 limb holding a * 2^64 mod p with p < 2^31
 * (crates/ring/src/cyclotomic_ring/models/babybear/mod.rs:18-26), i.e. the upper 32 bits of every word are zero.  The PACKED image
 * of a coefficient is the low half of that limb: the uint32_t (a * 2^64 mod p), canonical in [0, p) -- the same Montgomery residue
 * (R = 2^64, not 2^32) in four bytes.  A packed batch is batch * D such words, element-major like everything else.  These entry
 * points are the packed twins of sr_ntt_fwd/inv_batch_dev (CRT::elementwise_crt / ICRT::elementwise_icrt, crt.rs:10-49),
 * sr_ring_mul_batch_dev (RqPoly * &RqPoly, coeff_form.rs:250-258; operands only read, d_out may alias d_a, not d_b),
 * sr_pointwise_mul_batch_dev (ntt_form.rs:213-225) and sr_add/sub_batch_dev, value for value: unpack32(f_packed(pack32(x))) ==
 * f(x) bit for bit.  For D >= 4096 the register-tiled kernels read and write the packed words directly (half the boundary
 * bytes of the 8-byte layout); smaller degrees are widened into context-owned staging, computed and narrowed again.
 * sr_pack32_batch_dev takes the low word of every limb (the caller guarantees canonical images, whose high word is zero);
 * sr_unpack32_batch_dev zero-extends.  Neither may run in place. */
int sr_pack32_batch_dev(sr_ctx *ctx, uint32_t *d_out, const uint64_t *d_in, size_t batch, void *stream);
int sr_unpack32_batch_dev(sr_ctx *ctx, uint64_t *d_out, const uint32_t *d_in, size_t batch, void *stream);
int sr_ntt_fwd_packed32_batch_dev(sr_ctx *ctx, uint32_t *d_data, size_t batch, void *stream);
int sr_ntt_inv_packed32_batch_dev(sr_ctx *ctx, uint32_t *d_data, size_t batch, void *stream);
int sr_ring_mul_packed32_batch_dev(sr_ctx *ctx, uint32_t *d_out, const uint32_t *d_a, const uint32_t *d_b, size_t batch, void *stream);
int sr_pointwise_mul_packed32_batch_dev(sr_ctx *ctx, uint32_t *d_lhs_inout, const uint32_t *d_rhs, size_t batch, void *stream);
int sr_add_packed32_batch_dev(sr_ctx *ctx, uint32_t *d_lhs_inout, const uint32_t *d_rhs, size_t batch, void *stream);
int sr_sub_packed32_batch_dev(sr_ctx *ctx, uint32_t *d_lhs_inout, const uint32_t *d_rhs, size_t batch, void *stream);
/* Synthetic coefficients, uniform in [0,p), counter-based (same definition as the oracle's
 * sro_fill_uniform): fills n_coeffs coefficients starting at flat coefficient index first_coeff. */
int sr_fill_uniform_dev(sr_ctx *ctx, uint64_t seed, uint64_t first_coeff, size_t n_coeffs, uint64_t *d_out, void *stream);
/* Counts coefficients that are not canonical (>= p); used by validation code. */
int sr_count_noncanonical_dev(sr_ctx *ctx, const uint64_t *d_data, size_t n_coeffs, uint64_t *host_count, void *stream);

/* ---- per-kernel timing for the bench harness: when enabled, every kernel launch is bracketed by
 *      HIP events recorded on the stream it is launched on.  sr_ctx_profile_read drains them into
 *      SR_PROF_NTAGS accumulated-milliseconds / launch-count slots and resets the accumulators. ---- */
enum sr_prof_tag {
    SR_PROF_FWD_COLS = 0,  /* strided forward stages (D > one LDS tile)                      */
    SR_PROF_ROWS = 1,      /* in-tile stages; for ring_mul the fused fwd(a),fwd(b),mul,inv kernel */
    SR_PROF_INV_COLS = 2,  /* strided inverse stages                                          */
    SR_PROF_POINTWISE = 3,
    SR_PROF_OTHER = 4,
    SR_PROF_NTAGS = 5
};
/* on = 0: off; 1: every launch bracketed; N >= 2: every N-th launch only -- two event records around EVERY launch of a two-lane plan open
 * gaps in which the other lane's kernel runs alone, so fully bracketed steps read shorter in-flight durations than undisturbed ones; a
 * sparse sample (bench.py uses 7, coprime to the 3, 4 or 6 launches of a chunk) leaves the step as it runs.
 * sr_ctx_profile_read_sampled: ms_total / launches over the bracketed launches, seen = every launch that went by, per tag. */
int sr_ctx_profile_enable(sr_ctx *ctx, int on);
int sr_ctx_profile_read(sr_ctx *ctx, double ms_total[SR_PROF_NTAGS], uint64_t launches[SR_PROF_NTAGS]);
int sr_ctx_profile_read_sampled(sr_ctx *ctx, double ms_total[SR_PROF_NTAGS], uint64_t launches[SR_PROF_NTAGS], uint64_t seen[SR_PROF_NTAGS]);

/* Host-side self-test hook for the CPU test-suite: one scalar field operation computed by the same
 * source the kernels compile (fields.hpp).  field: 0 Goldilocks, 1 BabyBear, 2 Stark.
 * op: 0 add, 1 sub, 2 in-memory (Montgomery) product, 3 twiddle product, 4 table form of a[0]; field 0 only: 5 = the tuned path's
 * compile-time shift product a[0] * 2^b[0] mod p, 1 <= b[0] <= 95.
 * Not a compute path. */
int sr_selftest_field_op(int field, int op, const uint64_t *a, const uint64_t *b, uint64_t *out);

/* Test hook of the CHECKING build (libstarkrings_hip_check.so = the same sources compiled with -DSR_GL_CHECK_REPS): while the real
 * kernels of the tuned Goldilocks path run, every canonical butterfly counts a non-canonical input, every lazy butterfly a second
 * wrap or borrow, every result store a word >= p; the lazy nine-limb Stark arithmetic counts limb sums that leave int32 and
 * products that could overflow a column accumulator (csrc/fields.hpp: repcheck).  counters[0..6] as documented there, counters[7]
 * = the largest |limb| any Stark add / sub produced; reset != 0 clears them.  The counters are per-device symbols: the call visits EVERY
 * visible HIP device (synchronising each), sums [0..6] and takes the maximum of [7], so work done by contexts on any device is seen.
 * The product library returns SR_E_UNSUPPORTED: it carries no checks.
 * Not a compute path. */
int sr_selftest_rep_counters(uint64_t counters[8], int reset);

const char *sr_last_error_string(void);
const char *sr_version(void);

#ifdef __cplusplus
}
#endif
#endif /* STARK_RINGS_HIP_H */
