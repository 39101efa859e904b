// The prover's message of a sum-check round over a SUM OF PRODUCTS of dense multilinear extensions with ring coefficients
// (HyperPlonk's VirtualPolynomial, the shape of every claim a user of polynomials/multilinear_polynomial.rs actually proves):
//   g(x)     = sum_k c_k prod_{s < n_factors_k} f_{table_k[s]}(x)          at most 8 terms of at most 4 factors over at most 8 tables
//   round    p(t) = sum_{b < half} sum_k c_k prod_s ( lo[b] + t (hi[b] - lo[b]) ),  t = 0 .. d, d = max_k n_factors_k
//            (lo, hi) = (f[2b], f[2b + 1]) in leading order, (f[b], f[b + half]) in trailing order, as in sumcheck.hpp
//   sum      H = sum_b g(b)
// `*` is the slot product of the ring.  All sums are exact modular integers on canonical values, so neither the grid, the split nor
// the association of the sums changes a bit of the result: one term without coefficients is sumcheck.hpp's message bit for bit.
//
// One pass reads every DISTINCT table once, however many terms it is in.  The lane mapping, the records, the meeting of lane-groups in
// LDS and the sum over the records are those of sumcheck.hpp (mle::Lane, sum_groups_kernel, zero_kernel are used from there, not
// copied), and so are the records of the plan and the launch skeleton (plan_records, launch_plan).  Per pair a lane loads lo / hi of
// its unit of every table, and per point t it walks the terms with v_j(t) = v_j(t - 1) + (hi_j - lo_j) as sumcheck.hpp does.
//
// The term walk.  The table count of a kernel is a template parameter (4 or 8; a slot j >= n_tables is never loaded), the term
// structure is runtime data: 16 bits per term -- n_factors in bits 0-2, table[s] in bits 3 + 3 s .. 5 + 3 s -- in two 64-bit kernel
// arguments, decoded with scalar shifts.  v[] lives in registers, and a register array indexed with a runtime index goes to scratch
// (cdna_hip_programming.md rule 20), so a factor is selected by pick(): wave-uniform compares of the index against the statically
// unrolled j = 0 .. NT - 1.  The term loop itself is not unrolled: its body exists once per point.
//
// A term accumulates as  [c_k *] f_0 * ... * f_{m-2}  (canonical products: mul_boundary / SL::mul)  times  f_{m-1}  into the point's
// lazy sum (SumOfProducts<F> / SlotDot<SL>).  A single factor without a coefficient has no product and is added to the canonical sum.
// The coefficients are read once per lane into LDS -- a private stash [term][lane] for the power-of-two rings (no barrier: a lane
// reads what it wrote), shared per slot for the slot rings -- so that they cost neither registers nor a cache line per use.
//
// The flush interval counts accumulated TERMS.  Every lazy sum of a lane takes exactly one fma() per term and pair, so n_terms per
// pair; the sums are reduced into the canonical totals before a pair that would take them past kFlush = 64 fma() calls
// (since + n_terms > kFlush), hence never hold more than 64 products.  That is the interval of sumcheck.hpp, whose bounds apply
// word for word: against all-(p - 1) inputs, where the leading product and the last factor are canonical images below 2^64 (2^31
// for BabyBear-72),
//   SumOfProducts<Goldilocks>      four 96-bit sums of 32 x 32-bit products: 2^6 (2^32 - 1)^2 < 2^70
//   SlotDot<SlotG24> / <SlotFrog>  at most 2 x 4 partial products per term and sum: 2^6 * 8 * (2^32 - 1)^2 < 2^73
//   SlotDot<SlotB72>               at most 9 products of 31-bit images per term and sum: 2^6 * 9 * 2^62 < 2^72 (redc() wants < 2^29 terms)
//   SumOfProducts<BabyBear> / <Stark>  canonical after every term: no bound
// so every sum stays below 2^96 with 23 bits to spare.  The coefficient changes nothing: it enters through a canonical product.
//
// Truncated storage, per term: an element beyond the stored part of a table is zero and is never loaded.  A pair whose first element
// lies beyond a table has lo = hi = 0 for it, so v_j(t) = 0 at every t and every term that holds the table contributes exactly zero:
// the loop runs to the LONGEST term (host arithmetic: max over the terms of the min over their tables) and needs no per-term test.
#pragma once
#include "sumcheck.hpp"

namespace sr {
namespace vpoly {

enum { MAX_TABLES = 8, MAX_TERMS = 8, MAX_FACTORS = 4 };
using sumcheck::kFlush;
using sumcheck::MODE_LEADING;
using sumcheck::MODE_SUM;
using sumcheck::MODE_TRAILING;

// the tables of a call, by value in the kernel arguments: a captured graph holds no host pointer
struct Tables {
    const uint64_t *p[MAX_TABLES];
    size_t n[MAX_TABLES];  // stored elements
};
// the terms of a call: 16 bits each (see above), by value
struct Terms {
    uint64_t w[2];
    int n_terms;
    int n_tables;
};
struct Term {
    int n_factors;
    int table[MAX_FACTORS];
};
inline Terms pack_terms(const Term *t, int n_terms, int n_tables) {
    Terms r{{0, 0}, n_terms, n_tables};
    for (int k = 0; k < n_terms; k++) {
        uint64_t b = (uint64_t)t[k].n_factors;
        for (int s = 0; s < t[k].n_factors; s++) b |= (uint64_t)t[k].table[s] << (3 + 3 * s);
        r.w[k >> 2] |= b << (16 * (k & 3));
    }
    return r;
}
__device__ __forceinline__ unsigned term_bits(const Terms &tm, int k) { return (unsigned)((k < 4 ? tm.w[0] : tm.w[1]) >> (16 * (k & 3))) & 0xFFFFu; }

// v[idx] without a runtime register index: idx is wave-uniform, j is static
// a select of VALUES, word by word: a conditional read, or a select between two structs, is merged into a read of v[idx], i.e. scratch
template <class T>
__device__ __forceinline__ T sel(bool c, const T &a, const T &b) {
    return c ? a : b;
}
__device__ __forceinline__ U256 sel(bool c, const U256 &a, const U256 &b) {
    U256 r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.l[i] = c ? a.l[i] : b.l[i];
    return r;
}
template <class E, int NT>
__device__ __forceinline__ E pick(const E (&v)[NT], unsigned idx) {
    E x = v[0];
#pragma unroll
    for (int j = 1; j < NT; j++) x = sel(idx == (unsigned)j, v[j], x);
    return x;
}

// ---- power-of-two rings -----------------------------------------------------------------------------------------------------------
// One term at one point for coefficient n of the lane: bits = the term, ck = its coefficient (has_coef)
template <class F, int NT>
__device__ __forceinline__ void term_point(typename F::elem &total, SumOfProducts<F> &acc, const typename F::elem (&v)[NT], unsigned bits,
                                           bool has_coef, const typename F::elem &ck) {
    using E = typename F::elem;
    const int nl = (int)(bits & 7u) - 1;  // leading factors
    const E last = pick<E, NT>(v, (bits >> (3 + 3 * nl)) & 7u);
    // a lone factor without a coefficient: no product.  One unconditional add, so that the two ways never store through one pointer
    const bool lone = !has_coef && nl == 0;
    total = F::add(total, sel(lone, last, F::zero()));
    if (lone) return;
    E pr = sel(has_coef, ck, pick<E, NT>(v, (bits >> 3) & 7u));
    const int s0 = has_coef ? 0 : 1;
#pragma unroll
    for (int s = 0; s < MAX_FACTORS - 1; s++)
        if (s >= s0 && s < nl) pr = F::mul_boundary(pr, pick<E, NT>(v, (bits >> (3 + 3 * s)) & 7u));
    acc.fma(pr, last);
}

// NT table slots, up to NP points t0 .. t0 + np - 1 (PAIR) or the plain sum (!PAIR, NP == 1).  groups, lu, dst: as round_units of
// sumcheck.hpp.  lds: the coefficient stash [term][lane] (RW words each) and, after the loop, the meeting place of the lane-groups.
template <class F, int RW, int NT, int NP, bool PAIR>
__device__ __forceinline__ void round_units(uint64_t *dst, const Tables &tb, const Terms &tm, const uint64_t *coef, size_t count, size_t sb,
                                            size_t st, int lu, size_t groups, unsigned t0, unsigned np, unsigned np_total, uint64_t *lds) {
    using E = typename F::elem;
    using L = mle::Lane<F, RW>;
    const size_t flat = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t g = flat >> lu, c = flat & (((size_t)1 << lu) - 1);
    const bool in_block = lu < 8;  // uniform; the grid of such a launch is exact, so every lane reaches the barriers below
    if (!in_block && g >= groups) return;
    const bool has_coef = coef != nullptr;
    const int n_terms = tm.n_terms, n_tables = tm.n_tables;
    if (has_coef) {
        for (int k = 0; k < n_terms; k++) {
            L x;
            x.template load<false>(coef + ((((size_t)k) << lu) + c) * RW);
#pragma unroll
            for (int q = 0; q < RW; q++) lds[((size_t)k * 256 + threadIdx.x) * RW + q] = x.w[q];
        }
    }
    E total[NP][L::NC];
    SumOfProducts<F> acc[NP][L::NC];
#pragma unroll
    for (int i = 0; i < NP; i++)
#pragma unroll
        for (int n = 0; n < L::NC; n++) {
            total[i][n] = F::zero();
            acc[i][n].init();
        }
    unsigned since = 0;
    for (size_t b = g; b < count; b += groups) {
        const size_t e0 = b * sb, e1 = e0 + st;
        if (since + (unsigned)n_terms > kFlush) {
            since = 0;
#pragma unroll
            for (int i = 0; i < NP; i++)
#pragma unroll
                for (int n = 0; n < L::NC; n++) {
                    total[i][n] = F::add(total[i][n], acc[i][n].finish());
                    acc[i][n].init();
                }
        }
        since += (unsigned)n_terms;
        L lo[NT], hi[NT];
#pragma unroll
        for (int j = 0; j < NT; j++) {
            if (j < n_tables && e0 < tb.n[j]) lo[j].template load<true>(tb.p[j] + ((e0 << lu) + c) * RW);
            else lo[j].zero();
            if constexpr (PAIR) {
                if (j < n_tables && e1 < tb.n[j]) hi[j].template load<true>(tb.p[j] + ((e1 << lu) + c) * RW);
                else hi[j].zero();
            }
        }
#pragma unroll
        for (int n = 0; n < L::NC; n++) {
            E v[NT], dl[NT];
#pragma unroll
            for (int j = 0; j < NT; j++) {
                v[j] = lo[j].get(n);
                if constexpr (PAIR) {
                    dl[j] = F::sub(hi[j].get(n), v[j]);
                    for (unsigned q = 0; q < t0; q++) v[j] = F::add(v[j], dl[j]);
                }
            }
#pragma unroll
            for (int i = 0; i < NP; i++) {
                if ((unsigned)i < np) {
#pragma unroll 1
                    for (int k = 0; k < n_terms; k++) {
                        E ck = F::zero();
                        if (has_coef) {
                            L x;
#pragma unroll
                            for (int q = 0; q < RW; q++) x.w[q] = lds[((size_t)k * 256 + threadIdx.x) * RW + q];
                            ck = x.get(n);
                        }
                        term_point<F, NT>(total[i][n], acc[i][n], v, term_bits(tm, k), has_coef, ck);
                    }
                }
                if constexpr (PAIR) {
                    if (i + 1 < NP) {
                        if ((unsigned)(i + 1) < np) {
#pragma unroll
                            for (int j = 0; j < NT; j++) v[j] = F::add(v[j], dl[j]);
                        }
                    }
                }
            }
        }
    }
    if (in_block) __syncthreads();  // every lane of the workgroup has read its coefficients for the last time
#pragma unroll
    for (int i = 0; i < NP; i++) {
        if ((unsigned)i >= np) break;
        L r;
#pragma unroll
        for (int n = 0; n < L::NC; n++) {
            total[i][n] = F::add(total[i][n], acc[i][n].finish());
            r.put(n, total[i][n]);
        }
        if (!in_block) {
            r.store(dst + ((((g * np_total + t0 + i)) << lu) + c) * RW);
            continue;
        }
        const unsigned t = threadIdx.x, units = 1u << lu;
        if (i) __syncthreads();  // the previous point's sums have been read
#pragma unroll
        for (int q = 0; q < RW; q++) lds[t * RW + q] = r.w[q];
        __syncthreads();
        if (t < units) {  // lane-group 0 of the workgroup: t == c
            for (unsigned sg = 1; sg < (256u >> lu); sg++) {
                L x;
#pragma unroll
                for (int q = 0; q < RW; q++) x.w[q] = lds[(sg * units + t) * RW + q];
#pragma unroll
                for (int n = 0; n < L::NC; n++) r.put(n, F::add(r.get(n), x.get(n)));
            }
            r.store(dst + ((((blockIdx.x * (size_t)np_total + t0 + i)) << lu) + c) * RW);
        }
    }
}
// pair: the tables, the coefficients and dst are 16-byte aligned and k >= 1 (one-limb fields).  Dynamic LDS: lds_bytes() below.
template <class F, int NT, int NP, bool PAIR>
__global__ __launch_bounds__(256) void round_kernel(uint64_t *dst, Tables tb, Terms tm, const uint64_t *coef, size_t count, size_t sb, size_t st,
                                                    int k, int pair, size_t groups, unsigned t0, unsigned np, unsigned np_total) {
    extern __shared__ __align__(16) uint64_t vpoly_lds[];
    constexpr int RWMAX = sizeof(typename F::storage) == 8 ? 2 : (int)sizeof(typename F::storage) / 8;
    if constexpr (sizeof(typename F::storage) == 8) {
        if (pair) round_units<F, 2, NT, NP, PAIR>(dst, tb, tm, coef, count, sb, st, k - 1, groups, t0, np, np_total, vpoly_lds);
        else round_units<F, 1, NT, NP, PAIR>(dst, tb, tm, coef, count, sb, st, k, groups, t0, np, np_total, vpoly_lds);
    } else {
        round_units<F, RWMAX, NT, NP, PAIR>(dst, tb, tm, coef, count, sb, st, k, groups, t0, np, np_total, vpoly_lds);
    }
}

// ---- goldilocks24 / babybear72 / frog16: lane = slot ----------------------------------------------------------------------------------
template <class SL, int NT>
__device__ __forceinline__ void slot_pick(typename SL::F::elem *x, const typename SL::F::elem (&v)[NT][SL::W], unsigned idx) {
#pragma unroll
    for (int m = 0; m < SL::W; m++) x[m] = v[0][m];
#pragma unroll
    for (int j = 1; j < NT; j++)
#pragma unroll
        for (int m = 0; m < SL::W; m++) {
            const typename SL::F::elem vj = v[j][m];
            x[m] = idx == (unsigned)j ? vj : x[m];
        }
}
template <class SL, int NT>
__device__ __forceinline__ void slot_term_point(const typename SL::K &kc, typename SL::F::elem *total, SlotDot<SL> &acc,
                                                const typename SL::F::elem (&v)[NT][SL::W], unsigned bits, bool has_coef,
                                                const typename SL::F::elem *ck) {
    using F = typename SL::F;
    using E = typename F::elem;
    constexpr int W = SL::W;
    const int nl = (int)(bits & 7u) - 1;
    E last[W], pr[W], x[W];
    slot_pick<SL, NT>(last, v, (bits >> (3 + 3 * nl)) & 7u);
    const bool lone = !has_coef && nl == 0;
#pragma unroll
    for (int m = 0; m < W; m++) total[m] = F::add(total[m], lone ? last[m] : F::zero());
    if (lone) return;
    slot_pick<SL, NT>(pr, v, (bits >> 3) & 7u);
#pragma unroll
    for (int m = 0; m < W; m++) pr[m] = has_coef ? ck[m] : pr[m];
    const int s0 = has_coef ? 0 : 1;
#pragma unroll
    for (int s = 0; s < MAX_FACTORS - 1; s++)
        if (s >= s0 && s < nl) {
            slot_pick<SL, NT>(x, v, (bits >> (3 + 3 * s)) & 7u);
            SL::mul(pr, x, kc);
        }
    acc.fma(pr, last);
}
// A workgroup holds 256 / S lane-groups; they meet in LDS (slot_reduce_store) and the workgroup is record blockIdx.x.  The grid is
// exact (groups = gridDim.x * 256 / S), so every lane reaches the barriers.  The coefficients sit in LDS once per workgroup.
template <class SL, int NT, int NP, bool PAIR>
__global__ __launch_bounds__(256) void slot_round_kernel(typename SL::K kc, uint64_t *dst, Tables tb, Terms tm, const uint64_t *coef, size_t count,
                                                         size_t sb, size_t st, size_t groups, unsigned t0, unsigned np, unsigned np_total) {
    using F = typename SL::F;
    using E = typename F::elem;
    constexpr int W = SL::W, S = SL::D / SL::W;
    const size_t flat = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t g = flat / S;
    const int off = (int)(flat % S) * W;
    __shared__ E lds[256 * W];
    __shared__ E cl[MAX_TERMS * SL::D];
    const bool has_coef = coef != nullptr;
    const int n_terms = tm.n_terms, n_tables = tm.n_tables;
    if (has_coef) {
        for (int i = threadIdx.x; i < n_terms * SL::D; i += 256) cl[i] = F::load(coef + i);
        __syncthreads();
    }
    E total[NP][W];
    SlotDot<SL> acc[NP];
#pragma unroll
    for (int i = 0; i < NP; i++) {
        acc[i].init();
#pragma unroll
        for (int m = 0; m < W; m++) total[i][m] = F::zero();
    }
    unsigned since = 0;
    for (size_t b = g; b < count; b += groups) {
        const size_t e0 = b * sb, e1 = e0 + st;
        if (since + (unsigned)n_terms > kFlush) {
            since = 0;
#pragma unroll
            for (int i = 0; i < NP; i++) {
                E r[W];
                acc[i].finish(r, kc);
                acc[i].init();
#pragma unroll
                for (int m = 0; m < W; m++) total[i][m] = F::add(total[i][m], r[m]);
            }
        }
        since += (unsigned)n_terms;
        E v[NT][W], dl[NT][W];
#pragma unroll
        for (int j = 0; j < NT; j++) {
            if (j < n_tables && e0 < tb.n[j]) {
                slot_load<SL>(v[j], tb.p[j] + e0 * SL::D + off);
            } else {
#pragma unroll
                for (int m = 0; m < W; m++) v[j][m] = F::zero();
            }
            if constexpr (PAIR) {
                if (j < n_tables && e1 < tb.n[j]) {
                    slot_load<SL>(dl[j], tb.p[j] + e1 * SL::D + off);
#pragma unroll
                    for (int m = 0; m < W; m++) dl[j][m] = F::sub(dl[j][m], v[j][m]);
                } else {
#pragma unroll
                    for (int m = 0; m < W; m++) dl[j][m] = F::sub(F::zero(), v[j][m]);
                }
                for (unsigned q = 0; q < t0; q++)
#pragma unroll
                    for (int m = 0; m < W; m++) v[j][m] = F::add(v[j][m], dl[j][m]);
            }
        }
#pragma unroll
        for (int i = 0; i < NP; i++) {
            if ((unsigned)i < np) {
#pragma unroll 1
                for (int k = 0; k < n_terms; k++) {
                    E ck[W];
#pragma unroll
                    for (int m = 0; m < W; m++) ck[m] = has_coef ? cl[k * SL::D + off + m] : F::zero();
                    slot_term_point<SL, NT>(kc, total[i], acc[i], v, term_bits(tm, k), has_coef, ck);
                }
            }
            if constexpr (PAIR) {
                if (i + 1 < NP) {
                    if ((unsigned)(i + 1) < np) {
#pragma unroll
                        for (int j = 0; j < NT; j++)
#pragma unroll
                            for (int m = 0; m < W; m++) v[j][m] = F::add(v[j][m], dl[j][m]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NP; i++) {
        if ((unsigned)i >= np) break;
        E r[W];
        acc[i].finish(r, kc);
#pragma unroll
        for (int m = 0; m < W; m++) total[i][m] = F::add(total[i][m], r[m]);
        if (i) __syncthreads();  // the previous point's sums have been read
        slot_reduce_store<SL>(lds, total[i], dst + (blockIdx.x * (size_t)np_total + t0 + i) * SL::D);
    }
}

// ---- the plan: pure host arithmetic -------------------------------------------------------------------------------------------------
// The records are those of sumcheck.hpp (plan_records); only the points differ: d + 1 of them for the largest
// term, in launches of points_of<T>(table slots of the kernel).  tests/test_vpoly_isa.py holds the register count of every kernel.
inline int table_slots(int n_tables) { return n_tables <= 4 ? 4 : 8; }
template <class T>
constexpr int points_of(int slots) {
    if (std::is_same<T, Goldilocks>::value) return 5;
    if (std::is_same<T, BabyBear>::value) return 5;
    if (std::is_same<T, Stark>::value) return slots == 4 ? 2 : 1;    // two points over 8 slots: 268 registers
    if (std::is_same<T, SlotG24>::value) return slots == 4 ? 2 : 1;  // 258
    return 1;  // SlotB72 (17 96-bit sums per point), SlotFrog (Fq4 products)
}
inline int points_per_launch(int ring, int slots) {
    switch (ring) {
        case 0: return points_of<Goldilocks>(slots);
        case 1: return points_of<BabyBear>(slots);
        case 2: return points_of<Stark>(slots);
        case 3: return points_of<SlotG24>(slots);
        case 4: return points_of<SlotB72>(slots);
        default: return points_of<SlotFrog>(slots);
    }
}
using Plan = sumcheck::Plan;
inline bool plan(int ring, int k, size_t num_vars, int n_tables, int degree, int mode, Plan *p) {
    if (ring < 0 || ring > 5 || num_vars > sumcheck::MAX_VARS || n_tables < 1 || n_tables > MAX_TABLES || degree < 1 || degree > MAX_FACTORS ||
        mode < MODE_LEADING || mode > MODE_SUM)
        return false;
    if (mode != MODE_SUM && num_vars == 0) return false;
    *p = Plan{};
    p->count = mode == MODE_SUM ? (size_t)1 << num_vars : (size_t)1 << (num_vars - 1);
    p->np_total = mode == MODE_SUM ? 1 : degree + 1;
    p->np_launch = mode == MODE_SUM ? 1 : points_per_launch(ring, table_slots(n_tables));
    if (p->np_launch > p->np_total) p->np_launch = p->np_total;
    sumcheck::plan_records(ring, k, (p->np_total + p->np_launch - 1) / p->np_launch, p);
    return true;
}

// ---- launchers: the skeleton is sumcheck::launch_plan -------------------------------------------------------------------------------
using Shape = sumcheck::Shape;
// pairs (or indices) of one table in this mode
inline size_t pairs_of(int mode, size_t num_vars, size_t n) {
    if (mode == MODE_SUM) return n;
    const size_t half = (size_t)1 << (num_vars - 1);
    if (mode == MODE_LEADING) return (n + 1) / 2;
    return n < half ? n : half;
}
// the loop ends at the longest term; a term ends at its shortest table
inline Shape shape_of(int mode, size_t num_vars, const size_t *n_evals, const Term *terms, int n_terms) {
    size_t count = 0;
    for (int k = 0; k < n_terms; k++) {
        size_t nmin = n_evals[terms[k].table[0]];
        for (int s = 1; s < terms[k].n_factors; s++) nmin = n_evals[terms[k].table[s]] < nmin ? n_evals[terms[k].table[s]] : nmin;
        const size_t c = pairs_of(mode, num_vars, nmin);
        count = c > count ? c : count;
    }
    if (mode == MODE_SUM) return {count, 1, 0};
    if (mode == MODE_LEADING) return {count, 2, 1};
    return {count, 1, (size_t)1 << (num_vars - 1)};
}
// dynamic LDS of round_kernel: the coefficient stash, and at least the meeting place of the lane-groups (256 lanes x RW words); the slot
// kernels keep both in static LDS
template <class T>
inline size_t lds_bytes(int n_terms, bool has_coef, int pair) {
    if constexpr (sumcheck::kSlot<T>) {
        return 0;
    } else {
        const size_t rw = sizeof(typename T::storage) == 8 ? (pair ? 2 : 1) : sizeof(typename T::storage) / 8;
        return (size_t)(has_coef ? n_terms : 1) * 256 * rw * 8;
    }
}
template <class Fn>
inline void with_slots(int n_tables, Fn fn) {
    if (table_slots(n_tables) == 4) fn(std::integral_constant<int, 4>{});
    else fn(std::integral_constant<int, 8>{});
}
// The points in chunks of np_launch: np of the kernel's NP points from t0 on.  aligned: every table, the coefficients, out and work
// start on a 16-byte boundary.  Every term empty: nothing to visit.
template <class T>
inline hipError_t launch(const typename sumcheck::Family<T>::K &kc, const Plan &p, int mode, uint64_t *out, const Tables &tb, int n_tables,
                         const Term *terms, int n_terms, const uint64_t *coef, size_t num_vars, int k, bool aligned, uint64_t *work, hipStream_t s) {
    const sumcheck::Geometry ge = sumcheck::geometry_of<T>(k, aligned);
    const Shape sh = shape_of(mode, num_vars, tb.n, terms, n_terms);
    return sumcheck::launch_plan<T>(p, ge, sh.count == 0, out, work, s, [&](uint64_t *dst) {
        const dim3 g = ge.grid(p.groups), b(256);
        const size_t groups = ge.groups(p.groups), lds = lds_bytes<T>(n_terms, coef != nullptr, ge.pair);
        const Terms tm = pack_terms(terms, n_terms, n_tables);
        const unsigned np_total = (unsigned)p.np_total;
        for (unsigned t0 = 0; t0 < np_total; t0 += (unsigned)p.np_launch) {
            const unsigned np = np_total - t0 < (unsigned)p.np_launch ? np_total - t0 : (unsigned)p.np_launch;
            const auto one = [&](auto nt, auto round) {  // round: a round message (PAIR) or the plain sum
                constexpr int NT = decltype(nt)::value;
                constexpr bool PAIR = decltype(round)::value;
                constexpr int NP = PAIR ? points_of<T>(NT) : 1;
                if constexpr (sumcheck::kSlot<T>)
                    hipLaunchKernelGGL((slot_round_kernel<T, NT, NP, PAIR>), g, b, lds, s, kc, dst, tb, tm, coef, sh.count, sh.sb, sh.st, groups, t0, np,
                                       np_total);
                else
                    hipLaunchKernelGGL((round_kernel<T, NT, NP, PAIR>), g, b, lds, s, dst, tb, tm, coef, sh.count, sh.sb, sh.st, ge.k, ge.pair, groups,
                                       t0, np, np_total);
            };
            with_slots(n_tables, [&](auto nt) {
                if (mode == MODE_SUM) one(nt, std::false_type{});
                else one(nt, std::true_type{});
            });
        }
    });
}

}  // namespace vpoly
}  // namespace sr
