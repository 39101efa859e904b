// Sum-check rounds of a sum of products with a PER-PAIR WEIGHT: the eq(z, .) factor of a zero-check, a GKR layer claim or R1CS as one
// ring element per pair that is constant in the round's variable, not as one more table.
//   round    h(t) = sum_{b < half} w[b] * sum_k c_k prod_s ( lo_s[b] + t (hi_s[b] - lo_s[b]) ),  t = 0 .. d, d = max_k n_factors_k
//            the pairs (lo, hi) are those of sumcheck_vpoly.hpp in the same order; the weight is no factor and is not counted in d
//   fused    fold every distinct table at the challenge r as sumcheck_vpoly_fold.hpp does and take h of the round that follows from
//            the folded pair while it is in registers; w then holds 2^(num_vars - 2) elements, one per pair of the FOLDED tables
// w is indexed by the pair index b, read once per pair with the access width of the tables (non-temporal where the table loads are)
// and never written.  In the round that binds variable v of  sum_b eq(z, b) g(b)  the caller passes w = eq(z_rest, .) over the unbound
// coordinates and multiplies eq(z_v, t) and the product over the bound coordinates into h(t) itself (EqSumCheck of the mirrors): the
// eq factor costs one read of n / 4 elements per round, not a read, a fold and a write of a table, and one point less.
//
// Everything but the weight is taken from the neighbouring files, not copied: Tables, Terms, pick() / slot_pick(), the term encoding,
// the coefficient stash and lds_bytes(), SumOfProducts / SlotDot, shape_of and pairs_of (sumcheck_vpoly.hpp); Folded and its shape
// (sumcheck_vpoly_fold.hpp); load_pair, fold_pair, slot_fold_one (sumcheck_fold.hpp); the lane, the records, the meeting of the
// lane-groups and the launch skeleton (sumcheck.hpp).  No kernel of those files is changed or instantiated differently.
//
// The weight is the LEADING factor of every term's product: pr starts as w, or as c_k * w (one canonical product, formed where the
// term is walked).  So the lone-factor shortcut of sumcheck_vpoly.hpp has no case left -- a lone factor is w * f, a product like any
// other -- and every lazy sum takes exactly one fma(pr, last) per term and pair.  pr is a canonical product (or the canonical weight
// itself), last a canonical table value advanced by canonical additions: both operands are the canonical images below 2^64 (2^31
// for BabyBear-72) that sumcheck.hpp's bound assumes, and the sums are reduced before a pair that would take them past kFlush = 64
// accumulated terms (since + n_terms > kFlush).  The kFlush = 64 bound of sumcheck.hpp therefore carries over word for word:
//   SumOfProducts<Goldilocks>      four 96-bit sums of 32 x 32-bit products: 2^6 (2^32 - 1)^2 < 2^70
//   SlotDot<SlotG24> / <SlotFrog>  at most 2 x 4 partial products per term and sum: 2^6 * 8 * (2^32 - 1)^2 < 2^73
//   SlotDot<SlotB72>               at most 9 products of 31-bit images per term and sum: 2^6 * 9 * 2^62 < 2^72 (redc() wants < 2^29 terms)
//   SumOfProducts<BabyBear> / <Stark>  canonical after every term: no bound
// All sums are exact modular integers on canonical values, so neither the grid, the split nor the association changes a bit: with
// every weight one() the message equals sumcheck_vpoly.hpp's bit for bit, and the fused message equals the round call on the folded
// tables.
//
// Truncated storage is that of the unweighted kernels: the product loop ends at the longest term, and a weight whose pair is not
// visited is not read.  In place is sound for the trailing order only, as in sumcheck_fold.hpp.
//
// Points per launch (points_of / fused_points_of below): per family and slot count the largest number that leaves the kernel without
// scratch inside the family's register bound -- 256 registers, BabyBear 128 -- read from the gfx950 listing of
// tools/ubench/wsumcheck_isa.hip (tests/test_wsumcheck_isa.py pins every count; DESIGN_APPENDIX.md A.16).  Over 4 / 8 table slots:
//   round kernels   Goldilocks 5 / 5 (203 / 235 registers), BabyBear 5 / 5 (77 / 105), Stark 4 / 1 (224 / 202; five over 4 slots: 258,
//                   two over 8: 268), goldilocks24 3 / 1 (254 / 169; four over 4 slots spill, two over 8: 260), babybear72 1 / 1
//                   (190 / 252), frog16 1 / 1 (169 / 208; two points spill)
//   fused launch    Goldilocks 5 / 4 (221 / 232; five over 8 slots: 260 and scratch), BabyBear 5 / 3 (106 / 128; four: 133), Stark 2 / 1
//                   (248 / 237), goldilocks24 2 / 1 (217 / 183), babybear72 1 / 0 (222 / 169: over 8 slots the launch only folds, as in
//                   sumcheck_vpoly_fold.hpp), frog16 1 / 1 (188 / 237)
// babybear72 over 8 slots needs the weight out of the registers (weight_in_lds below).  The remaining points of a fused call come from
// the weighted round kernels over the FOLDED tables, into the same records with the same t0 / np_total convention.
//
// sumcheck_index.hpp holds copies of the four kernels below with a loader that also takes integer columns: a change to the flush, the
// meeting of the lane-groups or the store sequence here has to be made there as well.
#pragma once
#include "sumcheck_vpoly_fold.hpp"

namespace sr {
namespace wsumcheck {

using sumcheck::kFlush;
using vpoly::MAX_FACTORS;
using vpoly::Tables;
using vpoly::Term;
using vpoly::Terms;
using vpoly_fold::Folded;

// ---- power-of-two rings -----------------------------------------------------------------------------------------------------------
// One term at one point for one coefficient of the lane: w the pair's weight, ck the term's coefficient (has_coef)
template <class F, int NT>
__device__ __forceinline__ void term_point(SumOfProducts<F> &acc, const typename F::elem (&v)[NT], unsigned bits, bool has_coef,
                                           const typename F::elem &ck, const typename F::elem &w) {
    using E = typename F::elem;
    const int nl = (int)(bits & 7u) - 1;  // leading factors of the tables
    const E last = vpoly::pick<E, NT>(v, (bits >> (3 + 3 * nl)) & 7u);
    E pr = w;
    if (has_coef) pr = F::mul_boundary(ck, w);
#pragma unroll
    for (int s = 0; s < MAX_FACTORS - 1; s++)
        if (s < nl) pr = F::mul_boundary(pr, vpoly::pick<E, NT>(v, (bits >> (3 + 3 * s)) & 7u));
    acc.fma(pr, last);
}
// the walk of the terms at the points i < np of one pair, shared by the round and the fused kernel: v, dl of coefficient n; v is
// advanced point by point
template <class F, int RW, int NT, int NP>
__device__ __forceinline__ void pair_points(SumOfProducts<F> (&acc)[NP], typename F::elem (&v)[NT], const typename F::elem (&dl)[NT],
                                            const typename F::elem &w, const Terms &tm, bool has_coef, const uint64_t *lds, int n, unsigned np) {
    using E = typename F::elem;
    using L = mle::Lane<F, RW>;
    const int n_terms = tm.n_terms;
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
                term_point<F, NT>(acc[i], v, vpoly::term_bits(tm, k), has_coef, ck, w);
            }
        }
        if (i + 1 < NP) {
            if ((unsigned)(i + 1) < np) {
#pragma unroll
                for (int j = 0; j < NT; j++) v[j] = F::add(v[j], dl[j]);
            }
        }
    }
}
// the lane's sums of points i < np into record (g or blockIdx.x) at points t0 + i of np_total, as vpoly::round_units leaves them
template <class F, int RW, int NP>
__device__ __forceinline__ void store_points(uint64_t *dst, typename F::elem (&total)[NP][mle::Lane<F, RW>::NC],
                                             SumOfProducts<F> (&acc)[mle::Lane<F, RW>::NC][NP], bool in_block, size_t g, size_t c, int lu, unsigned t0,
                                             unsigned np, unsigned np_total, uint64_t *lds) {
    using L = mle::Lane<F, RW>;
    if (in_block) __syncthreads();  // every lane of the workgroup has read its coefficients for the last time
#pragma unroll
    for (int i = 0; i < NP; i++) {
        if ((unsigned)i >= np) break;
        L r;
#pragma unroll
        for (int n = 0; n < L::NC; n++) {
            total[i][n] = F::add(total[i][n], acc[n][i].finish());
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
template <class F, int NC, int NP>
__device__ __forceinline__ void flush_points(SumOfProducts<F> (&acc)[NC][NP], typename F::elem (&total)[NP][NC]) {
#pragma unroll
    for (int i = 0; i < NP; i++)
#pragma unroll
        for (int n = 0; n < NC; n++) {
            total[i][n] = F::add(total[i][n], acc[n][i].finish());
            acc[n][i].init();
        }
}
template <class F, int RW>
__device__ __forceinline__ void stash_coefficients(uint64_t *lds, const uint64_t *coef, int n_terms, int lu, size_t c) {
    for (int k = 0; k < n_terms; k++) {
        mle::Lane<F, RW> x;
        x.template load<false>(coef + ((((size_t)k) << lu) + c) * RW);
#pragma unroll
        for (int q = 0; q < RW; q++) lds[((size_t)k * 256 + threadIdx.x) * RW + q] = x.w[q];
    }
}

// NT table slots, up to NP points t0 .. t0 + np - 1.  wp: the weights, one element per pair.  The rest as vpoly::round_units.
template <class F, int RW, int NT, int NP>
__device__ __forceinline__ void round_units(uint64_t *dst, const Tables &tb, const Terms &tm, const uint64_t *coef, const uint64_t *wp, size_t count,
                                            size_t sb, size_t st, int lu, size_t groups, unsigned t0, unsigned np, unsigned np_total, uint64_t *lds) {
    using E = typename F::elem;
    using L = mle::Lane<F, RW>;
    const size_t flat = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t g = flat >> lu, c = flat & (((size_t)1 << lu) - 1);
    const bool in_block = lu < 8;  // uniform; the grid of such a launch is exact, so every lane reaches the barriers below
    if (!in_block && g >= groups) return;
    const bool has_coef = coef != nullptr;
    const int n_terms = tm.n_terms, n_tables = tm.n_tables;
    if (has_coef) stash_coefficients<F, RW>(lds, coef, n_terms, lu, c);
    E total[NP][L::NC];
    SumOfProducts<F> acc[L::NC][NP];
#pragma unroll
    for (int i = 0; i < NP; i++)
#pragma unroll
        for (int n = 0; n < L::NC; n++) {
            total[i][n] = F::zero();
            acc[n][i].init();
        }
    unsigned since = 0;
    for (size_t b = g; b < count; b += groups) {
        const size_t e0 = b * sb, e1 = e0 + st;
        if (since + (unsigned)n_terms > kFlush) {
            since = 0;
            flush_points<F>(acc, total);
        }
        since += (unsigned)n_terms;
        L lo[NT], hi[NT], wl;
        wl.template load<true>(wp + ((b << lu) + c) * RW);
#pragma unroll
        for (int j = 0; j < NT; j++) {
            if (j < n_tables && e0 < tb.n[j]) lo[j].template load<true>(tb.p[j] + ((e0 << lu) + c) * RW);
            else lo[j].zero();
            if (j < n_tables && e1 < tb.n[j]) hi[j].template load<true>(tb.p[j] + ((e1 << lu) + c) * RW);
            else hi[j].zero();
        }
#pragma unroll
        for (int n = 0; n < L::NC; n++) {
            E v[NT], dl[NT];
#pragma unroll
            for (int j = 0; j < NT; j++) {
                v[j] = lo[j].get(n);
                dl[j] = F::sub(hi[j].get(n), v[j]);
                for (unsigned q = 0; q < t0; q++) v[j] = F::add(v[j], dl[j]);
            }
            pair_points<F, RW, NT, NP>(acc[n], v, dl, wl.get(n), tm, has_coef, lds, n, np);
        }
    }
    store_points<F, RW, NP>(dst, total, acc, in_block, g, c, lu, t0, np, np_total, lds);
}
// pair: the tables, the weights, the coefficients and dst are 16-byte aligned and k >= 1 (one-limb fields).  Dynamic LDS:
// vpoly::lds_bytes().
template <class F, int NT, int NP>
__global__ __launch_bounds__(256) void round_kernel(uint64_t *dst, Tables tb, Terms tm, const uint64_t *coef, const uint64_t *wp, size_t count,
                                                    size_t sb, size_t st, int k, int pair, size_t groups, unsigned t0, unsigned np, unsigned np_total) {
    extern __shared__ __align__(16) uint64_t wsumcheck_lds[];
    constexpr int RWMAX = sizeof(typename F::storage) == 8 ? 2 : (int)sizeof(typename F::storage) / 8;
    if constexpr (sizeof(typename F::storage) == 8) {
        if (pair) round_units<F, 2, NT, NP>(dst, tb, tm, coef, wp, count, sb, st, k - 1, groups, t0, np, np_total, wsumcheck_lds);
        else round_units<F, 1, NT, NP>(dst, tb, tm, coef, wp, count, sb, st, k, groups, t0, np, np_total, wsumcheck_lds);
    } else {
        round_units<F, RWMAX, NT, NP>(dst, tb, tm, coef, wp, count, sb, st, k, groups, t0, np, np_total, wsumcheck_lds);
    }
}

// NT table slots, points 0 .. np - 1 (np <= NP) of np_total of the round over the FOLDED tables.  wp: one weight per pair of the folded
// tables.  The rest as vpoly_fold::fold_round_units.
template <class F, int RW, int NT, int NP>
__device__ __forceinline__ void fold_round_units(uint64_t *dst, const Tables &tb, const Folded &fo, const Terms &tm, const uint64_t *coef,
                                                 const uint64_t *wp, const uint64_t *rp, size_t count, size_t qmax, size_t sb, size_t st, size_t fst,
                                                 int lu, size_t groups, unsigned np, unsigned np_total, uint64_t *lds) {
    using E = typename F::elem;
    using L = mle::Lane<F, RW>;
    const size_t flat = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t g = flat >> lu, c = flat & (((size_t)1 << lu) - 1);
    const bool in_block = lu < 8;  // uniform; the grid of such a launch is exact, so every lane reaches the barriers below
    if (!in_block && g >= groups) return;
    const bool has_coef = coef != nullptr;
    const int n_terms = tm.n_terms, n_tables = tm.n_tables;
    if (has_coef) stash_coefficients<F, RW>(lds, coef, n_terms, lu, c);
    E total[NP][L::NC];
    SumOfProducts<F> acc[L::NC][NP];
#pragma unroll
    for (int i = 0; i < NP; i++)
#pragma unroll
        for (int n = 0; n < L::NC; n++) {
            total[i][n] = F::zero();
            acc[n][i].init();
        }
    L rr;
    rr.template load<false>(rp + c * RW);
    unsigned since = 0;
    for (size_t b = g; b < qmax; b += groups) {
        const size_t o0 = b * sb, o1 = o0 + st;
        L lo[NT], hi[NT];
#pragma unroll
        for (int j = 0; j < NT; j++) {
            if (j < n_tables && o0 < fo.n[j]) {  // its first input is stored
                L x0, x1;
                sumcheck_fold::load_pair<F, RW>(lo[j], x0, tb.p[j], tb.n[j], o0, sb, fst, lu, c);
                const bool second = o1 < fo.n[j];
                if (second) sumcheck_fold::load_pair<F, RW>(hi[j], x1, tb.p[j], tb.n[j], o1, sb, fst, lu, c);
                sumcheck_fold::fold_pair<F, RW>(lo[j], x0, rr);
                lo[j].store(fo.p[j] + ((o0 << lu) + c) * RW);
                if (second) {
                    sumcheck_fold::fold_pair<F, RW>(hi[j], x1, rr);
                    hi[j].store(fo.p[j] + ((o1 << lu) + c) * RW);
                } else {
                    hi[j].zero();
                }
            } else {
                lo[j].zero();
                hi[j].zero();
            }
        }
        if (b >= count) continue;  // beyond the longest folded term: every term has a zero factor at every t, and no weight is read
        if (since + (unsigned)n_terms > kFlush) {
            since = 0;
            flush_points<F>(acc, total);
        }
        since += (unsigned)n_terms;
        L wl;
        wl.template load<true>(wp + ((b << lu) + c) * RW);
#pragma unroll
        for (int n = 0; n < L::NC; n++) {
            E v[NT], dl[NT];
#pragma unroll
            for (int j = 0; j < NT; j++) {
                v[j] = lo[j].get(n);
                dl[j] = F::sub(hi[j].get(n), v[j]);
            }
            pair_points<F, RW, NT, NP>(acc[n], v, dl, wl.get(n), tm, has_coef, lds, n, np);
        }
    }
    store_points<F, RW, NP>(dst, total, acc, in_block, g, c, lu, 0, np, np_total, lds);
}
// pair: every table, folded table, the weights, the coefficients, r and dst are 16-byte aligned and k >= 1 (one-limb fields)
template <class F, int NT, int NP>
__global__ __launch_bounds__(256) void fold_round_kernel(uint64_t *dst, Tables tb, Folded fo, Terms tm, const uint64_t *coef, const uint64_t *wp,
                                                         const uint64_t *rp, size_t count, size_t qmax, size_t sb, size_t st, size_t fst, int k, int pair,
                                                         size_t groups, unsigned np, unsigned np_total) {
    extern __shared__ __align__(16) uint64_t wsumcheck_fold_lds[];
    constexpr int RWMAX = sizeof(typename F::storage) == 8 ? 2 : (int)sizeof(typename F::storage) / 8;
    if constexpr (sizeof(typename F::storage) == 8) {
        if (pair)
            fold_round_units<F, 2, NT, NP>(dst, tb, fo, tm, coef, wp, rp, count, qmax, sb, st, fst, k - 1, groups, np, np_total, wsumcheck_fold_lds);
        else fold_round_units<F, 1, NT, NP>(dst, tb, fo, tm, coef, wp, rp, count, qmax, sb, st, fst, k, groups, np, np_total, wsumcheck_fold_lds);
    } else {
        fold_round_units<F, RWMAX, NT, NP>(dst, tb, fo, tm, coef, wp, rp, count, qmax, sb, st, fst, k, groups, np, np_total, wsumcheck_fold_lds);
    }
}

// ---- goldilocks24 / babybear72 / frog16: lane = slot ---------------------------------------------------------------------------------
// WL: w points to the lane's words in LDS and is read there term by term, never kept in registers (weight_in_lds below)
template <class SL, int NT, bool WL>
__device__ __forceinline__ void slot_term_point(const typename SL::K &kc, SlotDot<SL> &acc, const typename SL::F::elem (&v)[NT][SL::W], unsigned bits,
                                                bool has_coef, const typename SL::F::elem *ck, const typename SL::F::elem *w) {
    using E = typename SL::F::elem;
    constexpr int W = SL::W;
    const int nl = (int)(bits & 7u) - 1;
    E last[W], pr[W], x[W];
    vpoly::slot_pick<SL, NT>(last, v, (bits >> (3 + 3 * nl)) & 7u);
#pragma unroll
    for (int m = 0; m < W; m++) {
        if constexpr (WL) pr[m] = *static_cast<const volatile E *>(w + m);
        else pr[m] = w[m];
    }
    if (has_coef) SL::mul(pr, ck, kc);
#pragma unroll
    for (int s = 0; s < MAX_FACTORS - 1; s++)
        if (s < nl) {
            vpoly::slot_pick<SL, NT>(x, v, (bits >> (3 + 3 * s)) & 7u);
            SL::mul(pr, x, kc);
        }
    acc.fma(pr, last);
}
// the walk of the terms at the points i < np of one pair; v is advanced point by point.  cl: the coefficients in LDS
template <class SL, int NT, int NP, int NA, bool WL>
__device__ __forceinline__ void slot_pair_points(const typename SL::K &kc, SlotDot<SL> (&acc)[NA], typename SL::F::elem (&v)[NT][SL::W],
                                                 const typename SL::F::elem (&dl)[NT][SL::W], const typename SL::F::elem *w, const Terms &tm,
                                                 bool has_coef, const typename SL::F::elem *cl, int off, unsigned np) {
    using F = typename SL::F;
    using E = typename F::elem;
    constexpr int W = SL::W;
    const int n_terms = tm.n_terms;
#pragma unroll
    for (int i = 0; i < NP; i++) {
        if ((unsigned)i < np) {
#pragma unroll 1
            for (int k = 0; k < n_terms; k++) {
                E ck[W];
#pragma unroll
                for (int m = 0; m < W; m++) ck[m] = has_coef ? cl[k * SL::D + off + m] : F::zero();
                slot_term_point<SL, NT, WL>(kc, acc[i], v, vpoly::term_bits(tm, k), has_coef, ck, w);
            }
        }
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
template <class SL, int NP, int NA>
__device__ __forceinline__ void slot_flush_points(const typename SL::K &kc, typename SL::F::elem (&total)[NA][SL::W], SlotDot<SL> (&acc)[NA]) {
    using F = typename SL::F;
#pragma unroll
    for (int i = 0; i < NP; i++) {
        typename F::elem r[SL::W];
        acc[i].finish(r, kc);
        acc[i].init();
#pragma unroll
        for (int m = 0; m < SL::W; m++) total[i][m] = F::add(total[i][m], r[m]);
    }
}
// babybear72 over 8 table slots: lo / hi of eight slots, the 17 96-bit sums of a point and the weight are past 256 registers, so the
// lane parks the pair's weight in LDS (its own 9 words) and the term walk reads it from there
template <class SL>
constexpr bool weight_in_lds(int slots) {
    return std::is_same<SL, SlotB72>::value && slots == 8;
}
// A workgroup holds 256 / S lane-groups; they meet in LDS (slot_reduce_store) and the workgroup is record blockIdx.x.  The grid is
// exact (groups = gridDim.x * 256 / S), so every lane reaches the barriers.  The coefficients sit in LDS once per workgroup.
template <class SL, int NT, int NP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void slot_round_kernel(typename SL::K kc, uint64_t *dst, Tables tb, Terms tm, const uint64_t *coef,
                                                         const uint64_t *wp, size_t count, size_t sb, size_t st, size_t groups, unsigned t0, unsigned np,
                                                         unsigned np_total) {
    using F = typename SL::F;
    using E = typename F::elem;
    constexpr int W = SL::W, S = SL::D / SL::W;
    const size_t flat = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t g = flat / S;
    const int off = (int)(flat % S) * W;
    __shared__ E lds[256 * W];
    __shared__ E cl[vpoly::MAX_TERMS * SL::D];
    constexpr bool WL = weight_in_lds<SL>(NT);
    __shared__ E wl[WL ? 256 * W : 1];
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
            slot_flush_points<SL, NP, NP>(kc, total, acc);
        }
        since += (unsigned)n_terms;
        E v[NT][W], dl[NT][W], w[W];
        slot_load<SL>(w, wp + b * SL::D + off);
        if constexpr (WL) {  // a lane reads what it wrote: no barrier
#pragma unroll
            for (int m = 0; m < W; m++) wl[threadIdx.x * W + m] = w[m];
        }
#pragma unroll
        for (int j = 0; j < NT; j++) {
            if (j < n_tables && e0 < tb.n[j]) {
                slot_load<SL>(v[j], tb.p[j] + e0 * SL::D + off);
            } else {
#pragma unroll
                for (int m = 0; m < W; m++) v[j][m] = F::zero();
            }
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
        if constexpr (WL) slot_pair_points<SL, NT, NP, NP, true>(kc, acc, v, dl, wl + threadIdx.x * W, tm, has_coef, cl, off, np);
        else slot_pair_points<SL, NT, NP, NP, false>(kc, acc, v, dl, w, tm, has_coef, cl, off, np);
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
// The fold of every slot is vpoly_fold::slot_fold_slots.  Two waves per SIMD is what 256 registers allow; said outright, as for
// slot_fold_round_kernel of sumcheck_fold.hpp.
template <class SL, int NT, int NP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void slot_fold_round_kernel(
    typename SL::K kc, uint64_t *dst, Tables tb, Folded fo, Terms tm, const uint64_t *coef, const uint64_t *wp, const uint64_t *rp, size_t count,
    size_t qmax, size_t sb, size_t st, size_t fst, size_t groups, unsigned np, unsigned np_total) {
    using F = typename SL::F;
    using E = typename F::elem;
    constexpr int W = SL::W, S = SL::D / SL::W;
    const size_t flat = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t g = flat / S;
    const int off = (int)(flat % S) * W;
    __shared__ E lds[256 * W];
    __shared__ E cl[vpoly::MAX_TERMS * SL::D];
    const bool has_coef = coef != nullptr;
    const int n_terms = tm.n_terms, n_tables = tm.n_tables;
    if (has_coef) {
        for (int i = threadIdx.x; i < n_terms * SL::D; i += 256) cl[i] = F::load(coef + i);
        __syncthreads();
    }
    constexpr int NA = NP ? NP : 1;  // NP == 0: the launch folds and leaves every point to the round kernels
    E total[NA][W], rr[W];
    SlotDot<SL> acc[NA];
#pragma unroll
    for (int i = 0; i < NP; i++) {
        acc[i].init();
#pragma unroll
        for (int m = 0; m < W; m++) total[i][m] = F::zero();
    }
    slot_load<SL>(rr, rp + off);
    unsigned since = 0;
    for (size_t b = g; b < qmax; b += groups) {
        const size_t o0 = b * sb, o1 = o0 + st;
        E v[NT][W], dl[NT][W];
        vpoly_fold::slot_fold_slots<SL, NT>(std::make_integer_sequence<int, NT>{}, v, dl, kc, tb, fo, n_tables, o0, o1, sb, fst, off, rr);
        if (b >= count) continue;  // no weight is read beyond the longest folded term
        if constexpr (NP > 0) {
            if (since + (unsigned)n_terms > kFlush) {
                since = 0;
                slot_flush_points<SL, NP, NA>(kc, total, acc);
            }
            since += (unsigned)n_terms;
            E w[W];
            slot_load<SL>(w, wp + b * SL::D + off);
            slot_pair_points<SL, NT, NP, NA, false>(kc, acc, v, dl, w, tm, has_coef, cl, off, np);
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
        slot_reduce_store<SL>(lds, total[i], dst + (blockIdx.x * (size_t)np_total + i) * SL::D);
    }
}

// ---- the plan: pure host arithmetic -------------------------------------------------------------------------------------------------
// points of one launch of the weighted round kernels / of the fused launch over `slots` table slots: the largest number within the
// family's register bound without scratch (tests/test_wsumcheck_isa.py holds the register counts)
template <class T>
constexpr int points_of(int slots) {
    if (std::is_same<T, Stark>::value) return slots == 4 ? 4 : 1;    // five points over 4 slots: 258 registers; two over 8: 268
    if (std::is_same<T, SlotG24>::value) return slots == 4 ? 3 : 1;  // four points over 4 slots spill; two over 8: 260
    return vpoly::points_of<T>(slots);  // Goldilocks, BabyBear: all five; babybear72, frog16: one (two spill)
}
template <class T>
constexpr int fused_points_of(int slots) {
    return vpoly_fold::fused_points_of<T>(slots);
}
template <class Fn>
inline int by_ring(int ring, Fn fn) {
    switch (ring) {
        case 0: return fn(sumcheck::Family<Goldilocks>{});
        case 1: return fn(sumcheck::Family<BabyBear>{});
        case 2: return fn(sumcheck::Family<Stark>{});
        case 3: return fn(sumcheck::Family<SlotG24>{});
        case 4: return fn(sumcheck::Family<SlotB72>{});
        default: return fn(sumcheck::Family<SlotFrog>{});
    }
}
template <class T, bool B>
constexpr int points_of_family(sumcheck::Family<T, B>, int slots) {
    return points_of<T>(slots);
}
template <class T, bool B>
constexpr int fused_points_of_family(sumcheck::Family<T, B>, int slots) {
    return fused_points_of<T>(slots);
}
inline int points_per_launch(int ring, int slots) {
    return by_ring(ring, [&](auto f) { return points_of_family(f, slots); });
}
inline int fused_points(int ring, int slots) {
    return by_ring(ring, [&](auto f) { return fused_points_of_family(f, slots); });
}
using Plan = sumcheck::Plan;
// the records and points of vpoly::plan with the points of a launch of the weighted kernels; a weighted plain sum does not exist
inline bool plan(int ring, int k, size_t num_vars, int n_tables, int degree, int order, Plan *p) {
    if (order != sumcheck::MODE_LEADING && order != sumcheck::MODE_TRAILING) return false;
    if (!vpoly::plan(ring, k, num_vars, n_tables, degree, order, p)) return false;
    p->np_launch = points_per_launch(ring, vpoly::table_slots(n_tables));
    if (p->np_launch > p->np_total) p->np_launch = p->np_total;
    sumcheck::plan_records(ring, k, (p->np_total + p->np_launch - 1) / p->np_launch, p);
    return true;
}
// the records of a weighted round in num_vars - 1 variables; the fused launch, the launches of the remaining points, the sum over the
// records
inline bool fold_plan(int ring, int k, size_t num_vars, int n_tables, int degree, int order, Plan *p) {
    if (num_vars < 2) return false;
    if (!plan(ring, k, num_vars - 1, n_tables, degree, order, p)) return false;
    const int fp = fused_points(ring, vpoly::table_slots(n_tables));
    const int rest = p->np_total > fp ? p->np_total - fp : 0;
    sumcheck::plan_records(ring, k, 1 + (rest + p->np_launch - 1) / p->np_launch, p);
    return true;
}

// ---- launchers: the skeleton is sumcheck::launch_plan -------------------------------------------------------------------------------
// one launch of the weighted round kernels: np of the kernel's points from t0 on
template <class T, int NT>
inline void launch_points(const typename sumcheck::Family<T>::K &kc, const sumcheck::Geometry &ge, const Plan &p, size_t lds, uint64_t *dst,
                          const Tables &tb, const Terms &tm, const uint64_t *coef, const uint64_t *weights, const vpoly::Shape &sh, unsigned t0,
                          unsigned np, hipStream_t s) {
    constexpr int NP = points_of<T>(NT);
    const dim3 g = ge.grid(p.groups), b(256);
    const size_t groups = ge.groups(p.groups);
    if constexpr (sumcheck::kSlot<T>)
        hipLaunchKernelGGL((slot_round_kernel<T, NT, NP>), g, b, lds, s, kc, dst, tb, tm, coef, weights, sh.count, sh.sb, sh.st, groups, t0, np,
                           (unsigned)p.np_total);
    else
        hipLaunchKernelGGL((round_kernel<T, NT, NP>), g, b, lds, s, dst, tb, tm, coef, weights, sh.count, sh.sb, sh.st, ge.k, ge.pair, groups, t0, np,
                           (unsigned)p.np_total);
}
// The points in chunks of np_launch.  aligned: every table, the weights, the coefficients, out and work start on a 16-byte boundary.
// Every term empty: nothing to visit.
template <class T>
inline hipError_t launch(const typename sumcheck::Family<T>::K &kc, const Plan &p, int order, uint64_t *out, const uint64_t *weights, const Tables &tb,
                         int n_tables, const Term *terms, int n_terms, const uint64_t *coef, size_t num_vars, int k, bool aligned, uint64_t *work,
                         hipStream_t s) {
    const sumcheck::Geometry ge = sumcheck::geometry_of<T>(k, aligned);
    const vpoly::Shape sh = vpoly::shape_of(order, num_vars, tb.n, terms, n_terms);
    return sumcheck::launch_plan<T>(p, ge, sh.count == 0, out, work, s, [&](uint64_t *dst) {
        const size_t lds = vpoly::lds_bytes<T>(n_terms, coef != nullptr, ge.pair);
        const Terms tm = vpoly::pack_terms(terms, n_terms, n_tables);
        const unsigned np_total = (unsigned)p.np_total;
        for (unsigned t0 = 0; t0 < np_total; t0 += (unsigned)p.np_launch) {
            const unsigned np = np_total - t0 < (unsigned)p.np_launch ? np_total - t0 : (unsigned)p.np_launch;
            vpoly::with_slots(n_tables, [&](auto nt) { launch_points<T, decltype(nt)::value>(kc, ge, p, lds, dst, tb, tm, coef, weights, sh, t0, np, s); });
        }
    });
}
// The fused launch, then the remaining points from the weighted round kernels over the folded tables.  fo.p holds the output
// pointers; n_out receives the elements written per table.  aligned: every table, folded table, the weights, the coefficients, r, out
// and work start on a 16-byte boundary.  Every table empty: nothing to visit.
template <class T>
inline hipError_t launch_fold(const typename sumcheck::Family<T>::K &kc, const Plan &p, int order, uint64_t *out, const uint64_t *weights,
                              const Tables &tb, Folded fo, const uint64_t *r, int n_tables, const Term *terms, int n_terms, const uint64_t *coef,
                              size_t num_vars, size_t *n_out, int k, bool aligned, uint64_t *work, hipStream_t s) {
    vpoly_fold::Shape sh;
    const bool any = vpoly_fold::shape_of(order, num_vars, tb.n, n_tables, terms, n_terms, &fo, &sh);
    for (int j = 0; j < n_tables; j++) n_out[j] = fo.n[j];
    const sumcheck::Geometry ge = sumcheck::geometry_of<T>(k, aligned);
    return sumcheck::launch_plan<T>(p, ge, !any, out, work, s, [&](uint64_t *dst) {
        const dim3 g = ge.grid(p.groups), b(256);
        const size_t groups = ge.groups(p.groups), lds = vpoly::lds_bytes<T>(n_terms, coef != nullptr, ge.pair);
        const Terms tm = vpoly::pack_terms(terms, n_terms, n_tables);
        const unsigned np_total = (unsigned)p.np_total;
        Tables ftb{};
        for (int j = 0; j < n_tables; j++) {
            ftb.p[j] = fo.p[j];
            ftb.n[j] = fo.n[j];
        }
        vpoly::with_slots(n_tables, [&](auto nt) {
            constexpr int NT = decltype(nt)::value, FP = fused_points_of<T>(NT);
            const unsigned fp = np_total < (unsigned)FP ? np_total : (unsigned)FP;
            if constexpr (sumcheck::kSlot<T>)
                hipLaunchKernelGGL((slot_fold_round_kernel<T, NT, FP>), g, b, lds, s, kc, dst, tb, fo, tm, coef, weights, r, sh.count, sh.qmax, sh.sb,
                                   sh.st, sh.fst, groups, fp, np_total);
            else
                hipLaunchKernelGGL((fold_round_kernel<T, NT, FP>), g, b, lds, s, dst, tb, fo, tm, coef, weights, r, sh.count, sh.qmax, sh.sb, sh.st,
                                   sh.fst, ge.k, ge.pair, groups, fp, np_total);
            if constexpr (FP <= MAX_FACTORS) {  // otherwise the fused launch has taken every point of every degree
                const vpoly::Shape rsh{sh.count, sh.sb, sh.st};
                for (unsigned t0 = fp; t0 < np_total; t0 += (unsigned)p.np_launch) {
                    const unsigned np = np_total - t0 < (unsigned)p.np_launch ? np_total - t0 : (unsigned)p.np_launch;
                    launch_points<T, NT>(kc, ge, p, lds, dst, ftb, tm, coef, weights, rsh, t0, np, s);
                }
            }
        });
    });
}

}  // namespace wsumcheck
}  // namespace sr
