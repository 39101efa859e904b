// Sum-check rounds of the RANGE (norm) CHECK of a lattice folding scheme: every entry of every table f_i lies in (-B, B) exactly when
//   sum_b eq(beta, b) * sum_i mu_i * P_B( f_i(b) ) = 0,     P_B(x) = prod_{j = -(B-1)}^{B-1} (x - R::from(j)),
// a claim of degree 2 B - 1 in each variable whose 2 B - 1 factors all come from ONE table.  The round message with the eq factor as a
// per-pair weight (sumcheck_weighted.hpp) is
//   h(t) = sum_{b < half} w[b] * sum_i mu_i * P_B( lo_i[b] + t (hi_i[b] - lo_i[b]) ),  t = 0 .. 2 B - 1
// with the pairs (lo, hi) of sumcheck.hpp in the same two orders.  The general term walk of sumcheck_vpoly.hpp would need 2 B - 1 table
// slots per table (f - j for every j), read and folded every round; here a table is read once and the shifts are constants:
//   P_B(x) = x * prod_{j = 1}^{B-1} (x^2 - j^2)                 B + 1 slot products per point, where the literal form needs 2 B - 1
// j^2 is R::from(j^2): in storage form a base-field constant (the Montgomery image F::mul_boundary(j^2, R^2) every field here stores),
// and in the slot rings it is subtracted from component 0 of the slot only -- R::from of an integer has the integer in component 0
// of every slot and zero elsewhere (fold_empty of capi.hip builds one() the same way).  The constants travel in the kernel arguments
// (Shifts<F>: seven storage words) and are read by a run-time loop over j: `bound` is a run-time argument, one kernel per family
// serves every B (DESIGN_APPENDIX.md A.18 has the listing's counts of the variants tried).
//
// Work per pair: the tables are walked ONE AT A TIME by a loop that is not unrolled.  For table i the lane loads lo, hi, forms
// dl = hi - lo and the hoisted canonical product c = mu_i * w (c = w without coefficients), and per point takes
//   s = v * v,  pr = c * prod_j (s - j^2)  (B - 1 canonical products),  acc[t].fma(pr, v)  (one lazy term),  v += dl.
// Only v, dl, c and w of one table are live beside the accumulators, so the register need does not grow with n_tables.
//
// Everything but the walk is taken from the neighbouring files, not copied: mle::Lane, the records, the meeting of the lane-groups
// and the launch skeleton (sumcheck.hpp: plan_records, geometry_of, launch_plan, sum_groups_kernel, zero_kernel), load_pair
// (sumcheck_fold.hpp), pairs_of, Tables and lds_bytes (sumcheck_vpoly.hpp), the coefficient stash, flush_points / slot_flush_points and
// store_points (sumcheck_weighted.hpp), SumOfProducts / SlotDot and kFlush.  No kernel of those files is changed or instantiated
// differently.
//
// Lazy sums.  Each accumulator takes exactly one fma(pr, v) per table and pair, so at most n_tables per pair, and the sums are reduced
// before a pair that would take them past kFlush = 64 accumulated terms (since + n_tables > kFlush).  pr is a canonical product (or
// the canonical weight times canonical factors), v a canonical table value advanced by canonical additions: both operands are the
// canonical images below 2^64 (2^31 for BabyBear-72) that sumcheck.hpp's bound assumes, which therefore carries over word for word:
//   SumOfProducts<Goldilocks>      four 96-bit sums of 32 x 32-bit products: 2^6 (2^32 - 1)^2 < 2^70
//   SlotDot<SlotG24> / <SlotFrog>  at most 2 x 4 partial products per term and sum: 2^6 * 8 * (2^32 - 1)^2 < 2^73
//   SlotDot<SlotB72>               at most 9 products of 31-bit images per term and sum: 2^6 * 9 * 2^62 < 2^72 (redc() wants < 2^29 terms)
//   SumOfProducts<BabyBear> / <Stark>  canonical after every term: no bound
// All sums are exact modular integers on canonical values, so neither the grid, the split, the association nor the factoring of P_B
// changes a bit of the result.
//
// Truncated storage: a pair of table i is visited exactly while its first element is stored; an absent second element is zero and is
// never loaded.  An unvisited pair has v(t) = 0 at every t and P_B(0) = 0 (the factor j = 0), so skipping it is exact.  The loop runs to
// the LONGEST table, so a weight whose pair no table visits is not read.  Every table empty: one launch that zeroes the output.
//
// Points per launch (points_of below): per family the largest number of the 2 B points that leaves the kernel without scratch inside
// the family's register bound -- 256 registers, BabyBear 128 -- read from the gfx950 listing of tools/ubench/range_isa.hip
// (tests/test_range_isa.py pins every count).  It does not depend on n_tables nor on B:
//   Goldilocks 7 (248 registers; eight: 276), BabyBear 8 (90; from nine on the unrolled tail of store_points no longer unrolls and the
//   sums go to scratch), Stark 3 (246; four: 295), goldilocks24 2 (220; three spill), babybear72 2 (214; three spill), frog16 2 (244;
//   three spill)
// A call of bound B takes ceil(2 B / points) launches, each of which reads the tables and the weights once.
#pragma once
#include "decompose.hpp"
#include "lincomb.hpp"
#include "sumcheck_weighted.hpp"

namespace sr {
namespace range {

enum { MAX_TABLES = 8, MAX_BOUND = 8 };
using sumcheck::kFlush;
using vpoly::Tables;

// the images of j^2, j = 1 .. MAX_BOUND - 1, in storage form; by value in the kernel arguments
template <class F>
struct Shifts {
    typename F::storage k[MAX_BOUND - 1];
};
template <class F>
inline Shifts<F> shifts_of() {
    Shifts<F> sh;
    for (int j = 1; j < MAX_BOUND; j++) F::store(&sh.k[j - 1], F::mul_boundary(dec::Consts<F>::from_u64((uint64_t)(j * j)), dec::Consts<F>::r2()));
    return sh;
}
// the invariant-checking build counts every word >= p that leaves the call (lincomb::leaves); nothing in the product library
template <class F>
__device__ __forceinline__ void leaves(const typename F::elem &v) {
#if defined(SR_GL_CHECK_REPS)
    lincomb::leaves<F>(v);
#else
    (void)v;
#endif
}

// ---- power-of-two rings -----------------------------------------------------------------------------------------------------------
// the points i < np of one table and pair for one coefficient of the lane: cw = [mu_i *] w; v is advanced point by point
template <class F, int NP>
__device__ __forceinline__ void table_points(SumOfProducts<F> (&acc)[NP], typename F::elem v, const typename F::elem &dl, const typename F::elem &cw,
                                             const Shifts<F> &sh, int bound, unsigned np) {
    using E = typename F::elem;
#pragma unroll
    for (int i = 0; i < NP; i++) {
        if ((unsigned)i < np) {
            const E s = F::mul_boundary(v, v);
            E pr = cw;
#pragma unroll 1
            for (int j = 0; j < bound - 1; j++) pr = F::mul_boundary(pr, F::sub(s, F::load(&sh.k[j])));
            acc[i].fma(pr, v);
        }
        if (i + 1 < NP) {
            if ((unsigned)(i + 1) < np) v = F::add(v, dl);
        }
    }
}
// up to NP points t0 .. t0 + np - 1 of np_total = 2 bound.  wp: the weights, one element per pair.  coef: mu, n_tables elements, or
// null.  groups, lu, dst, lds: as wsumcheck::round_units.
template <class F, int RW, int NP>
__device__ __forceinline__ void round_units(uint64_t *dst, const Tables &tb, int n_tables, const Shifts<F> &sh, int bound, const uint64_t *coef,
                                            const uint64_t *wp, size_t count, size_t sb, size_t st, int lu, size_t groups, unsigned t0, unsigned np,
                                            unsigned np_total, uint64_t *lds) {
    using E = typename F::elem;
    using L = mle::Lane<F, RW>;
    const size_t flat = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t g = flat >> lu, c = flat & (((size_t)1 << lu) - 1);
    const bool in_block = lu < 8;  // uniform; the grid of such a launch is exact, so every lane reaches the barriers below
    if (!in_block && g >= groups) return;
    const bool has_coef = coef != nullptr;
    if (has_coef) wsumcheck::stash_coefficients<F, RW>(lds, coef, n_tables, lu, c);
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
        const size_t e0 = b * sb;
        if (since + (unsigned)n_tables > kFlush) {
            since = 0;
            wsumcheck::flush_points<F>(acc, total);
        }
        since += (unsigned)n_tables;
        L wl;
        wl.template load<true>(wp + ((b << lu) + c) * RW);
#pragma unroll 1
        for (int i = 0; i < n_tables; i++) {
            const size_t n_i = tb.n[i];
            if (e0 >= n_i) continue;  // not visited: P_B(0) = 0
            L lo, hi, ck;
            sumcheck_fold::load_pair<F, RW>(lo, hi, tb.p[i], n_i, b, sb, st, lu, c);
            if (has_coef) {
#pragma unroll
                for (int q = 0; q < RW; q++) ck.w[q] = lds[((size_t)i * 256 + threadIdx.x) * RW + q];
            } else {
                ck.zero();
            }
#pragma unroll
            for (int n = 0; n < L::NC; n++) {
                E v = lo.get(n);
                const E dl = F::sub(hi.get(n), v);
                for (unsigned q = 0; q < t0; q++) v = F::add(v, dl);
                E cw = wl.get(n);
                if (has_coef) cw = F::mul_boundary(ck.get(n), cw);
                table_points<F, NP>(acc[n], v, dl, cw, sh, bound, np);
            }
        }
    }
#if defined(SR_GL_CHECK_REPS)
    wsumcheck::flush_points<F>(acc, total);
#pragma unroll
    for (int i = 0; i < NP; i++)
#pragma unroll
        for (int n = 0; n < L::NC; n++) leaves<F>(total[i][n]);
#endif
    wsumcheck::store_points<F, RW, NP>(dst, total, acc, in_block, g, c, lu, t0, np, np_total, lds);
}
// pair: the tables, the weights, the coefficients and dst are 16-byte aligned and k >= 1 (one-limb fields).  Dynamic LDS:
// vpoly::lds_bytes() with n_tables for n_terms.
template <class F, int NP>
__global__ __launch_bounds__(256) void round_kernel(uint64_t *dst, Tables tb, int n_tables, Shifts<F> sh, int bound, const uint64_t *coef,
                                                    const uint64_t *wp, size_t count, size_t sb, size_t st, int k, int pair, size_t groups, unsigned t0,
                                                    unsigned np, unsigned np_total) {
    extern __shared__ __align__(16) uint64_t range_lds[];
    constexpr int RWMAX = sizeof(typename F::storage) == 8 ? 2 : (int)sizeof(typename F::storage) / 8;
    if constexpr (sizeof(typename F::storage) == 8) {
        if (pair) round_units<F, 2, NP>(dst, tb, n_tables, sh, bound, coef, wp, count, sb, st, k - 1, groups, t0, np, np_total, range_lds);
        else round_units<F, 1, NP>(dst, tb, n_tables, sh, bound, coef, wp, count, sb, st, k, groups, t0, np, np_total, range_lds);
    } else {
        round_units<F, RWMAX, NP>(dst, tb, n_tables, sh, bound, coef, wp, count, sb, st, k, groups, t0, np, np_total, range_lds);
    }
}

// ---- goldilocks24 / babybear72 / frog16: lane = slot ---------------------------------------------------------------------------------
// A workgroup holds 256 / S lane-groups; they meet in LDS (slot_reduce_store) and the workgroup is record blockIdx.x.  The grid is
// exact (groups = gridDim.x * 256 / S), so every lane reaches the barriers.  The coefficients sit in LDS once per workgroup.  Two
// waves per SIMD is what 256 registers allow; said outright, as for the slot kernels of sumcheck_weighted.hpp.
template <class SL, int NP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void slot_round_kernel(
    typename SL::K kc, uint64_t *dst, Tables tb, int n_tables, Shifts<typename SL::F> sh, int bound, const uint64_t *coef, const uint64_t *wp,
    size_t count, size_t sb, size_t st, size_t groups, unsigned t0, unsigned np, unsigned np_total) {
    using F = typename SL::F;
    using E = typename F::elem;
    constexpr int W = SL::W, S = SL::D / SL::W;
    const size_t flat = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t g = flat / S;
    const int off = (int)(flat % S) * W;
    __shared__ E lds[256 * W];
    __shared__ E cl[MAX_TABLES * SL::D];
    const bool has_coef = coef != nullptr;
    if (has_coef) {
        for (int i = threadIdx.x; i < n_tables * SL::D; i += 256) cl[i] = F::load(coef + i);
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
        if (since + (unsigned)n_tables > kFlush) {
            since = 0;
            wsumcheck::slot_flush_points<SL, NP, NP>(kc, total, acc);
        }
        since += (unsigned)n_tables;
        E w[W];
        slot_load<SL>(w, wp + b * SL::D + off);
#pragma unroll 1
        for (int i = 0; i < n_tables; i++) {
            const size_t n_i = tb.n[i];
            if (e0 >= n_i) continue;  // not visited: P_B(0) = 0
            const uint64_t *tp = tb.p[i];
            E v[W], dl[W], cw[W];
            slot_load<SL>(v, tp + e0 * SL::D + off);
            if (e1 < n_i) {
                slot_load<SL>(dl, tp + e1 * SL::D + off);
#pragma unroll
                for (int m = 0; m < W; m++) dl[m] = F::sub(dl[m], v[m]);
            } else {
#pragma unroll
                for (int m = 0; m < W; m++) dl[m] = F::sub(F::zero(), v[m]);
            }
            for (unsigned q = 0; q < t0; q++)
#pragma unroll
                for (int m = 0; m < W; m++) v[m] = F::add(v[m], dl[m]);
#pragma unroll
            for (int m = 0; m < W; m++) cw[m] = w[m];
            if (has_coef) {
                E ck[W];
#pragma unroll
                for (int m = 0; m < W; m++) ck[m] = cl[i * SL::D + off + m];
                SL::mul(cw, ck, kc);
            }
#pragma unroll
            for (int p = 0; p < NP; p++) {
                if ((unsigned)p < np) {
                    E s[W], pr[W];
#pragma unroll
                    for (int m = 0; m < W; m++) {
                        s[m] = v[m];
                        pr[m] = cw[m];
                    }
                    SL::mul(s, v, kc);
#pragma unroll 1
                    for (int j = 0; j < bound - 1; j++) {
                        E x[W];
#pragma unroll
                        for (int m = 0; m < W; m++) x[m] = s[m];
                        x[0] = F::sub(s[0], F::load(&sh.k[j]));  // R::from(j^2): component 0 only
                        SL::mul(pr, x, kc);
                    }
                    acc[p].fma(pr, v);
                }
                if (p + 1 < NP) {
                    if ((unsigned)(p + 1) < np) {
#pragma unroll
                        for (int m = 0; m < W; m++) v[m] = F::add(v[m], dl[m]);
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
        for (int m = 0; m < W; m++) {
            total[i][m] = F::add(total[i][m], r[m]);
            leaves<F>(total[i][m]);
        }
        if (i) __syncthreads();  // the previous point's sums have been read
        slot_reduce_store<SL>(lds, total[i], dst + (blockIdx.x * (size_t)np_total + t0 + i) * SL::D);
    }
}

// ---- the plan: pure host arithmetic -------------------------------------------------------------------------------------------------
// points of one launch: the largest number within the family's register bound without scratch (tests/test_range_isa.py holds the
// register counts); independent of n_tables and of the bound
template <class T>
constexpr int points_of() {
    if (std::is_same<T, Goldilocks>::value) return 7;  // eight: 276 registers
    if (std::is_same<T, BabyBear>::value) return 8;    // nine: scratch (the tail of store_points is no longer unrolled)
    if (std::is_same<T, Stark>::value) return 3;       // four: 295 registers
    return 2;  // goldilocks24 (220), babybear72 (214), frog16 (244): three spill
}
inline int points_per_launch(int ring) {
    switch (ring) {
        case 0: return points_of<Goldilocks>();
        case 1: return points_of<BabyBear>();
        case 2: return points_of<Stark>();
        case 3: return points_of<SlotG24>();
        case 4: return points_of<SlotB72>();
        default: return points_of<SlotFrog>();
    }
}
using Plan = sumcheck::Plan;
// the records of sumcheck.hpp (plan_records) with 2 bound points in launches of points_of
inline bool plan(int ring, int k, size_t num_vars, int n_tables, int bound, int order, Plan *p) {
    if (ring < 0 || ring > 5 || num_vars < 1 || num_vars > sumcheck::MAX_VARS || n_tables < 1 || n_tables > MAX_TABLES || bound < 2 ||
        bound > MAX_BOUND || (order != sumcheck::MODE_LEADING && order != sumcheck::MODE_TRAILING))
        return false;
    *p = Plan{};
    p->count = (size_t)1 << (num_vars - 1);
    p->np_total = 2 * bound;
    p->np_launch = points_per_launch(ring);
    if (p->np_launch > p->np_total) p->np_launch = p->np_total;
    sumcheck::plan_records(ring, k, (p->np_total + p->np_launch - 1) / p->np_launch, p);
    return true;
}

// ---- launcher: the skeleton is sumcheck::launch_plan --------------------------------------------------------------------------------
// The points in chunks of np_launch.  aligned: every table, the weights, the coefficients, out and work start on a 16-byte boundary.
// Every table empty: nothing to visit.
template <class T>
inline hipError_t launch(const typename sumcheck::Family<T>::K &kc, const Plan &p, int order, uint64_t *out, const uint64_t *weights, const Tables &tb,
                         int n_tables, int bound, const uint64_t *coef, size_t num_vars, int k, bool aligned, uint64_t *work, hipStream_t s) {
    using F = typename sumcheck::Family<T>::F;
    const sumcheck::Geometry ge = sumcheck::geometry_of<T>(k, aligned);
    size_t nmax = 0;
    for (int j = 0; j < n_tables; j++) nmax = tb.n[j] > nmax ? tb.n[j] : nmax;
    const size_t count = vpoly::pairs_of(order, num_vars, nmax);  // the loop ends at the longest table
    const size_t sb = order == sumcheck::MODE_LEADING ? 2 : 1, st = order == sumcheck::MODE_LEADING ? 1 : (size_t)1 << (num_vars - 1);
    return sumcheck::launch_plan<T>(p, ge, count == 0, out, work, s, [&](uint64_t *dst) {
        constexpr int NP = points_of<T>();
        const dim3 g = ge.grid(p.groups), b(256);
        const size_t groups = ge.groups(p.groups), lds = vpoly::lds_bytes<T>(n_tables, coef != nullptr, ge.pair);
        const Shifts<F> sh = shifts_of<F>();
        const unsigned np_total = (unsigned)p.np_total;
        for (unsigned t0 = 0; t0 < np_total; t0 += (unsigned)p.np_launch) {
            const unsigned np = np_total - t0 < (unsigned)p.np_launch ? np_total - t0 : (unsigned)p.np_launch;
            if constexpr (sumcheck::kSlot<T>)
                hipLaunchKernelGGL((slot_round_kernel<T, NP>), g, b, lds, s, kc, dst, tb, n_tables, sh, bound, coef, weights, count, sb, st, groups, t0,
                                   np, np_total);
            else
                hipLaunchKernelGGL((round_kernel<T, NP>), g, b, lds, s, dst, tb, n_tables, sh, bound, coef, weights, count, sb, st, ge.k, ge.pair,
                                   groups, t0, np, np_total);
        }
    });
}

}  // namespace range
}  // namespace sr
