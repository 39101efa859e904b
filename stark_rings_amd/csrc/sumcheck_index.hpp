// Weighted sum-check rounds whose factors may be INTEGER COLUMNS: a slot of the sum of products is a table of ring elements or one
// uint64_t per row (or the progression start + e, which reads no memory) that stands for the table R::from(col[e]).
//   round    h(t) = sum_b w[b] * sum_k c_k prod_s ( lo_s[b] + t (hi_s[b] - lo_s[b]) )   exactly as sumcheck_weighted.hpp, where a column
//            slot's lo / hi are R::from of the pair of integers (col[2b], col[2b + 1]) or (col[b], col[b + half])
//   fused    every slot -- table or column -- is folded at r to a ring table of half the length, and the first points of the message
//            that follows come from the folded neighbours in registers; the remaining points come from the weighted round kernels of
//            sumcheck_weighted.hpp over the folded tables, which are all ring tables by then
// The selectors of a Plonkish gate, a 0/1 mask, a multiplicity column, sigma and id never exist as D words per row: the first message
// reads 8 bytes per row and column slot, the first fold reads 8 bytes and writes the folded ring table.
//
// Slot s < first is table s, slot s >= first is column s - first; the Tables record carries the stored length of either kind
// (a progression: 2^num_vars), so the shapes, the truncation rule and the plan's records are those of sumcheck_weighted.hpp unchanged.
//
// The helpers are reused as they are: pair_points / slot_pair_points (the term walk and the lazy sums), flush_points, store_points,
// stash_coefficients, weight_in_lds and the launch skeleton (sumcheck_weighted.hpp, sumcheck.hpp); load_pair / fold_pair /
// slot_fold_one for the table slots (sumcheck_fold.hpp); Embed<F> (lincomb_index.hpp).  The four kernel bodies -- round_units,
// fold_round_units, slot_round_kernel, slot_fold_round_kernel -- are COPIES of those of sumcheck_weighted.hpp in which only the operand
// loader is new (that file's templates were not to be edited): a change to the flush, the meeting of the lane-groups or the store
// sequence there has to be made here as well, as the note at its head says.
//
// R::from(x) in the memory image is Embed<F>::mul(prep(image of 1), x): the canonical product of the field's 1 and the raw integer,
// which takes any 64-bit x (values >= p are reduced by the product itself).  Power-of-two rings: that value in every coefficient of
// the lane.  goldilocks24 / babybear72 / frog16: in component 0 of the lane's slot, zero in the others.  From there a column pair is a
// table pair: the same canonical values go through the same F::sub / F::add / mul_boundary / SL::mul as the table R::from(col) would,
// so every word equals sr_lincomb_index_dev followed by the weighted call (tests/test_isumcheck_gpu.py).  The lazy-sum bound of
// sumcheck_weighted.hpp holds word for word: both operands of every fma() are canonical images.
//
// All lanes of a lane-group want the same col[e]: where a ring element spans whole waves (2^lu >= 64 lanes) the element index goes
// through readfirstlane, as in lincomb_index::column().  Columns are 8-byte loads with the default cache policy.
//
// Points per launch are wsumcheck::points_of / fused_points_of, those of the weighted kernels at the same slot count wherever the gfx950
// listing of tools/ubench/isumcheck_isa.hip stays without scratch inside the family's register bound (tests/test_isumcheck_isa.py).
#pragma once
#include "decompose.hpp"
#include "lincomb_index.hpp"
#include "sumcheck_weighted.hpp"

namespace sr {
namespace isumcheck {

using lincomb_index::Embed;
using sumcheck::kFlush;
using vpoly::MAX_TABLES;
using vpoly::Tables;
using vpoly::Term;
using vpoly::Terms;
using vpoly_fold::Folded;

enum { MAX_COLUMNS = 8 };

// the column slots of a call, by value in the kernel arguments; indexed by SLOT (entries below `first` are unused)
template <class F>
struct Columns {
    const uint64_t *p[MAX_TABLES];  // null: the progression start[s] + e
    uint64_t start[MAX_TABLES];
    int first;                     // slots below are tables
    typename Embed<F>::P one;      // the prepared image of the field's 1
};
// the image of 1 as Embed takes its first factor: host arithmetic
template <class F>
inline typename Embed<F>::P one_of() {
    return Embed<F>::prep(F::mul_boundary(dec::Consts<F>::one(), dec::Consts<F>::r2()));
}
// the image of R::from(col_s[e]) in one base-field component; e is below the column's stored length.  uniform: every lane of the wave
// has the same e
template <class F>
__device__ __forceinline__ typename F::elem embed(const Columns<F> &cl, int s, size_t e, bool uniform) {
    const uint64_t *p = cl.p[s];
    uint64_t x;
    if (!p) {
        x = cl.start[s] + e;
    } else {
        if (uniform) {
            const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)e), hi = __builtin_amdgcn_readfirstlane((uint32_t)(e >> 32));
            e = (size_t)lo | ((size_t)hi << 32);
        }
        x = p[e];
    }
    return Embed<F>::mul(cl.one, x);
}

// ---- power-of-two rings -----------------------------------------------------------------------------------------------------------
// element e of slot s for the lane's unit; e is below the slot's stored length
template <class F, int RW>
__device__ __forceinline__ void load_slot(mle::Lane<F, RW> &x, const Tables &tb, const Columns<F> &cl, int s, size_t e, int lu, size_t c,
                                          bool uniform) {
    if (s < cl.first) {
        x.template load<true>(tb.p[s] + ((e << lu) + c) * RW);
    } else {
        const typename F::elem v = embed<F>(cl, s, e, uniform);
#pragma unroll
        for (int n = 0; n < mle::Lane<F, RW>::NC; n++) x.put(n, v);
    }
}
// sumcheck_fold::load_pair for either kind of slot
template <class F, int RW>
__device__ __forceinline__ void load_pair(mle::Lane<F, RW> &a, mle::Lane<F, RW> &b, const Tables &tb, const Columns<F> &cl, int s, size_t o,
                                          size_t sb, size_t fst, int lu, size_t c, bool uniform) {
    if (s < cl.first) {
        sumcheck_fold::load_pair<F, RW>(a, b, tb.p[s], tb.n[s], o, sb, fst, lu, c);
    } else {
        const size_t e0 = o * sb, e1 = e0 + fst;
        load_slot<F, RW>(a, tb, cl, s, e0, lu, c, uniform);
        if (e1 < tb.n[s]) load_slot<F, RW>(b, tb, cl, s, e1, lu, c, uniform);
        else b.zero();
    }
}

// wsumcheck::round_units with the loader above
template <class F, int RW, int NT, int NP>
__device__ __forceinline__ void round_units(uint64_t *dst, const Tables &tb, const Columns<F> &cl, const Terms &tm, const uint64_t *coef,
                                            const uint64_t *wp, size_t count, size_t sb, size_t st, int lu, size_t groups, unsigned t0, unsigned np,
                                            unsigned np_total, uint64_t *lds) {
    using E = typename F::elem;
    using L = mle::Lane<F, RW>;
    const size_t flat = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t g = flat >> lu, c = flat & (((size_t)1 << lu) - 1);
    const bool in_block = lu < 8;  // uniform; the grid of such a launch is exact, so every lane reaches the barriers below
    if (!in_block && g >= groups) return;
    const bool uniform = lu >= 6;  // a workgroup is four waves of 64 consecutive lanes
    const bool has_coef = coef != nullptr;
    const int n_terms = tm.n_terms, n_tables = tm.n_tables;
    if (has_coef) wsumcheck::stash_coefficients<F, RW>(lds, coef, n_terms, lu, c);
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
            wsumcheck::flush_points<F>(acc, total);
        }
        since += (unsigned)n_terms;
        L lo[NT], hi[NT], wl;
        wl.template load<true>(wp + ((b << lu) + c) * RW);
#pragma unroll
        for (int j = 0; j < NT; j++) {
            if (j < n_tables && e0 < tb.n[j]) load_slot<F, RW>(lo[j], tb, cl, j, e0, lu, c, uniform);
            else lo[j].zero();
            if (j < n_tables && e1 < tb.n[j]) load_slot<F, RW>(hi[j], tb, cl, j, e1, lu, c, uniform);
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
            wsumcheck::pair_points<F, RW, NT, NP>(acc[n], v, dl, wl.get(n), tm, has_coef, lds, n, np);
        }
    }
    wsumcheck::store_points<F, RW, NP>(dst, total, acc, in_block, g, c, lu, t0, np, np_total, lds);
}
// pair: the tables, the weights, the coefficients and dst are 16-byte aligned and k >= 1 (one-limb fields).  Dynamic LDS:
// vpoly::lds_bytes().
template <class F, int NT, int NP>
__global__ __launch_bounds__(256) void round_kernel(uint64_t *dst, Tables tb, Columns<F> cl, Terms tm, const uint64_t *coef, const uint64_t *wp,
                                                    size_t count, size_t sb, size_t st, int k, int pair, size_t groups, unsigned t0, unsigned np,
                                                    unsigned np_total) {
    extern __shared__ __align__(16) uint64_t isumcheck_lds[];
    constexpr int RWMAX = sizeof(typename F::storage) == 8 ? 2 : (int)sizeof(typename F::storage) / 8;
    if constexpr (sizeof(typename F::storage) == 8) {
        if (pair) round_units<F, 2, NT, NP>(dst, tb, cl, tm, coef, wp, count, sb, st, k - 1, groups, t0, np, np_total, isumcheck_lds);
        else round_units<F, 1, NT, NP>(dst, tb, cl, tm, coef, wp, count, sb, st, k, groups, t0, np, np_total, isumcheck_lds);
    } else {
        round_units<F, RWMAX, NT, NP>(dst, tb, cl, tm, coef, wp, count, sb, st, k, groups, t0, np, np_total, isumcheck_lds);
    }
}

// The fold of slot J to lo = g[o0], hi = g[o1], both stored.  J is a template parameter and the slots are a fold expression, not a
// loop: with Stark's embedding four times per slot the body is past the size to which the compiler unrolls even a loop it is told to
// unroll, and a loop over j indexes lo[j] at run time, i.e. in scratch (as vpoly_fold::slot_fold_slot).
template <class F, int RW, int NT, int J>
__device__ __forceinline__ void fold_slot(mle::Lane<F, RW> (&lo)[NT], mle::Lane<F, RW> (&hi)[NT], const Tables &tb, const Columns<F> &cl,
                                          const Folded &fo, int n_tables, size_t o0, size_t o1, size_t sb, size_t fst, int lu, size_t c,
                                          bool uniform, const mle::Lane<F, RW> &rr) {
    using L = mle::Lane<F, RW>;
    if (J < n_tables && o0 < fo.n[J]) {  // its first input is stored
        L x0, x1;
        load_pair<F, RW>(lo[J], x0, tb, cl, J, o0, sb, fst, lu, c, uniform);
        const bool second = o1 < fo.n[J];
        if (second) load_pair<F, RW>(hi[J], x1, tb, cl, J, o1, sb, fst, lu, c, uniform);
        sumcheck_fold::fold_pair<F, RW>(lo[J], x0, rr);
        lo[J].store(fo.p[J] + ((o0 << lu) + c) * RW);
        if (second) {
            sumcheck_fold::fold_pair<F, RW>(hi[J], x1, rr);
            hi[J].store(fo.p[J] + ((o1 << lu) + c) * RW);
        } else {
            hi[J].zero();
        }
    } else {
        lo[J].zero();
        hi[J].zero();
    }
}
template <class F, int RW, int NT, int... J>
__device__ __forceinline__ void fold_slots(std::integer_sequence<int, J...>, mle::Lane<F, RW> (&lo)[NT], mle::Lane<F, RW> (&hi)[NT], const Tables &tb,
                                           const Columns<F> &cl, const Folded &fo, int n_tables, size_t o0, size_t o1, size_t sb, size_t fst, int lu,
                                           size_t c, bool uniform, const mle::Lane<F, RW> &rr) {
    (fold_slot<F, RW, NT, J>(lo, hi, tb, cl, fo, n_tables, o0, o1, sb, fst, lu, c, uniform, rr), ...);
}
// wsumcheck::fold_round_units with the loader above: a column slot is folded to a ring table like any other
template <class F, int RW, int NT, int NP>
__device__ __forceinline__ void fold_round_units(uint64_t *dst, const Tables &tb, const Columns<F> &cl, const Folded &fo, const Terms &tm,
                                                 const uint64_t *coef, const uint64_t *wp, const uint64_t *rp, size_t count, size_t qmax, size_t sb,
                                                 size_t st, size_t fst, int lu, size_t groups, unsigned np, unsigned np_total, uint64_t *lds) {
    using E = typename F::elem;
    using L = mle::Lane<F, RW>;
    const size_t flat = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t g = flat >> lu, c = flat & (((size_t)1 << lu) - 1);
    const bool in_block = lu < 8;  // uniform; the grid of such a launch is exact, so every lane reaches the barriers below
    if (!in_block && g >= groups) return;
    const bool uniform = lu >= 6;
    const bool has_coef = coef != nullptr;
    const int n_terms = tm.n_terms, n_tables = tm.n_tables;
    if (has_coef) wsumcheck::stash_coefficients<F, RW>(lds, coef, n_terms, lu, c);
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
        fold_slots<F, RW, NT>(std::make_integer_sequence<int, NT>{}, lo, hi, tb, cl, fo, n_tables, o0, o1, sb, fst, lu, c, uniform, rr);
        if (b >= count) continue;  // beyond the longest folded term: every term has a zero factor at every t, and no weight is read
        if (since + (unsigned)n_terms > kFlush) {
            since = 0;
            wsumcheck::flush_points<F>(acc, total);
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
            wsumcheck::pair_points<F, RW, NT, NP>(acc[n], v, dl, wl.get(n), tm, has_coef, lds, n, np);
        }
    }
    wsumcheck::store_points<F, RW, NP>(dst, total, acc, in_block, g, c, lu, 0, np, np_total, lds);
}
// pair: every table, folded table, the weights, the coefficients, r and dst are 16-byte aligned and k >= 1 (one-limb fields)
template <class F, int NT, int NP>
__global__ __launch_bounds__(256) void fold_round_kernel(uint64_t *dst, Tables tb, Columns<F> cl, Folded fo, Terms tm, const uint64_t *coef,
                                                         const uint64_t *wp, const uint64_t *rp, size_t count, size_t qmax, size_t sb, size_t st,
                                                         size_t fst, int k, int pair, size_t groups, unsigned np, unsigned np_total) {
    extern __shared__ __align__(16) uint64_t isumcheck_fold_lds[];
    constexpr int RWMAX = sizeof(typename F::storage) == 8 ? 2 : (int)sizeof(typename F::storage) / 8;
    if constexpr (sizeof(typename F::storage) == 8) {
        if (pair)
            fold_round_units<F, 2, NT, NP>(dst, tb, cl, fo, tm, coef, wp, rp, count, qmax, sb, st, fst, k - 1, groups, np, np_total,
                                           isumcheck_fold_lds);
        else
            fold_round_units<F, 1, NT, NP>(dst, tb, cl, fo, tm, coef, wp, rp, count, qmax, sb, st, fst, k, groups, np, np_total, isumcheck_fold_lds);
    } else {
        fold_round_units<F, RWMAX, NT, NP>(dst, tb, cl, fo, tm, coef, wp, rp, count, qmax, sb, st, fst, k, groups, np, np_total,
                                           isumcheck_fold_lds);
    }
}

// ---- goldilocks24 / babybear72 / frog16: lane = slot ---------------------------------------------------------------------------------
// element e of operand slot s for the lane's ring slot: a column's value sits in component 0, the others are zero
template <class SL>
__device__ __forceinline__ void slot_load_slot(typename SL::F::elem *x, const Tables &tb, const Columns<typename SL::F> &cl, int s, size_t e,
                                               int off) {
    using F = typename SL::F;
    if (s < cl.first) {
        slot_load<SL>(x, tb.p[s] + e * SL::D + off);
    } else {
        x[0] = embed<F>(cl, s, e, false);
#pragma unroll
        for (int m = 1; m < SL::W; m++) x[m] = F::zero();
    }
}
// sumcheck_fold::slot_fold_one for either kind of operand slot
template <class SL>
__device__ __forceinline__ void slot_fold_one(typename SL::F::elem *out, const typename SL::K &k, const Tables &tb,
                                              const Columns<typename SL::F> &cl, int s, size_t o, size_t sb, size_t fst, int off,
                                              const typename SL::F::elem *r) {
    using F = typename SL::F;
    constexpr int W = SL::W;
    if (s < cl.first) {
        sumcheck_fold::slot_fold_one<SL>(out, k, tb.p[s], tb.n[s], o, sb, fst, off, r);
        return;
    }
    const size_t e0 = o * sb, e1 = e0 + fst;
    typename F::elem d[W];
    slot_load_slot<SL>(out, tb, cl, s, e0, off);
    if (e1 < tb.n[s]) {
        slot_load_slot<SL>(d, tb, cl, s, e1, off);
#pragma unroll
        for (int m = 0; m < W; m++) d[m] = F::sub(d[m], out[m]);
    } else {
#pragma unroll
        for (int m = 0; m < W; m++) d[m] = F::sub(F::zero(), out[m]);
    }
    SL::mul(d, r, k);
#pragma unroll
    for (int m = 0; m < W; m++) out[m] = F::add(out[m], d[m]);
}
// vpoly_fold::slot_fold_slot with the loader above; J is a template parameter for the reason given there
template <class SL, int NT, int J>
__device__ __forceinline__ void slot_fold_slot(typename SL::F::elem (&v)[NT][SL::W], typename SL::F::elem (&dl)[NT][SL::W], const typename SL::K &kc,
                                               const Tables &tb, const Columns<typename SL::F> &cl, const Folded &fo, int n_tables, size_t o0,
                                               size_t o1, size_t sb, size_t fst, int off, const typename SL::F::elem *rr) {
    using F = typename SL::F;
    constexpr int W = SL::W;
    if (J < n_tables && o0 < fo.n[J]) {
        slot_fold_one<SL>(v[J], kc, tb, cl, J, o0, sb, fst, off, rr);
        slot_store<SL>(fo.p[J] + o0 * SL::D + off, v[J]);
        if (o1 < fo.n[J]) {
            slot_fold_one<SL>(dl[J], kc, tb, cl, J, o1, sb, fst, off, rr);
            slot_store<SL>(fo.p[J] + o1 * SL::D + off, dl[J]);
#pragma unroll
            for (int m = 0; m < W; m++) dl[J][m] = F::sub(dl[J][m], v[J][m]);
        } else {
#pragma unroll
            for (int m = 0; m < W; m++) dl[J][m] = F::sub(F::zero(), v[J][m]);
        }
    } else {
#pragma unroll
        for (int m = 0; m < W; m++) v[J][m] = dl[J][m] = F::zero();
    }
}
template <class SL, int NT, int... J>
__device__ __forceinline__ void slot_fold_slots(std::integer_sequence<int, J...>, typename SL::F::elem (&v)[NT][SL::W],
                                                typename SL::F::elem (&dl)[NT][SL::W], const typename SL::K &kc, const Tables &tb,
                                                const Columns<typename SL::F> &cl, const Folded &fo, int n_tables, size_t o0, size_t o1, size_t sb,
                                                size_t fst, int off, const typename SL::F::elem *rr) {
    (slot_fold_slot<SL, NT, J>(v, dl, kc, tb, cl, fo, n_tables, o0, o1, sb, fst, off, rr), ...);
}
// wsumcheck::slot_round_kernel with the loader above
template <class SL, int NT, int NP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void slot_round_kernel(
    typename SL::K kc, uint64_t *dst, Tables tb, Columns<typename SL::F> cl, Terms tm, const uint64_t *coef, const uint64_t *wp, size_t count,
    size_t sb, size_t st, size_t groups, unsigned t0, unsigned np, unsigned np_total) {
    using F = typename SL::F;
    using E = typename F::elem;
    constexpr int W = SL::W, S = SL::D / SL::W;
    const size_t flat = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t g = flat / S;
    const int off = (int)(flat % S) * W;
    __shared__ E lds[256 * W];
    __shared__ E cf[vpoly::MAX_TERMS * SL::D];
    constexpr bool WL = wsumcheck::weight_in_lds<SL>(NT);
    __shared__ E wl[WL ? 256 * W : 1];
    const bool has_coef = coef != nullptr;
    const int n_terms = tm.n_terms, n_tables = tm.n_tables;
    if (has_coef) {
        for (int i = threadIdx.x; i < n_terms * SL::D; i += 256) cf[i] = F::load(coef + i);
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
            wsumcheck::slot_flush_points<SL, NP, NP>(kc, total, acc);
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
                slot_load_slot<SL>(v[j], tb, cl, j, e0, off);
            } else {
#pragma unroll
                for (int m = 0; m < W; m++) v[j][m] = F::zero();
            }
            if (j < n_tables && e1 < tb.n[j]) {
                slot_load_slot<SL>(dl[j], tb, cl, j, e1, off);
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
        if constexpr (WL) wsumcheck::slot_pair_points<SL, NT, NP, NP, true>(kc, acc, v, dl, wl + threadIdx.x * W, tm, has_coef, cf, off, np);
        else wsumcheck::slot_pair_points<SL, NT, NP, NP, false>(kc, acc, v, dl, w, tm, has_coef, cf, off, np);
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
// wsumcheck::slot_fold_round_kernel with the loader above
template <class SL, int NT, int NP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void slot_fold_round_kernel(
    typename SL::K kc, uint64_t *dst, Tables tb, Columns<typename SL::F> cl, Folded fo, Terms tm, const uint64_t *coef, const uint64_t *wp,
    const uint64_t *rp, size_t count, size_t qmax, size_t sb, size_t st, size_t fst, size_t groups, unsigned np, unsigned np_total) {
    using F = typename SL::F;
    using E = typename F::elem;
    constexpr int W = SL::W, S = SL::D / SL::W;
    const size_t flat = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t g = flat / S;
    const int off = (int)(flat % S) * W;
    __shared__ E lds[256 * W];
    __shared__ E cf[vpoly::MAX_TERMS * SL::D];
    const bool has_coef = coef != nullptr;
    const int n_terms = tm.n_terms, n_tables = tm.n_tables;
    if (has_coef) {
        for (int i = threadIdx.x; i < n_terms * SL::D; i += 256) cf[i] = F::load(coef + i);
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
        slot_fold_slots<SL, NT>(std::make_integer_sequence<int, NT>{}, v, dl, kc, tb, cl, fo, n_tables, o0, o1, sb, fst, off, rr);
        if (b >= count) continue;  // no weight is read beyond the longest folded term
        if constexpr (NP > 0) {
            if (since + (unsigned)n_terms > kFlush) {
                since = 0;
                wsumcheck::slot_flush_points<SL, NP, NA>(kc, total, acc);
            }
            since += (unsigned)n_terms;
            E w[W];
            slot_load<SL>(w, wp + b * SL::D + off);
            wsumcheck::slot_pair_points<SL, NT, NP, NA, false>(kc, acc, v, dl, w, tm, has_coef, cf, off, np);
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

// ---- the plan ------------------------------------------------------------------------------------------------------------------------
// The kernels above hold the points of their weighted siblings (wsumcheck::points_of / fused_points_of at the same slot count), so the
// plan of a call over n_tables + n_index slots IS wsumcheck::plan / wsumcheck::fold_plan at that many slots: capi.hip calls those.
using Plan = sumcheck::Plan;

// ---- launchers: the skeleton is sumcheck::launch_plan -------------------------------------------------------------------------------
// The column operands as the caller gives them: column j is slot n_tables + j.  values null: the progression start + e.
struct ColumnArgs {
    const uint64_t *values[MAX_COLUMNS];
    uint64_t start[MAX_COLUMNS];
    int n;
};
template <class T>
inline Columns<typename sumcheck::Family<T>::F> columns_of(const ColumnArgs &ca, int n_tables) {
    using F = typename sumcheck::Family<T>::F;
    Columns<F> cl{};
    cl.first = n_tables;
    cl.one = one_of<F>();
    for (int j = 0; j < ca.n; j++) {
        cl.p[n_tables + j] = ca.values[j];
        cl.start[n_tables + j] = ca.start[j];
    }
    return cl;
}
// The points in chunks of np_launch.  tb: n_slots = n_tables + ca.n entries, a column's with a null pointer and its stored length
// (a progression: 2^num_vars).  aligned: every table, the weights, the coefficients, out and work start on a 16-byte boundary.
template <class T>
inline hipError_t launch(const typename sumcheck::Family<T>::K &kc, const Plan &p, int order, uint64_t *out, const uint64_t *weights, const Tables &tb,
                         int n_tables, const ColumnArgs &ca, const Term *terms, int n_terms, const uint64_t *coef, size_t num_vars, int k,
                         bool aligned, uint64_t *work, hipStream_t s) {
    const int n_slots = n_tables + ca.n;
    const sumcheck::Geometry ge = sumcheck::geometry_of<T>(k, aligned);
    const vpoly::Shape sh = vpoly::shape_of(order, num_vars, tb.n, terms, n_terms);
    return sumcheck::launch_plan<T>(p, ge, sh.count == 0, out, work, s, [&](uint64_t *dst) {
        const size_t lds = vpoly::lds_bytes<T>(n_terms, coef != nullptr, ge.pair);
        const Terms tm = vpoly::pack_terms(terms, n_terms, n_slots);
        const auto cl = columns_of<T>(ca, n_tables);
        const unsigned np_total = (unsigned)p.np_total;
        const dim3 g = ge.grid(p.groups), b(256);
        const size_t groups = ge.groups(p.groups);
        for (unsigned t0 = 0; t0 < np_total; t0 += (unsigned)p.np_launch) {
            const unsigned np = np_total - t0 < (unsigned)p.np_launch ? np_total - t0 : (unsigned)p.np_launch;
            vpoly::with_slots(n_slots, [&](auto nt) {
                constexpr int NT = decltype(nt)::value, NP = wsumcheck::points_of<T>(NT);
                if constexpr (sumcheck::kSlot<T>)
                    hipLaunchKernelGGL((slot_round_kernel<T, NT, NP>), g, b, lds, s, kc, dst, tb, cl, tm, coef, weights, sh.count, sh.sb, sh.st, groups,
                                       t0, np, np_total);
                else
                    hipLaunchKernelGGL((round_kernel<T, NT, NP>), g, b, lds, s, dst, tb, cl, tm, coef, weights, sh.count, sh.sb, sh.st, ge.k, ge.pair,
                                       groups, t0, np, np_total);
            });
        }
    });
}
// The fused launch, then the remaining points from the weighted round kernels over the folded tables.  fo.p holds the n_slots output
// pointers; n_out receives the elements written per slot.  aligned: as above, and every folded table and r.
template <class T>
inline hipError_t launch_fold(const typename sumcheck::Family<T>::K &kc, const Plan &p, int order, uint64_t *out, const uint64_t *weights,
                              const Tables &tb, Folded fo, const uint64_t *r, int n_tables, const ColumnArgs &ca, const Term *terms, int n_terms,
                              const uint64_t *coef, size_t num_vars, size_t *n_out, int k, bool aligned, uint64_t *work, hipStream_t s) {
    const int n_slots = n_tables + ca.n;
    vpoly_fold::Shape sh;
    const bool any = vpoly_fold::shape_of(order, num_vars, tb.n, n_slots, terms, n_terms, &fo, &sh);
    for (int j = 0; j < n_slots; j++) n_out[j] = fo.n[j];
    const sumcheck::Geometry ge = sumcheck::geometry_of<T>(k, aligned);
    return sumcheck::launch_plan<T>(p, ge, !any, out, work, s, [&](uint64_t *dst) {
        const dim3 g = ge.grid(p.groups), b(256);
        const size_t groups = ge.groups(p.groups), lds = vpoly::lds_bytes<T>(n_terms, coef != nullptr, ge.pair);
        const Terms tm = vpoly::pack_terms(terms, n_terms, n_slots);
        const auto cl = columns_of<T>(ca, n_tables);
        const unsigned np_total = (unsigned)p.np_total;
        Tables ftb{};
        for (int j = 0; j < n_slots; j++) {
            ftb.p[j] = fo.p[j];
            ftb.n[j] = fo.n[j];
        }
        vpoly::with_slots(n_slots, [&](auto nt) {
            constexpr int NT = decltype(nt)::value, FP = wsumcheck::fused_points_of<T>(NT);
            const unsigned fp = np_total < (unsigned)FP ? np_total : (unsigned)FP;
            if constexpr (sumcheck::kSlot<T>)
                hipLaunchKernelGGL((slot_fold_round_kernel<T, NT, FP>), g, b, lds, s, kc, dst, tb, cl, fo, tm, coef, weights, r, sh.count, sh.qmax,
                                   sh.sb, sh.st, sh.fst, groups, fp, np_total);
            else
                hipLaunchKernelGGL((fold_round_kernel<T, NT, FP>), g, b, lds, s, dst, tb, cl, fo, tm, coef, weights, r, sh.count, sh.qmax, sh.sb, sh.st,
                                   sh.fst, ge.k, ge.pair, groups, fp, np_total);
            if constexpr (FP <= vpoly::MAX_FACTORS) {  // otherwise the fused launch has taken every point of every degree
                const vpoly::Shape rsh{sh.count, sh.sb, sh.st};
                for (unsigned t0 = fp; t0 < np_total; t0 += (unsigned)p.np_launch) {
                    const unsigned np = np_total - t0 < (unsigned)p.np_launch ? np_total - t0 : (unsigned)p.np_launch;
                    wsumcheck::launch_points<T, NT>(kc, ge, p, lds, dst, ftb, tm, coef, weights, rsh, t0, np, s);
                }
            }
        });
    });
}

}  // namespace isumcheck
}  // namespace sr
