// A sum-check round of a SUM OF PRODUCTS in one pass over the tables: fold every distinct table at the challenge r of the round that has
// just ended and, while the two folded neighbours are still in registers, walk the terms for the message of the round that follows.
//   fold     g_j = f_j with one variable fixed at r, per distinct table slot j: g[o] = f[2o] + r (f[2o + 1] - f[2o]) in leading order,
//            f[o] + r (f[o + half] - f[o]) in trailing order -- fold_kernel<F, 1> / slot_fold_kernel<SL, 1> of mle.hpp, element for
//            element, through load_pair / fold_pair / slot_fold_one of sumcheck_fold.hpp
//   message  p(t) = sum_b sum_k c_k prod_s ( lo[b] + t (hi[b] - lo[b]) ), t = 0 .. d, over the pairs (lo, hi) = (g[2b], g[2b + 1]) or
//            (g[b], g[b + Q]), Q = 2^(num_vars - 2): round_units / slot_round_kernel of sumcheck_vpoly.hpp on the folded tables
// Both are exact modular arithmetic on canonical values, so the folded tables and the message are bit-identical to the calls made one
// after the other (a fold per table, then the round of sumcheck_vpoly.hpp in num_vars - 1 variables), whatever the grid or the split.
// Those calls move 2 n elements per table of n; this pass moves 1.5 n, plus 0.5 n for every launch of remaining points (below).
//
// The lane mapping is that of sumcheck.hpp: lane (g, c) owns unit c of the ring element, keeps unit c of r in registers for the whole
// launch and takes the QUADS b = g, g + groups, ...: f[4b .. 4b + 3] in leading order, f[b + i Q] in trailing order.  Slot by slot it
// loads the quad, folds it to the two elements of pair b and stores both; what stays live of a slot is lo and hi of the folded pair,
// exactly the state of the round kernel of sumcheck_vpoly.hpp -- the quads are never live together.  Then it walks the terms with
// term_point / slot_term_point of sumcheck_vpoly.hpp (pick(): no register is selected with a run-time index).  The coefficient stash
// in LDS, the records, the meeting of the lane-groups and the sum over the records are those of sumcheck_vpoly.hpp / sumcheck.hpp; the
// plan is the plan of a sum-of-products round in num_vars - 1 variables with the points split as below.
//
// The flush interval, re-derived with the fold in place.  A lazy sum takes one fma(pr, last) per term and pair.  `last` is a folded
// value advanced by canonical additions; `pr` is a canonical product (mul_boundary / SL::mul) of such values and, possibly, a
// coefficient.  A folded value is a + r (b - a) computed as F::add(a, F::mul_boundary(r, F::sub(b, a))) (SL::mul for the slot rings):
// canonical out of canonical a, b, r, the same image a load of the folded table would give the round kernel.  So both operands of
// every fma() are canonical images below 2^64 (2^31 for BabyBear-72) exactly as in sumcheck_vpoly.hpp, the sums are reduced before a
// pair that would take them past kFlush = 64 accumulated terms (since + n_terms > kFlush), and the bounds carry over word for word:
//   SumOfProducts<Goldilocks>      four 96-bit sums of 32 x 32-bit products: 2^6 (2^32 - 1)^2 < 2^70
//   SlotDot<SlotG24> / <SlotFrog>  at most 2 x 4 partial products per term and sum: 2^6 * 8 * (2^32 - 1)^2 < 2^73
//   SlotDot<SlotB72>               at most 9 products of 31-bit images per term and sum: 2^6 * 9 * 2^62 < 2^72 (redc() wants < 2^29 terms)
//   SumOfProducts<BabyBear> / <Stark>  canonical after every term: no bound
// The fold adds nothing to a lazy sum: its product is reduced at once.
//
// Truncated storage: every table is folded to ITS OWN length -- n_out = (n + 1) / 2 (leading) or min(n, 2^(num_vars-1)) (trailing)
// elements are written, nothing beyond them -- while the product loop ends at the longest term of the FOLDED tables (max over the
// terms of the min over their tables): the fold loop (qmax quads) and the product loop (`count`) have different ends.  An element of
// a quad beyond a table's stored part is zero and is not loaded; a folded element beyond n_out is zero and is not stored.
//
// In place (out table == in table) is sound for the trailing order only, as in sumcheck_fold.hpp: a lane reads the four elements of
// its own unit before it writes two of them, and no other lane touches these words.
//
// Points per fused launch (fused_points_of): as many as leave the kernel without scratch inside the family's register bound -- 256
// registers, BabyBear 128 (tests/test_vpoly_fold_isa.py holds every count; DESIGN_APPENDIX.md A.13).  Over 4 / 8 table slots:
// Goldilocks 5 / 4 (222 / 230 registers; five points over 8 slots: 258), BabyBear 5 / 3 (107 / 128; four over 8 slots: 134), Stark 2 / 1
// (242 / 239), goldilocks24 2 / 1 (216 / 183), babybear72 1 / 0 (212 / 169), frog16 1 / 1 (186 / 235).  babybear72 over 8 slots fuses no
// point: the 17 96-bit sums of the fold's product beside the 17 of a point and lo / hi of eight slots spill, so that launch only folds
// and stores (NP == 0) and every point comes from the round kernels.  The remaining points come from the round kernels of
// sumcheck_vpoly.hpp over the FOLDED tables (n / 2 per table and launch), in chunks of its points_of, into the same records with the
// same t0 / np_total convention.
#pragma once
#include "sumcheck_fold.hpp"
#include "sumcheck_vpoly.hpp"

namespace sr {
namespace vpoly_fold {

using sumcheck::kFlush;
using vpoly::MAX_TABLES;
using vpoly::Tables;
using vpoly::Term;
using vpoly::Terms;

// the folded tables of a call, by value in the kernel arguments.  Pair b of table j holds a stored element exactly when its first
// element does (b * sb < n[j]): the trailing loop never passes the quarter.
struct Folded {
    uint64_t *p[MAX_TABLES];
    size_t n[MAX_TABLES];  // elements written
};

// ---- power-of-two rings -----------------------------------------------------------------------------------------------------------
// NT table slots, points 0 .. np - 1 (np <= NP) of np_total.  sb, st: element strides of a pair of the FOLDED table (2, 1 or 1, Q);
// fst: distance of the two inputs of a fold (1 or 2 Q).  groups, lu, dst: as in sumcheck::round_units.  lds: the coefficient stash
// [term][lane] and, after the loop, the meeting place of the lane-groups, as in vpoly::round_units.
template <class F, int RW, int NT, int NP>
__device__ __forceinline__ void fold_round_units(uint64_t *dst, const Tables &tb, const Folded &fo, const Terms &tm, const uint64_t *coef,
                                                 const uint64_t *rp, size_t count, size_t qmax, size_t sb, size_t st, size_t fst, int lu,
                                                 size_t groups, unsigned np, unsigned np_total, uint64_t *lds) {
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
        if (b >= count) continue;  // beyond the longest folded term: every term has a zero factor at every t
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
#pragma unroll
        for (int n = 0; n < L::NC; n++) {
            E v[NT], dl[NT];
#pragma unroll
            for (int j = 0; j < NT; j++) {
                v[j] = lo[j].get(n);
                dl[j] = F::sub(hi[j].get(n), v[j]);
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
                        vpoly::term_point<F, NT>(total[i][n], acc[i][n], v, vpoly::term_bits(tm, k), has_coef, ck);
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
            r.store(dst + (((g * np_total + i) << lu) + c) * RW);
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
            r.store(dst + (((blockIdx.x * (size_t)np_total + i) << lu) + c) * RW);
        }
    }
}
// pair: every table, folded table, the coefficients, r and dst are 16-byte aligned and k >= 1 (one-limb fields).  Dynamic LDS:
// vpoly::lds_bytes().
template <class F, int NT, int NP>
__global__ __launch_bounds__(256) void fold_round_kernel(uint64_t *dst, Tables tb, Folded fo, Terms tm, const uint64_t *coef, const uint64_t *rp,
                                                         size_t count, size_t qmax, size_t sb, size_t st, size_t fst, int k, int pair, size_t groups,
                                                         unsigned np, unsigned np_total) {
    extern __shared__ __align__(16) uint64_t vpoly_fold_lds[];
    constexpr int RWMAX = sizeof(typename F::storage) == 8 ? 2 : (int)sizeof(typename F::storage) / 8;
    if constexpr (sizeof(typename F::storage) == 8) {
        if (pair) fold_round_units<F, 2, NT, NP>(dst, tb, fo, tm, coef, rp, count, qmax, sb, st, fst, k - 1, groups, np, np_total, vpoly_fold_lds);
        else fold_round_units<F, 1, NT, NP>(dst, tb, fo, tm, coef, rp, count, qmax, sb, st, fst, k, groups, np, np_total, vpoly_fold_lds);
    } else {
        fold_round_units<F, RWMAX, NT, NP>(dst, tb, fo, tm, coef, rp, count, qmax, sb, st, fst, k, groups, np, np_total, vpoly_fold_lds);
    }
}

// ---- goldilocks24 / babybear72 / frog16: lane = slot ---------------------------------------------------------------------------------
// The fold of slot J: v = g[o0], dl = g[o1] - g[o0] of its table, both stored.  J is a template parameter and the slots are a fold
// expression, not a loop: over eight slots of babybear72 the body is past the size to which the compiler unrolls even a loop it is
// told to unroll, and a loop over j indexes v[j] at run time, i.e. in scratch (cdna_hip_programming.md rule 20).
template <class SL, int NT, int J>
__device__ __forceinline__ void slot_fold_slot(typename SL::F::elem (&v)[NT][SL::W], typename SL::F::elem (&dl)[NT][SL::W], const typename SL::K &kc,
                                               const Tables &tb, const Folded &fo, int n_tables, size_t o0, size_t o1, size_t sb, size_t fst, int off,
                                               const typename SL::F::elem *rr) {
    using F = typename SL::F;
    constexpr int W = SL::W;
    if (J < n_tables && o0 < fo.n[J]) {
        sumcheck_fold::slot_fold_one<SL>(v[J], kc, tb.p[J], tb.n[J], o0, sb, fst, off, rr);
        slot_store<SL>(fo.p[J] + o0 * SL::D + off, v[J]);
        if (o1 < fo.n[J]) {
            sumcheck_fold::slot_fold_one<SL>(dl[J], kc, tb.p[J], tb.n[J], o1, sb, fst, off, rr);
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
                                                typename SL::F::elem (&dl)[NT][SL::W], const typename SL::K &kc, const Tables &tb, const Folded &fo,
                                                int n_tables, size_t o0, size_t o1, size_t sb, size_t fst, int off, const typename SL::F::elem *rr) {
    (slot_fold_slot<SL, NT, J>(v, dl, kc, tb, fo, n_tables, o0, o1, sb, fst, off, rr), ...);
}
// A workgroup holds 256 / S lane-groups; they meet in LDS (slot_reduce_store) and the workgroup is record blockIdx.x.  The grid is
// exact, so every lane reaches the barriers.  The coefficients sit in LDS once per workgroup.  Two waves per SIMD is what 256 registers
// allow; said outright, as for slot_fold_round_kernel of sumcheck_fold.hpp.
template <class SL, int NT, int NP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void slot_fold_round_kernel(
    typename SL::K kc, uint64_t *dst, Tables tb, Folded fo, Terms tm, const uint64_t *coef, const uint64_t *rp, size_t count, size_t qmax, size_t sb,
    size_t st, size_t fst, size_t groups, unsigned np, unsigned np_total) {
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
        slot_fold_slots<SL, NT>(std::make_integer_sequence<int, NT>{}, v, dl, kc, tb, fo, n_tables, o0, o1, sb, fst, off, rr);
        if (b >= count) continue;
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
#pragma unroll
        for (int i = 0; i < NP; i++) {
            if ((unsigned)i < np) {
#pragma unroll 1
                for (int k = 0; k < n_terms; k++) {
                    E ck[W];
#pragma unroll
                    for (int m = 0; m < W; m++) ck[m] = has_coef ? cl[k * SL::D + off + m] : F::zero();
                    vpoly::slot_term_point<SL, NT>(kc, total[i], acc[i], v, vpoly::term_bits(tm, k), has_coef, ck);
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
// Points the fused launch takes over `slots` table slots (tests/test_vpoly_fold_isa.py holds the register counts).
template <class T>
constexpr int fused_points_of(int slots) {
    if (std::is_same<T, Goldilocks>::value) return slots == 4 ? 5 : 4;  // five points over 8 slots: 258 registers
    if (std::is_same<T, BabyBear>::value) return slots == 4 ? 5 : 3;    // four: 134, past the 128 of four waves per SIMD
    if (std::is_same<T, SlotB72>::value) return slots == 4 ? 1 : 0;     // the fold's 17 sums beside a point's 17 and 8 slots: spills
    return vpoly::points_of<T>(slots);
}
inline int fused_points(int ring, int slots) {
    switch (ring) {
        case 0: return fused_points_of<Goldilocks>(slots);
        case 1: return fused_points_of<BabyBear>(slots);
        case 2: return fused_points_of<Stark>(slots);
        case 3: return fused_points_of<SlotG24>(slots);
        case 4: return fused_points_of<SlotB72>(slots);
        default: return fused_points_of<SlotFrog>(slots);
    }
}
using Plan = sumcheck::Plan;
// the records of a sum-of-products round in num_vars - 1 variables; the fused launch, the launches of the remaining points, the sum
// over the records
inline bool plan(int ring, int k, size_t num_vars, int n_tables, int degree, int order, Plan *p) {
    if (num_vars < 2 || (order != sumcheck::MODE_LEADING && order != sumcheck::MODE_TRAILING)) return false;
    if (!vpoly::plan(ring, k, num_vars - 1, n_tables, degree, order, p)) return false;
    const int fp = fused_points(ring, vpoly::table_slots(n_tables));
    const int rest = p->np_total > fp ? p->np_total - fp : 0;
    sumcheck::plan_records(ring, k, 1 + (rest + p->np_launch - 1) / p->np_launch, p);
    return true;
}

// ---- launchers: the skeleton is sumcheck::launch_plan -------------------------------------------------------------------------------
struct Shape {
    size_t count, qmax, sb, st, fst;  // quads in the product, quads to fold, strides (see fold_round_units)
};
// fills fo->n (fo->p is the caller's); false when every table is empty
inline bool shape_of(int order, size_t num_vars, const size_t *n_evals, int n_tables, const Term *terms, int n_terms, Folded *fo, Shape *sh) {
    const size_t half = (size_t)1 << (num_vars - 1);
    const bool leading = order == sumcheck::MODE_LEADING;
    size_t qmax = 0;
    for (int j = 0; j < n_tables; j++) {
        const size_t n = n_evals[j];
        fo->n[j] = leading ? (n + 1) / 2 : (n < half ? n : half);
        const size_t q = vpoly::pairs_of(order, num_vars - 1, fo->n[j]);
        qmax = q > qmax ? q : qmax;
    }
    const vpoly::Shape v = vpoly::shape_of(order, num_vars - 1, fo->n, terms, n_terms);  // the round over the folded tables
    *sh = Shape{v.count, qmax, v.sb, v.st, leading ? (size_t)1 : half};
    return qmax != 0;
}
// The fused launch, then the remaining points from the round kernels of sumcheck_vpoly.hpp over the folded tables.  fo.p holds the
// output pointers; n_out receives the elements written per table.  aligned: every table, folded table, the coefficients, r, out and
// work start on a 16-byte boundary.  Every table empty: nothing to visit.
template <class T>
inline hipError_t launch(const typename sumcheck::Family<T>::K &kc, const Plan &p, int order, uint64_t *out, const Tables &tb, Folded fo,
                         const uint64_t *r, int n_tables, const Term *terms, int n_terms, const uint64_t *coef, size_t num_vars, size_t *n_out, int k,
                         bool aligned, uint64_t *work, hipStream_t s) {
    Shape sh;
    const bool any = shape_of(order, num_vars, tb.n, n_tables, terms, n_terms, &fo, &sh);
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
            constexpr int NT = decltype(nt)::value, FP = fused_points_of<T>(NT), NP = vpoly::points_of<T>(NT);
            const unsigned fp = np_total < (unsigned)FP ? np_total : (unsigned)FP;
            if constexpr (sumcheck::kSlot<T>)
                hipLaunchKernelGGL((slot_fold_round_kernel<T, NT, FP>), g, b, lds, s, kc, dst, tb, fo, tm, coef, r, sh.count, sh.qmax, sh.sb, sh.st,
                                   sh.fst, groups, fp, np_total);
            else
                hipLaunchKernelGGL((fold_round_kernel<T, NT, FP>), g, b, lds, s, dst, tb, fo, tm, coef, r, sh.count, sh.qmax, sh.sb, sh.st, sh.fst, ge.k,
                                   ge.pair, groups, fp, np_total);
            if constexpr (FP <= vpoly::MAX_FACTORS) {  // otherwise the fused launch has taken every point of every degree
                for (unsigned t0 = fp; t0 < np_total; t0 += (unsigned)p.np_launch) {
                    const unsigned np = np_total - t0 < (unsigned)p.np_launch ? np_total - t0 : (unsigned)p.np_launch;
                    if constexpr (sumcheck::kSlot<T>)
                        hipLaunchKernelGGL((vpoly::slot_round_kernel<T, NT, NP, true>), g, b, lds, s, kc, dst, ftb, tm, coef, sh.count, sh.sb, sh.st,
                                           groups, t0, np, np_total);
                    else
                        hipLaunchKernelGGL((vpoly::round_kernel<T, NT, NP, true>), g, b, lds, s, dst, ftb, tm, coef, sh.count, sh.sb, sh.st, ge.k,
                                           ge.pair, groups, t0, np, np_total);
                }
            }
        });
    });
}

}  // namespace vpoly_fold
}  // namespace sr
