// A sum-check round in one pass over the tables: fold every table at the challenge r of the round that has just ended and, while the
// two folded neighbours are still in registers, accumulate the message of the round that follows.
//   fold     g_j = f_j with one variable fixed at r: g[o] = f[2o] + r (f[2o + 1] - f[2o]) in leading order, f[o] + r (f[o + half] - f[o])
//            in trailing order -- fold_kernel<F, 1> / slot_fold_kernel<SL, 1> of mle.hpp, element for element
//   message  p(t) = sum_b prod_j ( lo_j[b] + t (hi_j[b] - lo_j[b]) ), t = 0 .. d, over the pairs (lo, hi) = (g[2b], g[2b + 1]) or
//            (g[b], g[b + Q]), Q = 2^(num_vars - 2): round_units / slot_round_kernel of sumcheck.hpp on g_0 .. g_{d-1}
// Both are exact modular arithmetic on canonical values, so the folded tables and the message are bit-identical to the two calls made
// one after the other, whatever the grid or the split.  The two calls move 2 n elements per table of n (the fold reads n and writes n / 2,
// the message reads the n / 2 again); this pass moves 1.5 n.
//
// The lane mapping is that of sumcheck.hpp: lane (g, c) owns unit c of the ring element, keeps unit c of r in registers for the whole
// launch and takes the QUADS b = g, g + groups, ...: f[4b .. 4b + 3] in leading order, f[b], f[b + Q], f[b + 2Q], f[b + 3Q] in trailing
// order.  Table by table it loads the quad, folds it to the two elements of pair b, stores both; then it multiplies as round_units does.
// The records, the lazy sums (kFlush) and the last launch (sum_groups_kernel) are those of sumcheck.hpp; the plan is the plan of a round
// in num_vars - 1 variables.  The launch skeleton (geometry, destination, sum over the records) is sumcheck::launch_plan; this file adds
// the shape of a fold, the fused launch and the remaining points.
//
// Truncated storage: every table is folded to ITS OWN length -- n_out = (n + 1) / 2 (leading) or min(n, 2^(num_vars-1)) (trailing)
// elements are written, nothing beyond them -- while the product stops at the shortest folded table: the fold loop and the product loop
// have different ends (q[j] quads of table j, `count` = min_j q[j] of them in the product).  An element of a quad beyond a table's stored
// part is zero and is not loaded; a folded element beyond n_out is zero and is not stored.
//
// In place (out table == in table) is sound for the trailing order only: a lane reads f[b], f[b + Q], f[b + 2Q], f[b + 3Q] of its own
// unit before it writes g[b] and g[b + Q] there, and no other lane touches these words.
//
// Points per fused launch (fused_points_of), under the budget of sumcheck.hpp: nothing spills, at most 256 registers, BabyBear at most
// 128.  Goldilocks (58 / 154 / 190 / 226 registers for d = 1 .. 4; d = 4 was 206 without the fold) and BabyBear (54 / 80 / 94 / 108) take
// all d + 1 points in the fused launch for every d <= 4.  The fold's products are live next to the lazy sums, so the other families
// take fewer points in the fused launch than their round kernel takes per launch -- Stark 2, 3, 3, 2, goldilocks24 2, 3, 2, 2,
// babybear72 2, 2, 1, 1, frog16 2, 1, 1, 1 -- and the remaining ones come from the existing round_kernel / slot_round_kernel over the
// FOLDED tables (n / 2 per table, not n), in chunks of points_of, into the same records with the same t0 / np_total convention
// (tests/test_sumcheck_fold_isa.py holds every count; DESIGN_APPENDIX.md A.10).
#pragma once
#include "sumcheck.hpp"

namespace sr {
namespace sumcheck_fold {

using sumcheck::kFlush;
using sumcheck::MAX_TABLES;
using sumcheck::Tables;

// the folded tables of a call, by value in the kernel arguments
struct Folded {
    uint64_t *p[MAX_TABLES];
    size_t n[MAX_TABLES];  // elements written
    size_t q[MAX_TABLES];  // quads of the input table that hold a stored element = pairs of the folded table that do
};

// ---- power-of-two rings -----------------------------------------------------------------------------------------------------------
// g[o] of table j for the lane's unit: in elements o * sb and o * sb + fst (the second one zero beyond the stored part)
template <class F, int RW>
__device__ __forceinline__ void load_pair(mle::Lane<F, RW> &a, mle::Lane<F, RW> &b, const uint64_t *p, size_t n, size_t o, size_t sb, size_t fst,
                                          int lu, size_t c) {
    const size_t e0 = o * sb, e1 = e0 + fst;
    a.template load<true>(p + ((e0 << lu) + c) * RW);
    if (e1 < n) b.template load<true>(p + ((e1 << lu) + c) * RW);
    else b.zero();
}
template <class F, int RW>
__device__ __forceinline__ void fold_pair(mle::Lane<F, RW> &a, const mle::Lane<F, RW> &b, const mle::Lane<F, RW> &r) {
#pragma unroll
    for (int n = 0; n < mle::Lane<F, RW>::NC; n++) a.put(n, F::add(a.get(n), F::mul_boundary(r.get(n), F::sub(b.get(n), a.get(n)))));
}
// NT tables, points 0 .. NP - 1 of np_total.  sb, st: element strides of a pair of the FOLDED table (2, 1 or 1, Q); fst: distance of the
// two inputs of a fold (1 or 2 Q).  groups, lu, lds, dst: as in sumcheck::round_units.
template <class F, int RW, int NT, int NP>
__device__ __forceinline__ void fold_round_units(uint64_t *dst, const Tables &tb, const Folded &fo, const uint64_t *rp, size_t count, size_t qmax,
                                                 size_t sb, size_t st, size_t fst, int lu, size_t groups, unsigned np_total, uint64_t *lds) {
    using E = typename F::elem;
    using L = mle::Lane<F, RW>;
    const size_t flat = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t g = flat >> lu, c = flat & (((size_t)1 << lu) - 1);
    const bool in_block = lu < 8;  // uniform; the grid of such a launch is exact, so every lane reaches the barriers below
    if (!in_block && g >= groups) return;
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
            if (b < fo.q[j]) {  // o0 < fo.n[j]: its first input is stored
                L x0, x1;
                load_pair<F, RW>(lo[j], x0, tb.p[j], tb.n[j], o0, sb, fst, lu, c);
                const bool second = o1 < fo.n[j];
                if (second) load_pair<F, RW>(hi[j], x1, tb.p[j], tb.n[j], o1, sb, fst, lu, c);
                fold_pair<F, RW>(lo[j], x0, rr);
                lo[j].store(fo.p[j] + ((o0 << lu) + c) * RW);
                if (second) {
                    fold_pair<F, RW>(hi[j], x1, rr);
                    hi[j].store(fo.p[j] + ((o1 << lu) + c) * RW);
                } else {
                    hi[j].zero();
                }
            } else {
                lo[j].zero();
                hi[j].zero();
            }
        }
        if (b >= count) continue;  // beyond the shortest folded table: a zero factor at every t
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
                if constexpr (NT == 1) {
                    total[i][n] = F::add(total[i][n], v[0]);
                } else {
                    E pr = v[0];
#pragma unroll
                    for (int j = 1; j < NT - 1; j++) pr = F::mul_boundary(pr, v[j]);
                    acc[i][n].fma(pr, v[NT - 1]);
                }
                if (i + 1 < NP) {
#pragma unroll
                    for (int j = 0; j < NT; j++) v[j] = F::add(v[j], dl[j]);
                }
            }
        }
        if constexpr (NT > 1) {
            if (++since == kFlush) {
                since = 0;
#pragma unroll
                for (int i = 0; i < NP; i++)
#pragma unroll
                    for (int n = 0; n < L::NC; n++) {
                        total[i][n] = F::add(total[i][n], acc[i][n].finish());
                        acc[i][n].init();
                    }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NP; i++) {
        L r;
#pragma unroll
        for (int n = 0; n < L::NC; n++) {
            if constexpr (NT > 1) total[i][n] = F::add(total[i][n], acc[i][n].finish());
            r.put(n, total[i][n]);
        }
        if (!in_block) {
            r.store(dst + (((g * np_total + i) << lu) + c) * RW);
            continue;
        }
        const unsigned t = threadIdx.x, units = 1u << lu;
        __syncthreads();  // the previous point's sums have been read
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
// pair: every table, folded table, r and dst are 16-byte aligned and k >= 1 (one-limb fields)
template <class F, int NT, int NP>
__global__ __launch_bounds__(256) void fold_round_kernel(uint64_t *dst, Tables tb, Folded fo, const uint64_t *rp, size_t count, size_t qmax, size_t sb,
                                                         size_t st, size_t fst, int k, int pair, size_t groups, unsigned np_total) {
    constexpr int RWMAX = sizeof(typename F::storage) == 8 ? 2 : (int)sizeof(typename F::storage) / 8;
    __shared__ uint64_t lds[256 * RWMAX];
    if constexpr (sizeof(typename F::storage) == 8) {
        if (pair) fold_round_units<F, 2, NT, NP>(dst, tb, fo, rp, count, qmax, sb, st, fst, k - 1, groups, np_total, lds);
        else fold_round_units<F, 1, NT, NP>(dst, tb, fo, rp, count, qmax, sb, st, fst, k, groups, np_total, lds);
    } else {
        fold_round_units<F, RWMAX, NT, NP>(dst, tb, fo, rp, count, qmax, sb, st, fst, k, groups, np_total, lds);
    }
}

// ---- goldilocks24 / babybear72 / frog16: lane = slot ---------------------------------------------------------------------------------
// g[o] of table j for the lane's slot
template <class SL>
__device__ __forceinline__ void slot_fold_one(typename SL::F::elem *out, const typename SL::K &k, const uint64_t *p, size_t n, size_t o, size_t sb,
                                              size_t fst, int off, const typename SL::F::elem *r) {
    using F = typename SL::F;
    constexpr int W = SL::W;
    const size_t e0 = o * sb, e1 = e0 + fst;
    typename F::elem d[W];
    slot_load<SL>(out, p + e0 * SL::D + off);
    if (e1 < n) {
        slot_load<SL>(d, p + e1 * SL::D + off);
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
// Two waves per SIMD is what 256 registers allow; said outright, because left to its occupancy heuristic the compiler holds babybear72
// d = 4 to 132 registers and spills.
template <class SL, int NT, int NP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void slot_fold_round_kernel(typename SL::K k, uint64_t *dst, Tables tb, Folded fo, const uint64_t *rp, size_t count,
                                                              size_t qmax, size_t sb, size_t st, size_t fst, size_t groups, unsigned np_total) {
    using F = typename SL::F;
    using E = typename F::elem;
    constexpr int W = SL::W, S = SL::D / SL::W;
    const size_t flat = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t g = flat / S;
    const int off = (int)(flat % S) * W;
    __shared__ E lds[256 * W];
    E total[NP][W], rr[W];
    SlotDot<SL> acc[NP];
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
#pragma unroll
        for (int j = 0; j < NT; j++) {
            if (b < fo.q[j]) {
                slot_fold_one<SL>(v[j], k, tb.p[j], tb.n[j], o0, sb, fst, off, rr);
                slot_store<SL>(fo.p[j] + o0 * SL::D + off, v[j]);
                if (o1 < fo.n[j]) {
                    slot_fold_one<SL>(dl[j], k, tb.p[j], tb.n[j], o1, sb, fst, off, rr);
                    slot_store<SL>(fo.p[j] + o1 * SL::D + off, dl[j]);
#pragma unroll
                    for (int m = 0; m < W; m++) dl[j][m] = F::sub(dl[j][m], v[j][m]);
                } else {
#pragma unroll
                    for (int m = 0; m < W; m++) dl[j][m] = F::sub(F::zero(), v[j][m]);
                }
            } else {
#pragma unroll
                for (int m = 0; m < W; m++) v[j][m] = dl[j][m] = F::zero();
            }
        }
        if (b >= count) continue;
#pragma unroll
        for (int i = 0; i < NP; i++) {
            if constexpr (NT == 1) {
#pragma unroll
                for (int m = 0; m < W; m++) total[i][m] = F::add(total[i][m], v[0][m]);
            } else {
                E pr[W];
#pragma unroll
                for (int m = 0; m < W; m++) pr[m] = v[0][m];
#pragma unroll
                for (int j = 1; j < NT - 1; j++) SL::mul(pr, v[j], k);
                acc[i].fma(pr, v[NT - 1]);
            }
            if (i + 1 < NP) {
#pragma unroll
                for (int j = 0; j < NT; j++)
#pragma unroll
                    for (int m = 0; m < W; m++) v[j][m] = F::add(v[j][m], dl[j][m]);
            }
        }
        if constexpr (NT > 1) {
            if (++since == kFlush) {
                since = 0;
#pragma unroll
                for (int i = 0; i < NP; i++) {
                    E r[W];
                    acc[i].finish(r, k);
                    acc[i].init();
#pragma unroll
                    for (int m = 0; m < W; m++) total[i][m] = F::add(total[i][m], r[m]);
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NP; i++) {
        if constexpr (NT > 1) {
            E r[W];
            acc[i].finish(r, k);
#pragma unroll
            for (int m = 0; m < W; m++) total[i][m] = F::add(total[i][m], r[m]);
        }
        if (i) __syncthreads();  // the previous point's sums have been read
        slot_reduce_store<SL>(lds, total[i], dst + (blockIdx.x * (size_t)np_total + i) * SL::D);
    }
}

// ---- the plan: pure host arithmetic -------------------------------------------------------------------------------------------------
// Points the fused launch takes (tests/test_sumcheck_fold_isa.py holds the register counts).
template <class T>
constexpr int fused_points_of(int n_tables) {
    if (std::is_same<T, Stark>::value) return n_tables == 3 ? 3 : sumcheck::points_of<T>(n_tables);
    if (std::is_same<T, SlotG24>::value) return n_tables == 4 ? 2 : sumcheck::points_of<T>(n_tables);
    if (std::is_same<T, SlotB72>::value) return n_tables >= 3 ? 1 : 2;
    if (std::is_same<T, SlotFrog>::value) return n_tables >= 2 ? 1 : 2;
    return n_tables + 1;
}
inline int fused_points(int ring, int n_tables) {
    switch (ring) {
        case 0: return fused_points_of<Goldilocks>(n_tables);
        case 1: return fused_points_of<BabyBear>(n_tables);
        case 2: return fused_points_of<Stark>(n_tables);
        case 3: return fused_points_of<SlotG24>(n_tables);
        case 4: return fused_points_of<SlotB72>(n_tables);
        default: return fused_points_of<SlotFrog>(n_tables);
    }
}
using Plan = sumcheck::Plan;
// the records of a round in num_vars - 1 variables; the fused launch, the launches of the remaining points, the sum over the records
inline bool plan(int ring, int k, size_t num_vars, int n_tables, int order, Plan *p) {
    if (num_vars < 2 || (order != sumcheck::MODE_LEADING && order != sumcheck::MODE_TRAILING)) return false;
    if (!sumcheck::plan(ring, k, num_vars - 1, n_tables, order, p)) return false;
    const int rest = p->np_total - fused_points(ring, n_tables);
    sumcheck::plan_records(ring, k, 1 + (rest + p->np_launch - 1) / p->np_launch, p);
    return true;
}

// ---- launchers: the skeleton is sumcheck::launch_plan -------------------------------------------------------------------------------
struct Shape {
    size_t count, qmax, sb, st, fst;  // quads in the product, quads to fold, strides (see fold_round_units)
};
// fills fo->n, fo->q (fo->p is the caller's) and n_out; false when every table is empty
inline bool shape_of(int order, size_t num_vars, const size_t *n_evals, int n_tables, Folded *fo, Shape *sh) {
    const size_t half = (size_t)1 << (num_vars - 1), quarter = half >> 1;
    const bool leading = order == sumcheck::MODE_LEADING;
    *sh = leading ? Shape{~(size_t)0, 0, 2, 1, 1} : Shape{~(size_t)0, 0, 1, quarter, half};
    for (int j = 0; j < n_tables; j++) {
        const size_t n = n_evals[j];
        fo->n[j] = leading ? (n + 1) / 2 : (n < half ? n : half);
        fo->q[j] = leading ? (fo->n[j] + 1) / 2 : (fo->n[j] < quarter ? fo->n[j] : quarter);
        if (fo->q[j] < sh->count) sh->count = fo->q[j];
        if (fo->q[j] > sh->qmax) sh->qmax = fo->q[j];
    }
    return sh->qmax != 0;
}
// the points t0 .. of the remaining launches, from the round kernels of sumcheck.hpp over the folded tables: chunks of points_of, then
// the rest
template <class T, int NT>
inline void launch_rest(const typename sumcheck::Family<T>::K &kc, const sumcheck::Geometry &ge, size_t records, uint64_t *dst, const Tables &ftb,
                        const sumcheck::Shape &sh, unsigned np_total, hipStream_t s) {
    constexpr int FP = fused_points_of<T>(NT), P = sumcheck::points_of<T>(NT), REST = NT + 1 - FP, R = REST % P;
    if constexpr (REST > 0) {
        unsigned t0 = FP;
        if constexpr (REST >= P)
            for (int i = 0; i < REST / P; i++, t0 += P) sumcheck::launch_round<T, NT, P, true>(kc, ge, records, dst, ftb, sh, t0, np_total, s);
        if constexpr (R != 0) sumcheck::launch_round<T, NT, R, true>(kc, ge, records, dst, ftb, sh, t0, np_total, s);
    }
}
inline Tables folded_as_tables(const Folded &fo, int n_tables) {
    Tables t{};
    for (int j = 0; j < n_tables; j++) {
        t.p[j] = fo.p[j];
        t.n[j] = fo.n[j];
    }
    return t;
}
// The fused launch, then the remaining points.  fo.p holds the output pointers; n_out receives the elements written per table.
// aligned: every table, folded table, r, out and work start on a 16-byte boundary.  Every table empty: nothing to visit.
template <class T>
inline hipError_t launch(const typename sumcheck::Family<T>::K &kc, const Plan &p, int order, uint64_t *out, const Tables &tb, Folded fo,
                         const uint64_t *r, int n_tables, size_t num_vars, size_t *n_out, int k, bool aligned, uint64_t *work, hipStream_t s) {
    Shape sh;
    const bool any = shape_of(order, num_vars, tb.n, n_tables, &fo, &sh);
    for (int j = 0; j < n_tables; j++) n_out[j] = fo.n[j];
    const sumcheck::Geometry ge = sumcheck::geometry_of<T>(k, aligned);
    return sumcheck::launch_plan<T>(p, ge, !any, out, work, s, [&](uint64_t *dst) {
        const dim3 g = ge.grid(p.groups), b(256);
        const size_t groups = ge.groups(p.groups);
        const Tables ftb = folded_as_tables(fo, n_tables);
        sumcheck::with_tables(n_tables, [&](auto nt) {
            constexpr int NT = decltype(nt)::value, FP = fused_points_of<T>(NT);
            if constexpr (sumcheck::kSlot<T>)
                hipLaunchKernelGGL((slot_fold_round_kernel<T, NT, FP>), g, b, 0, s, kc, dst, tb, fo, r, sh.count, sh.qmax, sh.sb, sh.st, sh.fst, groups,
                                   (unsigned)p.np_total);
            else
                hipLaunchKernelGGL((fold_round_kernel<T, NT, FP>), g, b, 0, s, dst, tb, fo, r, sh.count, sh.qmax, sh.sb, sh.st, sh.fst, ge.k, ge.pair,
                                   groups, (unsigned)p.np_total);
            launch_rest<T, NT>(kc, ge, p.groups, dst, ftb, {sh.count, sh.sb, sh.st}, (unsigned)p.np_total, s);
        });
    });
}

}  // namespace sumcheck_fold
}  // namespace sr
