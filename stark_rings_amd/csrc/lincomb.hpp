// Linear combinations of tables of ring elements in CRT / NTT form with ring-element coefficients, several outputs from one pass:
//   out_m[e] = [bit K of uses_m] c_m[K]  +  sum_{k < K, bit k of uses_m} c_m[k] * T_k[e]        e < n, m < M, K <= 16, M <= 4
// the composition of three operators of crates/poly's DenseMultilinearExtension --
//   AddAssign<(R, &Self)>   mle/dense.rs:288-317   acc[e] += r x[e]        (sr_mul_elem_add_batch is this one alone)
//   MulAssign<R>            mle/dense.rs:370-374   self[e] *= r
//   Add<R>                  mle/dense.rs:386-395   self[e] + r
// -- in one pass: the leaves of a permutation or logUp argument (beta + f + gamma sigma, beta - sum_k gamma^k col_k), the fold
// sum_i rho_i f_i of many instances into one, the batching of many MLEs into one.  `*` is the slot product of the ring as in mle.hpp,
// `+` the slot sum.  The constant goes to every one of the n elements (the reference's Add<R> touches the stored evaluations only).
//
// Traffic in ring elements: (K + M) n for M outputs over K tables, against M (3 K + 3) n for the composition copy, *= c_0,
// += (c_k, T_k) ..., + const from the calls the library had; one reduction per output coefficient instead of K, because the lazy
// accumulators of the sum-check kernels (SumOfProducts, SlotDot) take 64 terms between reductions and a row has at most 17
// (sumcheck.hpp: the bounds at kFlush carry over unchanged).  The constant is added after finish().
//
// Mapping (sumcheck::round_units): lane (g, c) owns unit c of the ring element -- mle::Lane: a 16-byte pair of coefficients of a
// one-limb field where every buffer is aligned, one coefficient otherwise, one Stark coefficient; one Fq3 / Fq9 / Fq4 slot of the
// reference's own rings -- and walks the elements g, g + groups, ...  The M K coefficient units a lane needs do not change along its
// walk.  Two kernels per family:
//   REG   K <= kRegTables, M <= reg_outputs: the coefficient units are loaded once, before the walk, and stay in registers;
//   !REG  any K: a coefficient unit is read next to the table unit it multiplies, with the default cache policy (it is re-read by
//         every lane-group and should stay in L2); tables go four at a time, their loads issued before the products.
// Tables and outputs are non-temporal: each is touched once.  Outputs per launch and the bound of REG are per family the largest
// whose kernel has no scratch within 128 VGPRs (tools/ubench/lincomb_isa.hip, tests/test_lincomb_isa.py hold the counts); more
// outputs go in several launches, each of which reads the tables its outputs use once more.
//
// Truncated storage: elements of table k at or beyond n_evals[k] are zero and are never loaded.  A table no output of the launch
// uses is never loaded; a coefficient whose mask bit is clear is never read.
//
// In place (one output, out == a table): lane (g, c) reads unit c of T_k[e] and later writes unit c of out[e], and no other lane
// touches that unit.  With several launches a later one would read what an earlier one wrote: the entry points refuse it.
#pragma once
#include "mle.hpp"
#include "sumcheck.hpp"

namespace sr {
namespace lincomb {

enum { MAX_TABLES = 16, MAX_OUTPUTS = 4 };
constexpr int kRegTables = 4;

// the operands of a launch, by value in the kernel arguments: a captured graph holds no host pointer
struct Args {
    const uint64_t *t[MAX_TABLES];
    size_t ne[MAX_TABLES];  // stored elements
    uint64_t *out[MAX_OUTPUTS];
    uint32_t uses[MAX_OUTPUTS];
    const uint64_t *coef;  // row m of the launch: K + 1 elements at element m (K + 1)
};

// The invariant-checking build (-DSR_GL_CHECK_REPS, fields.hpp: repcheck) counts every word >= p that leaves the call; the sums
// themselves are counted where the sum-check kernels' are, inside F::add (canonical_in) on what finish() returns.  The product
// library compiles this to nothing.
template <class F>
__device__ __forceinline__ void leaves(const typename F::elem &v) {
    if constexpr (std::is_same<F, Goldilocks>::value) repcheck::leaves_library(v);
}

// ---- power-of-two rings -----------------------------------------------------------------------------------------------------------
template <class F, int RW, int M, bool REG>
__device__ __forceinline__ void lincomb_units(const Args &a, int K, size_t n, int lu, size_t groups) {
    using E = typename F::elem;
    using L = mle::Lane<F, RW>;
    const size_t flat = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t g = flat >> lu, c = flat & (((size_t)1 << lu) - 1);
    if (g >= groups) return;
    const size_t ew = (size_t)RW << lu, cu = c * RW;  // words of an element, word of this lane's unit
    uint32_t any = 0;
#pragma unroll
    for (int m = 0; m < M; m++) any |= a.uses[m];
    L cst[M];
#pragma unroll
    for (int m = 0; m < M; m++) {
        if ((a.uses[m] >> K) & 1u) cst[m].template load<false>(a.coef + ((size_t)m * (K + 1) + K) * ew + cu);
        else cst[m].zero();
    }
    if constexpr (REG) {
        L cf[M][kRegTables];
#pragma unroll
        for (int m = 0; m < M; m++)
#pragma unroll
            for (int k = 0; k < kRegTables; k++) {
                if (k < K && ((a.uses[m] >> k) & 1u)) cf[m][k].template load<false>(a.coef + ((size_t)m * (K + 1) + k) * ew + cu);
                else cf[m][k].zero();
            }
        for (size_t e = g; e < n; e += groups) {
            L t[kRegTables];
#pragma unroll
            for (int k = 0; k < kRegTables; k++) {
                if (k < K && ((any >> k) & 1u) && e < a.ne[k]) t[k].template load<true>(a.t[k] + e * ew + cu);
                else t[k].zero();
            }
#pragma unroll
            for (int m = 0; m < M; m++) {
                L o;
#pragma unroll
                for (int q = 0; q < L::NC; q++) {
                    SumOfProducts<F> acc;
                    acc.init();
#pragma unroll
                    for (int k = 0; k < kRegTables; k++)
                        if (k < K && ((a.uses[m] >> k) & 1u)) acc.fma(cf[m][k].get(q), t[k].get(q));
                    const E r = F::add(acc.finish(), cst[m].get(q));
                    leaves<F>(r);
                    o.put(q, r);
                }
                o.store(a.out[m] + e * ew + cu);
            }
        }
    } else {
        for (size_t e = g; e < n; e += groups) {
            SumOfProducts<F> acc[M][L::NC];
#pragma unroll
            for (int m = 0; m < M; m++)
#pragma unroll
                for (int q = 0; q < L::NC; q++) acc[m][q].init();
            for (int k0 = 0; k0 < K; k0 += 4) {
                L t[4];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int k = k0 + j;
                    if (k < K && ((any >> k) & 1u) && e < a.ne[k]) t[j].template load<true>(a.t[k] + e * ew + cu);
                    else t[j].zero();
                }
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int k = k0 + j;
                    if (k >= K) break;
#pragma unroll
                    for (int m = 0; m < M; m++) {
                        if (!((a.uses[m] >> k) & 1u)) continue;
                        L cf;
                        cf.template load<false>(a.coef + ((size_t)m * (K + 1) + k) * ew + cu);
#pragma unroll
                        for (int q = 0; q < L::NC; q++) acc[m][q].fma(cf.get(q), t[j].get(q));
                    }
                }
            }
#pragma unroll
            for (int m = 0; m < M; m++) {
                L o;
#pragma unroll
                for (int q = 0; q < L::NC; q++) {
                    const E r = F::add(acc[m][q].finish(), cst[m].get(q));
                    leaves<F>(r);
                    o.put(q, r);
                }
                o.store(a.out[m] + e * ew + cu);
            }
        }
    }
}
// pair: every buffer of the launch is 16-byte aligned and k >= 1 (one-limb fields)
template <class F, int M, bool REG>
__global__ __launch_bounds__(256) void lincomb_kernel(Args a, int K, size_t n, int k, int pair, size_t groups) {
    if constexpr (sizeof(typename F::storage) == 8) {
        if (pair) lincomb_units<F, 2, M, REG>(a, K, n, k - 1, groups);
        else lincomb_units<F, 1, M, REG>(a, K, n, k, groups);
    } else {
        lincomb_units<F, (int)sizeof(typename F::storage) / 8, M, REG>(a, K, n, k, groups);
    }
}

// ---- goldilocks24 / babybear72 / frog16: lane = slot (slot_fold_kernel's mapping), walking like the lanes above ----------------
template <class SL, int M, bool REG>
__global__ __launch_bounds__(256) void slot_lincomb_kernel(typename SL::K kc, Args a, int K, size_t n, size_t groups) {
    using F = typename SL::F;
    using E = typename F::elem;
    constexpr int W = SL::W, S = SL::D / SL::W;
    const size_t flat = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t g = flat / S;
    const int off = (int)(flat % S) * W;
    if (g >= groups) return;
    uint32_t any = 0;
#pragma unroll
    for (int m = 0; m < M; m++) any |= a.uses[m];
    E cst[M][W];
#pragma unroll
    for (int m = 0; m < M; m++) {
        if ((a.uses[m] >> K) & 1u) {
            slot_load<SL>(cst[m], a.coef + ((size_t)m * (K + 1) + K) * SL::D + off);
        } else {
#pragma unroll
            for (int w = 0; w < W; w++) cst[m][w] = F::zero();
        }
    }
    if constexpr (REG) {
        E cf[M][kRegTables][W];
#pragma unroll
        for (int m = 0; m < M; m++)
#pragma unroll
            for (int k = 0; k < kRegTables; k++) {
                if (k < K && ((a.uses[m] >> k) & 1u)) {
                    slot_load<SL>(cf[m][k], a.coef + ((size_t)m * (K + 1) + k) * SL::D + off);
                } else {
#pragma unroll
                    for (int w = 0; w < W; w++) cf[m][k][w] = F::zero();
                }
            }
        for (size_t e = g; e < n; e += groups) {
            E t[kRegTables][W];
#pragma unroll
            for (int k = 0; k < kRegTables; k++) {
                if (k < K && ((any >> k) & 1u) && e < a.ne[k]) {
#pragma unroll
                    for (int w = 0; w < W; w++) t[k][w] = F::load(a.t[k] + e * SL::D + off + w);
                } else {
#pragma unroll
                    for (int w = 0; w < W; w++) t[k][w] = F::zero();
                }
            }
#pragma unroll
            for (int m = 0; m < M; m++) {
                SlotDot<SL> acc;
                acc.init();
#pragma unroll
                for (int k = 0; k < kRegTables; k++)
                    if (k < K && ((a.uses[m] >> k) & 1u)) acc.fma(cf[m][k], t[k]);
                E r[W];
                acc.finish(r, kc);
#pragma unroll
                for (int w = 0; w < W; w++) {
                    r[w] = F::add(r[w], cst[m][w]);
                    leaves<F>(r[w]);
                }
                slot_store<SL>(a.out[m] + e * SL::D + off, r);
            }
        }
    } else {
        for (size_t e = g; e < n; e += groups) {
            SlotDot<SL> acc[M];
#pragma unroll
            for (int m = 0; m < M; m++) acc[m].init();
            for (int k = 0; k < K; k++) {
                if (!((any >> k) & 1u)) continue;
                E t[W];
                if (e < a.ne[k]) {
                    slot_load<SL>(t, a.t[k] + e * SL::D + off);
                } else {
#pragma unroll
                    for (int w = 0; w < W; w++) t[w] = F::zero();
                }
#pragma unroll
                for (int m = 0; m < M; m++) {
                    if (!((a.uses[m] >> k) & 1u)) continue;
                    E cf[W];
                    slot_load<SL>(cf, a.coef + ((size_t)m * (K + 1) + k) * SL::D + off);
                    acc[m].fma(cf, t);
                }
            }
#pragma unroll
            for (int m = 0; m < M; m++) {
                E r[W];
                acc[m].finish(r, kc);
#pragma unroll
                for (int w = 0; w < W; w++) {
                    r[w] = F::add(r[w], cst[m][w]);
                    leaves<F>(r[w]);
                }
                slot_store<SL>(a.out[m] + e * SL::D + off, r);
            }
        }
    }
}

// ---- the plan: pure host arithmetic -------------------------------------------------------------------------------------------------
// Outputs of one launch at most, per family type T (a field or a slot type): REG with K <= kRegTables, and the run-time-K kernel.  Zero:
// the family has no REG kernel within the budget.  tests/test_lincomb_isa.py holds the register counts behind every entry.
//   REG, M = 1 / 2:      Goldilocks 68 / 126, BabyBear 44 / 80, Stark 124 / 188, goldilocks24 115 / 150, babybear72 194 / -, frog16 150 / -
//   !REG, M = 1 .. 4:     Goldilocks 70 / 106 / 128 / 166, BabyBear 40 / 52 / 62 / 72, Stark 128 / 152 / - / -,
//                         goldilocks24 76 / 130 / - / -, babybear72 104 / 168 / - / -, frog16 106 / 188 / - / -
template <class T>
constexpr int kRegOutputs = std::is_same<T, Goldilocks>::value || std::is_same<T, BabyBear>::value ? 2
                            : std::is_same<T, Stark>::value || std::is_same<T, SlotG24>::value     ? 1
                                                                                                    : 0;
template <class T> constexpr int kRunOutputs = std::is_same<T, BabyBear>::value ? 4 : std::is_same<T, Goldilocks>::value ? 3 : 1;

template <class T>
constexpr bool use_reg(int n_tables, int n_outputs) {
    return n_tables <= kRegTables && n_outputs <= kRegOutputs<T>;
}
template <class T>
constexpr int outputs_of(int n_tables, int n_outputs) {
    return use_reg<T>(n_tables, n_outputs) ? n_outputs : (n_outputs < kRunOutputs<T> ? n_outputs : kRunOutputs<T>);
}
inline int outputs_per_launch(int ring, int n_tables, int n_outputs) {
    switch (ring) {
        case 0: return outputs_of<Goldilocks>(n_tables, n_outputs);
        case 1: return outputs_of<BabyBear>(n_tables, n_outputs);
        case 2: return outputs_of<Stark>(n_tables, n_outputs);
        case 3: return outputs_of<SlotG24>(n_tables, n_outputs);
        case 4: return outputs_of<SlotB72>(n_tables, n_outputs);
        default: return outputs_of<SlotFrog>(n_tables, n_outputs);
    }
}
struct Plan {
    int launches = 0, outputs_per_launch = 0;
};
inline bool plan(int ring, int n_tables, int n_outputs, Plan *p) {
    if (ring < 0 || ring > 5 || n_tables < 1 || n_tables > MAX_TABLES || n_outputs < 1 || n_outputs > MAX_OUTPUTS) return false;
    p->outputs_per_launch = outputs_per_launch(ring, n_tables, n_outputs);
    p->launches = (n_outputs + p->outputs_per_launch - 1) / p->outputs_per_launch;
    return true;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
// Lane-groups of a launch over n elements of 2^lu (or `units`) units: one element per lane-group while that does not exceed the fill
// target of the sum-check plans (sumcheck::kFillLanes), the walk beyond
inline size_t groups_for(size_t n, size_t units) {
    size_t cap = sumcheck::kFillLanes / units;
    if (cap < 1) cap = 1;
    return n < cap ? n : cap;
}
template <class T, int M>
inline void launch_m(const typename sumcheck::Family<T>::K &kc, bool reg, const Args &a, int K, size_t n, int k, bool aligned, hipStream_t s) {
    if constexpr (sumcheck::kSlot<T>) {
        constexpr size_t S = T::D / T::W;
        const size_t groups = groups_for(n, S);
        const dim3 g(mle::blocks_for(groups * S)), b(256);
        if constexpr (M <= kRegOutputs<T>) {
            if (reg) {
                hipLaunchKernelGGL((slot_lincomb_kernel<T, M, true>), g, b, 0, s, kc, a, K, n, groups);
                return;
            }
        }
        hipLaunchKernelGGL((slot_lincomb_kernel<T, M, false>), g, b, 0, s, kc, a, K, n, groups);
    } else {
        const sumcheck::Geometry ge = sumcheck::geometry_of<T>(k, aligned);
        const size_t groups = groups_for(n, (size_t)1 << ge.lu);
        const dim3 g(mle::blocks_for(groups << ge.lu)), b(256);
        if constexpr (M <= kRegOutputs<T>) {
            if (reg) {
                hipLaunchKernelGGL((lincomb_kernel<T, M, true>), g, b, 0, s, a, K, n, ge.k, ge.pair, groups);
                return;
            }
        }
        hipLaunchKernelGGL((lincomb_kernel<T, M, false>), g, b, 0, s, a, K, n, ge.k, ge.pair, groups);
    }
}
// One launch: the `m` outputs of `a` (m <= outputs_of<T>) over K tables.  reg: the call as a whole takes the REG kernel.
template <class T>
inline hipError_t launch(const typename sumcheck::Family<T>::K &kc, bool reg, int m, const Args &a, int K, size_t n, int k, bool aligned,
                         hipStream_t s) {
    static_assert(kRegOutputs<T> <= kRunOutputs<T>, "the switch below is bounded by kRunOutputs");
    if (m < 1 || m > kRunOutputs<T> || (reg && m > kRegOutputs<T>)) return hipErrorInvalidValue;
    switch (m) {
        case 1: launch_m<T, 1>(kc, reg, a, K, n, k, aligned, s); break;
        case 2:
            if constexpr (kRunOutputs<T> >= 2) launch_m<T, 2>(kc, reg, a, K, n, k, aligned, s);
            break;
        case 3:
            if constexpr (kRunOutputs<T> >= 3) launch_m<T, 3>(kc, reg, a, K, n, k, aligned, s);
            break;
        default:
            if constexpr (kRunOutputs<T> >= 4) launch_m<T, 4>(kc, reg, a, K, n, k, aligned, s);
            break;
    }
    return hipGetLastError();
}

}  // namespace lincomb
}  // namespace sr
