// Linear combinations with integer columns beside the tables of ring elements, and multiplicities counted from indices:
//   out_m[e] = [bit K+J of uses_m] c_m[K+J]  +  sum_{k < K, bit k} c_m[k] * T_k[e]  +  sum_{j < J, bit K+j} c_m[K+j] * R::from(col_j[e])
//   e < n, m < M;  0 <= K <= 16, 0 <= J <= 8, 1 <= K + J <= 16, M <= 4
// A column is one uint64_t per row (n_evals <= n stored values, the rest 0 and never read) or the progression start + e, which reads no
// memory: the reference's identity_permutation / random_permutation fixtures (crates/poly multilinear_polynomial.rs:79-133), the
// table side of a logUp lookup and its multiplicities never exist as D words per integer.  A row of coefficients has K + J + 1 ring
// elements -- tables, columns, the constant -- and the mask bits follow that order.  The tables' part is lincomb.hpp's sum, with one
// difference: few table terms are summed as canonical products instead of through the lazy accumulators (kDirectTerms below; the
// bits are the same, every value is canonical).
//
// R::from(x) is from_scalar(BaseRing::from(x)) in CRT / NTT form: x mod p in every coefficient of a power-of-two ring, in component 0
// of every slot of goldilocks24 / babybear72 / frog16 and zero in the others (sr_add_scalar_batch with ntt_form != 0), so
// c * R::from(x) scales every base-field component of c by x mod p (sr_scale_batch).  Per component that is one base-field product
// (W of them for a slot, not a W x W slot product), and it does NOT go through the lazy accumulators: SumOfProducts / SlotDot sum
// products of two memory images (each carries the factor R_b of the image, finish() takes one out), while the raw integer x carries
// none.  Embed<F>::mul(c', x) is a canonical product that takes x as it comes, added with F::add after finish():
//   Goldilocks   c' = c, Goldilocks::mul(c, x): defined for ANY 64-bit representative, so x >= p (p, p + 1, 2^64 - 1) needs no
//                reduction of its own and no bound of kFlush is touched;
//   BabyBear     c' = (c 2^32, c 2^64) by two Montgomery products with R2, then mont32(c 2^32, lo32(x)) + mont32(c 2^64, hi32(x)):
//                mont32 takes any 32-bit second factor (a b + m p < 2^64 for a < p), so the 64-bit x mod p is never formed;
//   Stark        c' = c: the image c R times the raw x is already the image of the product, so no conversion x -> x R and no
//                Montgomery step exist at all: the 256 x 64-bit product is reduced with 2^251 = -(17 2^192 + 1) (Embed<Stark>::mul),
//                a fraction of one 256-bit Montgomery product;
//   Frog         c' = c R, then mont_mul(c', x): mont_mul takes any 64-bit second factor for a first one below p.
// The REG kernels prepare c' once per lane before the walk; the run-time kernels prepare it beside the load of the coefficient.
// On the memory images each of these equals F::mul_boundary(c, image of F::tw_from_u64(x)), c times the field's own x mod p (fields.hpp),
// which is the definition of R::from; tests/test_lincomb_index_gpu.py holds them to it through the model and the forward transform.
//
// Mapping, cache policy, truncation and in-place are lincomb.hpp's: mle::Lane (16-byte pairs where every ring buffer is aligned;
// index arrays are 8-byte accesses and take no part in that), non-temporal tables and outputs, a table or column no output of the
// launch uses is never loaded, stored parts are never over-read.  All lanes of a lane-group want the same col_j[e]: where a ring element
// spans whole waves (2^lu >= 64 lanes) the element index goes through readfirstlane, so the address is wave-uniform -- in the gfx950
// listing (tools/ubench/lincomb_index_isa.hip) the load stays a global_load_dwordx2 on one address for the wave, one transaction,
// because the outputs' stores keep the compiler from proving the array unclobbered for a scalar load; below 64 lanes per element and
// on the slot rings neighbouring lanes read the same or the next word of one cache line.  Columns are read with the default policy:
// every wave of the lane-group re-reads the word.
//
// Two kernels per family, as in lincomb.hpp: REG (K + J <= kRegTerms, coefficients and their c' in registers) and the run-time one.
// Outputs per launch per family are the largest with no scratch within 128 VGPRs (tests/test_lincomb_index_isa.py holds the counts).
//
// Multiplicities: counts[t] = #{ i : idx[i] == t } as u64, t < T.  T <= kLdsBins = 4096 (16 KiB of LDS, four workgroups per CU still
// fit): 32-bit bins private to the workgroup, flushed once per workgroup with one 64-bit global atomic per non-empty bin; a workgroup
// walks fewer than 2^32 indices, so a bin cannot wrap.  Larger T: one 64-bit global atomic per index.  An index >= T is skipped and
// counted in the context's bad-index counter.  Integer atomics only: the result does not depend on their order.
#pragma once
#include "lincomb.hpp"

namespace sr {
namespace lincomb_index {

enum { MAX_TABLES = lincomb::MAX_TABLES, MAX_COLUMNS = 8, MAX_TERMS = 16, MAX_OUTPUTS = lincomb::MAX_OUTPUTS };
constexpr int kRegTerms = 4;
// Few table terms are summed as canonical products, not through the lazy accumulators.  SumOfProducts<Goldilocks> costs 12 VALU per
// term against 30 for mul_boundary + add (its own comment in ntt_generic.hpp), but its finish() is four reduce128, a mul_boundary, a
// mul and two adds once per output coefficient, which a row of one to four terms does not earn back; SlotDot<SlotG24> ends in fifteen
// reduce128 and five of each product, SlotDot<SlotB72> in seventeen two-step reductions.  Measured, not only counted (DESIGN_APPENDIX.md
// A.19; raw lines in profiles/index_columns/): a column of permutation leaves has ONE table term per output, and with the lazy sums
// the Goldilocks 2^16 x 2^12 call took 2.54 ms, 1.11 of the time of the call over three tables it replaces, although it moves 0.6 of
// the bytes -- bound by VALU, not by memory; with the direct sum it takes 1.59 ms (0.69), goldilocks24 x 2^23 went from 0.95 to 0.79.
// The price is a second table loop in the run-time kernels of these families, taken when the launch uses at most kDirectTerms tables
// (a launch-uniform branch).  BabyBear's and Stark's generic SumOfProducts is a sum of canonical products already; frog16's slot
// product costs what its finish does, and babybear72's earns back only up to two terms.
template <class T>
constexpr int kDirectTerms = std::is_same<T, Goldilocks>::value || std::is_same<T, SlotG24>::value ? 4 : std::is_same<T, SlotB72>::value ? 2 : 0;
// table terms of a launch: bits below K of the union of its masks
__device__ __forceinline__ int table_terms(uint32_t any, int K) { return __popc(any & ((1u << K) - 1u)); }

struct Args {
    const uint64_t *t[MAX_TABLES];
    size_t ne[MAX_TABLES];
    const uint64_t *col[MAX_COLUMNS];  // null: the progression start[j] + e
    size_t cne[MAX_COLUMNS];           // stored values
    uint64_t start[MAX_COLUMNS];
    uint64_t *out[MAX_OUTPUTS];
    uint32_t uses[MAX_OUTPUTS];
    const uint64_t *coef;  // row m of the launch: K + J + 1 elements at element m (K + J + 1)
};

// c * R::from(x) per base-field component, on memory images: prep() once per coefficient, mul() per integer (see the head of the file).
// put / get keep a prepared coefficient in the 64-bit words of the lane that held the coefficient.
template <class F> struct Embed;
template <> struct Embed<Goldilocks> {
    using P = uint64_t;
    SR_HD static P prep(uint64_t c) { return c; }
    SR_HD static uint64_t mul(P c, uint64_t x) { return Goldilocks::mul(c, x); }
    SR_HD static void put(uint64_t *w, P c) { w[0] = c; }
    SR_HD static P get(const uint64_t *w) { return w[0]; }
};
template <> struct Embed<BabyBear> {
    struct P {
        uint32_t c1, c2;  // c 2^32, c 2^64
    };
    SR_HD static P prep(uint32_t c) {
        P p;
        p.c1 = BabyBear::mont32(c, BabyBear::R2);
        p.c2 = BabyBear::mont32(p.c1, BabyBear::R2);
        return p;
    }
    SR_HD static uint32_t mul(P c, uint64_t x) {
        return BabyBear::add(BabyBear::mont32(c.c1, (uint32_t)x), BabyBear::mont32(c.c2, (uint32_t)(x >> 32)));
    }
    SR_HD static void put(uint64_t *w, P c) { w[0] = (uint64_t)c.c1 | ((uint64_t)c.c2 << 32); }
    SR_HD static P get(const uint64_t *w) {
        P p;
        p.c1 = (uint32_t)w[0];
        p.c2 = (uint32_t)(w[0] >> 32);
        return p;
    }
};
template <> struct Embed<Stark> {
    using P = Stark::elem;
    SR_HD static P prep(const Stark::elem &c) { return c; }
    // c x mod p for a canonical c and any 64-bit x, no Montgomery step: V = c x < 2^316 = L + H 2^251 (L < 2^251, H < 2^65) and
    // 2^251 = -(17 2^192 + 1), so V = L - H - 17 H 2^192; 17 H = h0 + h1 2^59 (h0 < 2^59, h1 < 2^11) and h1 2^59 2^192 = h1 2^251
    // folds once more: V = (L + h1 + 17 h1 2^192) - (H + h0 2^192) = A - B with A < 2^251 + 2^208 < 2 p and B < 2^251 + 2^65 < p.
    SR_HD static Stark::elem mul(const P &c, uint64_t x) {
        typedef unsigned __int128 u128;
        const uint32_t x0 = (uint32_t)x, x1 = (uint32_t)(x >> 32);
        uint32_t v[10];
        uint64_t t = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            t += (uint64_t)c.l[i] * x0;
            v[i] = (uint32_t)t;
            t >>= 32;
        }
        v[8] = (uint32_t)t;
        t = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            t += (uint64_t)c.l[i] * x1 + v[i + 1];  // (2^32 - 1)^2 + 2 (2^32 - 1) < 2^64
            v[i + 1] = (uint32_t)t;
            t >>= 32;
        }
        v[9] = (uint32_t)t;
        const u128 h = (u128)(v[7] >> 27) | ((u128)v[8] << 5) | ((u128)v[9] << 37), h17 = h * 17u;
        const uint64_t h0 = (uint64_t)h17 & (((uint64_t)1 << 59) - 1);
        const uint32_t h1 = (uint32_t)(h17 >> 59);
        Stark::elem a, b = Stark::zero(), u;
        t = (uint64_t)v[0] + h1;
        a.l[0] = (uint32_t)t;
#pragma unroll
        for (int i = 1; i < 8; i++) {
            t = (t >> 32) + (i == 7 ? v[7] & 0x07FFFFFFu : v[i]) + (i == 6 ? 17u * h1 : 0u);
            a.l[i] = (uint32_t)t;
        }
        b.l[0] = (uint32_t)h;
        b.l[1] = (uint32_t)(h >> 32);
        b.l[2] = (uint32_t)(h >> 64);
        b.l[6] = (uint32_t)h0;
        b.l[7] = (uint32_t)(h0 >> 32);
        const uint32_t borrow = Stark::sub_raw(u, a, Stark::modulus());
        return Stark::sub(borrow ? a : u, b);
    }
    SR_HD static void put(uint64_t *w, const P &c) { Stark::store(reinterpret_cast<Stark::storage *>(w), c); }
    SR_HD static P get(const uint64_t *w) { return Stark::load(reinterpret_cast<const Stark::storage *>(w)); }
};
template <> struct Embed<Frog> {
    using P = uint64_t;
    SR_HD static P prep(uint64_t c) { return Frog::mont_mul(c, Frog::R2); }
    SR_HD static uint64_t mul(P c, uint64_t x) { return Frog::mont_mul(c, x); }
    SR_HD static void put(uint64_t *w, P c) { w[0] = c; }
    SR_HD static P get(const uint64_t *w) { return w[0]; }
};

// col_j[e]; uniform: every lane of the wave has the same e
__device__ __forceinline__ uint64_t column(const Args &a, int j, size_t e, bool uniform) {
    const uint64_t *p = a.col[j];
    if (!p) return a.start[j] + e;
    if (e >= a.cne[j]) return 0;
    if (uniform) {
        const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)e), hi = __builtin_amdgcn_readfirstlane((uint32_t)(e >> 32));
        e = (size_t)lo | ((size_t)hi << 32);
    }
    return p[e];
}

// ---- power-of-two rings -----------------------------------------------------------------------------------------------------------
template <class F, int RW, int M, bool REG>
__device__ __forceinline__ void index_units(const Args &a, int K, int J, size_t n, int lu, size_t groups) {
    using E = typename F::elem;
    using L = mle::Lane<F, RW>;
    using EM = Embed<F>;
    constexpr int SW = (int)sizeof(typename F::storage) / 8;  // words of a coefficient
    constexpr int G = RW >= 4 ? 2 : 4;  // tables whose loads the run-time kernel issues before their products
    const size_t flat = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t g = flat >> lu, c = flat & (((size_t)1 << lu) - 1);
    if (g >= groups) return;
    const int T = K + J;
    const size_t ew = (size_t)RW << lu, cu = c * RW, row = (size_t)(T + 1) * ew;
    const bool uniform = lu >= 6;  // a workgroup is four waves of 64 consecutive lanes
    uint32_t any = 0;
#pragma unroll
    for (int m = 0; m < M; m++) any |= a.uses[m];
    L cst[M];
#pragma unroll
    for (int m = 0; m < M; m++) {
        if ((a.uses[m] >> T) & 1u) cst[m].template load<false>(a.coef + m * row + (size_t)T * ew + cu);
        else cst[m].zero();
    }
    if constexpr (REG) {
        // slot s < K: table s; K <= s < T: column s - K, its coefficient kept as Embed's c'
        L cf[M][kRegTerms];
#pragma unroll
        for (int m = 0; m < M; m++)
#pragma unroll
            for (int s = 0; s < kRegTerms; s++) {
                if (s < T && ((a.uses[m] >> s) & 1u)) {
                    cf[m][s].template load<false>(a.coef + m * row + (size_t)s * ew + cu);
                    if (s >= K) {
#pragma unroll
                        for (int q = 0; q < L::NC; q++) EM::put(cf[m][s].w + q * SW, EM::prep(cf[m][s].get(q)));
                    }
                } else {
                    cf[m][s].zero();
                }
            }
        for (size_t e = g; e < n; e += groups) {
            L t[kRegTerms];  // a column's integer in word 0
#pragma unroll
            for (int s = 0; s < kRegTerms; s++) {
                t[s].zero();
                if (s < T && ((any >> s) & 1u)) {
                    if (s < K) {
                        if (e < a.ne[s]) t[s].template load<true>(a.t[s] + e * ew + cu);
                    } else {
                        t[s].w[0] = column(a, s - K, e, uniform);
                    }
                }
            }
#pragma unroll
            for (int m = 0; m < M; m++) {
                L o;
#pragma unroll
                for (int q = 0; q < L::NC; q++) {
                    E r;
                    if constexpr (kDirectTerms<F> >= kRegTerms) {
                        r = cst[m].get(q);
#pragma unroll
                        for (int s = 0; s < kRegTerms; s++)
                            if (s < K && ((a.uses[m] >> s) & 1u)) r = F::add(r, F::mul_boundary(cf[m][s].get(q), t[s].get(q)));
                    } else {
                        SumOfProducts<F> acc;
                        acc.init();
#pragma unroll
                        for (int s = 0; s < kRegTerms; s++)
                            if (s < K && ((a.uses[m] >> s) & 1u)) acc.fma(cf[m][s].get(q), t[s].get(q));
                        r = F::add(acc.finish(), cst[m].get(q));
                    }
#pragma unroll
                    for (int s = 0; s < kRegTerms; s++)
                        if (s >= K && s < T && ((a.uses[m] >> s) & 1u)) r = F::add(r, EM::mul(EM::get(cf[m][s].w + q * SW), t[s].w[0]));
                    lincomb::leaves<F>(r);
                    o.put(q, r);
                }
                o.store(a.out[m] + e * ew + cu);
            }
        }
    } else {
        for (size_t e = g; e < n; e += groups) {
            L o[M];
            if (kDirectTerms<F> > 0 && table_terms(any, K) <= kDirectTerms<F>) {
#pragma unroll
                for (int m = 0; m < M; m++) o[m] = cst[m];
                for (int k0 = 0; k0 < K; k0 += G) {
                    L t[G];
#pragma unroll
                    for (int j = 0; j < G; j++) {
                        const int k = k0 + j;
                        if (k < K && ((any >> k) & 1u) && e < a.ne[k]) t[j].template load<true>(a.t[k] + e * ew + cu);
                        else t[j].zero();
                    }
#pragma unroll
                    for (int j = 0; j < G; j++) {
                        const int k = k0 + j;
                        if (k >= K) break;
#pragma unroll
                        for (int m = 0; m < M; m++) {
                            if (!((a.uses[m] >> k) & 1u)) continue;
                            L cf;
                            cf.template load<false>(a.coef + m * row + (size_t)k * ew + cu);
#pragma unroll
                            for (int q = 0; q < L::NC; q++) o[m].put(q, F::add(o[m].get(q), F::mul_boundary(cf.get(q), t[j].get(q))));
                        }
                    }
                }
            } else {
                SumOfProducts<F> acc[M][L::NC];
#pragma unroll
                for (int m = 0; m < M; m++)
#pragma unroll
                    for (int q = 0; q < L::NC; q++) acc[m][q].init();
                for (int k0 = 0; k0 < K; k0 += G) {
                    L t[G];
#pragma unroll
                    for (int j = 0; j < G; j++) {
                        const int k = k0 + j;
                        if (k < K && ((any >> k) & 1u) && e < a.ne[k]) t[j].template load<true>(a.t[k] + e * ew + cu);
                        else t[j].zero();
                    }
#pragma unroll
                    for (int j = 0; j < G; j++) {
                        const int k = k0 + j;
                        if (k >= K) break;
#pragma unroll
                        for (int m = 0; m < M; m++) {
                            if (!((a.uses[m] >> k) & 1u)) continue;
                            L cf;
                            cf.template load<false>(a.coef + m * row + (size_t)k * ew + cu);
#pragma unroll
                            for (int q = 0; q < L::NC; q++) acc[m][q].fma(cf.get(q), t[j].get(q));
                        }
                    }
                }
#pragma unroll
                for (int m = 0; m < M; m++)
#pragma unroll
                    for (int q = 0; q < L::NC; q++) o[m].put(q, F::add(acc[m][q].finish(), cst[m].get(q)));
            }
            for (int j = 0; j < J; j++) {
                if (!((any >> (K + j)) & 1u)) continue;
                const uint64_t x = column(a, j, e, uniform);
#pragma unroll
                for (int m = 0; m < M; m++) {
                    if (!((a.uses[m] >> (K + j)) & 1u)) continue;
                    L cf;
                    cf.template load<false>(a.coef + m * row + (size_t)(K + j) * ew + cu);
#pragma unroll
                    for (int q = 0; q < L::NC; q++) o[m].put(q, F::add(o[m].get(q), EM::mul(EM::prep(cf.get(q)), x)));
                }
            }
#pragma unroll
            for (int m = 0; m < M; m++) {
#pragma unroll
                for (int q = 0; q < L::NC; q++) lincomb::leaves<F>(o[m].get(q));
                o[m].store(a.out[m] + e * ew + cu);
            }
        }
    }
}
// pair: every ring buffer of the launch is 16-byte aligned and k >= 1 (one-limb fields)
template <class F, int M, bool REG>
__global__ __launch_bounds__(256) void lincomb_index_kernel(Args a, int K, int J, size_t n, int k, int pair, size_t groups) {
    if constexpr (sizeof(typename F::storage) == 8) {
        if (pair) index_units<F, 2, M, REG>(a, K, J, n, k - 1, groups);
        else index_units<F, 1, M, REG>(a, K, J, n, k, groups);
    } else {
        index_units<F, (int)sizeof(typename F::storage) / 8, M, REG>(a, K, J, n, k, groups);
    }
}

// ---- goldilocks24 / babybear72 / frog16: lane = slot ---------------------------------------------------------------------------
// REG is built for the slot types whose prepared coefficient is one base-field element (Goldilocks, Frog)
template <class SL, int M, bool REG>
__global__ __launch_bounds__(256) void slot_lincomb_index_kernel(typename SL::K kc, Args a, int K, int J, size_t n, size_t groups) {
    using F = typename SL::F;
    using E = typename F::elem;
    using EM = Embed<F>;
    constexpr int W = SL::W, S = SL::D / SL::W;
    const size_t flat = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t g = flat / S;
    const int off = (int)(flat % S) * W;
    if (g >= groups) return;
    const int T = K + J;
    const size_t row = (size_t)(T + 1) * SL::D;
    uint32_t any = 0;
#pragma unroll
    for (int m = 0; m < M; m++) any |= a.uses[m];
    E cst[M][W];
#pragma unroll
    for (int m = 0; m < M; m++) {
        if ((a.uses[m] >> T) & 1u) {
            slot_load<SL>(cst[m], a.coef + m * row + (size_t)T * SL::D + off);
        } else {
#pragma unroll
            for (int w = 0; w < W; w++) cst[m][w] = F::zero();
        }
    }
    if constexpr (REG) {
        static_assert(std::is_same<typename EM::P, E>::value && std::is_same<E, uint64_t>::value,
                      "the prepared coefficient takes the coefficient's register, a column's integer component 0 of the table's");
        E cf[M][kRegTerms][W];
#pragma unroll
        for (int m = 0; m < M; m++)
#pragma unroll
            for (int s = 0; s < kRegTerms; s++) {
                if (s < T && ((a.uses[m] >> s) & 1u)) {
                    slot_load<SL>(cf[m][s], a.coef + m * row + (size_t)s * SL::D + off);
                    if (s >= K) {
#pragma unroll
                        for (int w = 0; w < W; w++) cf[m][s][w] = EM::prep(cf[m][s][w]);
                    }
                } else {
#pragma unroll
                    for (int w = 0; w < W; w++) cf[m][s][w] = F::zero();
                }
            }
        for (size_t e = g; e < n; e += groups) {
            E t[kRegTerms][W];
#pragma unroll
            for (int s = 0; s < kRegTerms; s++) {
#pragma unroll
                for (int w = 0; w < W; w++) t[s][w] = F::zero();
                if (s < T && ((any >> s) & 1u)) {
                    if (s < K) {
                        if (e < a.ne[s]) {
#pragma unroll
                            for (int w = 0; w < W; w++) t[s][w] = F::load(a.t[s] + e * SL::D + off + w);
                        }
                    } else {
                        t[s][0] = column(a, s - K, e, false);
                    }
                }
            }
#pragma unroll
            for (int m = 0; m < M; m++) {
                E r[W];
                if constexpr (kDirectTerms<SL> >= kRegTerms) {
#pragma unroll
                    for (int w = 0; w < W; w++) r[w] = cst[m][w];
#pragma unroll
                    for (int s = 0; s < kRegTerms; s++)
                        if (s < K && ((a.uses[m] >> s) & 1u)) {
                            E pr[W];
#pragma unroll
                            for (int w = 0; w < W; w++) pr[w] = t[s][w];
                            slot_fma<SL>(r, pr, cf[m][s], kc);
                        }
                } else {
                    SlotDot<SL> acc;
                    acc.init();
#pragma unroll
                    for (int s = 0; s < kRegTerms; s++)
                        if (s < K && ((a.uses[m] >> s) & 1u)) acc.fma(cf[m][s], t[s]);
                    acc.finish(r, kc);
#pragma unroll
                    for (int w = 0; w < W; w++) r[w] = F::add(r[w], cst[m][w]);
                }
#pragma unroll
                for (int s = 0; s < kRegTerms; s++)
                    if (s >= K && s < T && ((a.uses[m] >> s) & 1u)) {
#pragma unroll
                        for (int w = 0; w < W; w++) r[w] = F::add(r[w], EM::mul(cf[m][s][w], t[s][0]));
                    }
#pragma unroll
                for (int w = 0; w < W; w++) lincomb::leaves<F>(r[w]);
                slot_store<SL>(a.out[m] + e * SL::D + off, r);
            }
        }
    } else {
        for (size_t e = g; e < n; e += groups) {
            E r[M][W];
            if (kDirectTerms<SL> > 0 && table_terms(any, K) <= kDirectTerms<SL>) {
#pragma unroll
                for (int m = 0; m < M; m++)
#pragma unroll
                    for (int w = 0; w < W; w++) r[m][w] = cst[m][w];
                for (int k = 0; k < K; k++) {
                    if (!((any >> k) & 1u) || e >= a.ne[k]) continue;   // a zero table element adds nothing
                    E t[W];
                    slot_load<SL>(t, a.t[k] + e * SL::D + off);
#pragma unroll
                    for (int m = 0; m < M; m++) {
                        if (!((a.uses[m] >> k) & 1u)) continue;
                        E cf[W], pr[W];
                        slot_load<SL>(cf, a.coef + m * row + (size_t)k * SL::D + off);
#pragma unroll
                        for (int w = 0; w < W; w++) pr[w] = t[w];
                        slot_fma<SL>(r[m], pr, cf, kc);
                    }
                }
            } else {
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
                        slot_load<SL>(cf, a.coef + m * row + (size_t)k * SL::D + off);
                        acc[m].fma(cf, t);
                    }
                }
#pragma unroll
                for (int m = 0; m < M; m++) {
                    acc[m].finish(r[m], kc);
#pragma unroll
                    for (int w = 0; w < W; w++) r[m][w] = F::add(r[m][w], cst[m][w]);
                }
            }
            for (int j = 0; j < J; j++) {
                if (!((any >> (K + j)) & 1u)) continue;
                const uint64_t x = column(a, j, e, false);
#pragma unroll
                for (int m = 0; m < M; m++) {
                    if (!((a.uses[m] >> (K + j)) & 1u)) continue;
                    E cf[W];
                    slot_load<SL>(cf, a.coef + m * row + (size_t)(K + j) * SL::D + off);
#pragma unroll
                    for (int w = 0; w < W; w++) r[m][w] = F::add(r[m][w], EM::mul(EM::prep(cf[w]), x));
                }
            }
#pragma unroll
            for (int m = 0; m < M; m++) {
#pragma unroll
                for (int w = 0; w < W; w++) lincomb::leaves<F>(r[m][w]);
                slot_store<SL>(a.out[m] + e * SL::D + off, r[m]);
            }
        }
    }
}

// ---- the plan: pure host arithmetic -------------------------------------------------------------------------------------------------
// Outputs of one launch at most, per family type T: REG with K + J <= kRegTerms, and the run-time kernel.  Zero: the family has no REG
// kernel within the budget.  VGPRs of the gfx950 listing (tests/test_lincomb_index_isa.py):
//   REG, M = 1 / 2:       Goldilocks 70 / 120, BabyBear 64 / 114, Stark 156 / -, goldilocks24 116 / 178, babybear72 - (its prepared
//                         coefficient is two words), frog16 149 / -
//   run-time, M = 1 .. 4: Goldilocks 72 / 106 / 126 / 166, BabyBear 44 / 52 / 62 / 72, Stark 116 / 146 / - / -,
//                         goldilocks24 82 / 134 / - / -, babybear72 107 / 170 / - / -, frog16 108 / 188 / - / -
// Stark's run-time kernel issues the loads of two tables before their products, not four (G in index_units): four keep 32 registers
// and take it to 132.
template <class T>
constexpr int kRegOutputs = std::is_same<T, Goldilocks>::value || std::is_same<T, BabyBear>::value ? 2 : std::is_same<T, SlotG24>::value ? 1 : 0;
template <class T> constexpr int kRunOutputs = std::is_same<T, BabyBear>::value ? 4 : std::is_same<T, Goldilocks>::value ? 3 : 1;

template <class T>
constexpr bool use_reg(int n_terms, int n_outputs) {
    return n_terms <= kRegTerms && n_outputs <= kRegOutputs<T>;
}
template <class T>
constexpr int outputs_of(int n_terms, int n_outputs) {
    return use_reg<T>(n_terms, n_outputs) ? n_outputs : (n_outputs < kRunOutputs<T> ? n_outputs : kRunOutputs<T>);
}
inline int outputs_per_launch(int ring, int n_terms, int n_outputs) {
    switch (ring) {
        case 0: return outputs_of<Goldilocks>(n_terms, n_outputs);
        case 1: return outputs_of<BabyBear>(n_terms, n_outputs);
        case 2: return outputs_of<Stark>(n_terms, n_outputs);
        case 3: return outputs_of<SlotG24>(n_terms, n_outputs);
        case 4: return outputs_of<SlotB72>(n_terms, n_outputs);
        default: return outputs_of<SlotFrog>(n_terms, n_outputs);
    }
}
// n_index == 0 is lincomb.hpp's call and takes its plan
inline bool plan(int ring, int n_tables, int n_index, int n_outputs, lincomb::Plan *p) {
    if (n_index == 0) return lincomb::plan(ring, n_tables, n_outputs, p);
    if (ring < 0 || ring > 5 || n_tables < 0 || n_tables > MAX_TABLES || n_index < 0 || n_index > MAX_COLUMNS || n_tables + n_index < 1 ||
        n_tables + n_index > MAX_TERMS || n_outputs < 1 || n_outputs > MAX_OUTPUTS)
        return false;
    p->outputs_per_launch = outputs_per_launch(ring, n_tables + n_index, n_outputs);
    p->launches = (n_outputs + p->outputs_per_launch - 1) / p->outputs_per_launch;
    return true;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
template <class T, int M>
inline void launch_m(const typename sumcheck::Family<T>::K &kc, bool reg, const Args &a, int K, int J, size_t n, int k, bool aligned,
                     hipStream_t s) {
    if constexpr (sumcheck::kSlot<T>) {
        constexpr size_t S = T::D / T::W;
        const size_t groups = lincomb::groups_for(n, S);
        const dim3 g(mle::blocks_for(groups * S)), b(256);
        if constexpr (M <= kRegOutputs<T>) {
            if (reg) {
                hipLaunchKernelGGL((slot_lincomb_index_kernel<T, M, true>), g, b, 0, s, kc, a, K, J, n, groups);
                return;
            }
        }
        hipLaunchKernelGGL((slot_lincomb_index_kernel<T, M, false>), g, b, 0, s, kc, a, K, J, n, groups);
    } else {
        const sumcheck::Geometry ge = sumcheck::geometry_of<T>(k, aligned);
        const size_t groups = lincomb::groups_for(n, (size_t)1 << ge.lu);
        const dim3 g(mle::blocks_for(groups << ge.lu)), b(256);
        if constexpr (M <= kRegOutputs<T>) {
            if (reg) {
                hipLaunchKernelGGL((lincomb_index_kernel<T, M, true>), g, b, 0, s, a, K, J, n, ge.k, ge.pair, groups);
                return;
            }
        }
        hipLaunchKernelGGL((lincomb_index_kernel<T, M, false>), g, b, 0, s, a, K, J, n, ge.k, ge.pair, groups);
    }
}
// One launch: the `m` outputs of `a` (m <= outputs_of<T>) over K tables and J columns.  reg: the call as a whole takes the REG kernel.
template <class T>
inline hipError_t launch(const typename sumcheck::Family<T>::K &kc, bool reg, int m, const Args &a, int K, int J, size_t n, int k,
                         bool aligned, hipStream_t s) {
    static_assert(kRegOutputs<T> <= kRunOutputs<T>, "the switch below is bounded by kRunOutputs");
    reg = reg && m <= kRegOutputs<T>;
    if (m < 1 || m > kRunOutputs<T>) return hipErrorInvalidValue;
    switch (m) {
        case 1: launch_m<T, 1>(kc, reg, a, K, J, n, k, aligned, s); break;
        case 2:
            if constexpr (kRunOutputs<T> >= 2) launch_m<T, 2>(kc, reg, a, K, J, n, k, aligned, s);
            break;
        case 3:
            if constexpr (kRunOutputs<T> >= 3) launch_m<T, 3>(kc, reg, a, K, J, n, k, aligned, s);
            break;
        default:
            if constexpr (kRunOutputs<T> >= 4) launch_m<T, 4>(kc, reg, a, K, J, n, k, aligned, s);
            break;
    }
    return hipGetLastError();
}

// ---- multiplicities -------------------------------------------------------------------------------------------------------------
constexpr size_t kLdsBins = 4096;
constexpr size_t kCountPerBlock = 4096;  // indices a workgroup takes before the grid stops growing

template <bool LDS>
__global__ __launch_bounds__(256) void index_count_kernel(unsigned long long *counts, const uint64_t *idx, size_t n, size_t n_bins,
                                                          unsigned long long *bad) {
    __shared__ uint32_t bins[LDS ? kLdsBins : 1];
    if constexpr (LDS) {
        for (size_t t = threadIdx.x; t < n_bins; t += blockDim.x) bins[t] = 0;
        __syncthreads();
    }
    unsigned long long skipped = 0;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t t = __builtin_nontemporal_load(idx + i);
        if (t >= n_bins) {
            skipped++;
            continue;
        }
        if constexpr (LDS) atomicAdd(&bins[t], 1u);
        else atomicAdd(counts + t, 1ull);
    }
    if (skipped) atomicAdd(bad, skipped);
    if constexpr (LDS) {
        __syncthreads();
        for (size_t t = threadIdx.x; t < n_bins; t += blockDim.x) {
            const uint32_t v = bins[t];
            if (v) atomicAdd(counts + t, (unsigned long long)v);
        }
    }
}
// workgroups: one per kCountPerBlock indices up to 2048, and never so few that one would walk 2^32 indices (n < 2^48)
inline unsigned count_blocks(size_t n) {
    size_t b = (n + kCountPerBlock - 1) / kCountPerBlock;
    if (b > 2048) b = 2048;
    const size_t least = (n >> 31) + 1;
    if (b < least) b = least;
    return (unsigned)b;
}
// counts is cleared by the caller on the same stream (hipMemsetAsync) before this launch
inline hipError_t launch_count(uint64_t *counts, const uint64_t *idx, size_t n, size_t n_bins, unsigned long long *bad, hipStream_t s) {
    const dim3 g(count_blocks(n)), b(256);
    unsigned long long *c = reinterpret_cast<unsigned long long *>(counts);
    if (n_bins <= kLdsBins) hipLaunchKernelGGL((index_count_kernel<true>), g, b, 0, s, c, idx, n, n_bins, bad);
    else hipLaunchKernelGGL((index_count_kernel<false>), g, b, 0, s, c, idx, n, n_bins, bad);
    return hipGetLastError();
}

}  // namespace lincomb_index
}  // namespace sr
