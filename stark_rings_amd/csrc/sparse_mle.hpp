// Sparse multilinear extensions over ring elements in CRT / NTT form: the arithmetic half of crates/poly's
//   precompute_eq                                  mle/sparse.rs:381-394   out[b] = prod_i (bit i of b ? g[i] : 1 - g[i])
//   SparseMultilinearExtension::fix_variables      mle/sparse.rs:170-207   result[idx >> w] += eq(point, idx & mask) * value
//   evaluate                                       mle/sparse.rs:53-56     every variable fixed
// `a * b` is the slot product of the ring: mul_boundary of the base field for the fully split power-of-two rings, the Fq3 / Fq9 /
// Fq4 product for the reference's own rings.  Every operation is exact arithmetic on canonical values, so neither the order of the
// factors of an eq value nor the order in which a sum is taken changes a bit of the result: the reference's windows of log2(nnz)
// variables and its doubling recurrence are implementation details, and the device picks its own.
//
// A lane owns one UNIT of a ring element: a 16-byte pair of coefficients of a one-limb field (one coefficient where the buffers are
// not 16-byte aligned or D = 1), one Stark coefficient, one slot of the reference's rings.  U = units per element, a power of two.
//
// eq_kernel: one launch, no workspace.  A lane takes unit c of a block of 2^J consecutive outputs: it forms the product over the
// high n - J bits of the block index once, then expands the J low bits in registers (v[u + 2^i] = v[u] g_i, v[u] -= v[u + 2^i],
// the reference's own step).  blockIdx.y = window: the same launch builds the tables of every window of a fold.
//
// fold_kernel: the stored entries are cut into `spans` of L consecutive entries; lane (span, unit) walks its entries in order.
// Entry j contributes eq(point, idx[j] & mask) vals[j] to run r (seg[r] <= j < seg[r + 1]; idx ascends, so equal keys
// idx >> n_fixed are contiguous).  The eq factor is a product over windows of wbits variables: with tables (TAB) one gather per
// window from the eq tables eq_kernel built into the workspace, without (wbits = 1) point[i] or 1 - point[i] on the fly.  The last
// factor goes through the sum of products (SumOfProducts / SlotDot), finished once per run.  A run that lies inside one span is
// written to out[r] directly.  A run that crosses a span boundary leaves one partial element per span it touches: in slot
// 2 s of `part` when it began before span s (at most one such run per span), in slot 2 s + 1 when it began in span s and goes on
// (at most one).  combine_kernel, launched only when a run can cross a boundary, adds them: workgroup s looks at the run that leaves
// span s through its end and, if that run began in span s, sums slot 2 s + 1 and the slots 2 s' of the spans s' it reaches.
// No atomics, no hashing; the order of the additions does not matter (canonical field elements).
//
// Nothing here reads a workspace word the same call did not write: the tables are written in full by eq_kernel, and combine_kernel
// reads exactly the partial slots fold_kernel wrote (the same run arithmetic on seg decides both).
// Bounds: r stays below n_out and table indices are masked to the table size whatever idx and seg hold, so a corrupt index array
// gives wrong values, never an access outside the buffers.
#pragma once
#include "mle.hpp"

namespace sr {
namespace smle {

struct One {  // the memory image of the base field's 1
    uint64_t w[4];
};

// ---- units ----------------------------------------------------------------------------------------------------------------------
// F: the field the products are chained in; AF: the field of the sum of products (StarkL on the lazy Stark path, else F)
template <class F, class AF, int RW>
struct PowOps {
    using K = int;
    using E = typename F::elem;
    using S = typename F::storage;
    using U = mle::Lane<F, RW>;
    static constexpr int kWords = RW, NC = U::NC;
    static __device__ __forceinline__ void set_one(U &x, const One &one) {
#pragma unroll
        for (int n = 0; n < NC; n++) x.put(n, F::load(reinterpret_cast<const S *>(one.w)));
    }
    static __device__ __forceinline__ void mul(U &x, const U &y, const K &) {
#pragma unroll
        for (int n = 0; n < NC; n++) x.put(n, F::mul_boundary(x.get(n), y.get(n)));
    }
    static __device__ __forceinline__ void add(U &x, const U &y) {
#pragma unroll
        for (int n = 0; n < NC; n++) x.put(n, F::add(x.get(n), y.get(n)));
    }
    static __device__ __forceinline__ void sub(U &x, const U &y) {
#pragma unroll
        for (int n = 0; n < NC; n++) x.put(n, F::sub(x.get(n), y.get(n)));
    }
    static __device__ __forceinline__ void one_minus(U &x, const One &one) {
#pragma unroll
        for (int n = 0; n < NC; n++) x.put(n, F::sub(F::load(reinterpret_cast<const S *>(one.w)), x.get(n)));
    }
    struct Acc {
        SumOfProducts<AF> a[NC];
        __device__ __forceinline__ void init() {
#pragma unroll
            for (int n = 0; n < NC; n++) a[n].init();
        }
        __device__ __forceinline__ void fma(const U &x, const U &y, const K &) {
            using AS = typename AF::storage;
#pragma unroll
            for (int n = 0; n < NC; n++) a[n].fma(AF::load(reinterpret_cast<const AS *>(x.w) + n), AF::load(reinterpret_cast<const AS *>(y.w) + n));
        }
        __device__ __forceinline__ void finish(U &out, const K &) const {
            using AS = typename AF::storage;
#pragma unroll
            for (int n = 0; n < NC; n++) AF::store(reinterpret_cast<AS *>(out.w) + n, a[n].finish());
        }
    };
    using Sum = Acc;
};

template <class SL>
struct SlotOps {
    using K = typename SL::K;
    using F = typename SL::F;
    using E = typename F::elem;
    static constexpr int kWords = SL::W;
    struct U {
        E v[SL::W];
        template <bool NT>
        __device__ __forceinline__ void load(const uint64_t *p) {
#pragma unroll
            for (int i = 0; i < SL::W; i++) {
                const uint64_t t = NT ? __builtin_nontemporal_load(p + i) : p[i];
                v[i] = F::load(&t);
            }
        }
        __device__ __forceinline__ void store(uint64_t *p) const {
#pragma unroll
            for (int i = 0; i < SL::W; i++) {
                uint64_t t;
                F::store(&t, v[i]);
                __builtin_nontemporal_store(t, p + i);
            }
        }
    };
    // one(): component 0 of every slot is the base field's 1
    static __device__ __forceinline__ void set_one(U &x, const One &one) {
        x.v[0] = F::load(one.w);
#pragma unroll
        for (int i = 1; i < SL::W; i++) x.v[i] = F::zero();
    }
    static __device__ __forceinline__ void mul(U &x, const U &y, const K &k) { SL::mul(x.v, y.v, k); }
    static __device__ __forceinline__ void add(U &x, const U &y) {
#pragma unroll
        for (int i = 0; i < SL::W; i++) x.v[i] = F::add(x.v[i], y.v[i]);
    }
    static __device__ __forceinline__ void sub(U &x, const U &y) {
#pragma unroll
        for (int i = 0; i < SL::W; i++) x.v[i] = F::sub(x.v[i], y.v[i]);
    }
    static __device__ __forceinline__ void one_minus(U &x, const One &one) {
        x.v[0] = F::sub(F::load(one.w), x.v[0]);
#pragma unroll
        for (int i = 1; i < SL::W; i++) x.v[i] = F::sub(F::zero(), x.v[i]);
    }
    // babybear72 sums its products unreduced (SlotDot, small_linalg.hpp).  The 96-bit accumulators of the other two (45 and 63
    // registers) push the fold past the 128 VGPRs of four waves per SIMD, so they take the slot product and add.
    static constexpr bool kDot = std::is_same<SL, SlotB72>::value;
    struct Acc {
        SlotDot<SL> d;
        __device__ __forceinline__ void init() { d.init(); }
        __device__ __forceinline__ void fma(const U &x, const U &y, const K &) { d.fma(x.v, y.v); }
        __device__ __forceinline__ void finish(U &out, const K &k) const { d.finish(out.v, k); }
    };
    struct AccPlain {
        U s;
        __device__ __forceinline__ void init() {
#pragma unroll
            for (int i = 0; i < SL::W; i++) s.v[i] = F::zero();
        }
        __device__ __forceinline__ void fma(const U &x, const U &y, const K &k) {
            U t = x;
            SL::mul(t.v, y.v, k);
            add(s, t);
        }
        __device__ __forceinline__ void finish(U &out, const K &) const { out = s; }
    };
    using Sum = typename std::conditional<kDot, Acc, AccPlain>::type;
};

// ---- the eq table ---------------------------------------------------------------------------------------------------------------
// Window t = blockIdx.y holds the variables t wbits .. min(n_vars, (t + 1) wbits) - 1 and writes its table at element t 2^wbits
// of `out` (sr_eq_table: wbits = n_vars, one window).  lu = log2 U.  A window of no variables is the single element one().
template <class O, int J>
__global__ __launch_bounds__(256) void eq_kernel(typename O::K k, One one, uint64_t *out, const uint64_t *pt, unsigned n_vars, unsigned wbits,
                                                 int lu) {
    using U = typename O::U;
    constexpr int KW = O::kWords;
    const unsigned t = blockIdx.y, v0 = t * wbits;
    const unsigned nv = n_vars - v0 < wbits ? n_vars - v0 : wbits, je = nv < (unsigned)J ? nv : (unsigned)J;
    out += (((size_t)t << wbits) << lu) * KW;
    pt += ((size_t)v0 << lu) * KW;
    const size_t units = ((size_t)1 << (nv - je)) << lu, umask = ((size_t)1 << lu) - 1;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < units; i += (size_t)gridDim.x * blockDim.x) {
        const size_t hb = i >> lu, c = i & umask;
        U v[1 << J];
        O::set_one(v[0], one);
        for (unsigned q = je; q < nv; q++) {
            U g;
            g.template load<false>(pt + (((size_t)q << lu) + c) * KW);
            if (!((hb >> (q - je)) & 1)) O::one_minus(g, one);
            if (q == je) v[0] = g;
            else O::mul(v[0], g, k);
        }
#pragma unroll
        for (int q = 0; q < J; q++)
            if ((unsigned)q < je) {
                U g;
                g.template load<false>(pt + (((size_t)q << lu) + c) * KW);
#pragma unroll
                for (int u = 0; u < (1 << q); u++) {
                    v[u + (1 << q)] = v[u];
                    O::mul(v[u + (1 << q)], g, k);
                    O::sub(v[u], v[u + (1 << q)]);
                }
            }
#pragma unroll
        for (int u = 0; u < (1 << J); u++)
            if ((unsigned)u < (1u << je)) v[u].store(out + ((((hb << je) + u) << lu) + c) * KW);
    }
}

// ---- the fold -------------------------------------------------------------------------------------------------------------------
// the run that holds entry j: the largest r < n_out with seg[r] <= j (seg[0] = 0)
__device__ __forceinline__ size_t run_of(const uint64_t *seg, size_t n_out, uint64_t j) {
    size_t lo = 0, hi = n_out;  // seg[lo] <= j < seg[hi] (seg[n_out] = nnz)
    while (hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;
        if (seg[mid] <= j) lo = mid;
        else hi = mid;
    }
    return lo;
}

// fac: TAB ? the eq tables (window t at element t 2^wbits) : the point (wbits = 1).  n_fixed >= 1.
template <class O, bool TAB>
__global__ __launch_bounds__(256) void fold_kernel(typename O::K k, One one, uint64_t *out, const uint64_t *vals, const uint64_t *idx,
                                                   const uint64_t *seg, size_t n_out, size_t nnz, const uint64_t *fac, unsigned n_fixed,
                                                   unsigned wbits, size_t spans, size_t len, uint64_t *part, int lu) {
    using U = typename O::U;
    constexpr int KW = O::kWords;
    const size_t gid = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t s = gid >> lu, c = gid & (((size_t)1 << lu) - 1);
    if (s >= spans) return;
    const size_t j0 = s * len;
    if (j0 >= nnz) return;
    const size_t j1 = nnz - j0 < len ? nnz : j0 + len;
    const unsigned nf = (n_fixed + wbits - 1) / wbits, last_bits = n_fixed - (nf - 1) * wbits;
    const uint64_t wmask = ((uint64_t)1 << wbits) - 1, lmask = ((uint64_t)1 << last_bits) - 1;
    auto factor = [&](U &g, uint64_t x, unsigned t) {
        const uint64_t b = (x >> (t * wbits)) & (t + 1 == nf ? lmask : wmask);
        if constexpr (TAB) {
            g.template load<false>(fac + (((((size_t)t << wbits) + b) << lu) + c) * KW);
        } else {
            g.template load<false>(fac + (((size_t)t << lu) + c) * KW);
            if (!b) O::one_minus(g, one);
        }
    };
    size_t r = run_of(seg, n_out, j0);
    uint64_t run_end = seg[r + 1];
    bool began_before = seg[r] < j0;
    typename O::Sum acc;
    acc.init();
    U res;
#pragma unroll 1
    for (size_t j = j0; j < j1; j++) {
        if (j == run_end && r + 1 < n_out) {  // the run ended inside this span
            acc.finish(res, k);
            res.store(began_before ? part + (((2 * s) << lu) + c) * KW : out + ((r << lu) + c) * KW);
            acc.init();
            began_before = false;
            r++;
            run_end = seg[r + 1];
        }
        const uint64_t x = idx[j];
        U a, g;
        a.template load<true>(vals + ((j << lu) + c) * KW);
#pragma unroll 1
        for (unsigned t = 0; t + 1 < nf; t++) {
            factor(g, x, t);
            O::mul(a, g, k);
        }
        factor(g, x, nf - 1);
        acc.fma(a, g, k);
    }
    acc.finish(res, k);
    uint64_t *dst = began_before ? part + (((2 * s) << lu) + c) * KW : run_end > j1 ? part + (((2 * s + 1) << lu) + c) * KW : out + ((r << lu) + c) * KW;
    res.store(dst);
}

// Workgroup (s, chunk of UC units): G = 256 / UC lanes per unit share the partial elements of the run that leaves span s, and meet in LDS.
template <class O>
__global__ __launch_bounds__(256) void combine_kernel(uint64_t *out, const uint64_t *seg, size_t n_out, size_t nnz, size_t len, const uint64_t *part,
                                                      int lu) {
    using U = typename O::U;
    constexpr int KW = O::kWords;
    __shared__ U lds[256];
    const int luc = lu < 8 ? lu : 8, uc = 1 << luc, groups = 256 >> luc;
    const size_t chunks = (size_t)1 << (lu - luc);
    const size_t s = blockIdx.x / chunks, c = ((blockIdx.x % chunks) << luc) + (threadIdx.x & (uc - 1));
    const int g = threadIdx.x >> luc;
    const size_t je = (s + 1) * len - 1;  // the last entry of span s
    if (je + 1 >= nnz) return;
    const size_t r = run_of(seg, n_out, je);
    const uint64_t b = seg[r], e = seg[r + 1];
    if (b < s * len || e <= je + 1) return;  // began in an earlier span (its workgroup sums it), or ends with this span
    size_t s1 = (size_t)((e - 1) / len);
    const size_t smax = (nnz - 1) / len;
    if (s1 > smax) s1 = smax;
    const size_t count = s1 - s + 1;  // partial m: slot 2 s + 1 for m = 0, slot 2 (s + m) beyond
    U sum;
    bool have = false;
    for (size_t m = g; m < count; m += groups) {
        const size_t slot = m ? 2 * (s + m) : 2 * s + 1;
        U x;
        x.template load<false>(part + ((slot << lu) + c) * KW);
        if (have) O::add(sum, x);
        else sum = x;
        have = true;
    }
    if (have) lds[threadIdx.x] = sum;
    __syncthreads();
    if (g == 0) {  // count >= 2 > g: this lane has a partial
        const int top = count < (size_t)groups ? (int)count : groups;
        for (int gg = 1; gg < top; gg++) O::add(sum, lds[(gg << luc) + (threadIdx.x & (uc - 1))]);
        sum.store(out + ((r << lu) + c) * KW);
    }
}

// ---- the plan: pure host arithmetic ---------------------------------------------------------------------------------------------
// Variables the eq kernel expands in registers (mle.hpp settled on the same counts for the dense fold: 128 VGPRs)
template <class F> constexpr int kEqJ = mle::kMaxJ<F>;
template <class SL> constexpr int kSlotEqJ = mle::kSlotMaxJ<SL>;
// Window of the eq tables and the entry count from which a fold builds them (DESIGN_APPENDIX.md A.7 holds the measurements);
// include/stark_rings_hip.h publishes both (SR_SMLE_WINDOW_BITS, SR_SMLE_TABLE_MIN_NNZ)
constexpr unsigned kWindowBits = 8;
constexpr size_t kTableMinNnz = 1024;
constexpr size_t kMaxTableElems = ((63 + kWindowBits - 1) / kWindowBits) << kWindowBits;  // K of the workspace bound
constexpr int kTargetLanesLog2 = 18;  // lanes a fold launch aims for: four waves per SIMD on 256 CUs

// log2 of the units per element the plan counts with (an unaligned one-limb buffer runs twice as many lanes on the same spans)
inline int plan_log2_units(int ring, int k) {
    switch (ring) {
        case 0: case 1: return k >= 1 ? k - 1 : 0;
        case 2: return k;
        case 3: case 4: return 3;
        default: return 2;
    }
}
struct Plan {
    int launches = 1;
    bool copy = false, tables = false, combine = false;
    unsigned wbits = 1, n_tables = 0;
    size_t table_elems = 0, spans = 0, len = 0, part_elems = 0, work_elems = 0;
};
// false: bad arguments (n_out > nnz, n_out == 0 with entries, n_fixed >= 64).  `window`: the table window for measurements (0: the default)
inline bool plan(int ring, int k, size_t nnz, size_t n_out, size_t n_fixed, Plan *p, unsigned window = 0, size_t table_min = kTableMinNnz) {
    if (ring < 0 || ring > 5 || n_fixed >= 64 || n_out > nnz || (nnz && !n_out)) return false;
    *p = Plan{};
    if (nnz == 0) return true;
    if (n_fixed == 0) {
        p->copy = true;
        return true;
    }
    const int lu = plan_log2_units(ring, k);
    const size_t target = lu >= kTargetLanesLog2 ? 1 : (size_t)1 << (kTargetLanesLog2 - lu);
    size_t spans = nnz / 2 < target ? nnz / 2 : target;
    if (spans < 1) spans = 1;
    p->len = (nnz + spans - 1) / spans;
    p->spans = (nnz + p->len - 1) / p->len;
    p->combine = p->spans > 1 && n_out < nnz;  // nnz runs of one entry cannot cross a span boundary
    p->part_elems = p->combine ? 2 * p->spans : 0;
    p->tables = n_fixed >= 2 && nnz >= table_min;
    if (p->tables) {
        p->wbits = window ? window : kWindowBits;
        if (p->wbits > n_fixed) p->wbits = (unsigned)n_fixed;
        p->n_tables = (unsigned)((n_fixed + p->wbits - 1) / p->wbits);
        p->table_elems = (size_t)p->n_tables << p->wbits;
    }
    p->work_elems = p->table_elems + p->part_elems;
    p->launches = 1 + (p->tables ? 1 : 0) + (p->combine ? 1 : 0);
    return true;
}

// ---- launches -------------------------------------------------------------------------------------------------------------------
inline unsigned grid_for(size_t lanes) {
    size_t blocks = (lanes + 255) / 256;
    if (blocks > 0xFFFFFFull) blocks = 0xFFFFFFull;
    return (unsigned)(blocks ? blocks : 1);
}
// n_windows tables of at most wbits variables each (sr_eq_table: one window of n_vars)
template <class O, int J>
inline hipError_t launch_eq(const typename O::K &k, const One &one, uint64_t *out, const uint64_t *pt, unsigned n_vars, unsigned wbits,
                            unsigned n_windows, int lu, hipStream_t s) {
    const unsigned top = wbits < n_vars ? wbits : n_vars, je = top < (unsigned)J ? top : (unsigned)J;
    const dim3 g(grid_for(((size_t)1 << (top - je)) << lu), n_windows);
    hipLaunchKernelGGL((eq_kernel<O, J>), g, dim3(256), 0, s, k, one, out, pt, n_vars, wbits, lu);
    return hipGetLastError();
}
// the launches of a plan that is neither empty nor a copy; work = [tables | partial elements]
template <class O, int J>
inline hipError_t launch_fold(const typename O::K &k, const One &one, const Plan &p, uint64_t *out, const uint64_t *vals, const uint64_t *idx,
                              const uint64_t *seg, size_t n_out, size_t nnz, const uint64_t *pt, unsigned n_fixed, uint64_t *work, int lu,
                              size_t elem_words, hipStream_t s) {
    uint64_t *part = work + p.table_elems * elem_words;
    if (p.tables)
        if (hipError_t e = launch_eq<O, J>(k, one, work, pt, n_fixed, p.wbits, p.n_tables, lu, s)) return e;
    const dim3 g(grid_for(p.spans << lu));
    if (p.tables) hipLaunchKernelGGL((fold_kernel<O, true>), g, dim3(256), 0, s, k, one, out, vals, idx, seg, n_out, nnz, work, n_fixed, p.wbits, p.spans, p.len, part, lu);
    else hipLaunchKernelGGL((fold_kernel<O, false>), g, dim3(256), 0, s, k, one, out, vals, idx, seg, n_out, nnz, pt, n_fixed, 1u, p.spans, p.len, part, lu);
    if (hipError_t e = hipGetLastError()) return e;
    if (p.combine) {
        const size_t chunks = (size_t)1 << (lu > 8 ? lu - 8 : 0);
        hipLaunchKernelGGL((combine_kernel<O>), dim3((unsigned)((p.spans - 1) * chunks)), dim3(256), 0, s, out, seg, n_out, nnz, p.len, part, lu);
        return hipGetLastError();
    }
    return hipSuccess;
}

}  // namespace smle
}  // namespace sr
