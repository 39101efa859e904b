// Dense multilinear extensions over ring elements in CRT / NTT form: the folds of crates/poly --
//   DenseMultilinearExtension::fix_variables       mle/dense.rs:171-199   self[b] = self[2b] + r (self[2b+1] - self[2b]), the
//                                                  least significant index bit first ("leading" order)
//   fix_last_variables / fix_last_variable_helper  polynomials/multilinear_polynomial.rs:227-286   self[b] = self[b] + r (self[b+half]
//                                                  - self[b]), the most significant index bit first ("trailing" order)
//   evaluate                                       mle/dense.rs:107-113   every variable fixed
//   AddAssign<(R, &Self)>                          mle/dense.rs:288-317   acc[e] += r x[e]
// `r x` is the slot product of the ring: mul_boundary of the base field for the fully split power-of-two rings, the Fq3 / Fq9 / Fq4
// product (small_slot_mul, frog_fq4_mul) for the reference's own rings.
//
// One launch folds J variables: output element b is the fold of the 2^J input elements b * sb + t * st (t < 2^J, in ring
// elements); bit i of t is the variable the launch's point element i fixes.  Leading order: sb = 2^J, st = 1; trailing order on a
// table of 2^m elements: sb = 1, st = 2^(m - J).  The partial folds are exact field arithmetic on canonical values, so the order in
// which a launch takes its J variables does not change a bit of the result (the fold is sum_t eq(point, t) in[t] either way).
//
// Truncated storage (dense.rs:35-54, 397-407): input elements at or beyond n_in are zero and are never loaded; a group whose
// first element is already beyond n_in is all zero (its other elements lie further up in both orders) and is written without any
// load.  n_out elements are written, zeros included.
//
// In place (out == in) is sound for the trailing order only: lane (b, c) reads in[b + t st] (t = 0 is b itself, every other one lies
// at or above st >= n_out) and writes out[b]: no other lane reads or writes that location.  In leading order element b is an
// input of output b >> J, which another workgroup computes.
#pragma once
#include "frog_ring.hpp"
#include "ntt_generic.hpp"
#include "small_linalg.hpp"
#include "small_rings.hpp"

namespace sr {
namespace mle {

typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));

// the 2^J - 1 folds of one coefficient: level i pairs neighbours and uses point value r[i]
template <class F, int J>
__device__ __forceinline__ typename F::elem fold_tree(typename F::elem *v, const typename F::elem *r) {
#pragma unroll
    for (int i = 0; i < J; i++)
#pragma unroll
        for (int u = 0; u < (1 << (J - 1 - i)); u++) v[u] = F::add(v[2 * u], F::mul_boundary(r[i], F::sub(v[2 * u + 1], v[2 * u])));
    return v[0];
}

// ---- power-of-two rings ---------------------------------------------------------------------------------------------------------
// A lane owns RW raw u64 words of the output element: two adjacent coefficients of a one-limb field (one 16-byte access per input
// element) where the buffers are 16-byte aligned, one coefficient otherwise; one Stark coefficient (two 16-byte accesses).
template <class F, int RW>
struct Lane {
    using E = typename F::elem;
    using S = typename F::storage;
    static constexpr int kWords = RW;
    static constexpr int NC = RW * 8 / (int)sizeof(S);  // coefficients per lane
    alignas(16) uint64_t w[RW];
    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int i = 0; i < RW; i++) w[i] = 0;
    }
    // NT: the table is read once and written once (non-temporal); the point is re-read by every workgroup and stays in L2
    template <bool NT>
    __device__ __forceinline__ void load(const uint64_t *p) {
        if constexpr (RW == 1) {
            w[0] = NT ? __builtin_nontemporal_load(p) : *p;
        } else {
#pragma unroll
            for (int i = 0; i < RW / 2; i++) {
                const u64x2 *q = reinterpret_cast<const u64x2 *>(p) + i;
                const u64x2 x = NT ? __builtin_nontemporal_load(q) : *q;
                w[2 * i] = x.x;
                w[2 * i + 1] = x.y;
            }
        }
    }
    __device__ __forceinline__ void store(uint64_t *p) const {
        if constexpr (RW == 1) {
            __builtin_nontemporal_store(w[0], p);
        } else {
#pragma unroll
            for (int i = 0; i < RW / 2; i++) {
                u64x2 x;
                x.x = w[2 * i];
                x.y = w[2 * i + 1];
                __builtin_nontemporal_store(x, reinterpret_cast<u64x2 *>(p) + i);
            }
        }
    }
    __device__ __forceinline__ E get(int n) const { return F::load(reinterpret_cast<const S *>(w) + n); }
    __device__ __forceinline__ void put(int n, const E &e) { F::store(reinterpret_cast<S *>(w) + n, e); }
};

// output units [first, units) of the launch; a unit is RW words, `lu` = log2 of the units per ring element
template <class F, int J, int RW>
__device__ __forceinline__ void fold_units(uint64_t *out, const uint64_t *in, const uint64_t *pt, size_t first, size_t units, int lu,
                                           size_t n_in, size_t sb, size_t st) {
    using E = typename F::elem;
    using L = Lane<F, RW>;
    const size_t gid = blockIdx.x * (size_t)blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    const size_t umask = ((size_t)1 << lu) - 1;
    for (size_t i = first + gid; i < units; i += stride) {
        const size_t b = i >> lu, c = i & umask, base = b * sb;
        L v[1 << J], r[J > 0 ? J : 1];
        if (base >= n_in) {  // the whole group lies in the truncated (zero) part of the table
            v[0].zero();
            v[0].store(out + i * RW);
            continue;
        }
#pragma unroll
        for (int t = 0; t < (1 << J); t++) {
            const size_t e = base + t * st;
            if (e < n_in) v[t].template load<true>(in + ((e << lu) + c) * RW);
            else v[t].zero();
        }
#pragma unroll
        for (int q = 0; q < J; q++) r[q].template load<false>(pt + (((size_t)q << lu) + c) * RW);
#pragma unroll
        for (int n = 0; n < L::NC; n++) {
            E x[1 << J], rr[J > 0 ? J : 1];
#pragma unroll
            for (int t = 0; t < (1 << J); t++) x[t] = v[t].get(n);
#pragma unroll
            for (int q = 0; q < J; q++) rr[q] = r[q].get(n);
            v[0].put(n, fold_tree<F, J>(x, rr));
        }
        v[0].store(out + i * RW);
    }
}

// k = log2 D.  n_out elements are written; see the head of the file for n_in, sb, st.
template <class F, int J>
__global__ __launch_bounds__(256) void fold_kernel(typename F::storage *out, const typename F::storage *in, const typename F::storage *pt,
                                                   size_t n_out, size_t n_in, size_t sb, size_t st, int k) {
    uint64_t *o = reinterpret_cast<uint64_t *>(out);
    const uint64_t *a = reinterpret_cast<const uint64_t *>(in), *p = reinterpret_cast<const uint64_t *>(pt);
    if constexpr (sizeof(typename F::storage) == 8) {
        // D >= 2: a pair of coefficients never straddles two elements, and every element starts on a 16-byte boundary when the buffer does
        if (k >= 1 && (((uintptr_t)o | (uintptr_t)a | (uintptr_t)p) & 15u) == 0) fold_units<F, J, 2>(o, a, p, 0, n_out << (k - 1), k - 1, n_in, sb, st);
        else fold_units<F, J, 1>(o, a, p, 0, n_out << k, k, n_in, sb, st);
    } else {
        fold_units<F, J, (int)sizeof(typename F::storage) / 8>(o, a, p, 0, n_out << k, k, n_in, sb, st);
    }
}

// acc[e D + i] += r[i] x[e D + i] for n coefficients (a whole number of elements); acc and x are the same buffer or disjoint
template <class F>
__global__ __launch_bounds__(256) void mul_elem_add_kernel(typename F::storage *acc, const typename F::storage *x, const typename F::storage *r,
                                                           size_t n, size_t dmask) {
    using E = typename F::elem;
    uint64_t *pa = reinterpret_cast<uint64_t *>(acc);
    const uint64_t *px = reinterpret_cast<const uint64_t *>(x), *pr = reinterpret_cast<const uint64_t *>(r);
    const size_t gid = blockIdx.x * (size_t)blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    auto run = [&](auto lane, size_t units, size_t umask) {
        using L = decltype(lane);
        constexpr int RW = L::kWords;
        for (size_t i = gid; i < units; i += stride) {
            L a, b, c;
            a.template load<true>(pa + i * RW);
            b.template load<true>(px + i * RW);
            c.template load<false>(pr + (i & umask) * RW);
#pragma unroll
            for (int m = 0; m < L::NC; m++) {
                const E s = F::add(a.get(m), F::mul_boundary(c.get(m), b.get(m)));
                a.put(m, s);
            }
            a.store(pa + i * RW);
        }
    };
    if constexpr (sizeof(typename F::storage) == 8) {
        if (dmask != 0 && (((uintptr_t)pa | (uintptr_t)px | (uintptr_t)pr) & 15u) == 0) run(Lane<F, 2>{}, n >> 1, dmask >> 1);
        else run(Lane<F, 1>{}, n, dmask);
    } else {
        run(Lane<F, (int)sizeof(typename F::storage) / 8>{}, n, dmask);
    }
}

// ---- goldilocks24 / babybear72 / frog16 -----------------------------------------------------------------------------------------
// Lane-to-slot mapping: lane i of the launch owns slot i of the flat output table (slot = W consecutive words, S = D / W slots per
// element, element-major), the mapping of small_linalg.hpp.  The 64 lanes of a wave therefore own 64 consecutive slots, and for each
// of the 2^J input elements they read ONE contiguous span of 64 W words (1.5 / 4.5 / 2 KiB): every cache line a wave touches is used
// in full by that wave's W loads, and the store is the same span of the output.  (One element per lane, the mapping of the
// transform kernels, would put a wave's accesses D words apart.)
template <class SL, int J>
__global__ __launch_bounds__(256) void slot_fold_kernel(typename SL::K k, uint64_t *out, const uint64_t *in, const uint64_t *pt, size_t n_out,
                                                        size_t n_in, size_t sb, size_t st) {
    using F = typename SL::F;
    using E = typename F::elem;
    constexpr int W = SL::W, S = SL::D / SL::W;
    const size_t slots = n_out * S;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < slots; i += (size_t)gridDim.x * blockDim.x) {
        const size_t b = i / S, base = b * sb;
        const int off = (int)(i % S) * W;
        E v[1 << J][W], r[J > 0 ? J : 1][W];
        if (base >= n_in) {
#pragma unroll
            for (int m = 0; m < W; m++) out[i * W + m] = 0;
            continue;
        }
#pragma unroll
        for (int t = 0; t < (1 << J); t++) {
            const size_t e = base + t * st;
            if (e < n_in) {
                slot_load<SL>(v[t], in + e * SL::D + off);
            } else {
#pragma unroll
                for (int m = 0; m < W; m++) v[t][m] = F::zero();
            }
        }
#pragma unroll
        for (int q = 0; q < J; q++) slot_load<SL>(r[q], pt + (size_t)q * SL::D + off);
#pragma unroll
        for (int q = 0; q < J; q++)
#pragma unroll
            for (int u = 0; u < (1 << (J - 1 - q)); u++) {
                E d[W];
#pragma unroll
                for (int m = 0; m < W; m++) d[m] = F::sub(v[2 * u + 1][m], v[2 * u][m]);
                SL::mul(d, r[q], k);
#pragma unroll
                for (int m = 0; m < W; m++) v[u][m] = F::add(v[2 * u][m], d[m]);
            }
        slot_store<SL>(out + i * W, v[0]);
    }
}
// acc[e] += r x[e], one slot per lane (the same mapping)
template <class SL>
__global__ __launch_bounds__(256) void slot_mul_elem_add_kernel(typename SL::K k, uint64_t *acc, const uint64_t *x, const uint64_t *r, size_t batch) {
    using F = typename SL::F;
    using E = typename F::elem;
    constexpr int W = SL::W, S = SL::D / SL::W;
    const size_t slots = batch * S;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < slots; i += (size_t)gridDim.x * blockDim.x) {
        E a[W], b[W], c[W];
        slot_load<SL>(a, acc + i * W);
        slot_load<SL>(b, x + i * W);
        slot_load<SL>(c, r + (i % S) * W);
        SL::mul(b, c, k);
#pragma unroll
        for (int m = 0; m < W; m++) a[m] = F::add(a[m], b[m]);
        slot_store<SL>(acc + i * W, a);
    }
}

// Variables one launch folds at most: the largest J whose kernel stays within 128 VGPRs, i.e. four waves per SIMD for 256-lane
// workgroups (tests/test_mle_isa.py holds the counts: Stark J = 3 needs 140, babybear72 J = 3 144)
template <class F> constexpr int kMaxJ = std::is_same<F, Stark>::value ? 2 : 3;
template <class SL> constexpr int kSlotMaxJ = std::is_same<SL, SlotB72>::value ? 2 : 3;

// ---- host side ------------------------------------------------------------------------------------------------------------------
// workgroups of 256 lanes for `units` lane-sized pieces of work: one piece per lane below the launch-size limit (stream_blocks)
inline unsigned blocks_for(size_t units) {
    size_t blocks = (units + 255) / 256;
    if (blocks > 0xFFFFFFull) blocks = 0xFFFFFFull;
    return (unsigned)(blocks ? blocks : 1);
}
template <class F>
inline size_t units_of(size_t n_out, int k) {  // as fold_kernel splits the output when its buffers are aligned
    return sizeof(typename F::storage) == 8 && k >= 1 ? n_out << (k - 1) : n_out << k;
}
template <class F>
inline hipError_t launch_fold(int j, uint64_t *out, const uint64_t *in, const uint64_t *pt, size_t n_out, size_t n_in, size_t sb, size_t st,
                              int k, hipStream_t s) {
    using S = typename F::storage;
    const dim3 g(blocks_for(units_of<F>(n_out, k))), b(256);
    S *o = reinterpret_cast<S *>(out);
    const S *a = reinterpret_cast<const S *>(in), *p = reinterpret_cast<const S *>(pt);
    switch (j) {
        case 0: hipLaunchKernelGGL((fold_kernel<F, 0>), g, b, 0, s, o, a, p, n_out, n_in, sb, st, k); break;
        case 1: hipLaunchKernelGGL((fold_kernel<F, 1>), g, b, 0, s, o, a, p, n_out, n_in, sb, st, k); break;
        case 2: hipLaunchKernelGGL((fold_kernel<F, 2>), g, b, 0, s, o, a, p, n_out, n_in, sb, st, k); break;
        case 3:
            if constexpr (kMaxJ<F> >= 3) {
                hipLaunchKernelGGL((fold_kernel<F, 3>), g, b, 0, s, o, a, p, n_out, n_in, sb, st, k);
                break;
            }
            return hipErrorInvalidValue;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
template <class SL>
inline hipError_t launch_slot_fold(const typename SL::K &kc, int j, uint64_t *out, const uint64_t *in, const uint64_t *pt, size_t n_out,
                                   size_t n_in, size_t sb, size_t st, hipStream_t s) {
    const dim3 g(blocks_for(n_out * (SL::D / SL::W))), b(256);
    switch (j) {
        case 0: hipLaunchKernelGGL((slot_fold_kernel<SL, 0>), g, b, 0, s, kc, out, in, pt, n_out, n_in, sb, st); break;
        case 1: hipLaunchKernelGGL((slot_fold_kernel<SL, 1>), g, b, 0, s, kc, out, in, pt, n_out, n_in, sb, st); break;
        case 2: hipLaunchKernelGGL((slot_fold_kernel<SL, 2>), g, b, 0, s, kc, out, in, pt, n_out, n_in, sb, st); break;
        case 3:
            if constexpr (kSlotMaxJ<SL> >= 3) {
                hipLaunchKernelGGL((slot_fold_kernel<SL, 3>), g, b, 0, s, kc, out, in, pt, n_out, n_in, sb, st);
                break;
            }
            return hipErrorInvalidValue;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
template <class SL>
inline hipError_t launch_slot_mul_elem_add(const typename SL::K &kc, uint64_t *acc, const uint64_t *x, const uint64_t *r, size_t batch, hipStream_t s) {
    hipLaunchKernelGGL((slot_mul_elem_add_kernel<SL>), dim3(blocks_for(batch * (SL::D / SL::W))), dim3(256), 0, s, kc, acc, x, r, batch);
    return hipGetLastError();
}

// ---- the plan: pure host arithmetic ---------------------------------------------------------------------------------------------
enum { ORDER_LEADING = 0, ORDER_TRAILING = 1, MAX_VARS = 47, MAX_LAUNCHES = MAX_VARS };
// Variables one launch folds at most, per ring id (include/stark_rings_hip.h: enum sr_ring).  DESIGN_APPENDIX.md ("Multilinear
// folds") holds the measurements behind the choice.
inline int max_vars_per_launch(int ring) {
    switch (ring) {
        case 0: return kMaxJ<Goldilocks>;
        case 1: return kMaxJ<BabyBear>;
        case 2: return kMaxJ<Stark>;
        case 3: return kSlotMaxJ<SlotG24>;
        case 4: return kSlotMaxJ<SlotB72>;
        default: return kSlotMaxJ<SlotFrog>;
    }
}
struct Plan {
    int launches = 0;
    int j[MAX_LAUNCHES] = {};
    size_t work_elems = 0;  // ring elements of workspace an out-of-place fold needs
};
// false: bad arguments.  n_fixed = 0 is one launch (copy and zero-pad).
inline bool plan(int ring, size_t num_vars, size_t n_fixed, int order, Plan *p) {
    if (ring < 0 || ring > 5 || num_vars > MAX_VARS || n_fixed > num_vars || (order != ORDER_LEADING && order != ORDER_TRAILING)) return false;
    *p = Plan{};
    const int jmax = max_vars_per_launch(ring);
    size_t left = n_fixed;
    do {
        const int j = (int)(left < (size_t)jmax ? left : (size_t)jmax);
        p->j[p->launches++] = j;
        left -= j;
    } while (left);
    // intermediate tables: trailing order writes the first one and folds it in place; leading order cannot fold in place and
    // alternates between two regions, the first and the second intermediate table
    if (p->launches >= 2) {
        const size_t t1 = (size_t)1 << (num_vars - p->j[0]);
        p->work_elems = t1;
        if (order == ORDER_LEADING && p->launches >= 3) p->work_elems += t1 >> p->j[1];
    }
    return true;
}

}  // namespace mle
}  // namespace sr
