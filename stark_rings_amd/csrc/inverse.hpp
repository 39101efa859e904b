// Batch inversion of tables of ring elements in CRT / NTT form, slot by slot:
//   out[e] = num[e] * den[e]^-1        e < n        (num absent: one(), as absent numerators are in frac_tree.hpp)
// Field::inverse / ark_ff::batch_inversion of the reference on every slot of every element: the base field for the fully split
// power-of-two rings, Fq3 / Fq9 / Fq4 for the reference's own rings.  `*` is the slot product of the ring as in mle.hpp.
//
// Montgomery's trick.  Lane (g, c) owns unit c (mle::Lane: a 16-byte pair of coefficients of a one-limb field where every buffer is
// aligned, one coefficient otherwise, one Stark coefficient; one Fq3 / Fq9 / Fq4 slot) of the C consecutive elements g C .. g C + C - 1:
//   forward   pre_i = x_0 ... x_(i-1), kept in registers beside the x_i
//   once      inv = (x_0 ... x_(C-1))^(|F| - 2)                                                  (fermat() below)
//   backward  out_i = inv * pre_i (* num_i), inv = inv * x_i
// 3 (C - 1) products a chunk (4 C - 3 with numerators) and one inversion of I products, I / C a unit.  pre_0 is one() and is never
// multiplied by.  All 64 lanes of a wave run fermat() together whether they need it or not, so only C amortises it; C is bounded by
// registers (kChunk below; tools/ubench/inverse_isa.hip, tests/test_inverse_isa.py hold the counts).
//
// The walks are serial chains of dependent products.  A pair lane carries two independent chains (its two coefficients); beyond that
// nothing is interleaved in a lane: the kernels stay within 128 VGPRs, four waves per SIMD, and the other waves fill the pipe.
//
// Zeros.  A zero unit enters the products as one() and leaves as zero, with or without a numerator (ark_ff::batch_inversion skips
// zeros): a select on the unit's zero mask, no divergent arm.  Every zero coefficient / slot met is counted: a ballot per unit position,
// its popcount summed per wave, one atomic a wave.  A ring element is a unit of the ring exactly when none of its slots is zero.
//
// fermat(): x^(|F| - 2) by a chain that is fixed per family.  With u = x^(2^8 - 1) (10 products), the exponent is read from its top
// bit: eight set bits in a row are eight squarings and a product by u, any other bit a squaring and, if set, a product by x.  The
// exponents of the base fields are almost all runs of ones (Goldilocks 2^64 - 2^32 - 1, BabyBear 2^31 - 2^27 - 1, Stark 2^251 + 2^196 +
// 2^192 - 1), which is where this saves over square-and-multiply: 86 against 125, 48 against 59, 286 against 444 products;
// tools/model_inverse.py writes the chains out, checks their exponents and counts them.  Three units are live: x, u and the power.
//
// Memory: den is read once, num once, out written once, all non-temporal.  out may be exactly den or exactly num: a lane reads a unit
// before it writes that same unit, and no other lane touches it.  One read is not of a lane's own unit: a position a lane does not have
// (beyond n, or a lane beyond the last group) loads the same unit of element n - 1, so that every load is in bounds and unconditional.
// In place the owner of that element may be storing to it at that moment.  This is intended: the loaded value is replaced by one()
// before any arithmetic (a select on `have`), takes part in no count and is never stored, so whatever the load returns changes nothing.
#pragma once
#include "lincomb.hpp"
#include "sparse_mle.hpp"

namespace sr {
namespace inverse {

// ---- |F| - 2 of the slot field, 64-bit words from the least significant --------------------------------------------------------------
template <class T> struct Exponent;
template <> struct Exponent<Goldilocks> {  // p - 2 = 2^64 - 2^32 - 1
    static constexpr int kBits = 64;
    SR_HD static constexpr uint64_t word(int i) { return i == 0 ? 0xFFFFFFFEFFFFFFFFull : 0; }
};
template <> struct Exponent<BabyBear> {  // p - 2 = 2^31 - 2^27 - 1
    static constexpr int kBits = 31;
    SR_HD static constexpr uint64_t word(int i) { return i == 0 ? 0x0000000077FFFFFFull : 0; }
};
template <> struct Exponent<Stark> {  // p - 2 = 2^251 + 2^196 + 2^192 - 1
    static constexpr int kBits = 252;
    SR_HD static constexpr uint64_t word(int i) { return i >= 0 && i < 3 ? ~0ull : i == 3 ? 0x0800000000000010ull : 0; }
};
template <> struct Exponent<SlotG24> {  // q^3 - 2, q = 2^64 - 2^32 + 1
    static constexpr int kBits = 192;
    SR_HD static constexpr uint64_t word(int i) {
        return i == 0 ? 0xFFFFFFFCFFFFFFFFull : i == 1 ? 0xFFFFFFF900000005ull : i == 2 ? 0xFFFFFFFD00000005ull : 0;
    }
};
template <> struct Exponent<SlotB72> {  // q^9 - 2, q = 15 * 2^27 + 1
    static constexpr int kBits = 279;
    SR_HD static constexpr uint64_t word(int i) {
        return i == 0   ? 0xE900000437FFFFFFull
               : i == 1 ? 0x154FE008A6D80007ull
               : i == 2 ? 0x641F3352D9FD7106ull
               : i == 3 ? 0xE9D6D777B6D3FB74ull
               : i == 4 ? 0x0000000000479B38ull
                        : 0;
    }
};
template <> struct Exponent<SlotFrog> {  // q^4 - 2, q = 0xDCD31BD79EC2DD19
    static constexpr int kBits = 256;
    SR_HD static constexpr uint64_t word(int i) {
        return i == 0   ? 0x6963B001EE6709DFull
               : i == 1 ? 0x0FFC412D6682EDA2ull
               : i == 2 ? 0x9FD162F5B675E821ull
               : i == 3 ? 0x8DBB966C782280E5ull
                        : 0;
    }
};
constexpr int kRun = 8;  // u = x^(2^kRun - 1)

// bits pos .. pos - kRun + 1 of the exponent (pos >= kRun - 1)
template <class T>
SR_HD constexpr unsigned exponent_window(int pos) {
    const int lo = pos - (kRun - 1), wi = lo >> 6, sh = lo & 63;
    uint64_t v = Exponent<T>::word(wi) >> sh;
    if (sh > 64 - kRun) v |= Exponent<T>::word(wi + 1) << (64 - sh);
    return (unsigned)(v & ((1u << kRun) - 1));
}
// products of the chain (squarings included): what tools/model_inverse.py counts for the same exponent
template <class T>
constexpr int chain_products() {
    int n = 10;  // u: (1 + 1) + (2 + 1) + (4 + 1)
    for (int pos = Exponent<T>::kBits - 2; pos >= 0;) {
        if (pos >= kRun - 1 && exponent_window<T>(pos) == (1u << kRun) - 1) {
            n += kRun + 1;
            pos -= kRun;
        } else {
            n += 1 + (int)((Exponent<T>::word(pos >> 6) >> (pos & 63)) & 1);
            pos -= 1;
        }
    }
    return n;
}

// ---- units: the zero mask of a unit and the select on it -------------------------------------------------------------------------
template <class F, int RW>
struct PowUnit {
    using T = F;
    using Ops = smle::PowOps<F, F, RW>;
    using U = typename Ops::U;
    using K = typename Ops::K;
    static constexpr int NC = U::NC, SW = RW / U::NC;  // coefficients of a unit, words of a coefficient
    static __device__ __forceinline__ unsigned zeros(const U &x) {  // bit n: coefficient n is zero
        unsigned m = 0;
#pragma unroll
        for (int n = 0; n < NC; n++) {
            uint64_t any = 0;
#pragma unroll
            for (int j = 0; j < SW; j++) any |= x.w[n * SW + j];
            m |= (unsigned)(any == 0) << n;
        }
        return m;
    }
    // coefficient n of x becomes that of y where bit n of m is set
    static __device__ __forceinline__ void select(U &x, unsigned m, const U &y) {
#pragma unroll
        for (int n = 0; n < NC; n++)
#pragma unroll
            for (int j = 0; j < SW; j++) x.w[n * SW + j] = (m >> n) & 1u ? y.w[n * SW + j] : x.w[n * SW + j];
    }
    static __device__ __forceinline__ void set_zero(U &x) { x.zero(); }
    static __device__ __forceinline__ void leaves(const U &x) {  // the invariant-checking build counts a word >= p that leaves the call
#pragma unroll
        for (int n = 0; n < NC; n++) lincomb::leaves<F>(x.get(n));
    }
};
template <class SL>
struct SlotUnit {
    using T = SL;
    using Ops = smle::SlotOps<SL>;
    using U = typename Ops::U;
    using K = typename Ops::K;
    using F = typename SL::F;
    static constexpr int NC = 1;
    static __device__ __forceinline__ unsigned zeros(const U &x) {
        typename F::elem any = x.v[0];
#pragma unroll
        for (int i = 1; i < SL::W; i++) any |= x.v[i];
        return any == 0;
    }
    static __device__ __forceinline__ void select(U &x, unsigned m, const U &y) {
#pragma unroll
        for (int i = 0; i < SL::W; i++) x.v[i] = m ? y.v[i] : x.v[i];
    }
    static __device__ __forceinline__ void set_zero(U &x) {
#pragma unroll
        for (int i = 0; i < SL::W; i++) x.v[i] = F::zero();
    }
    static __device__ __forceinline__ void leaves(const U &x) {
#pragma unroll
        for (int i = 0; i < SL::W; i++) lincomb::leaves<F>(x.v[i]);
    }
};

template <class UT> constexpr unsigned kAll = (1u << UT::NC) - 1;  // every coefficient of a unit
template <class UT>
__device__ __forceinline__ void square(typename UT::U &x, const typename UT::K &kc) {
    const typename UT::U t = x;
    UT::Ops::mul(x, t, kc);
}
// x^(|F| - 2); x != 0 in every coefficient / slot
template <class UT>
__device__ __forceinline__ typename UT::U fermat(const typename UT::U &x, const typename UT::K &kc) {
    using U = typename UT::U;
    using X = Exponent<typename UT::T>;
    U u = x;
#pragma unroll 1
    for (int k = 1; k < kRun; k <<= 1) {  // u = x^(2^k - 1)  ->  x^(2^2k - 1)
        U t = u;
#pragma unroll 1
        for (int j = 0; j < k; j++) square<UT>(t, kc);
        UT::Ops::mul(u, t, kc);
    }
    U acc = x;
#pragma unroll 1
    for (int pos = X::kBits - 2; pos >= 0;) {
        const bool run = pos >= kRun - 1 && exponent_window<typename UT::T>(pos) == (1u << kRun) - 1;
        const int nsq = run ? kRun : 1;
        const bool by = run || ((X::word(pos >> 6) >> (pos & 63)) & 1);
#pragma unroll 1
        for (int j = 0; j < nsq; j++) square<UT>(acc, kc);
        if (by) {
            U m = x;
            UT::select(m, run ? kAll<UT> : 0u, u);  // by value: a conditional between two units would put both into scratch
            UT::Ops::mul(acc, m, kc);
        }
        pos -= nsq;
    }
    return acc;
}

// fn(integral_constant<I>), I = FROM .. 0
template <int FROM, class Fn>
__device__ __forceinline__ void down_from(Fn &&fn) {
    fn(std::integral_constant<int, FROM>{});
    if constexpr (FROM > 0) down_from<FROM - 1>(fn);
}

// One chunk: unit `at` (a word offset within the element) of the elements e0 .. e0 + C - 1, `ew` words apart; adds the wave's zero
// units to zc (wave-uniform).  Every lane of the wave gets here, live or not: the ballots see the whole wave.  A position a lane does
// not have (beyond n, or a lane beyond the last group) reads the last element instead -- in bounds, n >= 1 -- and takes one() by value;
// it counts nothing and stores nothing.
template <class UT, int C, bool HN>
__device__ __forceinline__ void chunk(uint64_t *out, const uint64_t *num, const uint64_t *den, const typename UT::K &kc, const typename UT::U &id,
                                      bool live, size_t e0, size_t n, size_t ew, size_t at, unsigned long long &zc) {
    using U = typename UT::U;
    U x[C], pre[C > 1 ? C : 1];
    unsigned zm[C];
    U acc;
#pragma unroll
    for (int i = 0; i < C; i++) {
        const bool have = live && e0 + i < n;
        x[i].template load<true>(den + (have ? e0 + i : n - 1) * ew + at);
        zm[i] = have ? UT::zeros(x[i]) : 0u;
        UT::select(x[i], have ? zm[i] : kAll<UT>, id);
#pragma unroll
        for (int c = 0; c < UT::NC; c++) zc += __popcll(__ballot((zm[i] >> c) & 1u));
        if (i == 0) {
            acc = x[0];
        } else {
            pre[i] = acc;
            UT::Ops::mul(acc, x[i], kc);
        }
    }
    U inv = fermat<UT>(acc, kc);
    U zero;
    UT::set_zero(zero);
    // unrolled by recursion, not by pragma: the body of a frog16 or goldilocks24 step is past the size at which the pragma is honoured,
    // and a walk that is a loop indexes x and pre at run time
    down_from<C - 1>([&](auto step) {
        constexpr int i = decltype(step)::value;
        const bool have = live && e0 + i < n;
        U o = inv, nm;
        if constexpr (i > 0) UT::Ops::mul(o, pre[i], kc);
        if constexpr (HN) nm.template load<true>(num + (have ? e0 + i : n - 1) * ew + at);
        if constexpr (i > 0) UT::Ops::mul(inv, x[i], kc);
        if constexpr (HN) UT::Ops::mul(o, nm, kc);
        UT::select(o, zm[i], zero);
        UT::leaves(o);
        if (have) o.store(out + (e0 + i) * ew + at);
    });
}

// lanes of the launch = groups x 2^lu units, group-major: the lanes of a wave own consecutive units of one chunk of elements
template <class UT, int C, bool HN>
__device__ __forceinline__ void walk(uint64_t *out, const uint64_t *num, const uint64_t *den, const typename UT::K &kc, const smle::One &one, size_t n,
                                     size_t groups, int lu, size_t ew, size_t uw, unsigned long long *zeros) {
    typename UT::U id;
    UT::Ops::set_one(id, one);
    unsigned long long zc = 0;
    const size_t lanes = groups << lu, umask = ((size_t)1 << lu) - 1, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t base = blockIdx.x * (size_t)blockDim.x; base < lanes; base += stride) {  // the same trips for every lane of a workgroup
        const size_t flat = base + threadIdx.x, g = flat >> lu, c = flat & umask;
        chunk<UT, C, HN>(out, num, den, kc, id, g < groups, g * C, n, ew, c * uw, zc);
    }
    if ((threadIdx.x & 63u) == 0 && zc) atomicAdd(zeros, zc);
}

// pair: every buffer of the launch is 16-byte aligned and k >= 1 (one-limb fields)
template <class F, int C, bool HN>
__global__ __launch_bounds__(256) void inverse_kernel(uint64_t *out, const uint64_t *num, const uint64_t *den, smle::One one, size_t n, size_t groups,
                                                      int k, int pair, unsigned long long *zeros) {
    constexpr int SW = (int)sizeof(typename F::storage) / 8;
    const size_t ew = (size_t)SW << k;
    if constexpr (SW == 1) {
        if (pair) walk<PowUnit<F, 2>, C, HN>(out, num, den, 0, one, n, groups, k - 1, ew, 2, zeros);
        else walk<PowUnit<F, 1>, C, HN>(out, num, den, 0, one, n, groups, k, ew, 1, zeros);
    } else {
        walk<PowUnit<F, SW>, C, HN>(out, num, den, 0, one, n, groups, k, ew, SW, zeros);
    }
}
template <class SL, int C, bool HN>
__global__ __launch_bounds__(256) void slot_inverse_kernel(typename SL::K kc, uint64_t *out, const uint64_t *num, const uint64_t *den, smle::One one,
                                                           size_t n, size_t groups, unsigned long long *zeros) {
    walk<SlotUnit<SL>, C, HN>(out, num, den, kc, one, n, groups, SL::D / SL::W == 8 ? 3 : 2, SL::D, SL::W, zeros);
}

// ---- the plan: pure host arithmetic -------------------------------------------------------------------------------------------------
// Elements of a chunk, per family type T (a field or a slot type) and with or without numerators: the largest power of two whose kernel
// has no scratch within 128 VGPRs, four waves per SIMD (tests/test_inverse_isa.py holds the counts; DESIGN_APPENDIX.md A.20 the
// measurements).  VGPRs without / with numerators, the next chunk in brackets:
//   Goldilocks 8: 128 (16: 225) / 4: 82 (8: 130)     BabyBear 8: 94 (16: 174) / 8: 94 (16: 174)     Stark 4: 124 (8: 200) / 2: 96 (4: 132)
//   goldilocks24 4: 92 (8: 163) / 4: 96 (8: 165)     babybear72 2: 125 (4: 146) / 2: 128 (4: 152)     frog16 4: 120 (8: 188) / 4: 120 (8: 188)
template <class T, bool HN>
constexpr int kChunk = std::is_same<T, Goldilocks>::value ? (HN ? 4 : 8)
                       : std::is_same<T, BabyBear>::value ? 8
                       : std::is_same<T, Stark>::value    ? (HN ? 2 : 4)
                       : std::is_same<T, SlotB72>::value  ? 2
                                                          : 4;
template <bool HN>
inline int chunk_of(int ring) {
    switch (ring) {
        case 0: return kChunk<Goldilocks, HN>;
        case 1: return kChunk<BabyBear, HN>;
        case 2: return kChunk<Stark, HN>;
        case 3: return kChunk<SlotG24, HN>;
        case 4: return kChunk<SlotB72, HN>;
        default: return kChunk<SlotFrog, HN>;
    }
}
struct Plan {
    int launches = 0;
    size_t work_elems = 0, chunk_elems = 0;
};
inline bool plan(int ring, size_t n, bool has_num, Plan *p) {
    if (ring < 0 || ring > 5) return false;
    *p = Plan{};
    p->launches = n ? 1 : 0;
    p->chunk_elems = (size_t)(has_num ? chunk_of<true>(ring) : chunk_of<false>(ring));
    return true;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
// C0 = 0: the family's chunks.  Any other C0 is for the benchmarks (tools/ubench/inverse_bench.hip: chunk 1 is a Fermat inversion per unit).
template <class T, int C0 = 0>
inline hipError_t launch(const typename sumcheck::Family<T>::K &kc, uint64_t *out, const uint64_t *num, const uint64_t *den, const smle::One &one,
                         size_t n, int k, bool aligned, unsigned long long *zeros, hipStream_t s) {
    constexpr int CN = C0 ? C0 : kChunk<T, true>, CO = C0 ? C0 : kChunk<T, false>;
    if (n == 0) return hipSuccess;
    const size_t groups = num ? (n + CN - 1) / CN : (n + CO - 1) / CO;
    const sumcheck::Geometry ge = sumcheck::geometry_of<T>(k, aligned);
    const dim3 g(mle::blocks_for(groups << ge.lu)), b(256);
    if constexpr (sumcheck::kSlot<T>) {
        if (num) hipLaunchKernelGGL((slot_inverse_kernel<T, CN, true>), g, b, 0, s, kc, out, num, den, one, n, groups, zeros);
        else hipLaunchKernelGGL((slot_inverse_kernel<T, CO, false>), g, b, 0, s, kc, out, num, den, one, n, groups, zeros);
    } else {
        if (num) hipLaunchKernelGGL((inverse_kernel<T, CN, true>), g, b, 0, s, out, num, den, one, n, groups, ge.k, ge.pair, zeros);
        else hipLaunchKernelGGL((inverse_kernel<T, CO, false>), g, b, 0, s, out, num, den, one, n, groups, ge.k, ge.pair, zeros);
    }
    return hipGetLastError();
}

}  // namespace inverse
}  // namespace sr
