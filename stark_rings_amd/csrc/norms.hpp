// Norms of a flat slice of base-field coefficients, per group of `group` consecutive coefficients --
//   WithLinfNorm::linf_norm / WithL2Norm::l2_norm_squared over [Fq]   crates/ring/src/traits.rs:6-36
//   per element: |signed representative|, its square                   balanced_decomposition/convertible_ring.rs:49-66
//   signed representative                                              fq_convertible.rs:20-34 (Fp64), stark_prime/decomposition.rs:40-52
// A coefficient leaves Montgomery form and becomes sign + magnitude (dec::Mag<F>, the step the decomposition starts with; the sign is
// dropped); linf = max |s| and l2sq = sum s^2 are exact integers, so every order of combining partial results gives the same bits:
// nothing here depends on the grid, the schedule or the workspace's previous contents.
//
// A RECORD is what one group produces and what every partial result looks like: [linf: LW words][l2sq: SW words], little-endian u64
// words of the standard-form integer, only the parts `which` asks for.
//   one-limb fields (Goldilocks, BabyBear, Frog): LW = 1; s^2 < 2^126 and at most 2^64 coefficients: l2sq < 2^190, SW = 3
//   Stark: LW = 4; |s| <= (p - 1) / 2 < 2^251, s^2 < 2^502: l2sq < 2^566, SW = 9
//
// Two shapes (plan() decides, sr_norm_plan reports):
//   WIDE    group >= kWideMin.  A group is cut into B contiguous spans, one workgroup each; the workgroup reduces per lane, per wave
//           (cross-lane exchange) and through LDS, and writes ONE record with plain stores: to the output when B = 1, else to the
//           workspace, where a second launch (fold_kernel) combines the B records of each group.  One-limb fields read 16 bytes per
//           lane, non-temporal, kUnroll loads in flight; a group that starts on an odd word has a one-coefficient head, an odd rest a tail.
//   NARROW  group < kWideMin.  L = 2^floor(log2 min(group, 64)) lanes share a group, 64 / L neighbouring groups a wave: the wave reads
//           one contiguous span, reduces within each set of L lanes, and the first lane of a set writes the group's record.  One launch.
#pragma once
#include <type_traits>

#include "decompose.hpp"
#include "fields.hpp"

namespace sr {
namespace norms {

enum { LINF = 1, L2SQ = 2 };
typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));

template <class F> constexpr bool kOneLimb = sizeof(typename F::storage) == 8;
template <class F> constexpr int kLinfWords = kOneLimb<F> ? 1 : 4;
template <class F> constexpr int kL2Words = kOneLimb<F> ? 3 : 9;
// the accumulators are as wide as the records, so no lane, wave or workgroup can overflow one whatever share of the slice it is handed:
// bits of s^2, plus 64 for the largest coefficient count a size_t holds, against the bits of the l2sq words
static_assert(126 + 64 <= 64 * kL2Words<Goldilocks> && 126 + 64 <= 64 * kL2Words<Frog> && 60 + 64 <= 64 * kL2Words<BabyBear>,
              "one-limb l2sq accumulator");
static_assert(502 + 64 <= 64 * kL2Words<Stark>, "Stark l2sq accumulator");

template <class F, int W>
struct Rec {
    static constexpr int NL = (W & LINF) ? kLinfWords<F> : 0, NS = (W & L2SQ) ? kL2Words<F> : 0, WORDS = NL + NS;
    uint64_t w[WORDS];
    SR_HD void zero() {
#pragma unroll
        for (int i = 0; i < WORDS; i++) w[i] = 0;
    }
    // max of the linf parts (compared from the top word), sum with carry of the l2sq parts
    SR_HD void combine(const Rec &o) {
        if constexpr (NL == 1) {
            w[0] = o.w[0] > w[0] ? o.w[0] : w[0];
        } else if constexpr (NL > 1) {
            bool gt = false, lt = false;
#pragma unroll
            for (int i = NL - 1; i >= 0; i--) {
                const bool open = !(gt | lt);
                gt |= open & (o.w[i] > w[i]);
                lt |= open & (o.w[i] < w[i]);
            }
#pragma unroll
            for (int i = 0; i < NL; i++) w[i] = gt ? o.w[i] : w[i];
        }
        uint64_t c = 0;
#pragma unroll
        for (int i = NL; i < WORDS; i++) {
            const uint64_t t = w[i] + c, u = t + o.w[i];
            c = (uint64_t)(t < c) + (uint64_t)(u < t);  // at most one of the two
            w[i] = u;
        }
    }
    SR_HD void load(const uint64_t *p) {
#pragma unroll
        for (int i = 0; i < WORDS; i++) w[i] = p[i];
    }
    SR_HD void store(uint64_t *p) const {
#pragma unroll
        for (int i = 0; i < WORDS; i++) p[i] = w[i];
    }
};

// ---- one coefficient into a lane's accumulator ------------------------------------------------------------------------------------
// one-limb fields: the accumulator is the record itself
template <class F, int W>
struct Acc {
    Rec<F, W> r;
    SR_HD void zero() { r.zero(); }
    SR_HD void take(typename F::elem img) {
        const uint64_t m = dec::Mag<F>::from_image(img).m;  // <= (p - 1) / 2 < 2^63
        if constexpr ((W & LINF) != 0) r.w[0] = m > r.w[0] ? m : r.w[0];
        if constexpr ((W & L2SQ) != 0) {
            uint64_t lo, hi;
            if constexpr (std::is_same<F, BabyBear>::value) {  // m < 2^30: one product
                lo = (uint64_t)(uint32_t)m * (uint32_t)m;
                hi = 0;
            } else {  // m = a1 2^32 + a0, a1 < 2^31: m^2 = a0^2 + a0 a1 2^33 + a1^2 2^64, three 32 x 32 -> 64-bit products
                const uint32_t a0 = (uint32_t)m, a1 = (uint32_t)(m >> 32);
                const uint64_t p00 = (uint64_t)a0 * a0, p01 = (uint64_t)a0 * a1, p11 = (uint64_t)a1 * a1;
                lo = p00 + (p01 << 33);
                hi = p11 + (p01 >> 31) + (uint64_t)(lo < p00);  // < 2^62
            }
            uint64_t *s = r.w + Rec<F, W>::NL;
            s[0] += lo;
            const uint64_t t = s[1] + hi, u = t + (uint64_t)(s[0] < lo);
            s[2] += (uint64_t)(t < hi) + (uint64_t)(u < t);
            s[1] = u;
        }
    }
    SR_HD Rec<F, W> rec() const { return r; }
};
// a^2 of eight 32-bit limbs as sixteen: the 28 products above the diagonal once (operand scanning: limb + product + carry fits 64
// bits), doubled by a one-bit shift, plus the eight squares on the diagonal
SR_HD void square_limbs(const uint32_t a[8], uint32_t r[16]) {
    uint32_t t[16];
#pragma unroll
    for (int i = 0; i < 16; i++) t[i] = 0;
#pragma unroll
    for (int i = 0; i < 7; i++) {
        uint64_t c = 0;
#pragma unroll
        for (int j = i + 1; j < 8; j++) {
            const uint64_t uv = (uint64_t)a[i] * a[j] + t[i + j] + c;
            t[i + j] = (uint32_t)uv;
            c = uv >> 32;
        }
        t[i + 8] = (uint32_t)c;
    }
    uint32_t top = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const uint32_t x = t[i];
        t[i] = (x << 1) | top;
        top = x >> 31;
    }
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint64_t d = (uint64_t)a[i] * a[i];
        c += (uint64_t)t[2 * i] + (uint32_t)d;
        r[2 * i] = (uint32_t)c;
        c >>= 32;
        c += (uint64_t)t[2 * i + 1] + (d >> 32);
        r[2 * i + 1] = (uint32_t)c;
        c >>= 32;
    }
}
// Stark: 32-bit limbs while accumulating (the carry chains of fields.hpp), u64 words in the record
template <int W>
struct Acc<Stark, W> {
    U256 mx;
    uint32_t sm[18];
    SR_HD void zero() {
        mx = Stark::zero();
#pragma unroll
        for (int i = 0; i < 18; i++) sm[i] = 0;
    }
    SR_HD void take(const U256 &img) {
        const U256 m = dec::Mag<Stark>::from_image(img).m;
        if constexpr ((W & LINF) != 0) {
            U256 d;
            if (Stark::sub_raw(d, mx, m)) mx = m;  // borrow: mx < m
        }
        if constexpr ((W & L2SQ) != 0) {
            uint32_t sq[16];
            square_limbs(m.l, sq);
            uint64_t c = 0;
#pragma unroll
            for (int i = 0; i < 18; i++) {
                c += (uint64_t)sm[i] + (i < 16 ? sq[i] : 0u);
                sm[i] = (uint32_t)c;
                c >>= 32;
            }
        }
    }
    SR_HD Rec<Stark, W> rec() const {
        Rec<Stark, W> r;
        if constexpr ((W & LINF) != 0) {
#pragma unroll
            for (int i = 0; i < 4; i++) r.w[i] = (uint64_t)mx.l[2 * i] | ((uint64_t)mx.l[2 * i + 1] << 32);
        }
        if constexpr ((W & L2SQ) != 0) {
#pragma unroll
            for (int i = 0; i < 9; i++) r.w[Rec<Stark, W>::NL + i] = (uint64_t)sm[2 * i] | ((uint64_t)sm[2 * i + 1] << 32);
        }
        return r;
    }
};

#if defined(__HIPCC__)
// ---- cross-lane and workgroup reduction -------------------------------------------------------------------------------------------
// every lane of the wave ends with the combination over its set of `lanes` neighbours (a power of two, at most 64)
template <class R>
__device__ __forceinline__ void reduce_lanes(R &r, int lanes) {
    for (int m = lanes >> 1; m > 0; m >>= 1) {
        R o;
#pragma unroll
        for (int i = 0; i < R::WORDS; i++) o.w[i] = __shfl_xor((unsigned long long)r.w[i], m);
        r.combine(o);
    }
}
constexpr int kMaxWaves = 16;  // of a workgroup (1024 lanes)
// the record of the whole workgroup, valid in lane 0 of wave 0; `lds` holds kMaxWaves records and is free again on return
template <class R>
__device__ __forceinline__ void reduce_block(R &r, uint64_t *lds) {
    reduce_lanes(r, 64);
    const int wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    if ((threadIdx.x & 63) == 0) r.store(lds + wave * R::WORDS);
    __syncthreads();
    if (threadIdx.x == 0)
        for (int i = 1; i < nw; i++) {
            R o;
            o.load(lds + i * R::WORDS);
            r.combine(o);
        }
    __syncthreads();
}

// ---- loads: d_coeffs is 8-byte aligned only.  A Stark coefficient is read as four non-temporal words, which the compiler issues as two
// 16-byte loads (global memory takes them at any dword alignment) -----------------------------------------------------------------
template <class F>
__device__ __forceinline__ typename F::elem load_coeff(const uint64_t *p) {
    if constexpr (kOneLimb<F>) {
        const uint64_t v = __builtin_nontemporal_load(p);
        return F::load(reinterpret_cast<const typename F::storage *>(&v));
    } else {
        U256 e;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint64_t q = __builtin_nontemporal_load(p + i);
            e.l[2 * i] = (uint32_t)q;
            e.l[2 * i + 1] = (uint32_t)(q >> 32);
        }
        return e;
    }
}

// loads in flight per lane of the wide kernel: eight 16-byte pairs of a one-limb field, two Stark coefficients
template <class F> constexpr int kUnroll = kOneLimb<F> ? 8 : 2;
// coefficients one lane-load covers
template <class F> constexpr int kPerLoad = kOneLimb<F> ? 2 : 1;
constexpr size_t kWideMin = 1024;       // smallest group the wide shape takes
constexpr size_t kMaxParts = 1 << 15;   // partial records of one call at most (B > 1): bounds the workspace and the second launch
constexpr unsigned kMaxGrid = 0xFFFFFFu;

// WIDE: unit u = g * parts + b is span b of group g; its record goes to dst + u * WORDS (the output itself when parts = 1)
template <class F, int W>
__global__ __launch_bounds__(256) void wide_kernel(uint64_t *dst, const uint64_t *coeffs, size_t group, size_t n_groups, size_t parts) {
    using R = Rec<F, W>;
    constexpr int LIMBS = kOneLimb<F> ? 1 : 4, U = kUnroll<F>;
    __shared__ uint64_t lds[kMaxWaves * R::WORDS];
    const size_t units = n_groups * parts;
    for (size_t u = blockIdx.x; u < units; u += gridDim.x) {
        const size_t g = u / parts, b = u - g * parts;
        const uint64_t *p = coeffs + g * group * LIMBS;
        Acc<F, W> acc;
        acc.zero();
        if constexpr (kOneLimb<F>) {
            // [head: one coefficient when p is not 16-byte aligned][pairs][tail: one coefficient when what is left is odd]
            const size_t head = ((uintptr_t)p >> 3) & 1, pairs = (group - head) >> 1, tail = (group - head) & 1;
            const size_t per = (pairs + parts - 1) / parts, first = b * per, last = first + per < pairs ? first + per : pairs;
            const u64x2 *q = reinterpret_cast<const u64x2 *>(p + head);
            for (size_t i = first + threadIdx.x; i < last; i += 256 * U) {
                u64x2 v[U];
#pragma unroll
                for (int t = 0; t < U; t++) {
                    const size_t j = i + (size_t)t * 256;
                    v[t] = j < last ? __builtin_nontemporal_load(q + j) : u64x2{0, 0};  // zero is the image of 0
                }
#pragma unroll
                for (int t = 0; t < U; t++) {
                    const typename F::storage s[2] = {v[t].x, v[t].y};
                    acc.take(F::load(&s[0]));
                    acc.take(F::load(&s[1]));
                }
            }
            if (b == 0 && threadIdx.x == 0 && head) acc.take(load_coeff<F>(p));
            if (b == 0 && threadIdx.x == 1 && tail) acc.take(load_coeff<F>(p + group - 1));
        } else {
            const size_t per = (group + parts - 1) / parts, first = b * per, last = first + per < group ? first + per : group;
            for (size_t i = first + threadIdx.x; i < last; i += 256 * U) {
#pragma unroll
                for (int t = 0; t < U; t++) {
                    const size_t j = i + (size_t)t * 256;
                    if (j < last) acc.take(load_coeff<F>(p + j * LIMBS));
                }
            }
        }
        R r = acc.rec();
        reduce_block(r, lds);
        if (threadIdx.x == 0) r.store(dst + u * R::WORDS);
    }
}

// NARROW: `lanes` lanes per group (a power of two), 64 / lanes groups per wave
template <class F, int W>
__global__ __launch_bounds__(256) void narrow_kernel(uint64_t *out, const uint64_t *coeffs, size_t group, size_t n_groups, int lanes) {
    using R = Rec<F, W>;
    constexpr int LIMBS = kOneLimb<F> ? 1 : 4, U = kOneLimb<F> ? 4 : 2;
    const int lane = threadIdx.x & 63, per_wave = 64 / lanes, sub = lane / lanes, l = lane & (lanes - 1);
    const size_t tiles = (n_groups + per_wave - 1) / per_wave, waves = (size_t)gridDim.x * (blockDim.x >> 6);
    for (size_t tile = blockIdx.x * (size_t)(blockDim.x >> 6) + (threadIdx.x >> 6); tile < tiles; tile += waves) {
        const size_t g = tile * per_wave + sub;
        const bool live = g < n_groups;
        const uint64_t *p = coeffs + g * group * LIMBS;
        Acc<F, W> acc;
        acc.zero();
        for (size_t i = l; i < group; i += (size_t)lanes * U) {  // the same trips for every lane of a set; sets agree on `group`
            typename F::elem v[U];
#pragma unroll
            for (int t = 0; t < U; t++) {
                const size_t j = i + (size_t)t * lanes;
                v[t] = live && j < group ? load_coeff<F>(p + j * LIMBS) : F::zero();
            }
#pragma unroll
            for (int t = 0; t < U; t++) acc.take(v[t]);
        }
        R r = acc.rec();
        reduce_lanes(r, lanes);
        if (live && l == 0) r.store(out + g * R::WORDS);
    }
}

// second launch of a wide call with parts > 1: out record g = the combination of the `parts` records work[g * parts ..].
// parts <= 64: lanes = 2^ceil(log2 parts) lanes per group as in narrow_kernel; otherwise one workgroup per group.
template <class F, int W>
__global__ __launch_bounds__(1024) void fold_kernel(uint64_t *out, const uint64_t *work, size_t n_groups, size_t parts, int lanes) {
    using R = Rec<F, W>;
    __shared__ uint64_t lds[kMaxWaves * R::WORDS];
    if (lanes) {
        const int lane = threadIdx.x & 63, per_wave = 64 / lanes, sub = lane / lanes, l = lane & (lanes - 1);
        const size_t tiles = (n_groups + per_wave - 1) / per_wave, waves = (size_t)gridDim.x * (blockDim.x >> 6);
        for (size_t tile = blockIdx.x * (size_t)(blockDim.x >> 6) + (threadIdx.x >> 6); tile < tiles; tile += waves) {
            const size_t g = tile * per_wave + sub;
            R r;
            r.zero();
            if (g < n_groups && (size_t)l < parts) r.load(work + (g * parts + l) * R::WORDS);
            reduce_lanes(r, lanes);
            if (g < n_groups && l == 0) r.store(out + g * R::WORDS);
        }
        return;
    }
    for (size_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
        R r;
        r.zero();
        for (size_t i = threadIdx.x; i < parts; i += blockDim.x) {
            R o;
            o.load(work + (g * parts + i) * R::WORDS);
            r.combine(o);
        }
        reduce_block(r, lds);
        if (threadIdx.x == 0) r.store(out + g * R::WORDS);
    }
}
#endif  // __HIPCC__

// ---- the plan: pure host arithmetic -----------------------------------------------------------------------------------------------
struct Plan {
    size_t n_groups = 0, group = 0;
    size_t words_per_group = 0;
    bool wide = false;
    size_t parts = 1;  // wide: workgroups (and partial records, when > 1) per group
    int lanes = 1;     // narrow: lanes per group
    int launches = 1;
    size_t work_words = 0;
};
inline int pow2_floor(size_t v) {  // v >= 1
    int r = 1;
    while ((size_t)r * 2 <= v && r < 64) r *= 2;
    return r;
}
// limbs = u64 words per coefficient (1 or 4).  false: bad arguments (the caller names them).  An empty slice (l2sq only) is one
// group of no coefficients.  The partial records of a call number n_groups * parts <= max(n_groups, kMaxParts) when parts > 1, i.e.
// the workspace is at most kMaxParts records: 2^15 * 4 words = 1 MiB for a one-limb field, 2^15 * 13 words = 3.25 MiB for Stark.
inline bool plan(int limbs, size_t n_coeffs, size_t group, int which, Plan *p) {
    if (which < 1 || which > 3 || group == 0 || n_coeffs % group != 0 || (n_coeffs == 0 && (which & LINF))) return false;
    *p = Plan{};
    const bool one = limbs == 1;
    p->words_per_group = ((which & LINF) ? (one ? 1 : 4) : 0) + ((which & L2SQ) ? (one ? 3 : 9) : 0);
    p->n_groups = n_coeffs ? n_coeffs / group : 1;
    p->group = n_coeffs ? group : 0;
    p->wide = p->group >= kWideMin;
    if (p->wide) {
        const size_t loads = p->group / (one ? 2 : 1), chunk = 256 * (size_t)(one ? 8 : 2);  // kPerLoad, 256 lanes x kUnroll
        const size_t want = (loads + chunk - 1) / chunk, room = kMaxParts / p->n_groups;
        p->parts = want < room ? want : (room ? room : 1);
        if (p->parts > 1) {
            p->launches = 2;
            p->work_words = p->n_groups * p->parts * p->words_per_group;
        }
    } else {
        p->lanes = p->group ? pow2_floor(p->group) : 1;
    }
    return true;
}

#if defined(__HIPCC__)
template <class F, int W>
inline hipError_t launch_w(const Plan &p, uint64_t *out, const uint64_t *coeffs, uint64_t *work, hipStream_t s) {
    static_assert(kUnroll<F> * kPerLoad<F> * 256 == (kOneLimb<F> ? 4096 : 512), "plan() sizes the spans by the wide kernel's chunk");
    if (p.wide) {
        const size_t units = p.n_groups * p.parts;
        hipLaunchKernelGGL((wide_kernel<F, W>), dim3((unsigned)(units < kMaxGrid ? units : kMaxGrid)), dim3(256), 0, s, p.parts > 1 ? work : out,
                           coeffs, p.group, p.n_groups, p.parts);
        if (p.parts > 1) {
            int lanes = 0;
            if (p.parts <= 64) lanes = pow2_floor(p.parts) < (int)p.parts ? 2 * pow2_floor(p.parts) : (int)p.parts;
            const size_t blocks = lanes ? (p.n_groups + (size_t)(64 / lanes) * 4 - 1) / ((size_t)(64 / lanes) * 4) : p.n_groups;
            hipLaunchKernelGGL((fold_kernel<F, W>), dim3((unsigned)(blocks < kMaxGrid ? blocks : kMaxGrid)), dim3(lanes ? 256 : 1024), 0, s, out, work,
                               p.n_groups, p.parts, lanes);
        }
    } else {
        const size_t per_block = (size_t)(64 / p.lanes) * 4, blocks = (p.n_groups + per_block - 1) / per_block;
        hipLaunchKernelGGL((narrow_kernel<F, W>), dim3((unsigned)(blocks < kMaxGrid ? blocks : kMaxGrid)), dim3(256), 0, s, out, coeffs, p.group,
                           p.n_groups, p.lanes);
    }
    return hipGetLastError();
}
// the launches of `p` on stream s; `work` holds p.work_words words (unused when that is 0)
template <class F>
inline hipError_t launch(const Plan &p, int which, uint64_t *out, const uint64_t *coeffs, uint64_t *work, hipStream_t s) {
    switch (which) {
        case LINF: return launch_w<F, LINF>(p, out, coeffs, work, s);
        case L2SQ: return launch_w<F, L2SQ>(p, out, coeffs, work, s);
        case LINF | L2SQ: return launch_w<F, LINF | L2SQ>(p, out, coeffs, work, s);
        default: return hipErrorInvalidValue;
    }
}
#endif

}  // namespace norms
}  // namespace sr
