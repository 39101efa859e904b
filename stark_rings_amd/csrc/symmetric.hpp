// Symmetric matrices of ring elements in CRT / NTT form, packed as the reference stores them: SymmetricMatrix<F>
// (crates/linear_algebra/src/symmetric_matrix.rs:14-92) is a Vec<Vec<F>> whose row i holds the i + 1 entries (i, 0) .. (i, i); here the
// rows are flattened, entry (i, j) with j <= i is ring element i (i + 1) / 2 + j.
//   Gram        out(i, j) = sum_{t < m} a[i][t] * a[j][t] over the rows of a dense n x m matrix: what SymmetricMatrix::from_par_fn
//               (symmetric_matrix.rs:76-90) yields for the inner-product closure |i, j| <s_i, s_j> (the closure is the caller's)
//   recompose   recompose_left_right_symmetric_matrix (crates/ring/src/balanced_decomposition/mod.rs:354-386): G^T M G for the gadget
//               matrix G = I_n (x) powers, out(i, j) = sum_{a, b < d} mat[(i d + a, j d + b)] * (powers[a] * powers[b])
// `*` is the slot product of the ring: mul_boundary of the base field for the fully split power-of-two rings (lane = slot, sums in
// SumOfProducts<F>), the Fq3 / Fq9 / Fq4 product for the reference's own rings (sums in SlotDot<SL>).  All sums are exact modular
// integers on canonical values, so the order of summation does not change a bit of the result.
//
// Gram, power-of-two rings: the register block of matmul_kernel (RB x CB outputs per lane, RB = 2 CB), both operands rows of A.  Row
// block bi needs the column blocks 0 .. 2 bi + 1, so the tiles of the lower triangle are numbered bi (bi + 1) + cb and no workgroup is
// launched above the diagonal; a tile on the diagonal masks its stores to j <= i.
// Gram, slot rings: the 2 x 2 LDS-staged block of slot_matmul_kernel over the triangular tile index bi (bi + 1) / 2 + bj.
// Few tiles over a long inner dimension (a handful of witness vectors): the inner dimension is cut into nsplit spans, workgroup
// (tile, span) writes a partial packed matrix into the caller's workspace and sum_parts_kernel adds them -- the scheme of
// slot_matvec_kernel / slot_sum_kernel with the caller's workspace in place of context scratch.  nsplit is host arithmetic on the
// shape alone (gram_plan), so the plan needs no device.
//
// Recompose: launch 1 writes the d^2 weights powers[a] * powers[b] into the workspace, launch 2 streams mat once -- one product per
// term against the weight.  The symmetric lookup (l > k reads (l, k)) only ever swaps inside the diagonal blocks i == j.
#pragma once
#include "frog_ring.hpp"
#include "mle.hpp"
#include "ntt_generic.hpp"
#include "small_linalg.hpp"
#include "small_rings.hpp"

namespace sr {
namespace symm {

SR_HD size_t packed_index(size_t i, size_t j) { return i * (i + 1) / 2 + j; }
// largest b with b (b + 1) / 2 <= t: the row of packed index t
__device__ __forceinline__ size_t tri_row(size_t t) {
    size_t b = (size_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while (b * (b + 1) / 2 > t) b--;
    while ((b + 1) * (b + 2) / 2 <= t) b++;
    return b;
}

// ---- Gram, power-of-two rings ---------------------------------------------------------------------------------------------------
// grid: (tile, span) major, slot chunk minor.  dst = out (nsplit == 1) or the workspace, span sp at dst + sp * packed elements.
template <class F, int RB, int CB>
__global__ __launch_bounds__(256) void gram_kernel(typename F::storage *dst, const typename F::storage *a, size_t n, size_t m, int k,
                                                   unsigned nsplit, size_t span) {
    static_assert(RB == 2 * CB, "tile numbering");
    const size_t d = (size_t)1 << k;
    const size_t chunks = (d + 255) >> 8;
    const size_t slot = (blockIdx.x % chunks) * (size_t)blockDim.x + threadIdx.x;
    const size_t unit = blockIdx.x / chunks, tile = unit / nsplit, sp = unit % nsplit;
    const size_t bi = tri_row(tile >> 1), cb = tile - bi * (bi + 1);  // tiles before row block bi: bi (bi + 1), an even number
    const size_t r0 = bi * RB, c0 = cb * CB;
    if (slot >= d || c0 >= n) return;
    const size_t t0 = sp * span, t1 = t0 + span < m ? t0 + span : m;
    SumOfProducts<F> acc[RB][CB];
#pragma unroll
    for (int r = 0; r < RB; r++)
#pragma unroll
        for (int c = 0; c < CB; c++) acc[r][c].init();
    for (size_t t = t0; t < t1; t++) {
        typename F::elem av[RB], bv[CB];
#pragma unroll
        for (int r = 0; r < RB; r++) av[r] = r0 + r < n ? F::load(a + (((r0 + r) * m + t) << k) + slot) : F::zero();
#pragma unroll
        for (int c = 0; c < CB; c++) bv[c] = c0 + c < n ? F::load(a + (((c0 + c) * m + t) << k) + slot) : F::zero();
#pragma unroll
        for (int r = 0; r < RB; r++)
#pragma unroll
            for (int c = 0; c < CB; c++) acc[r][c].fma(av[r], bv[c]);
    }
    const size_t packed = n * (n + 1) / 2;
    typename F::storage *o = dst + ((sp * packed) << k) + slot;
#pragma unroll
    for (int r = 0; r < RB; r++)
#pragma unroll
        for (int c = 0; c < CB; c++)
            if (r0 + r < n && c0 + c <= r0 + r) F::store(o + (packed_index(r0 + r, c0 + c) << k), acc[r][c].finish());
}

// out[i] = sum_sp part[sp * total + i] over the `total` coefficients of a packed matrix
template <class F>
__global__ __launch_bounds__(256) void sum_parts_kernel(typename F::storage *out, const typename F::storage *part, size_t total, unsigned nsplit) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        typename F::elem sum = F::load(part + i);
        for (unsigned sp = 1; sp < nsplit; sp++) sum = F::add(sum, F::load(part + sp * total + i));
        F::store(out + i, sum);
    }
}

// ---- Gram, slot rings -------------------------------------------------------------------------------------------------------------
// slot_matmul_kernel with A on both sides: lane t = (output o = t / 64, term group g, slot s); per step of G inner indices the 2 x G
// elements of rows i0, i0 + 1 and of rows j0, j0 + 1 go through LDS once.  blockIdx.x = tile * nsplit + span.
template <class SL>
__global__ __launch_bounds__(256) void slot_gram_kernel(typename SL::K k, uint64_t *dst, const uint64_t *a, size_t n, size_t m, unsigned nsplit,
                                                        size_t span) {
    using E = typename SL::F::elem;
    constexpr int S = SL::D / SL::W, G = 64 / S, D = SL::D, W = SL::W;
    static_assert(64 % S == 0, "slot layout");
    __shared__ E lds[4 * G * D > 256 * W ? 4 * G * D : 256 * W];  // [rows i0, i0 + 1: 2 x G elements | rows j0, j0 + 1], then the partial sums
    const size_t tile = blockIdx.x / nsplit, sp = blockIdx.x % nsplit;
    const size_t bi = tri_row(tile), bj = tile - bi * (bi + 1) / 2;
    const size_t i0 = bi * 2, j0 = bj * 2;
    const int t = threadIdx.x, o = t >> 6, u = t & 63, g = u / S, s = u % S;
    const int oi = o >> 1, oj = o & 1;
    const size_t e0 = sp * span, e1 = e0 + span < m ? e0 + span : m;
    E x[W], z[W], res[W];
    SlotDot<SL> acc;
    acc.init();
    for (size_t t0 = e0; t0 < e1; t0 += G) {
        __syncthreads();  // the previous step's reads are done
        for (int idx = t; idx < 4 * G * D; idx += 256) {
            const int el = idx / D, w = idx % D, side = el / (2 * G), q = el % (2 * G);
            const size_t row = (side ? j0 : i0) + q / G, tt = t0 + q % G;
            E val = SL::F::zero();
            if (row < n && tt < e1) val = SL::F::load(a + (row * m + tt) * D + w);
            lds[idx] = val;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < W; q++) {
            x[q] = lds[(oi * G + g) * D + s * W + q];
            z[q] = lds[((2 + oj) * G + g) * D + s * W + q];
        }
        acc.fma(x, z);  // terms beyond the span were loaded as zero
    }
    acc.finish(res, k);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < W; q++) lds[((o * G + g) * S + s) * W + q] = res[q];
    __syncthreads();
    const size_t ii = i0 + oi, jj = j0 + oj;
    if (ii < n && jj <= ii) {
        uint64_t *y = dst + (sp * (n * (n + 1) / 2) + packed_index(ii, jj)) * D;
        for (int c = u; c < D; c += 64) {
            E sum = lds[(o * G) * D + c];
            for (int gg = 1; gg < G; gg++) sum = SL::F::add(sum, lds[(o * G + gg) * D + c]);
            SL::F::store(y + c, sum);
        }
    }
}

// ---- recompose -----------------------------------------------------------------------------------------------------------------
// w[a d + b] = powers[a] * powers[b]: d^2 elements, lane = coefficient
template <class F>
__global__ __launch_bounds__(256) void weights_kernel(typename F::storage *w, const typename F::storage *powers, size_t d, int k) {
    const size_t total = (d * d) << k, dm = ((size_t)1 << k) - 1;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t e = i >> k, c = i & dm, pa = e / d, pb = e % d;
        F::store(w + i, F::mul_boundary(F::load(powers + (pa << k) + c), F::load(powers + (pb << k) + c)));
    }
}
template <class SL>
__global__ __launch_bounds__(256) void slot_weights_kernel(typename SL::K k, uint64_t *w, const uint64_t *powers, size_t d) {
    using E = typename SL::F::elem;
    constexpr int W = SL::W, S = SL::D / SL::W;
    const size_t total = d * d * S;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t e = i / S, pa = e / d, pb = e % d;
        const int off = (int)(i % S) * W;
        E x[W], y[W];
        slot_load<SL>(x, powers + pa * SL::D + off);
        slot_load<SL>(y, powers + pb * SL::D + off);
        SL::mul(x, y, k);
        slot_store<SL>(w + i * W, x);
    }
}
// the packed position of mat[(k, l)]
SR_HD size_t sym_index(size_t k, size_t l) { return l <= k ? packed_index(k, l) : packed_index(l, k); }

// Lane = RW raw words of one output element (mle::Lane: a 16-byte pair of coefficients of a one-limb field where the buffers are
// aligned, one coefficient otherwise, one Stark coefficient); grid: output element major, unit chunk minor.  mat is read once
// (non-temporal), the d^2 weights by every workgroup.  FA: the field the sums run on (StarkL for Stark contexts on lazy limbs).
template <class F, class FA, int RW>
__device__ __forceinline__ void recompose_units(uint64_t *out, const uint64_t *mat, const uint64_t *w, size_t n, size_t d, int lu) {
    using L = mle::Lane<F, RW>;
    using SA = typename FA::storage;
    const size_t units = (size_t)1 << lu, chunks = (units + 255) >> 8;
    const size_t c = (blockIdx.x % chunks) * (size_t)blockDim.x + threadIdx.x, e = blockIdx.x / chunks;
    if (c >= units) return;
    const size_t i = tri_row(e), j = e - i * (i + 1) / 2;
    SumOfProducts<FA> acc[L::NC];
#pragma unroll
    for (int q = 0; q < L::NC; q++) acc[q].init();
    for (size_t pa = 0; pa < d; pa++)
        for (size_t pb = 0; pb < d; pb++) {
            L x, y;
            x.template load<true>(mat + ((sym_index(i * d + pa, j * d + pb) << lu) + c) * RW);
            y.template load<false>(w + (((pa * d + pb) << lu) + c) * RW);
#pragma unroll
            for (int q = 0; q < L::NC; q++) acc[q].fma(FA::load(reinterpret_cast<const SA *>(x.w) + q), FA::load(reinterpret_cast<const SA *>(y.w) + q));
        }
    L r;
#pragma unroll
    for (int q = 0; q < L::NC; q++) FA::store(reinterpret_cast<SA *>(r.w) + q, acc[q].finish());
    r.store(out + ((e << lu) + c) * RW);
}
template <class F, class FA>
__global__ __launch_bounds__(256) void recompose_kernel(uint64_t *out, const uint64_t *mat, const uint64_t *w, size_t n, size_t d, int k, int pair) {
    if constexpr (sizeof(typename F::storage) == 8) {
        if (pair) recompose_units<F, FA, 2>(out, mat, w, n, d, k - 1);
        else recompose_units<F, FA, 1>(out, mat, w, n, d, k);
    } else {
        recompose_units<F, FA, (int)sizeof(typename F::storage) / 8>(out, mat, w, n, d, k);
    }
}
// one workgroup per output element: lane (term group g, slot s) takes every G-th of the d^2 terms, the partial sums meet in LDS
template <class SL>
__global__ __launch_bounds__(256) void slot_recompose_kernel(typename SL::K k, uint64_t *out, const uint64_t *mat, const uint64_t *w, size_t n, size_t d) {
    using E = typename SL::F::elem;
    constexpr int S = SL::D / SL::W, G = 256 / S;
    static_assert(256 % S == 0 && SL::D <= 256, "slot layout");
    __shared__ E lds[256 * SL::W];
    const size_t e = blockIdx.x, i = tri_row(e), j = e - i * (i + 1) / 2;
    const int g = threadIdx.x / S, s = threadIdx.x % S;
    E x[SL::W], z[SL::W], res[SL::W];
    SlotDot<SL> acc;
    acc.init();
    for (size_t q = g; q < d * d; q += G) {
        const size_t pa = q / d, pb = q % d;
        slot_load<SL>(x, mat + sym_index(i * d + pa, j * d + pb) * SL::D + s * SL::W);
        slot_load<SL>(z, w + q * SL::D + s * SL::W);
        acc.fma(x, z);
    }
    acc.finish(res, k);
    slot_reduce_store<SL>(lds, res, out + e * SL::D);
}

// ---- the plans: pure host arithmetic ----------------------------------------------------------------------------------------------
// A launch is kept below 2^24 workgroups of 256 lanes (2^32 lanes).  kFillBlocks: four workgroups on each of 256 compute units; a
// Gram with fewer tiles than that cuts its inner dimension, at most kMaxSplit ways and never below kMinTerms inner indices per lane.
constexpr size_t kMaxBlocks = 0xFFFFFFull, kFillBlocks = 1024, kMinTerms = 4;  // slot rings: per lane and span, as slot_matvec_splits
constexpr unsigned kMaxSplit = 64;

inline bool mul_overflows(size_t a, size_t b, size_t *out) {
    if (a && b > (size_t)-1 / a) return true;
    *out = a * b;
    return false;
}
// n (n + 1) / 2; false when it does not fit a size_t
inline bool packed_elems(size_t n, size_t *out) {
    if (n == (size_t)-1) return false;
    return !(n & 1 ? mul_overflows(n, (n + 1) / 2, out) : mul_overflows(n / 2, n + 1, out));
}
// The register block of a Gram lane: matmul_dev's 8 x 4 for BabyBear (one register per sum) and 4 x 2 for Goldilocks (96-bit sums);
// Stark's 4 x 2 needs 184 VGPRs (140 on lazy limbs), 2 x 1 keeps it at 72 (59), within the four waves per SIMD of 256-lane workgroups
// (tests/test_symm_isa.py holds the counts)
template <class F> struct GramBlock {
    static constexpr int RB = std::is_same<F, BabyBear>::value ? 8 : std::is_same<F, Goldilocks>::value ? 4 : 2, CB = RB / 2;
};
struct RingShape {
    bool pow2;
    size_t degree;
    size_t chunks;    // workgroups per element (power-of-two rings)
    int rb;           // rows of a Gram tile
    size_t min_span;  // inner indices a span of a split Gram holds at least
};
// ring: enum sr_ring of include/stark_rings_hip.h.  A power-of-two lane walks its span alone (64 terms at least); a slot-ring
// workgroup takes G = 64 / S indices per step.
inline RingShape ring_shape(int ring, int k) {
    const size_t d = (size_t)1 << k;
    switch (ring) {
        case 0: return {true, d, (d + 255) >> 8, GramBlock<Goldilocks>::RB, 64};
        case 1: return {true, d, (d + 255) >> 8, GramBlock<BabyBear>::RB, 64};
        case 2: return {true, d, (d + 255) >> 8, GramBlock<Stark>::RB, 64};
        case 3: return {false, SlotG24::D, 1, 2, kMinTerms * 64 / (SlotG24::D / SlotG24::W)};
        case 4: return {false, SlotB72::D, 1, 2, kMinTerms * 64 / (SlotB72::D / SlotB72::W)};
        default: return {false, SlotFrog::D, 1, 2, kMinTerms * 64 / (SlotFrog::D / SlotFrog::W)};
    }
}
struct GramPlan {
    size_t packed = 0, tiles = 0, span = 0, work_elems = 0;
    unsigned nsplit = 1;
    int launches = 0;
};
inline bool gram_plan(int ring, int k, size_t n, size_t m, GramPlan *p) {
    *p = GramPlan{};
    if (ring < 0 || ring > 5 || !packed_elems(n, &p->packed)) return false;
    if (n == 0) return true;
    const RingShape sh = ring_shape(ring, k);
    const size_t nb = (n + sh.rb - 1) / sh.rb;
    if (nb > kMaxBlocks) return false;
    p->tiles = sh.pow2 ? nb * (nb + 1) : nb * (nb + 1) / 2;
    size_t blocks;
    if (mul_overflows(p->tiles, sh.chunks, &blocks) || blocks > kMaxBlocks) return false;
    size_t want = blocks >= kFillBlocks ? 1 : (kFillBlocks + blocks - 1) / blocks;
    if (want > m / sh.min_span) want = m / sh.min_span;
    if (want > kMaxSplit) want = kMaxSplit;
    if (want < 1) want = 1;
    p->span = (m + want - 1) / want;
    p->nsplit = m ? (unsigned)((m + p->span - 1) / p->span) : 1;  // no empty span
    p->launches = p->nsplit > 1 ? 2 : 1;
    if (p->nsplit > 1 && mul_overflows(p->packed, p->nsplit, &p->work_elems)) return false;
    return true;
}
struct RecomposePlan {
    size_t packed_in = 0, packed_out = 0, work_elems = 0;
    int launches = 0;
};
// false: d == 0 (the reference divides by it), an overflowing size or a grid past one launch's limit
inline bool recompose_plan(int ring, int k, size_t n, size_t d, RecomposePlan *p) {
    *p = RecomposePlan{};
    size_t nd, dd, blocks;
    if (ring < 0 || ring > 5 || d == 0 || mul_overflows(n, d, &nd) || !packed_elems(nd, &p->packed_in) || !packed_elems(n, &p->packed_out)) return false;
    if (n == 0) return true;
    const RingShape sh = ring_shape(ring, k);
    if (mul_overflows(d, d, &dd) || mul_overflows(dd, sh.degree, &blocks)) return false;  // the weights: lanes walk a grid-stride loop
    if (mul_overflows(p->packed_out, sh.chunks, &blocks) || blocks > kMaxBlocks) return false;
    p->work_elems = dd;
    p->launches = 2;
    return true;
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------
// F: the field of the storage; FA: the field the sums of products run on
template <class F, class FA>
inline hipError_t launch_gram(const GramPlan &p, uint64_t *out, const uint64_t *a, size_t n, size_t m, int k, uint64_t *work, hipStream_t s) {
    using S = typename FA::storage;
    constexpr int RB = GramBlock<F>::RB, CB = GramBlock<F>::CB;
    const size_t chunks = (((size_t)1 << k) + 255) >> 8;
    uint64_t *dst = p.nsplit > 1 ? work : out;
    hipLaunchKernelGGL((gram_kernel<FA, RB, CB>), dim3((unsigned)(p.tiles * p.nsplit * chunks)), dim3(256), 0, s, reinterpret_cast<S *>(dst),
                       reinterpret_cast<const S *>(a), n, m, k, p.nsplit, p.span);
    if (p.nsplit > 1) {
        using SF = typename F::storage;
        const size_t total = p.packed << k;
        hipLaunchKernelGGL((sum_parts_kernel<F>), dim3(mle::blocks_for(total)), dim3(256), 0, s, reinterpret_cast<SF *>(out),
                           reinterpret_cast<const SF *>(work), total, p.nsplit);
    }
    return hipGetLastError();
}
template <class SL>
inline hipError_t launch_slot_gram(const typename SL::K &kc, const GramPlan &p, uint64_t *out, const uint64_t *a, size_t n, size_t m, uint64_t *work,
                                   hipStream_t s) {
    hipLaunchKernelGGL((slot_gram_kernel<SL>), dim3((unsigned)(p.tiles * p.nsplit)), dim3(256), 0, s, kc, p.nsplit > 1 ? work : out, a, n, m, p.nsplit,
                       p.span);
    if (p.nsplit > 1) {
        const size_t total = p.packed * SL::D;
        hipLaunchKernelGGL((sum_parts_kernel<typename SL::F>), dim3(mle::blocks_for(total)), dim3(256), 0, s, out, work, total, p.nsplit);
    }
    return hipGetLastError();
}
template <class F, class FA>
inline hipError_t launch_recompose(const RecomposePlan &p, uint64_t *out, const uint64_t *mat, const uint64_t *powers, size_t n, size_t d, int k,
                                   uint64_t *work, bool aligned, hipStream_t s) {
    using S = typename F::storage;
    hipLaunchKernelGGL((weights_kernel<F>), dim3(mle::blocks_for((d * d) << k)), dim3(256), 0, s, reinterpret_cast<S *>(work),
                       reinterpret_cast<const S *>(powers), d, k);
    const int pair = sizeof(S) == 8 && k >= 1 && aligned;
    const size_t units = (size_t)1 << (pair ? k - 1 : k), chunks = (units + 255) >> 8;
    hipLaunchKernelGGL((recompose_kernel<F, FA>), dim3((unsigned)(p.packed_out * chunks)), dim3(256), 0, s, out, mat, work, n, d, k, pair);
    return hipGetLastError();
}
template <class SL>
inline hipError_t launch_slot_recompose(const typename SL::K &kc, const RecomposePlan &p, uint64_t *out, const uint64_t *mat, const uint64_t *powers,
                                        size_t n, size_t d, uint64_t *work, hipStream_t s) {
    hipLaunchKernelGGL((slot_weights_kernel<SL>), dim3(mle::blocks_for(d * d * (SL::D / SL::W))), dim3(256), 0, s, kc, work, powers, d);
    hipLaunchKernelGGL((slot_recompose_kernel<SL>), dim3((unsigned)p.packed_out), dim3(256), 0, s, kc, out, mat, work, n, d);
    return hipGetLastError();
}

}  // namespace symm
}  // namespace sr
