// Fraction trees: every layer of the binary tree that sums fractions p_i / q_i over a table of ring elements in CRT / NTT form without
// ever dividing -- the circuit of the layered (GKR) fractional sum-check behind logUp lookup and range arguments.  A node is a pair
// (p, q); layer 0 is the 2^n leaves, layer k (1 <= k <= n) has 2^(n-k) nodes, and a node combines its children (l, r) as
//   p = p_l * q_r + p_r * q_l        q = q_l * q_r
// with the children of prod_tree.hpp: (2i, 2i+1) in leading order, (i, i + half) in trailing order.  `*` is the slot product of the
// ring (sr_product_batch, sr_prod_tree), `+` the slot sum (sr_add_batch).  The q side alone is exactly the product tree of the q
// leaves, word for word.
//
// One launch produces J levels of both sides from the layer below them, with the groups, register order and output indexing of
// ptree::tree_units: a thread holds the 2^J numerators and 2^J denominators of its group, forms level after level in registers and
// stores every node's p and q to the level's own layer of the two planar outputs (the layout of prod_tree.hpp, each).  Per node
// t = p_u * q_{u+h}, then p_u = t + p_{u+h} * q_u, and only then q_u = q_u * q_{u+h}: the numerator needs the old q_u.
//
// Truncated leaves: input elements at or beyond n_in are the neutral fraction (zero(), one()) and are never loaded; a group whose
// first element is beyond n_in is neutral throughout.  HP = false (a call's first launch only, when no numerators are stored): every
// stored leaf has numerator one(), and nothing is read for it.  The general formula is applied all the same -- the first level's
// products by one() are not skipped: they are exact, and the kernel waits on memory, not on the vector pipe.
#pragma once
#include "prod_tree.hpp"

namespace sr {
namespace ftree {

using ptree::each_node;
using ptree::Node;
using ptree::rev;

// ---- power-of-two rings ---------------------------------------------------------------------------------------------------------
template <class F, int J, int RW, bool HP>
__device__ __forceinline__ void tree_units(uint64_t *pout, uint64_t *qout, const uint64_t *pin, const uint64_t *qin, const smle::One &one,
                                           size_t units, int lu, size_t n_in, int m, bool tr) {
    using L = mle::Lane<F, RW>;
    using Ops = smle::PowOps<F, F, RW>;
    const size_t gid = blockIdx.x * (size_t)blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    const size_t umask = ((size_t)1 << lu) - 1;
    const size_t sb = tr ? 1 : (size_t)1 << J, st = tr ? (size_t)1 << (m - J) : 1;
    L id;
    Ops::set_one(id, one);
    for (size_t i = gid; i < units; i += stride) {
        const size_t b = i >> lu, c = i & umask, base = b * sb;
        const bool live = base < n_in;  // else the whole group lies in the truncated (neutral) part of the table
        L p[1 << J], q[1 << J];
#pragma unroll
        for (int t = 0; t < (1 << J); t++) {
            const size_t e = base + (size_t)(tr ? t : rev(t, J)) * st;
            if (live && e < n_in) {
                const size_t at = ((e << lu) + c) * RW;
                q[t].template load<true>(qin + at);
                if constexpr (HP) p[t].template load<true>(pin + at);
                else p[t] = id;
            } else {
                q[t] = id;
                p[t].zero();
            }
        }
        // a neutral group takes the same path (0 * 1 + 0 * 1 = 0, 1 * 1 = 1): one set of stores, no branch around the arithmetic
        each_node<J>([&](auto node) {
            using N = Node<J, decltype(node)::value>;
            const size_t o = N::layer(m) + (tr ? b + (size_t)N::u * st : (b << N::lh) + (size_t)rev(N::u, N::lh));
            const size_t at = ((o << lu) + c) * RW;
            L t = p[N::u], s = p[N::u + N::h];
            Ops::mul(t, q[N::u + N::h], 0);
            Ops::mul(s, q[N::u], 0);
            Ops::add(t, s);
            p[N::u] = t;
            Ops::mul(q[N::u], q[N::u + N::h], 0);
            p[N::u].store(pout + at);
            q[N::u].store(qout + at);
        });
    }
}

// k = log2 D, m = log2 of the nodes of the input layer (m >= J).  The J levels are written in full behind `pout` and `qout`.
template <class F, int J, bool HP>
__global__ __launch_bounds__(256) void tree_kernel(typename F::storage *pout, typename F::storage *qout, const typename F::storage *pin,
                                                   const typename F::storage *qin, smle::One one, size_t n_in, int m, int tr, int k) {
    uint64_t *po = reinterpret_cast<uint64_t *>(pout), *qo = reinterpret_cast<uint64_t *>(qout);
    const uint64_t *pi = reinterpret_cast<const uint64_t *>(pin), *qi = reinterpret_cast<const uint64_t *>(qin);
    const size_t groups = (size_t)1 << (m - J);
    if constexpr (sizeof(typename F::storage) == 8) {
        // D >= 2: a pair of coefficients never straddles two elements, and every element starts on a 16-byte boundary when the buffer does
        const uintptr_t all = (uintptr_t)po | (uintptr_t)qo | (uintptr_t)qi | (HP ? (uintptr_t)pi : 0);
        if (k >= 1 && (all & 15u) == 0) tree_units<F, J, 2, HP>(po, qo, pi, qi, one, groups << (k - 1), k - 1, n_in, m, tr != 0);
        else tree_units<F, J, 1, HP>(po, qo, pi, qi, one, groups << k, k, n_in, m, tr != 0);
    } else {
        tree_units<F, J, (int)sizeof(typename F::storage) / 8, HP>(po, qo, pi, qi, one, groups << k, k, n_in, m, tr != 0);
    }
}

// ---- goldilocks24 / babybear72 / frog16 -----------------------------------------------------------------------------------------
// The one-slot-per-lane mapping of ptree::slot_tree_kernel.
template <class SL, int J, bool HP>
__global__ __launch_bounds__(256) void slot_tree_kernel(typename SL::K k, uint64_t *pout, uint64_t *qout, const uint64_t *pin,
                                                        const uint64_t *qin, smle::One one, size_t n_in, int m, int tr) {
    using Ops = smle::SlotOps<SL>;
    using U = typename Ops::U;
    using F = typename SL::F;
    constexpr int W = SL::W, S = SL::D / SL::W;
    const size_t slots = ((size_t)1 << (m - J)) * S;
    const size_t sb = tr ? 1 : (size_t)1 << J, st = tr ? (size_t)1 << (m - J) : 1;
    U id, zr;
    Ops::set_one(id, one);
#pragma unroll
    for (int w = 0; w < W; w++) zr.v[w] = F::zero();
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < slots; i += (size_t)gridDim.x * blockDim.x) {
        const size_t b = i / S, base = b * sb;
        const int off = (int)(i % S) * W;
        const bool live = base < n_in;
        U p[1 << J], q[1 << J];
        if (live) {
#pragma unroll
            for (int t = 0; t < (1 << J); t++) {
                const size_t e = base + (size_t)(tr ? t : rev(t, J)) * st;
                if (e < n_in) {
                    q[t].template load<true>(qin + e * SL::D + off);
                    if constexpr (HP) p[t].template load<true>(pin + e * SL::D + off);
                    else p[t] = id;
                } else {
                    q[t] = id;
                    p[t] = zr;
                }
            }
        }
        each_node<J>([&](auto node) {
            using N = Node<J, decltype(node)::value>;
            const size_t o = N::layer(m) + (tr ? b + (size_t)N::u * st : (b << N::lh) + (size_t)rev(N::u, N::lh));
            if (live) {
                U t = p[N::u], s = p[N::u + N::h];
                Ops::mul(t, q[N::u + N::h], k);
                Ops::mul(s, q[N::u], k);
                Ops::add(t, s);
                p[N::u] = t;
                Ops::mul(q[N::u], q[N::u + N::h], k);
                p[N::u].store(pout + o * SL::D + off);
                q[N::u].store(qout + o * SL::D + off);
            } else {  // a neutral group: no load and no slot product
                zr.store(pout + o * SL::D + off);
                id.store(qout + o * SL::D + off);
            }
        });
    }
}

// Levels one launch produces at most: the largest J <= 3 whose kernel has no scratch and stays within 128 VGPRs, i.e. four waves per
// SIMD for 256-lane workgroups (tests/test_frac_tree_isa.py holds the counts)
template <class F> constexpr int kMaxJ = std::is_same<F, BabyBear>::value ? 3 : 2;  // J = 3 needs 152 (Goldilocks), 173 (Stark)
template <class SL> constexpr int kSlotMaxJ = std::is_same<SL, SlotB72>::value ? 1 : 2;  // babybear72 J = 2 needs 144; J = 3: 130 (goldilocks24), 172 (frog16)

// ---- host side ------------------------------------------------------------------------------------------------------------------
template <class F, bool HP>
inline hipError_t launch_tree(int j, uint64_t *pout, uint64_t *qout, const uint64_t *pin, const uint64_t *qin, const smle::One &one, size_t n_in,
                              int m, bool tr, int k, hipStream_t s) {
    using S = typename F::storage;
    if (j < 1 || j > kMaxJ<F> || m < j) return hipErrorInvalidValue;
    const dim3 g(mle::blocks_for(mle::units_of<F>((size_t)1 << (m - j), k))), b(256);
    S *po = reinterpret_cast<S *>(pout), *qo = reinterpret_cast<S *>(qout);
    const S *pi = reinterpret_cast<const S *>(pin), *qi = reinterpret_cast<const S *>(qin);
    switch (j) {
        case 1: hipLaunchKernelGGL((tree_kernel<F, 1, HP>), g, b, 0, s, po, qo, pi, qi, one, n_in, m, (int)tr, k); break;
        case 2:
            if constexpr (kMaxJ<F> >= 2) hipLaunchKernelGGL((tree_kernel<F, 2, HP>), g, b, 0, s, po, qo, pi, qi, one, n_in, m, (int)tr, k);
            break;
        default:
            if constexpr (kMaxJ<F> >= 3) hipLaunchKernelGGL((tree_kernel<F, 3, HP>), g, b, 0, s, po, qo, pi, qi, one, n_in, m, (int)tr, k);
            break;
    }
    return hipGetLastError();
}
template <class SL, bool HP>
inline hipError_t launch_slot_tree(const typename SL::K &kc, int j, uint64_t *pout, uint64_t *qout, const uint64_t *pin, const uint64_t *qin,
                                   const smle::One &one, size_t n_in, int m, bool tr, hipStream_t s) {
    if (j < 1 || j > kSlotMaxJ<SL> || m < j) return hipErrorInvalidValue;
    const dim3 g(mle::blocks_for(((size_t)1 << (m - j)) * (SL::D / SL::W))), b(256);
    switch (j) {
        case 1: hipLaunchKernelGGL((slot_tree_kernel<SL, 1, HP>), g, b, 0, s, kc, pout, qout, pin, qin, one, n_in, m, (int)tr); break;
        case 2:
            if constexpr (kSlotMaxJ<SL> >= 2) hipLaunchKernelGGL((slot_tree_kernel<SL, 2, HP>), g, b, 0, s, kc, pout, qout, pin, qin, one, n_in, m, (int)tr);
            break;
        default:
            if constexpr (kSlotMaxJ<SL> >= 3) hipLaunchKernelGGL((slot_tree_kernel<SL, 3, HP>), g, b, 0, s, kc, pout, qout, pin, qin, one, n_in, m, (int)tr);
            break;
    }
    return hipGetLastError();
}

// ---- the plan: pure host arithmetic ---------------------------------------------------------------------------------------------
inline int max_levels_per_launch(int ring) {
    switch (ring) {
        case 0: return kMaxJ<Goldilocks>;
        case 1: return kMaxJ<BabyBear>;
        case 2: return kMaxJ<Stark>;
        case 3: return kSlotMaxJ<SlotG24>;
        case 4: return kSlotMaxJ<SlotB72>;
        default: return kSlotMaxJ<SlotFrog>;
    }
}
using Plan = ptree::Plan;  // launches, j[], layer_elems (2^num_vars - 1, per output)
// false: bad arguments.  The split is that of ptree::plan: full launches first, the remainder last; num_vars = 0 is no launch at all.
inline bool plan(int ring, size_t num_vars, int order, Plan *p) {
    if (ring < 0 || ring > 5 || num_vars > mle::MAX_VARS || (order != mle::ORDER_LEADING && order != mle::ORDER_TRAILING)) return false;
    *p = Plan{};
    const int jmax = max_levels_per_launch(ring);
    for (size_t left = num_vars; left;) {
        const int j = (int)(left < (size_t)jmax ? left : (size_t)jmax);
        p->j[p->launches++] = j;
        left -= j;
    }
    p->layer_elems = ((size_t)1 << num_vars) - 1;
    return true;
}
using ptree::layer_offset;

}  // namespace ftree
}  // namespace sr
