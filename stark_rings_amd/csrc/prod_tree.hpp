// Grand products: every layer of the binary product tree over a table of ring elements in CRT / NTT form -- the circuit of the
// division-free (layered, GKR) product argument.  Layer 0 is the 2^n leaves; layer k (1 <= k <= n) has 2^(n-k) elements, with
// `half` the size of layer k:
//   leading order    L_k[i] = L_{k-1}[2i] * L_{k-1}[2i+1]     the pairs DenseMultilinearExtension::fix_variables folds
//   trailing order   L_k[i] = L_{k-1}[i] * L_{k-1}[i + half]  the pairs fix_last_variables folds: the two operands of a layer are the
//                                                             contiguous lower and upper halves of the layer below
// `*` is the slot product of the ring, as in sr_product_batch: mul_boundary of the base field for the fully split power-of-two rings,
// the Fq3 / Fq9 / Fq4 product (small_slot_mul, frog_fq4_mul) for the reference's own rings.
//
// One launch produces J levels from the layer below them (m variables, 2^m elements), the way mle.hpp folds J variables per launch:
// group b (b < 2^(m-J)) holds the 2^J input elements b * sb + t * st (t < 2^J; leading: sb = 2^J, st = 1; trailing: sb = 1,
// st = 2^(m-J)), read once; the 2^J - 1 products are formed level by level in registers and each level is stored to its own layer.
// The registers hold the group in the order that makes every level pair slot u with slot u + h (h the size of the level): in
// trailing order slot t is input t; in leading order slot t is input rev_J(t), the bits of t reversed, so that the partner of an
// even input is its neighbour.  Slot u of the level of size h is then output (trailing) b + u * st or (leading) b * h + rev(u) of
// that level's layer.
//
// Truncated leaves: input elements at or beyond n_in are one() and are never loaded; a group whose first element is already beyond
// n_in is all ones (its other elements lie further up in both orders) and is written as one() without any load.  Every layer is
// written in full, ones included.
//
// The layers of one call lie one behind the other, layer 1 first: layer k at element offset 2^n - 2^(n-k+1) of a buffer of 2^n - 1
// elements, the root last.  Within a launch `out` points at the first level it produces.
#pragma once
#include "mle.hpp"
#include "sparse_mle.hpp"

#include <utility>

namespace sr {
namespace ptree {

// the low `bits` bits of t, reversed
__host__ __device__ constexpr int rev(int t, int bits) {
    int r = 0;
    for (int i = 0; i < bits; i++) r |= ((t >> i) & 1) << (bits - 1 - i);
    return r;
}

// Node P (P < 2^J - 1) of a group's tree, the nodes numbered level by level: level q = 1 .. J has h = 2^(J-q) nodes, node u of it is
// slot u times slot u + h.  The nodes are visited by a pack expansion, not by loops, so that every store is straight-line code.
template <int J, int P>
struct Node {
    static constexpr int level() {
        int q = 1;
        while (P >= (1 << J) - (1 << (J - q))) q++;
        return q;
    }
    static constexpr int q = level(), lh = J - q, h = 1 << lh, u = P - ((1 << J) - 2 * h);
    // element offset of the level's layer behind the launch's first one; m = log2 of the elements of the launch's input layer
    static __device__ __forceinline__ size_t layer(int m) { return ((size_t)1 << m) - ((size_t)1 << (m - q + 1)); }
};
template <class Fn, int... P>
__device__ __forceinline__ void each_node_of(Fn &&fn, std::integer_sequence<int, P...>) {
    (fn(std::integral_constant<int, P>{}), ...);
}
template <int J, class Fn>
__device__ __forceinline__ void each_node(Fn &&fn) {
    each_node_of(fn, std::make_integer_sequence<int, (1 << J) - 1>{});
}

// ---- power-of-two rings ---------------------------------------------------------------------------------------------------------
// The lane mapping of mle::fold_units: a lane owns RW raw u64 words of every element of its group -- two adjacent coefficients of a
// one-limb field (one 16-byte access per element) where the buffers are 16-byte aligned, one coefficient otherwise; one Stark
// coefficient (two 16-byte accesses).  A unit is RW words, `lu` = log2 of the units per ring element.
template <class F, int J, int RW>
__device__ __forceinline__ void tree_units(uint64_t *out, const uint64_t *in, const smle::One &one, size_t units, int lu, size_t n_in, int m,
                                           bool tr) {
    using L = mle::Lane<F, RW>;
    using Ops = smle::PowOps<F, F, RW>;
    const size_t gid = blockIdx.x * (size_t)blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    const size_t umask = ((size_t)1 << lu) - 1;
    const size_t sb = tr ? 1 : (size_t)1 << J, st = tr ? (size_t)1 << (m - J) : 1;
    L id;
    Ops::set_one(id, one);
    for (size_t i = gid; i < units; i += stride) {
        const size_t b = i >> lu, c = i & umask, base = b * sb;
        const bool live = base < n_in;  // else the whole group lies in the truncated (one) part of the table
        L v[1 << J];
#pragma unroll
        for (int t = 0; t < (1 << J); t++) {
            const size_t e = base + (size_t)(tr ? t : rev(t, J)) * st;
            if (live && e < n_in) v[t].template load<true>(in + ((e << lu) + c) * RW);
            else v[t] = id;
        }
        // a group of ones takes the same path (1 * 1 = 1): one set of stores, no branch around the products
        each_node<J>([&](auto node) {
            using N = Node<J, decltype(node)::value>;
            const size_t o = N::layer(m) + (tr ? b + (size_t)N::u * st : (b << N::lh) + (size_t)rev(N::u, N::lh));
#pragma unroll
            for (int n = 0; n < L::NC; n++) v[N::u].put(n, F::mul_boundary(v[N::u].get(n), v[N::u + N::h].get(n)));
            v[N::u].store(out + ((o << lu) + c) * RW);
        });
    }
}

// k = log2 D, m = log2 of the elements of the input layer (m >= J).  The J levels are written in full behind `out`.
template <class F, int J>
__global__ __launch_bounds__(256) void tree_kernel(typename F::storage *out, const typename F::storage *in, smle::One one, size_t n_in, int m,
                                                   int tr, int k) {
    uint64_t *o = reinterpret_cast<uint64_t *>(out);
    const uint64_t *a = reinterpret_cast<const uint64_t *>(in);
    const size_t groups = (size_t)1 << (m - J);
    if constexpr (sizeof(typename F::storage) == 8) {
        // D >= 2: a pair of coefficients never straddles two elements, and every element starts on a 16-byte boundary when the buffer does
        if (k >= 1 && (((uintptr_t)o | (uintptr_t)a) & 15u) == 0) tree_units<F, J, 2>(o, a, one, groups << (k - 1), k - 1, n_in, m, tr != 0);
        else tree_units<F, J, 1>(o, a, one, groups << k, k, n_in, m, tr != 0);
    } else {
        tree_units<F, J, (int)sizeof(typename F::storage) / 8>(o, a, one, groups << k, k, n_in, m, tr != 0);
    }
}

// ---- goldilocks24 / babybear72 / frog16 -----------------------------------------------------------------------------------------
// The one-slot-per-lane mapping of mle::slot_fold_kernel: lane i owns slot i of the flat table of groups, so the 64 lanes of a wave
// read one contiguous span per input element and write one per output element.
template <class SL, int J>
__global__ __launch_bounds__(256) void slot_tree_kernel(typename SL::K k, uint64_t *out, const uint64_t *in, smle::One one, size_t n_in, int m,
                                                        int tr) {
    using Ops = smle::SlotOps<SL>;
    using U = typename Ops::U;
    constexpr int W = SL::W, S = SL::D / SL::W;
    const size_t slots = ((size_t)1 << (m - J)) * S;
    const size_t sb = tr ? 1 : (size_t)1 << J, st = tr ? (size_t)1 << (m - J) : 1;
    U id;
    Ops::set_one(id, one);
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < slots; i += (size_t)gridDim.x * blockDim.x) {
        const size_t b = i / S, base = b * sb;
        const int off = (int)(i % S) * W;
        const bool live = base < n_in;
        U v[1 << J];
        if (live) {
#pragma unroll
            for (int t = 0; t < (1 << J); t++) {
                const size_t e = base + (size_t)(tr ? t : rev(t, J)) * st;
                if (e < n_in) v[t].template load<true>(in + e * SL::D + off);
                else v[t] = id;
            }
        }
        each_node<J>([&](auto node) {
            using N = Node<J, decltype(node)::value>;
            const size_t o = N::layer(m) + (tr ? b + (size_t)N::u * st : (b << N::lh) + (size_t)rev(N::u, N::lh));
            if (live) {
                Ops::mul(v[N::u], v[N::u + N::h], k);
                v[N::u].store(out + o * SL::D + off);
            } else {  // a group of ones: no load and no slot product
                id.store(out + o * SL::D + off);
            }
        });
    }
}

// Levels one launch produces at most: the largest J <= 3 whose kernel has no scratch and stays within 128 VGPRs, i.e. four waves per
// SIMD for 256-lane workgroups (tests/test_prod_tree_isa.py holds the counts)
template <class F> constexpr int kMaxJ = 3;
template <class SL> constexpr int kSlotMaxJ = std::is_same<SL, SlotB72>::value ? 2 : 3;  // babybear72 J = 3 needs 152

// ---- host side ------------------------------------------------------------------------------------------------------------------
template <class F>
inline hipError_t launch_tree(int j, uint64_t *out, const uint64_t *in, const smle::One &one, size_t n_in, int m, bool tr, int k, hipStream_t s) {
    using S = typename F::storage;
    if (j < 1 || j > kMaxJ<F> || m < j) return hipErrorInvalidValue;
    const dim3 g(mle::blocks_for(mle::units_of<F>((size_t)1 << (m - j), k))), b(256);
    S *o = reinterpret_cast<S *>(out);
    const S *a = reinterpret_cast<const S *>(in);
    switch (j) {
        case 1: hipLaunchKernelGGL((tree_kernel<F, 1>), g, b, 0, s, o, a, one, n_in, m, (int)tr, k); break;
        case 2: hipLaunchKernelGGL((tree_kernel<F, 2>), g, b, 0, s, o, a, one, n_in, m, (int)tr, k); break;
        default:
            if constexpr (kMaxJ<F> >= 3) hipLaunchKernelGGL((tree_kernel<F, 3>), g, b, 0, s, o, a, one, n_in, m, (int)tr, k);
            break;
    }
    return hipGetLastError();
}
template <class SL>
inline hipError_t launch_slot_tree(const typename SL::K &kc, int j, uint64_t *out, const uint64_t *in, const smle::One &one, size_t n_in, int m,
                                   bool tr, hipStream_t s) {
    if (j < 1 || j > kSlotMaxJ<SL> || m < j) return hipErrorInvalidValue;
    const dim3 g(mle::blocks_for(((size_t)1 << (m - j)) * (SL::D / SL::W))), b(256);
    switch (j) {
        case 1: hipLaunchKernelGGL((slot_tree_kernel<SL, 1>), g, b, 0, s, kc, out, in, one, n_in, m, (int)tr); break;
        case 2: hipLaunchKernelGGL((slot_tree_kernel<SL, 2>), g, b, 0, s, kc, out, in, one, n_in, m, (int)tr); break;
        default:
            if constexpr (kSlotMaxJ<SL> >= 3) hipLaunchKernelGGL((slot_tree_kernel<SL, 3>), g, b, 0, s, kc, out, in, one, n_in, m, (int)tr);
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
struct Plan {
    int launches = 0;
    int j[mle::MAX_LAUNCHES] = {};
    size_t layer_elems = 0;  // 2^num_vars - 1
};
// false: bad arguments.  The split follows mle::plan: full launches first, the remainder last; num_vars = 0 is no launch at all.
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
// element offset of layer k (1 <= k <= num_vars) in the buffer of a call
inline size_t layer_offset(size_t num_vars, size_t k) { return ((size_t)1 << num_vars) - ((size_t)1 << (num_vars - k + 1)); }

}  // namespace ptree
}  // namespace sr
