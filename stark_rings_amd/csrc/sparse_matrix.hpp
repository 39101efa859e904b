// Sparse matrices of ring elements in CRT / NTT form, as CSR (vals, cols, row_ptr: the triple of sr_spmv_ntt_dev):
//   transpose   SparseMatrix::transpose (crates/linear_algebra/src/ops.rs:46-62): a stable counting sort by column; Matrix::transpose
//               (ops.rs:9-44) for dense data
//   product     SparseMatrix::checked_mul_mat (sparse_matrix.rs:219-281): entry (i, j) = sum over the common k of a_ik * b_kj, products
//               that are zero skipped, the entry stored iff one product was not zero
// The index work is host arithmetic (transpose_pattern, spgemm_pattern: no device, no context); the device moves and multiplies
// whole ring elements by position:
//   move_kernel     out[t] = in[perm[t]] (the values of a sparse transpose) or out[j][i] = in[i][j] (dense), 16 bytes per lane where
//                   the buffers allow it
//   spgemm_kernel   out[e] = sum_t a[pair_a[t]] * b[pair_b[t]] over the pair list of structural entry e, lane = slot, sums in
//                   SumOfProducts<F> (the accumulators of matmul_kernel / gram_kernel); slot_spgemm_kernel for the reference's own
//                   rings: one workgroup per entry, lane = (term group, slot), sums in SlotDot<SL>
//   count_dead_kernel   the entries whose flag stayed 0, added to a context counter
// `*` is the slot product.  Every slot is a field (Fp, Fq3, Fq9, Fq4), so a slot product is zero iff one factor's slot is zero, and
// a product of ring elements is zero iff that holds in every slot: a lane sets its entry's flag when both factors are non-zero in
// its slot.  Inputs are canonical, so "zero" is the all-zero memory image.  All sums are exact modular integers: adding the zero
// products, and any order of the sum, gives the reference's bits.
//
// No span split: a lane (power-of-two rings) walks the pair list of its entry alone, a slot-ring workgroup cuts it over its
// 256 / S term groups.  The plan sees (n_out, n_pairs) only, never the list lengths, so a split could only cut every list at the
// same length; lists are bounded by the row length of A, entries are many, and n_out * chunks workgroups fill the chip long before
// a list is long enough to matter.  spgemm_plan therefore asks for no workspace.
#pragma once
#include <vector>

#include "frog_ring.hpp"
#include "mle.hpp"
#include "ntt_generic.hpp"
#include "small_linalg.hpp"
#include "small_rings.hpp"

namespace sr {
namespace spm {

constexpr size_t kMaxBlocks = 0xFFFFFFull;  // a launch stays below 2^24 workgroups of 256 lanes (2^32 lanes)
constexpr int kLaunches = 2;                // the numeric kernel and the count of the dead entries (the flags are cleared by a memset node)

// ---- host: patterns ---------------------------------------------------------------------------------------------------------------
// Stable counting sort of the stored entries by column: row c of the transpose lists (original row, position) in ascending
// original row, whatever the order inside the input rows.  Returns nullptr or the reason the input is refused.
inline const char *transpose_pattern(const uint32_t *cols, const uint64_t *row_ptr, size_t nrows, size_t ncols, uint64_t *t_row_ptr,
                                     uint32_t *t_cols, uint32_t *perm) {
    if (!row_ptr || !t_row_ptr) return "null pointer";
    if (nrows > 0xFFFFFFFFull) return "more than 2^32 - 1 rows (row indices are 32-bit)";
    if (row_ptr[0] != 0) return "row_ptr[0] is not 0";
    for (size_t r = 0; r < nrows; r++)
        if (row_ptr[r] > row_ptr[r + 1]) return "row_ptr is not monotone";
    const uint64_t nnz = row_ptr[nrows];
    if (nnz > 0xFFFFFFFFull) return "2^32 or more stored entries (positions are 32-bit)";
    if (nnz && (!cols || !t_cols || !perm)) return "null pointer";
    for (size_t c = 0; c <= ncols; c++) t_row_ptr[c] = 0;
    for (uint64_t j = 0; j < nnz; j++) {
        if (cols[j] >= ncols) return "column index out of range";
        t_row_ptr[(size_t)cols[j] + 1]++;
    }
    for (size_t c = 0; c < ncols; c++) t_row_ptr[c + 1] += t_row_ptr[c];
    // t_row_ptr[c] serves as the fill cursor of column c and is shifted back afterwards
    for (size_t r = 0; r < nrows; r++)
        for (uint64_t j = row_ptr[r]; j < row_ptr[r + 1]; j++) {
            const uint64_t pos = t_row_ptr[cols[j]]++;
            t_cols[pos] = (uint32_t)r;
            perm[pos] = (uint32_t)j;
        }
    for (size_t c = ncols; c > 0; c--) t_row_ptr[c] = t_row_ptr[c - 1];
    t_row_ptr[0] = 0;
    return nullptr;
}
// rows strictly ascending, indices below ncols
inline const char *check_sorted(const uint32_t *cols, const uint64_t *row_ptr, size_t nrows, size_t ncols, const char *unsorted,
                                const char *range) {
    for (size_t r = 0; r < nrows; r++)
        for (uint64_t j = row_ptr[r]; j < row_ptr[r + 1]; j++) {
            if (cols[j] >= ncols) return range;
            if (j > row_ptr[r] && cols[j] <= cols[j - 1]) return unsorted;
        }
    return nullptr;
}
// The structural product of A (n x m) and B (m x p).  Column j of the result is built from column j of B (the rows of B^T) and
// the columns of A (the rows of A^T): for k ascending in column j of B, every row i with a_ik stored gains the pair (a_ik, b_kj) --
// so the pairs of (i, j) ascend in k, and since j ascends in the outer loop a stable counting sort of the entries by i leaves every
// output row ascending in j.  Cost: nnz_a + nnz_b + n_pairs + n + m + p steps, no walk over the n x p grid, no comparison sort.
// fill == false: only *n_out and *n_pairs are written.
inline const char *spgemm_pattern(const uint32_t *a_cols, const uint64_t *a_row_ptr, size_t n, size_t m, const uint32_t *b_cols,
                                  const uint64_t *b_row_ptr, size_t p, bool fill, uint64_t *out_row_ptr, uint32_t *out_cols, uint64_t *pair_ptr,
                                  uint32_t *pair_a, uint32_t *pair_b, size_t *n_out, size_t *n_pairs) {
    if (!a_row_ptr || !b_row_ptr || !n_out || !n_pairs) return "null pointer";
    if (p > 0xFFFFFFFFull) return "more than 2^32 - 1 columns (column indices are 32-bit)";
    std::vector<uint64_t> at_ptr(m + 1), bt_ptr(p + 1);
    std::vector<uint32_t> at_rows, at_pos, bt_rows, bt_pos;
    {
        // the transposes validate row_ptr, the entry counts and the index ranges
        if (a_row_ptr[0] == 0 && n <= 0xFFFFFFFFull && a_row_ptr[n] <= 0xFFFFFFFFull) {
            at_rows.resize(a_row_ptr[n]);
            at_pos.resize(a_row_ptr[n]);
        }
        if (const char *e = transpose_pattern(a_cols, a_row_ptr, n, m, at_ptr.data(), at_rows.data(), at_pos.data())) return e;
        if (b_row_ptr[0] == 0 && m <= 0xFFFFFFFFull && b_row_ptr[m] <= 0xFFFFFFFFull) {
            bt_rows.resize(b_row_ptr[m]);
            bt_pos.resize(b_row_ptr[m]);
        }
        if (const char *e = transpose_pattern(b_cols, b_row_ptr, m, p, bt_ptr.data(), bt_rows.data(), bt_pos.data())) return e;
    }
    if (const char *e = check_sorted(a_cols, a_row_ptr, n, m, "a row of A does not ascend strictly", "column index out of range")) return e;
    if (const char *e = check_sorted(b_cols, b_row_ptr, m, p, "a row of B does not ascend strictly", "column index out of range")) return e;

    // pass 1: the entries in (j, first touch of i) order -- their rows and pair counts
    std::vector<size_t> mark(n, 0), slot(n, 0);  // mark[i] == j + 1: row i has an entry in column j, numbered slot[i]
    std::vector<uint32_t> e_row;
    std::vector<uint64_t> e_pairs;
    size_t entries = 0, pairs = 0;
    for (size_t j = 0; j < p; j++)
        for (uint64_t u = bt_ptr[j]; u < bt_ptr[j + 1]; u++) {
            const uint32_t k = bt_rows[u];
            for (uint64_t v = at_ptr[k]; v < at_ptr[k + 1]; v++) {
                const uint32_t i = at_rows[v];
                if (mark[i] != j + 1) {
                    mark[i] = j + 1;
                    slot[i] = entries++;
                    if (fill) {
                        e_row.push_back(i);
                        e_pairs.push_back(0);
                    }
                }
                if (fill) e_pairs[slot[i]]++;
                pairs++;
            }
        }
    *n_out = entries;
    *n_pairs = pairs;
    if (!fill) return nullptr;
    // the counts are known and nothing of the caller's is written yet: refuse the null buffers here, not by a counting walk of its own
    if (!out_row_ptr || !pair_ptr || (entries && !out_cols) || (pairs && (!pair_a || !pair_b))) return "null pointer (all five arrays, or none to count)";

    // the stable counting sort by row: final position of every entry, then the pair offsets in final order
    for (size_t i = 0; i <= n; i++) out_row_ptr[i] = 0;
    for (size_t e = 0; e < entries; e++) out_row_ptr[(size_t)e_row[e] + 1]++;
    for (size_t i = 0; i < n; i++) out_row_ptr[i + 1] += out_row_ptr[i];
    std::vector<uint64_t> cursor(out_row_ptr, out_row_ptr + n), final_pos(entries);
    for (size_t e = 0; e < entries; e++) final_pos[e] = cursor[e_row[e]]++;
    pair_ptr[0] = 0;
    for (size_t e = 0; e < entries; e++) pair_ptr[final_pos[e] + 1] = e_pairs[e];
    for (size_t e = 0; e < entries; e++) pair_ptr[e + 1] += pair_ptr[e];
    // pass 2: the same walk writes the columns and the pairs; e_pairs becomes the fill cursor of every entry
    for (size_t e = 0; e < entries; e++) e_pairs[e] = pair_ptr[final_pos[e]];
    std::fill(mark.begin(), mark.end(), 0);
    size_t next = 0;
    for (size_t j = 0; j < p; j++)
        for (uint64_t u = bt_ptr[j]; u < bt_ptr[j + 1]; u++) {
            const uint32_t k = bt_rows[u];
            for (uint64_t v = at_ptr[k]; v < at_ptr[k + 1]; v++) {
                const uint32_t i = at_rows[v];
                if (mark[i] != j + 1) {
                    mark[i] = j + 1;
                    slot[i] = next++;
                    out_cols[final_pos[slot[i]]] = (uint32_t)j;
                }
                const uint64_t t = e_pairs[slot[i]]++;
                pair_a[t] = at_pos[v];
                pair_b[t] = bt_pos[u];
            }
        }
    return nullptr;
}

// ---- gather and dense transpose ---------------------------------------------------------------------------------------------------
// Output element e (a ring element of `units` lanes of V words each) is input element perm[e], or, without perm, the element
// (e % nrows, e / nrows) of a dense nrows x ncols matrix.  grid: output element major, unit chunk minor, so the source index is the
// same for every lane of a workgroup (one scalar load).  perm[e] >= n_in: the element is left unwritten and counted once.
template <int V>
__global__ __launch_bounds__(256) void move_kernel(uint64_t *out, const uint64_t *in, const uint32_t *perm, size_t n_in, size_t nrows,
                                                   size_t ncols, size_t units, unsigned long long *bad) {
    const size_t chunks = (units + 255) >> 8;
    const size_t e = blockIdx.x / chunks, u = (blockIdx.x % chunks) * (size_t)blockDim.x + threadIdx.x;
    size_t src;
    if (perm) {
        src = perm[e];
        if (src >= n_in) {
            if (blockIdx.x % chunks == 0 && threadIdx.x == 0) atomicAdd(bad, 1ull);
            return;
        }
    } else {
        src = (e % nrows) * ncols + e / nrows;
    }
    if (u >= units) return;
    if constexpr (V == 2) {
        const mle::u64x2 x = reinterpret_cast<const mle::u64x2 *>(in)[src * units + u];
        __builtin_nontemporal_store(x, reinterpret_cast<mle::u64x2 *>(out) + e * units + u);
    } else {
        __builtin_nontemporal_store(in[src * units + u], out + e * units + u);
    }
}

// ---- numeric phase ----------------------------------------------------------------------------------------------------------------
template <class S>
__device__ __forceinline__ bool image_nonzero(const S &x) {
    if constexpr (sizeof(S) == 8) {
        return x != 0;
    } else {
        return (x.q[0] | x.q[1] | x.q[2] | x.q[3]) != 0;
    }
}
// grid: entry major, slot chunk minor -- the entries of one output row are neighbours, so the row of A they share stays in L2.  The
// pair offsets and positions depend on blockIdx alone: scalar loads.  A position outside its value array is skipped.
template <class F>
__global__ __launch_bounds__(256) void spgemm_kernel(typename F::storage *out, uint32_t *live, const typename F::storage *a, size_t nnz_a,
                                                     const typename F::storage *b, size_t nnz_b, const uint64_t *pair_ptr, const uint32_t *pair_a,
                                                     const uint32_t *pair_b, size_t n_pairs, int k) {
    using S = typename F::storage;
    const size_t d = (size_t)1 << k;
    const size_t chunks = (d + 255) >> 8;
    const size_t slot = (blockIdx.x % chunks) * (size_t)blockDim.x + threadIdx.x;
    const size_t e = blockIdx.x / chunks;
    if (slot >= d) return;
    uint64_t t0 = pair_ptr[e], t1 = pair_ptr[e + 1];
    if (t1 > n_pairs) t1 = n_pairs;
    SumOfProducts<F> acc;
    acc.init();
    bool any = false;
    for (uint64_t t = t0; t < t1; t++) {
        const size_t pa = pair_a[t], pb = pair_b[t];
        if (pa >= nnz_a || pb >= nnz_b) continue;
        const S x = a[(pa << k) + slot], y = b[(pb << k) + slot];
        any |= image_nonzero(x) && image_nonzero(y);
        acc.fma(F::load(&x), F::load(&y));
    }
    F::store(out + (e << k) + slot, acc.finish());
    if (any) live[e] = 1;  // every writer stores the same word
}
// One workgroup per entry: lane (term group g, slot s) takes every G-th pair, the partial sums meet in LDS (slot_reduce_store).
template <class SL>
__global__ __launch_bounds__(256) void slot_spgemm_kernel(typename SL::K k, uint64_t *out, uint32_t *live, const uint64_t *a, size_t nnz_a,
                                                          const uint64_t *b, size_t nnz_b, const uint64_t *pair_ptr, const uint32_t *pair_a,
                                                          const uint32_t *pair_b, size_t n_pairs) {
    using E = typename SL::F::elem;
    constexpr int S = SL::D / SL::W, G = 256 / S;
    static_assert(256 % S == 0 && SL::D <= 256, "slot layout");
    __shared__ E lds[256 * SL::W];
    const size_t e = blockIdx.x;
    const int g = threadIdx.x / S, s = threadIdx.x % S;
    uint64_t t1 = pair_ptr[e + 1];
    if (t1 > n_pairs) t1 = n_pairs;
    E x[SL::W], z[SL::W], res[SL::W];
    SlotDot<SL> acc;
    acc.init();
    int any = 0;
    for (uint64_t t = pair_ptr[e] + g; t < t1; t += G) {
        const size_t pa = pair_a[t], pb = pair_b[t];
        if (pa >= nnz_a || pb >= nnz_b) continue;
        slot_load<SL>(x, a + pa * SL::D + s * SL::W);
        slot_load<SL>(z, b + pb * SL::D + s * SL::W);
        E ox = x[0], oz = z[0];
#pragma unroll
        for (int q = 1; q < SL::W; q++) {
            ox |= x[q];
            oz |= z[q];
        }
        any |= ox != 0 && oz != 0;
        acc.fma(x, z);
    }
    acc.finish(res, k);
    any = __syncthreads_or(any);
    slot_reduce_store<SL>(lds, res, out + e * SL::D);
    if (threadIdx.x == 0 && any) live[e] = 1;
}
// *dead += the number of flags that are 0
__global__ __launch_bounds__(256) void count_dead_kernel(const uint32_t *live, size_t n, unsigned long long *dead) {
    unsigned long long mine = 0;
    for (size_t base = blockIdx.x * (size_t)blockDim.x; base < n; base += (size_t)gridDim.x * blockDim.x) {
        const size_t i = base + threadIdx.x;
        mine += (unsigned long long)__syncthreads_count(i < n && live[i] == 0);
    }
    if (threadIdx.x == 0 && mine) atomicAdd(dead, mine);
}

// ---- plans and launchers ----------------------------------------------------------------------------------------------------------
// workgroups per ring element of the numeric kernel (power-of-two rings: 256 slots each; slot rings: the whole element)
inline size_t spgemm_chunks(int ring, int k) { return ring <= 2 ? (((size_t)1 << k) + 255) >> 8 : 1; }
// false: the grid of n_out entries exceeds one launch
inline bool spgemm_plan(int ring, int k, size_t n_out, size_t n_pairs, size_t *work_elems, int *launches) {
    (void)n_pairs;
    *work_elems = 0;
    *launches = n_out ? kLaunches : 0;
    return n_out <= kMaxBlocks / spgemm_chunks(ring, k);
}
// words: u64 words per ring element.  false: the grid exceeds one launch
inline bool move_grid(size_t n_out, size_t words, bool aligned, int *v, size_t *units, size_t *blocks) {
    *v = aligned && words % 2 == 0 ? 2 : 1;
    *units = words / *v;
    const size_t chunks = (*units + 255) >> 8;
    if (n_out > kMaxBlocks / chunks) return false;
    *blocks = n_out * chunks;
    return true;
}
inline hipError_t launch_move(uint64_t *out, const uint64_t *in, const uint32_t *perm, size_t n_in, size_t nrows, size_t ncols, int v, size_t units,
                              size_t blocks, unsigned long long *bad, hipStream_t s) {
    if (v == 2) hipLaunchKernelGGL((move_kernel<2>), dim3((unsigned)blocks), dim3(256), 0, s, out, in, perm, n_in, nrows, ncols, units, bad);
    else hipLaunchKernelGGL((move_kernel<1>), dim3((unsigned)blocks), dim3(256), 0, s, out, in, perm, n_in, nrows, ncols, units, bad);
    return hipGetLastError();
}
struct SpgemmArgs {
    uint64_t *out;
    uint32_t *live;
    const uint64_t *a, *b;
    size_t nnz_a, nnz_b;
    const uint64_t *pair_ptr;
    const uint32_t *pair_a, *pair_b;
    size_t n_out, n_pairs;
    unsigned long long *dead;  // null: the dead entries are not counted (the host form reads the flags itself)
};
inline hipError_t finish_spgemm(const SpgemmArgs &g, hipStream_t s) {
    if (g.dead) {
        size_t blocks = (g.n_out + 255) >> 8;
        if (blocks > 1024) blocks = 1024;
        hipLaunchKernelGGL(count_dead_kernel, dim3((unsigned)blocks), dim3(256), 0, s, g.live, g.n_out, g.dead);
    }
    return hipGetLastError();
}
// F: the field the sums of products run on (StarkL for Stark contexts on lazy limbs)
template <class F>
inline hipError_t launch_spgemm(const SpgemmArgs &g, int k, hipStream_t s) {
    using S = typename F::storage;
    if (hipError_t e = hipMemsetAsync(g.live, 0, g.n_out * sizeof(uint32_t), s)) return e;
    const size_t chunks = (((size_t)1 << k) + 255) >> 8;
    hipLaunchKernelGGL((spgemm_kernel<F>), dim3((unsigned)(g.n_out * chunks)), dim3(256), 0, s, reinterpret_cast<S *>(g.out), g.live,
                       reinterpret_cast<const S *>(g.a), g.nnz_a, reinterpret_cast<const S *>(g.b), g.nnz_b, g.pair_ptr, g.pair_a, g.pair_b, g.n_pairs, k);
    if (hipError_t e = hipGetLastError()) return e;
    return finish_spgemm(g, s);
}
template <class SL>
inline hipError_t launch_slot_spgemm(const typename SL::K &kc, const SpgemmArgs &g, hipStream_t s) {
    if (hipError_t e = hipMemsetAsync(g.live, 0, g.n_out * sizeof(uint32_t), s)) return e;
    hipLaunchKernelGGL((slot_spgemm_kernel<SL>), dim3((unsigned)g.n_out), dim3(256), 0, s, kc, g.out, g.live, g.a, g.nnz_a, g.b, g.nnz_b, g.pair_ptr,
                       g.pair_a, g.pair_b, g.n_pairs);
    if (hipError_t e = hipGetLastError()) return e;
    return finish_spgemm(g, s);
}

}  // namespace spm
}  // namespace sr
