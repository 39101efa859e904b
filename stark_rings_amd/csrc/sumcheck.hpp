// The prover's message of a sum-check round over a product of dense multilinear extensions in CRT / NTT form:
//   round    p(t) = sum_{b < half} prod_j ( lo_j[b] + t (hi_j[b] - lo_j[b]) ),  t = 0 .. d, d = the number of tables;
//            (lo, hi) = (f[2b], f[2b + 1]) in leading order -- the summand is fix_variables with the point [R::from(t)]
//            (mle/dense.rs:171-199) -- and (f[b], f[b + half]) in trailing order (fix_last_variables,
//            polynomials/multilinear_polynomial.rs:251-286)
//   sum      H = sum_{b < 2^num_vars} prod_j f_j[b], the `sum` random_mle_list returns (multilinear_polynomial.rs:19-49)
// `*` is the slot product of the ring, as in mle.hpp.  t lo + t (hi - lo) needs no product: v_j(t) = v_j(t - 1) + (hi_j - lo_j).
// All sums are exact modular integers on canonical values, so neither the grid nor the split changes a bit of the result.
//
// One pass reads every table once.  Lane (g, c) owns unit c of the ring element (mle::Lane: a 16-byte pair of coefficients of a
// one-limb field where the tables are aligned, one coefficient otherwise, one Stark coefficient; one Fq3 / Fq9 / Fq4 slot of the
// reference's own rings) and takes the pairs b = g, g + groups, g + 2 groups, ...: the lanes of a wave read consecutive units of
// consecutive elements.  An element with fewer than 256 units puts 256 / units lane-groups into one workgroup; their sums meet in LDS,
// so a workgroup leaves ONE record of d + 1 partial elements whatever the degree.  One record (D alone fills the device, or a short
// table): it is written to `out`.  Otherwise record r goes to the caller's workspace and sum_groups_kernel adds the records -- the
// scheme of gram_kernel / sum_parts_kernel (symmetric.hpp); the number of records is host arithmetic on the shape alone (plan), so
// the plan needs no device.
//
// The host side below the kernels is shared with sumcheck_fold.hpp and sumcheck_vpoly.hpp: the records of a shape (plan_records), the
// geometry of a launch (Geometry, geometry_of) and the launches of a plan (launch_plan); a family adds its own shape and launches.
//
// Truncated storage: a pair whose first element lies beyond the stored part of ANY table has a zero factor at every t and is never
// visited (the loop ends at the shortest table); a second element beyond a table's stored part is zero and is not loaded.
#pragma once
#include "frog_ring.hpp"
#include "mle.hpp"
#include "ntt_generic.hpp"
#include "small_linalg.hpp"
#include "small_rings.hpp"

namespace sr {
namespace sumcheck {

enum { MODE_LEADING = 0, MODE_TRAILING = 1, MODE_SUM = 2, MAX_TABLES = 4, MAX_VARS = 47 };

// the tables of a call, by value in the kernel arguments: a captured graph holds no host pointer
struct Tables {
    const uint64_t *p[MAX_TABLES];
    size_t n[MAX_TABLES];  // stored elements
};

// Terms a lazy accumulator takes between two reductions into the canonical running sum.  Against all-(p - 1) inputs:
//   SumOfProducts<Goldilocks>  four 96-bit sums of 32 x 32-bit products: 2^6 (2^32 - 1)^2 < 2^70
//   SlotDot<SlotG24> / <SlotFrog>  96-bit sums of at most 2 x 4 partial products (the middle class of one exponent) per term:
//                              2^6 * 8 * (2^32 - 1)^2 < 2^73
//   SlotDot<SlotB72>           96-bit sums of at most 9 products of 31-bit images per term: 2^6 * 9 * 2^62 < 2^72, and its redc()
//                              wants fewer than 2^29 terms
//   SumOfProducts<BabyBear> / <Stark>  canonical after every term (mul_boundary_pre is the whole Montgomery product): no bound
// so every sum stays below 2^96 with 23 bits to spare.  The interval is this short because a plan that fills the device leaves a lane
// few terms (a table of 1 GiB gives a Goldilocks lane 128): a longer one would be reached by no table a test can afford.  One finish()
// per 64 terms is about 100 VALU instructions against 64 x 12 for the Goldilocks terms of one point, and under 2 % of all a pair costs
// at d = 2 (differences, running points, canonical products); 4 - 6 % of the products of the slot rings.
constexpr unsigned kFlush = 64;

// ---- power-of-two rings -----------------------------------------------------------------------------------------------------------
// NT tables, points t0 .. t0 + NP - 1 (PAIR) or the plain product (!PAIR, NP == 1).  groups: lane-groups of the launch.  lu < 8: a
// workgroup holds 256 >> lu of them, which meet in lds (256 lanes x RW words), and is record blockIdx.x; otherwise a lane-group is a
// record of its own.  dst: element (record * np_total + t0 + i) of the workspace, or of `out` when there is one record.
template <class F, int RW, int NT, int NP, bool PAIR>
__device__ __forceinline__ void round_units(uint64_t *dst, const Tables &tb, size_t count, size_t sb, size_t st, int lu, size_t groups,
                                            unsigned t0, unsigned np_total, uint64_t *lds) {
    using E = typename F::elem;
    using L = mle::Lane<F, RW>;
    const size_t flat = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t g = flat >> lu, c = flat & (((size_t)1 << lu) - 1);
    const bool in_block = lu < 8;  // uniform; the grid of such a launch is exact, so every lane reaches the barriers below
    if (!in_block && g >= groups) return;
    E total[NP][L::NC];
    SumOfProducts<F> acc[NP][L::NC];
#pragma unroll
    for (int i = 0; i < NP; i++)
#pragma unroll
        for (int n = 0; n < L::NC; n++) {
            total[i][n] = F::zero();
            acc[i][n].init();
        }
    unsigned since = 0;
    for (size_t b = g; b < count; b += groups) {
        const size_t e0 = b * sb, e1 = e0 + st;
        L lo[NT], hi[NT];
#pragma unroll
        for (int j = 0; j < NT; j++) {
            lo[j].template load<true>(tb.p[j] + ((e0 << lu) + c) * RW);
            if constexpr (PAIR) {
                if (e1 < tb.n[j]) hi[j].template load<true>(tb.p[j] + ((e1 << lu) + c) * RW);
                else hi[j].zero();
            }
        }
#pragma unroll
        for (int n = 0; n < L::NC; n++) {
            E v[NT], dl[NT];
#pragma unroll
            for (int j = 0; j < NT; j++) {
                v[j] = lo[j].get(n);
                if constexpr (PAIR) {
                    dl[j] = F::sub(hi[j].get(n), v[j]);
                    for (unsigned q = 0; q < t0; q++) v[j] = F::add(v[j], dl[j]);
                }
            }
#pragma unroll
            for (int i = 0; i < NP; i++) {
                if constexpr (NT == 1) {
                    total[i][n] = F::add(total[i][n], v[0]);
                } else {
                    E pr = v[0];
#pragma unroll
                    for (int j = 1; j < NT - 1; j++) pr = F::mul_boundary(pr, v[j]);
                    acc[i][n].fma(pr, v[NT - 1]);
                }
                if constexpr (PAIR) {
                    if (i + 1 < NP) {
#pragma unroll
                        for (int j = 0; j < NT; j++) v[j] = F::add(v[j], dl[j]);
                    }
                }
            }
        }
        if constexpr (NT > 1) {
            if (++since == kFlush) {
                since = 0;
#pragma unroll
                for (int i = 0; i < NP; i++)
#pragma unroll
                    for (int n = 0; n < L::NC; n++) {
                        total[i][n] = F::add(total[i][n], acc[i][n].finish());
                        acc[i][n].init();
                    }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NP; i++) {
        L r;
#pragma unroll
        for (int n = 0; n < L::NC; n++) {
            if constexpr (NT > 1) total[i][n] = F::add(total[i][n], acc[i][n].finish());
            r.put(n, total[i][n]);
        }
        if (!in_block) {
            r.store(dst + ((((g * np_total + t0 + i)) << lu) + c) * RW);
            continue;
        }
        const unsigned t = threadIdx.x, units = 1u << lu;
        __syncthreads();  // the previous point's sums have been read
#pragma unroll
        for (int q = 0; q < RW; q++) lds[t * RW + q] = r.w[q];
        __syncthreads();
        if (t < units) {  // lane-group 0 of the workgroup: t == c
            for (unsigned sg = 1; sg < (256u >> lu); sg++) {
                L x;
#pragma unroll
                for (int q = 0; q < RW; q++) x.w[q] = lds[(sg * units + t) * RW + q];
#pragma unroll
                for (int n = 0; n < L::NC; n++) r.put(n, F::add(r.get(n), x.get(n)));
            }
            r.store(dst + ((((blockIdx.x * (size_t)np_total + t0 + i)) << lu) + c) * RW);
        }
    }
}
// pair: the tables and dst are 16-byte aligned and k >= 1 (one-limb fields)
template <class F, int NT, int NP, bool PAIR>
__global__ __launch_bounds__(256) void round_kernel(uint64_t *dst, Tables tb, size_t count, size_t sb, size_t st, int k, int pair, size_t groups,
                                                    unsigned t0, unsigned np_total) {
    constexpr int RWMAX = sizeof(typename F::storage) == 8 ? 2 : (int)sizeof(typename F::storage) / 8;
    __shared__ uint64_t lds[256 * RWMAX];
    if constexpr (sizeof(typename F::storage) == 8) {
        if (pair) round_units<F, 2, NT, NP, PAIR>(dst, tb, count, sb, st, k - 1, groups, t0, np_total, lds);
        else round_units<F, 1, NT, NP, PAIR>(dst, tb, count, sb, st, k, groups, t0, np_total, lds);
    } else {
        round_units<F, RWMAX, NT, NP, PAIR>(dst, tb, count, sb, st, k, groups, t0, np_total, lds);
    }
}

// ---- goldilocks24 / babybear72 / frog16: lane = slot (slot_fold_kernel's mapping) ------------------------------------------------
// A workgroup holds 256 / S lane-groups (S = 8 or 4 slots per element); they meet in LDS (slot_reduce_store) and the workgroup is
// record blockIdx.x.  The grid is exact (groups = gridDim.x * 256 / S), so every lane reaches the barriers.
template <class SL, int NT, int NP, bool PAIR>
__global__ __launch_bounds__(256) void slot_round_kernel(typename SL::K k, uint64_t *dst, Tables tb, size_t count, size_t sb, size_t st,
                                                         size_t groups, unsigned t0, unsigned np_total) {
    using F = typename SL::F;
    using E = typename F::elem;
    constexpr int W = SL::W, S = SL::D / SL::W;
    const size_t flat = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t g = flat / S;
    const int off = (int)(flat % S) * W;
    __shared__ E lds[256 * W];
    E total[NP][W];
    SlotDot<SL> acc[NP];
#pragma unroll
    for (int i = 0; i < NP; i++) {
        acc[i].init();
#pragma unroll
        for (int m = 0; m < W; m++) total[i][m] = F::zero();
    }
    unsigned since = 0;
    for (size_t b = g; b < count; b += groups) {
        const size_t e0 = b * sb, e1 = e0 + st;
        E v[NT][W], dl[NT][W];
#pragma unroll
        for (int j = 0; j < NT; j++) {
            slot_load<SL>(v[j], tb.p[j] + e0 * SL::D + off);
            if constexpr (PAIR) {
                if (e1 < tb.n[j]) {
                    slot_load<SL>(dl[j], tb.p[j] + e1 * SL::D + off);
#pragma unroll
                    for (int m = 0; m < W; m++) dl[j][m] = F::sub(dl[j][m], v[j][m]);
                } else {
#pragma unroll
                    for (int m = 0; m < W; m++) dl[j][m] = F::sub(F::zero(), v[j][m]);
                }
                for (unsigned q = 0; q < t0; q++)
#pragma unroll
                    for (int m = 0; m < W; m++) v[j][m] = F::add(v[j][m], dl[j][m]);
            }
        }
#pragma unroll
        for (int i = 0; i < NP; i++) {
            if constexpr (NT == 1) {
#pragma unroll
                for (int m = 0; m < W; m++) total[i][m] = F::add(total[i][m], v[0][m]);
            } else {
                E pr[W];
#pragma unroll
                for (int m = 0; m < W; m++) pr[m] = v[0][m];
#pragma unroll
                for (int j = 1; j < NT - 1; j++) SL::mul(pr, v[j], k);
                acc[i].fma(pr, v[NT - 1]);
            }
            if constexpr (PAIR) {
                if (i + 1 < NP) {
#pragma unroll
                    for (int j = 0; j < NT; j++)
#pragma unroll
                        for (int m = 0; m < W; m++) v[j][m] = F::add(v[j][m], dl[j][m]);
                }
            }
        }
        if constexpr (NT > 1) {
            if (++since == kFlush) {
                since = 0;
#pragma unroll
                for (int i = 0; i < NP; i++) {
                    E r[W];
                    acc[i].finish(r, k);
                    acc[i].init();
#pragma unroll
                    for (int m = 0; m < W; m++) total[i][m] = F::add(total[i][m], r[m]);
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NP; i++) {
        if constexpr (NT > 1) {
            E r[W];
            acc[i].finish(r, k);
#pragma unroll
            for (int m = 0; m < W; m++) total[i][m] = F::add(total[i][m], r[m]);
        }
        if (i) __syncthreads();  // the previous point's sums have been read
        slot_reduce_store<SL>(lds, total[i], dst + (blockIdx.x * (size_t)np_total + t0 + i) * SL::D);
    }
}

// out[i] = sum_g part[g * total + i] (g: the records) over the `total` coefficients of the d + 1 (or one) output elements; four independent chains
template <class F>
__global__ __launch_bounds__(256) void sum_groups_kernel(typename F::storage *out, const typename F::storage *part, size_t total, size_t groups) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        typename F::elem s[4] = {F::zero(), F::zero(), F::zero(), F::zero()};
        size_t g = 0;
        for (; g + 4 <= groups; g += 4)
#pragma unroll
            for (int u = 0; u < 4; u++) s[u] = F::add(s[u], F::load(part + (g + u) * total + i));
        for (; g < groups; g++) s[0] = F::add(s[0], F::load(part + g * total + i));
        F::store(out + i, F::add(F::add(s[0], s[1]), F::add(s[2], s[3])));
    }
}
// some table is empty: every output word is zero, no table is loaded
__global__ __launch_bounds__(256) void zero_kernel(uint64_t *out, size_t words) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < words; i += (size_t)gridDim.x * blockDim.x) out[i] = 0;
}

// ---- the plan: pure host arithmetic -------------------------------------------------------------------------------------------------
// kFillLanes: four workgroups of 256 lanes on each of 256 compute units.  A shape whose units per element do not reach that takes its
// pairs in several records -- workgroups for elements below 256 units, whole lane-groups above -- at most kMaxGroups
// (include/stark_rings_hip.h: SR_MLE_ROUND_MAX_GROUPS; 1024 records of 256 lanes are the fill target) and never fewer than kMinPairs
// pairs per lane.
constexpr size_t kFillLanes = (size_t)1 << 18, kMaxGroups = 1024, kMinPairs = 16;

// Points one launch takes.  d + 1 accumulators beside 2 d operands: where one launch for all points would need more than 256
// registers per lane (a single wave per SIMD) the points go in several launches, each of which reads the tables once; frog16 at d = 4
// needs 264 even with two points (Fq4 products) and takes one point per launch, five launches whose instruction count together is
// that of 2 + 2 + 1.  Nothing spills to scratch (tests/test_sumcheck_isa.py holds every count).  The one-limb fields take all d + 1
// points at once for every d <= 4: they read each table exactly once per call.
template <class T>
constexpr int points_of(int n_tables) {
    if (std::is_same<T, Stark>::value) return n_tables >= 4 ? 2 : n_tables + 1;
    if (std::is_same<T, SlotG24>::value) return n_tables == 3 ? 2 : n_tables == 4 ? 3 : n_tables + 1;
    if (std::is_same<T, SlotB72>::value) return n_tables >= 3 ? 2 : n_tables + 1;  // 17 96-bit sums per point
    if (std::is_same<T, SlotFrog>::value) return n_tables >= 4 ? 1 : n_tables >= 2 ? 2 : n_tables + 1;
    return n_tables + 1;
}
inline int points_per_launch(int ring, int n_tables) {
    switch (ring) {
        case 0: return points_of<Goldilocks>(n_tables);
        case 1: return points_of<BabyBear>(n_tables);
        case 2: return points_of<Stark>(n_tables);
        case 3: return points_of<SlotG24>(n_tables);
        case 4: return points_of<SlotB72>(n_tables);
        default: return points_of<SlotFrog>(n_tables);
    }
}
// log2 of the units per element as the plan counts them (the aligned case for the one-limb fields)
inline int log2_units(int ring, int k) {
    switch (ring) {
        case 0: case 1: return k >= 1 ? k - 1 : 0;
        case 2: return k;
        case 3: case 4: return 3;
        default: return 2;
    }
}
// lane-groups of a record for elements of 2^lu units
inline size_t groups_per_record(int lu) { return lu < 8 ? (size_t)256 >> lu : 1; }

struct Plan {
    size_t count = 0;   // pairs (round modes) or indices (sum) of the full table
    size_t groups = 1;  // records
    int np_total = 1, np_launch = 1, launches = 1;
    size_t work_elems = 0;
};
// The records of a shape, for all three families (sumcheck_fold.hpp, sumcheck_vpoly.hpp): groups, launches and work_elems of a plan
// whose count and np_total are set and whose points go in point_launches launches.
inline void plan_records(int ring, int k, int point_launches, Plan *p) {
    const int lu = log2_units(ring, k);
    const size_t per_record = groups_per_record(lu);      // lane-groups of a record
    const size_t lanes = lu < 8 ? 256 : (size_t)1 << lu;  // lanes of a record
    size_t want = lanes >= kFillLanes ? 1 : kFillLanes / lanes;
    if (want > p->count / (kMinPairs * per_record)) want = p->count / (kMinPairs * per_record);
    if (want > kMaxGroups) want = kMaxGroups;
    if (want < 1) want = 1;
    // the points in several launches: the launches meet in the workspace as well (at least two records, the second possibly empty), so
    // that a plan without a workspace is always a single launch
    if (point_launches > 1 && want < 2) want = 2;
    p->groups = want;
    p->launches = point_launches + (want > 1 ? 1 : 0);
    p->work_elems = want > 1 ? want * (size_t)p->np_total : 0;
}
inline bool plan(int ring, int k, size_t num_vars, int n_tables, int mode, Plan *p) {
    if (ring < 0 || ring > 5 || num_vars > MAX_VARS || n_tables < 1 || n_tables > MAX_TABLES || mode < MODE_LEADING || mode > MODE_SUM) return false;
    if (mode != MODE_SUM && num_vars == 0) return false;
    *p = Plan{};
    p->count = mode == MODE_SUM ? (size_t)1 << num_vars : (size_t)1 << (num_vars - 1);
    p->np_total = mode == MODE_SUM ? 1 : n_tables + 1;
    p->np_launch = mode == MODE_SUM ? 1 : points_per_launch(ring, n_tables);
    plan_records(ring, k, (p->np_total + p->np_launch - 1) / p->np_launch, p);
    return true;
}

// ---- the launch skeleton of all three families --------------------------------------------------------------------------------------
// A family type T is a field (the power-of-two rings) or a slot type (goldilocks24 / babybear72 / frog16); the slot kernels take the
// ring's constants SL::K first, the field kernels take k and pair instead.
template <class T>
constexpr bool kSlot = std::is_same<T, SlotG24>::value || std::is_same<T, SlotB72>::value || std::is_same<T, SlotFrog>::value;
struct NoConsts {};
template <class T, bool = kSlot<T>>
struct Family {
    using F = T;
    using K = NoConsts;
};
template <class T>
struct Family<T, true> {
    using F = typename T::F;
    using K = typename T::K;
};
// The geometry of a call.  pair: a lane owns a 16-byte pair of coefficients -- a one-limb field, k >= 1, and every buffer of the call
// starts on a 16-byte boundary.  An unaligned call has twice the units the plan counted: the same records, at 256 units and above
// twice the lanes.  A slot ring has 8 or 4 units (slots) whatever the alignment; its kernels take neither k nor pair.
struct Geometry {
    int k, pair, lu;  // lu: log2 of the units of an element
    size_t words;     // 64-bit words of an element
    size_t groups(size_t records) const { return records * groups_per_record(lu); }  // lane-groups of the launch
    dim3 grid(size_t records) const { return dim3((unsigned)(lu < 8 ? records : records << (lu - 8))); }
};
template <class T>
inline Geometry geometry_of(int k, bool aligned) {
    if constexpr (kSlot<T>) {
        return {0, 0, T::D / T::W == 8 ? 3 : 2, (size_t)T::D};
    } else {
        const int pair = sizeof(typename T::storage) == 8 && k >= 1 && aligned;
        return {k, pair, pair ? k - 1 : k, ((size_t)1 << k) * (sizeof(typename T::storage) / 8)};
    }
}
// The launches of a plan, one after the other on `s`.  Nothing to visit: one launch that zeroes `out`.  Otherwise points(dst) enqueues
// the family's own launches, which leave record r at element r * np_total of dst -- the workspace, or `out` when there is one record --
// and the sum over the records follows.
template <class T, class Points>
inline hipError_t launch_plan(const Plan &p, const Geometry &ge, bool nothing, uint64_t *out, uint64_t *work, hipStream_t s, Points points) {
    using F = typename Family<T>::F;
    using S = typename F::storage;
    const size_t words = (size_t)p.np_total * ge.words;
    if (nothing) {
        hipLaunchKernelGGL(zero_kernel, dim3(mle::blocks_for(words)), dim3(256), 0, s, out, words);
        return hipGetLastError();
    }
    points(p.groups > 1 ? work : out);
    if (p.groups > 1) {
        const size_t total = words / (sizeof(S) / 8);
        hipLaunchKernelGGL((sum_groups_kernel<F>), dim3(mle::blocks_for(total)), dim3(256), 0, s, reinterpret_cast<S *>(out),
                           reinterpret_cast<const S *>(work), total, p.groups);
    }
    return hipGetLastError();
}

// ---- the launches of a round message --------------------------------------------------------------------------------------------------
struct Shape {
    size_t count, sb, st;  // pairs to visit (already cut to the shortest table), element strides of a pair
};
inline Shape shape_of(int mode, size_t num_vars, const size_t *n_evals, int n_tables) {
    size_t nmin = n_evals[0];
    for (int j = 1; j < n_tables; j++) nmin = n_evals[j] < nmin ? n_evals[j] : nmin;
    if (mode == MODE_SUM) return {nmin, 1, 0};
    const size_t half = (size_t)1 << (num_vars - 1);
    if (mode == MODE_LEADING) return {(nmin + 1) / 2, 2, 1};
    return {nmin < half ? nmin : half, 1, half};
}
// one launch: NP points from t0 on (sumcheck_fold.hpp takes its remaining points from here as well)
template <class T, int NT, int NP, bool PAIR>
inline void launch_round(const typename Family<T>::K &kc, const Geometry &ge, size_t records, uint64_t *dst, const Tables &tb, const Shape &sh,
                         unsigned t0, unsigned np_total, hipStream_t s) {
    const dim3 g = ge.grid(records), b(256);
    if constexpr (kSlot<T>)
        hipLaunchKernelGGL((slot_round_kernel<T, NT, NP, PAIR>), g, b, 0, s, kc, dst, tb, sh.count, sh.sb, sh.st, ge.groups(records), t0, np_total);
    else
        hipLaunchKernelGGL((round_kernel<T, NT, NP, PAIR>), g, b, 0, s, dst, tb, sh.count, sh.sb, sh.st, ge.k, ge.pair, ge.groups(records), t0,
                           np_total);
}
// np is the launch's chunk of points: points_of (P) or the remainder of d + 1 (R) -- the only two kernels a (family type, d) pair reaches
template <class T, int NT, bool PAIR>
inline void launch_np(const typename Family<T>::K &kc, const Geometry &ge, int np, size_t records, uint64_t *dst, const Tables &tb, const Shape &sh,
                      unsigned t0, unsigned np_total, hipStream_t s) {
    constexpr int P = PAIR ? points_of<T>(NT) : 1, R = PAIR ? (NT + 1) % P : 0;
    if (np == P) launch_round<T, NT, P, PAIR>(kc, ge, records, dst, tb, sh, t0, np_total, s);
    if constexpr (R != 0)
        if (np == R) launch_round<T, NT, R, PAIR>(kc, ge, records, dst, tb, sh, t0, np_total, s);
}
// fn(integral_constant NT) for n_tables in 1 .. 4
template <class Fn>
inline void with_tables(int n_tables, Fn fn) {
    switch (n_tables) {
        case 1: fn(std::integral_constant<int, 1>{}); break;
        case 2: fn(std::integral_constant<int, 2>{}); break;
        case 3: fn(std::integral_constant<int, 3>{}); break;
        default: fn(std::integral_constant<int, 4>{}); break;
    }
}
// The points in chunks of np_launch.  aligned: every table, out and work start on a 16-byte boundary.  An empty table: nothing to visit.
template <class T>
inline hipError_t launch(const typename Family<T>::K &kc, const Plan &p, int mode, uint64_t *out, const Tables &tb, int n_tables, size_t num_vars,
                         int k, bool aligned, uint64_t *work, hipStream_t s) {
    const Geometry ge = geometry_of<T>(k, aligned);
    const Shape sh = shape_of(mode, num_vars, tb.n, n_tables);
    return launch_plan<T>(p, ge, sh.count == 0, out, work, s, [&](uint64_t *dst) {
        for (int t0 = 0; t0 < p.np_total; t0 += p.np_launch) {
            const int np = p.np_total - t0 < p.np_launch ? p.np_total - t0 : p.np_launch;
            with_tables(n_tables, [&](auto nt) {
                if (mode == MODE_SUM) launch_np<T, decltype(nt)::value, false>(kc, ge, np, p.groups, dst, tb, sh, (unsigned)t0, (unsigned)p.np_total, s);
                else launch_np<T, decltype(nt)::value, true>(kc, ge, np, p.groups, dst, tb, sh, (unsigned)t0, (unsigned)p.np_total, s);
            });
        }
    });
}

}  // namespace sumcheck
}  // namespace sr
