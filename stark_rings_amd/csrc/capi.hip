// C ABI of the MI355X backend (include/stark_rings_hip.h).  Host-side set-up and launch logic only;
// kernels live in ntt_generic.hpp / ntt_goldilocks.hpp / small_rings.hpp.
//
// No CPU fallback exists on purpose: without a HIP device every compute entry point fails.
#include "../../include/stark_rings_hip.h"

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <initializer_list>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "fields.hpp"
#include "ntt_generic.hpp"
#include "ntt_goldilocks.hpp"
#include "ntt_regtile.hpp"
#include "small_rings.hpp"
#include "small_linalg.hpp"
#include "decompose.hpp"
#include "wire.hpp"
#include "frog_ring.hpp"
#include "ntt_stark.hpp"
#include "packed32.hpp"
#include "mle.hpp"
#include "norms.hpp"
#include "sparse_mle.hpp"
#include "symmetric.hpp"
#include "sparse_matrix.hpp"
#include "sumcheck.hpp"
#include "sumcheck_fold.hpp"
#include "sumcheck_vpoly.hpp"
#include "sumcheck_vpoly_fold.hpp"
#include "sumcheck_weighted.hpp"
#include "prod_tree.hpp"
#include "frac_tree.hpp"
#include "lincomb.hpp"
#include "lincomb_index.hpp"
#include "inverse.hpp"
#include "range_check.hpp"
#include "sumcheck_index.hpp"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(SR_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));          \
    } while (0)

enum KernelTag { K_FWD_COLS = 0, K_ROWS = 1, K_INV_COLS = 2, K_POINTWISE = 3, K_OTHER = 4, K_NTAGS = 5 };

struct Prof {
    bool on = false;
    // stride > 1: only every stride-th launch is bracketed by events (sr_ctx_profile_enable(ctx, stride)).  Two event records around
    // EVERY launch of a two-lane plan open a gap on that lane in which the other lane's kernel runs alone, so fully bracketed steps
    // report shorter in-flight durations than the timed steps have (70-82 against 90-97 us for the config-2 rows kernel, round 4);
    // a sparse sample leaves the step as it runs.  `seen` counts every launch, `launches` the bracketed ones.
    unsigned stride = 1;
    uint64_t tick = 0;
    bool open = false;  // the launch between gl_prof_begin and gl_prof_end is a bracketed one
    struct Pair {
        hipEvent_t a, b;
        int tag;
    };
    std::vector<Pair> pending;
    double ms[K_NTAGS] = {0, 0, 0, 0, 0};
    uint64_t launches[K_NTAGS] = {0, 0, 0, 0, 0};
    uint64_t seen[K_NTAGS] = {0, 0, 0, 0, 0};
    bool sample(int tag) {
        seen[tag]++;
        return tick++ % stride == 0;
    }
};

// The kernel path of a context, chosen once by sr_ctx_create_ex (after init_pow2: GL_FAST needs the tuned tables built)
enum Path {
    FROG,           // the reference's own rings (frog_ring.hpp, small_rings.hpp)
    SMALL_G24,
    SMALL_B72,
    RT_BABYBEAR,    // register-tiled (ntt_regtile.hpp), 2^12 <= D <= 2^24
    RT_GOLDILOCKS,  // the same for Goldilocks under SR_PLAN_GL_REGTILE (a cross-check)
    GL_FAST,        // tuned Goldilocks (ntt_goldilocks.hpp), 2^8 <= D <= 2^22
    STARK_TUNED,    // Stark, k >= 4: the register-tiled kernels of ntt_stark.hpp on StarkL (SR_PLAN_STARK_GENERIC_ON_LAZY: STARK_LAZY)
    STARK_LAZY,     // Stark: the generic kernels on StarkL (nine 28-bit limbs, lazy carries; stark_lazy.hpp)
    GENERIC         // the generic kernels (ntt_generic.hpp) on the ring's own field
};
// Stark transforms and sums of products run on StarkL (SR_PLAN_STARK_NO_LAZY and D = 1: on sr::Stark)
bool on_stark_lazy(Path p) { return p == STARK_TUNED || p == STARK_LAZY; }

// The context's device buffers, each grow-only (grow() below).  The host-pointer temporaries and the pipeline stages are never
// live in the same call, so they share the HOST_* slots.
enum Buf {
    OPERAND_A,     // operand scratch: the column-stage image of b in a fused ring product (every path), the packed intermediates of the
    OPERAND_B,     // register-tiled path; a two-lane plan carves four chunk buffers out of OPERAND_A (on_lanes)
    WIDE_A,        // the widened operands of packed-u32 calls below D = 4096 (packed_via_wide)
    WIDE_B,
    MATVEC_PARTS,  // the row parts of a short-and-wide small-ring mat-vec
    FOLD_0,        // the partial elements of sr_sum_batch_dev / sr_product_batch_dev; FOLD_0 also holds the small rings' product tree
    FOLD_1,
    HOST_0,        // the host-pointer calls: device copies of their operands and results; the staging buffers of host_pipeline
    HOST_1,        // (HOST_0, HOST_1: a / out and b of its first lane; HOST_2, HOST_3 of its second lane)
    HOST_2,
    HOST_3,
    HOST_4,
    ELEMENT,       // the one element of sr_mul_elem_batch (written by a blocking copy: no other call uses it)
    N_BUFS
};
// graph: a captured graph can hold the buffer (a _dev call may use it), so it may not move once a capture has been seen
// (sr_ctx::scratch_frozen).  The others are used only by host-pointer calls, which hold the context's mutex and synchronise before they
// return.
constexpr struct {
    const char *name;
    bool graph;
} kBufs[N_BUFS] = {{"OPERAND_A", true}, {"OPERAND_B", true}, {"WIDE_A", true}, {"WIDE_B", true}, {"MATVEC_PARTS", true},
                   {"FOLD_0", true},    {"FOLD_1", true},    {"HOST_0", false}, {"HOST_1", false}, {"HOST_2", false},
                   {"HOST_3", false},   {"HOST_4", false},   {"ELEMENT", false}};
static_assert(kBufs[N_BUFS - 1].name != nullptr, "one kBufs entry per buffer");

}  // namespace

struct sr_ctx {
    int ring = 0;
    int k = 0;          // log2 D (pow2 rings)
    size_t degree = 0;  // D
    int limbs = 1;      // u64 limbs per coefficient
    int device = 0;
    int log_tile = 12;
    Path path = GENERIC;
    sr::rt::Hooks rt_hooks{};
    sr_plan plan{};         // fixed at creation (sr_ctx_create_ex); the library reads no environment variable
    void *buf[N_BUFS] = {};
    size_t buf_bytes[N_BUFS] = {};
    // the graph-held buffers are shared by every call on this context: a call on another stream first waits for the previous user
    hipEvent_t scratch_free = nullptr;
    hipStream_t scratch_stream = nullptr;
    bool scratch_used = false;
    void *tables = nullptr;  // [tw (D elems) | itw (D elems)] in table form
    size_t table_bytes = 0;
    // inverse stage-0 constants (table form): plain inverse, and fused ring-mul (with boundary correction)
    unsigned char inv_scale0[40], inv_scale1[40], mul_scale0[40], mul_scale1[40];
    bool stark_one_tile = false;  // the ring element is one tile of st::tile_kernel (D <= 2048 unless SR_ST_WHOLE_MAX says otherwise)
    sr::GlLanes gl_lanes;  // the two-lane plans (tuned Goldilocks, register-tiled) on two internal streams (events created on first use)
    // sr_plan.lanes = 0 (auto): the plan the context settled on -- 0 undecided, 1 one stream, 2 two lanes -- measured ONCE on this
    // process's actual stream-to-hardware-queue mapping (lanes_autoselect); lanes_probe_ms = what the two plans took ([0] two lanes,
    // [1] one stream; 0 = not measured).  probe_chunk != 0 only while the probe runs: the one-stream plan's chunk for that run.
    int lanes_choice = 0;
    double lanes_probe_ms[2] = {0, 0};
    size_t lanes_probe_elems = 0;
    size_t probe_chunk = 0;
    bool probing = false;
    // A _dev call has been seen on a stream under capture: a captured graph holds the graph-held buffers of this context, so they may
    // no longer move -- from then on only sr_ctx_reserve_scratch (explicit, blocking, documented to invalidate earlier graphs) grows
    // one; an asynchronous call that would have to fails with SR_E_INVALID instead of freeing memory a graph still writes to.
    bool scratch_frozen = false;
    hipStream_t stream = nullptr;
    hipStream_t out_stream = nullptr;  // device-to-host copies of the chunked host pipeline
    unsigned long long *d_counter = nullptr;
    std::mutex mu;
    Prof prof;
    sr::SmallRingConsts small{};
    sr::FrogConsts frog{};
    sr::GoldilocksFastTables gl_fast{};
};

namespace {

struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};
// The preamble of an entry point once its arguments are checked: the context's mutex, then its device; st = the caller's stream
struct Call {
    std::lock_guard<std::mutex> lk;
    DeviceGuard g;
    hipStream_t st;
    explicit Call(sr_ctx *c, void *stream = nullptr) : lk(c->mu), g(c->device), st((hipStream_t)stream) {}
};

// RAII for optional per-kernel event timing on the launch stream
struct ProfScope {
    sr_ctx *c;
    hipStream_t s;
    int tag;
    hipEvent_t a = nullptr, b = nullptr;
    bool sampled = false;
    ProfScope(sr_ctx *ctx, hipStream_t st, int t) : c(ctx), s(st), tag(t) {
        sampled = c->prof.on && c->prof.sample(tag);
        if (sampled) {
            (void)hipEventCreate(&a);
            (void)hipEventCreate(&b);
            (void)hipEventRecord(a, s);
        }
    }
    ~ProfScope() {
        if (sampled) {
            (void)hipEventRecord(b, s);
            c->prof.pending.push_back({a, b, tag});
        }
    }
};

// timing hooks handed to the tuned Goldilocks launcher (tags: 0 strided fwd, 1 rows, 2 strided inv)
void gl_prof_begin(void *user, int tag, hipStream_t st) {
    sr_ctx *c = (sr_ctx *)user;
    c->prof.open = false;
    if (!c->prof.on) return;
    Prof::Pair p;
    p.tag = tag == 0 ? K_FWD_COLS : (tag == 1 ? K_ROWS : K_INV_COLS);
    if (!c->prof.sample(p.tag)) return;
    (void)hipEventCreate(&p.a);
    (void)hipEventCreate(&p.b);
    (void)hipEventRecord(p.a, st);
    c->prof.pending.push_back(p);
    c->prof.open = true;
}
void gl_prof_end(void *user, hipStream_t st) {
    sr_ctx *c = (sr_ctx *)user;
    if (!c->prof.open || c->prof.pending.empty()) return;
    (void)hipEventRecord(c->prof.pending.back().b, st);
    c->prof.open = false;
}

template <class F>
void exponent_pm1_shift(int shift, uint64_t out[4]);  // (p-1) >> shift
template <>
void exponent_pm1_shift<sr::Goldilocks>(int shift, uint64_t out[4]) {
    out[0] = shift < 64 ? (sr::Goldilocks::P - 1) >> shift : 0;
    out[1] = out[2] = out[3] = 0;
}
template <>
void exponent_pm1_shift<sr::BabyBear>(int shift, uint64_t out[4]) {
    out[0] = shift < 64 ? ((uint64_t)sr::BabyBear::P - 1) >> shift : 0;
    out[1] = out[2] = out[3] = 0;
}
template <>
void exponent_pm1_shift<sr::Stark>(int shift, uint64_t out[4]) {
    const uint64_t pm1[4] = {0, 0, 0, 0x0800000000000011ull};
    int ws = shift / 64, bs = shift % 64;
    for (int i = 0; i < 4; i++) {
        uint64_t lo = i + ws < 4 ? pm1[i + ws] : 0, hi = i + ws + 1 < 4 ? pm1[i + ws + 1] : 0;
        out[i] = bs ? (lo >> bs) | (hi << (64 - bs)) : lo;
    }
}
template <>
void exponent_pm1_shift<sr::StarkL>(int shift, uint64_t out[4]) {
    exponent_pm1_shift<sr::Stark>(shift, out);
}
template <class F>
void exponent_pm2(uint64_t out[4]);  // p - 2
template <>
void exponent_pm2<sr::Goldilocks>(uint64_t out[4]) {
    out[0] = sr::Goldilocks::P - 2;
    out[1] = out[2] = out[3] = 0;
}
template <>
void exponent_pm2<sr::BabyBear>(uint64_t out[4]) {
    out[0] = (uint64_t)sr::BabyBear::P - 2;
    out[1] = out[2] = out[3] = 0;
}
template <>
void exponent_pm2<sr::Stark>(uint64_t out[4]) {
    out[0] = out[1] = out[2] = ~0ull;
    out[3] = 0x0800000000000010ull;
}
template <>
void exponent_pm2<sr::StarkL>(uint64_t out[4]) {
    exponent_pm2<sr::Stark>(out);
}
template <class F>
constexpr int kappa_bits() {  // mul_tw(x, y) = x * y * 2^-kappa_bits
    return std::is_same<F, sr::Goldilocks>::value ? 0
           : (std::is_same<F, sr::BabyBear>::value ? 32 : (std::is_same<F, sr::StarkL>::value ? sr::StarkL::kTableBits : 256));
}
template <class F>
constexpr int default_log_tile() {
    // Stark: 512 coefficients x 32 B = 16 KiB per tile (two tiles in the fused product): five workgroups per CU.  With 1024
    // coefficients (two per CU) the rows kernel took 3.23 ms at D = 2^12, batch 2^12; with 512 it takes 2.39 ms.
    return (std::is_same<F, sr::Stark>::value || std::is_same<F, sr::StarkL>::value) ? 9 : 12;
}

template <class F>
typename F::elem inv_tw(typename F::elem x) {
    uint64_t e[4];
    exponent_pm2<F>(e);
    return sr::pow_tw<F>(x, e, 4);
}
template <class F>
typename F::elem pow_small(typename F::elem x, uint64_t e) {
    uint64_t w[1] = {e};
    return sr::pow_tw<F>(x, w, 1);
}

template <class F>
int init_pow2(sr_ctx *c, bool stark_tuned = false) {
    using E = typename F::elem;
    const int k = c->k;
    if (k > F::kTwoAdicity - 1) return fail(SR_E_INVALID, "log2_degree exceeds the field's 2-adicity");
    c->log_tile = default_log_tile<F>();
    if (c->plan.log_tile >= 8 && c->plan.log_tile <= 12) c->log_tile = c->plan.log_tile;  // tuning knob of the generic kernels
    if (k > 2 * c->log_tile && !stark_tuned) return fail(SR_E_INVALID, "log2_degree too large for the two-level kernels");
    const size_t d = c->degree;
    size_t extra = 0;
    if constexpr (std::is_same<F, sr::Goldilocks>::value) extra = sr::gl_fast_extra_bytes(k);
    c->table_bytes = 2 * d * sizeof(E) + extra;
    HIP_TRY(hipMalloc(&c->tables, c->table_bytes));

    // psi = g^((p-1)/2D)  (equals ROOTS_OF_UNITY_32[1] for Stark, D = 16)
    uint64_t e[4];
    exponent_pm1_shift<F>(k + 1, e);
    E psi = sr::pow_tw<F>(F::tw_from_u64(F::kGenerator), e, 4);
    E psi_inv = inv_tw<F>(psi);
    std::vector<E> pows(k + 1), ipows(k + 1);
    pows[0] = psi;
    ipows[0] = psi_inv;
    for (int j = 1; j <= k; j++) {
        pows[j] = F::mul_tw(pows[j - 1], pows[j - 1]);
        ipows[j] = F::mul_tw(ipows[j - 1], ipows[j - 1]);
    }
    E *d_pows = nullptr;
    HIP_TRY(hipMalloc(&d_pows, 2 * (k + 1) * sizeof(E)));
    HIP_TRY(hipMemcpy(d_pows, pows.data(), (k + 1) * sizeof(E), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_pows + (k + 1), ipows.data(), (k + 1) * sizeof(E), hipMemcpyHostToDevice));
    E *tw = (E *)c->tables, *itw = tw + d;
    unsigned blocks = (unsigned)((d + 255) / 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(sr::build_tables_kernel<F>, dim3(blocks), dim3(256), 0, c->stream, tw, itw, k, d_pows,
                       d_pows + (k + 1));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipFree(d_pows));

    // inverse stage-0 constants.  D^-1, and for the fused product D^-1 * kappa / R_b so that
    // mul_tw(A~, B~) (= A B R_b^2 / kappa) comes out as (A B) R_b, the in-memory image of the product.
    E dinv = inv_tw<F>(F::tw_from_u64((uint64_t)d));
    E two = F::tw_from_u64(2);
    E kappa = pow_small<F>(two, kappa_bits<F>());
    E rb_inv = inv_tw<F>(pow_small<F>(two, F::kBoundaryBits));
    E fused = F::mul_tw(dinv, F::mul_tw(kappa, rb_inv));
    E half_turn_inv = k >= 1 ? ipows[k - 1] : F::tw_one();  // psi^-(D/2) = itw[1]
    E s0 = sr::Lazy<F>::table(dinv), s1 = sr::Lazy<F>::table(F::mul_tw(dinv, half_turn_inv));
    E m0 = sr::Lazy<F>::table(fused), m1 = sr::Lazy<F>::table(F::mul_tw(fused, half_turn_inv));
    memcpy(c->inv_scale0, &s0, sizeof(E));
    memcpy(c->inv_scale1, &s1, sizeof(E));
    memcpy(c->mul_scale0, &m0, sizeof(E));
    memcpy(c->mul_scale1, &m1, sizeof(E));
    if constexpr (std::is_same<F, sr::Goldilocks>::value) {
        // tuned-path tables live right behind [tw | itw] so one broadcast of the block ships everything
        if (sr::gl_fast_init(c->gl_fast, k, (const uint64_t *)tw, (const uint64_t *)itw, (uint64_t *)(itw + d),
                             (const uint64_t *)pows.data(), (const uint64_t *)ipows.data(), (uint64_t)dinv,
                             (uint64_t)fused, !(c->plan.flags & SR_PLAN_GL_NO_COLS256), c->plan.chunk_polys, c->stream))
            return fail(SR_E_HIP, "goldilocks fast-path table build failed");
        c->gl_fast.keep_cols = !(c->plan.flags & SR_PLAN_GL_PLAIN_COLS);
        c->gl_fast.split_rows = (c->plan.flags & SR_PLAN_GL_SPLIT_ROWS) != 0 && k > 12;
    }
    return SR_OK;
}

template <class F>
sr::NttParams<F> make_params(const sr_ctx *c, bool fused) {
    using E = typename F::elem;
    sr::NttParams<F> p;
    p.k = c->k;
    p.log_tile = c->log_tile;
    p.s_rows = c->k > c->log_tile ? c->k - c->log_tile : 0;
    p.tw = (const E *)c->tables;
    p.itw = p.tw + c->degree;
    memcpy(&p.scale0, fused ? c->mul_scale0 : c->inv_scale0, sizeof(E));
    memcpy(&p.scale1, fused ? c->mul_scale1 : c->inv_scale1, sizeof(E));
    return p;
}

template <class F>
size_t lds_bytes(const sr_ctx *c, bool two_buffers) {
    return ((size_t)F::kLdsWords * 4u << c->log_tile) * (two_buffers ? 2 : 1);
}

template <class F, int MODE>
int launch_rows(sr_ctx *c, typename F::storage *a, const typename F::storage *b, typename F::storage *out,
                size_t batch, bool fused_scale, hipStream_t st) {
    const size_t n = batch << c->k;
    const size_t tiles = (n + ((size_t)1 << c->log_tile) - 1) >> c->log_tile;
    if (tiles > 0x7FFFFFFFull) return fail(SR_E_INVALID, "batch too large for one launch");
    auto p = make_params<F>(c, fused_scale);
    ProfScope ps(c, st, K_ROWS);
    hipLaunchKernelGGL((sr::rows_kernel<F, MODE>), dim3((unsigned)tiles), dim3(sr::kThreads),
                       lds_bytes<F>(c, MODE == sr::MODE_MUL), st, a, b, out, n, p);
    HIP_TRY(hipGetLastError());
    return SR_OK;
}
template <class F, int MODE>
int launch_cols(sr_ctx *c, typename F::storage *a, const typename F::storage *src, size_t batch, bool fused_scale, hipStream_t st) {
    const size_t blocks = batch << (c->k - c->log_tile);
    if (blocks > 0x7FFFFFFFull) return fail(SR_E_INVALID, "batch too large for one launch");
    auto p = make_params<F>(c, fused_scale);
    ProfScope ps(c, st, MODE == sr::MODE_FWD ? K_FWD_COLS : K_INV_COLS);
    hipLaunchKernelGGL((sr::cols_kernel<F, MODE>), dim3((unsigned)blocks), dim3(sr::kThreads), lds_bytes<F>(c, false),
                       st, a, src, batch, p);
    HIP_TRY(hipGetLastError());
    return SR_OK;
}

template <class F>
int fwd_dev(sr_ctx *c, uint64_t *d, size_t batch, hipStream_t st) {
    auto *a = reinterpret_cast<typename F::storage *>(d);
    if (c->k == 0 || batch == 0) return SR_OK;
    if (c->k > c->log_tile) {
        int rc = launch_cols<F, sr::MODE_FWD>(c, a, a, batch, false, st);
        if (rc) return rc;
    }
    return launch_rows<F, sr::MODE_FWD>(c, a, nullptr, a, batch, false, st);
}
template <class F>
int inv_dev(sr_ctx *c, uint64_t *d, size_t batch, hipStream_t st) {
    auto *a = reinterpret_cast<typename F::storage *>(d);
    if (c->k == 0 || batch == 0) return SR_OK;
    int rc = launch_rows<F, sr::MODE_INV>(c, a, nullptr, a, batch, false, st);
    if (rc) return rc;
    if (c->k > c->log_tile) return launch_cols<F, sr::MODE_INV>(c, a, a, batch, false, st);
    return SR_OK;
}
template <class F>
int pointwise_bcast_dev(sr_ctx *c, uint64_t *lhs, const uint64_t *r, size_t n_coeffs, hipStream_t st) {
    if (n_coeffs == 0) return SR_OK;
    ProfScope ps(c, st, K_POINTWISE);
    hipLaunchKernelGGL(sr::pointwise_bcast_kernel<F>, dim3(sr::stream_blocks<F>(n_coeffs)), dim3(256), 0, st,
                       reinterpret_cast<typename F::storage *>(lhs), reinterpret_cast<const typename F::storage *>(r), n_coeffs,
                       (size_t)c->degree - 1);
    HIP_TRY(hipGetLastError());
    return SR_OK;
}
template <class F>
int pointwise_dev(sr_ctx *c, uint64_t *lhs, const uint64_t *rhs, size_t n_coeffs, hipStream_t st) {
    if (n_coeffs == 0) return SR_OK;
    const unsigned blocks = sr::stream_blocks<F>(n_coeffs);
    ProfScope ps(c, st, K_POINTWISE);
    hipLaunchKernelGGL(sr::pointwise_kernel<F>, dim3((unsigned)blocks), dim3(256), 0, st,
                       reinterpret_cast<typename F::storage *>(lhs),
                       reinterpret_cast<const typename F::storage *>(rhs), n_coeffs);
    HIP_TRY(hipGetLastError());
    return SR_OK;
}
template <class F>
int addsub_dev(sr_ctx *c, uint64_t *lhs, const uint64_t *rhs, size_t n_coeffs, bool sub, hipStream_t st) {
    if (n_coeffs == 0) return SR_OK;
    const unsigned blocks = sr::stream_blocks<F>(n_coeffs);
    ProfScope ps(c, st, K_POINTWISE);
    auto *l = reinterpret_cast<typename F::storage *>(lhs);
    auto *r = reinterpret_cast<const typename F::storage *>(rhs);
    if (sub)
        hipLaunchKernelGGL((sr::addsub_kernel<F, true>), dim3((unsigned)blocks), dim3(256), 0, st, l, r, n_coeffs);
    else
        hipLaunchKernelGGL((sr::addsub_kernel<F, false>), dim3((unsigned)blocks), dim3(256), 0, st, l, r, n_coeffs);
    HIP_TRY(hipGetLastError());
    return SR_OK;
}
template <class F>
int matvec_dev(sr_ctx *c, uint64_t *y, const uint64_t *m, const uint64_t *v, size_t nrows, size_t ncols, hipStream_t st) {
    using S = typename F::storage;
    if (nrows == 0) return SR_OK;
    // RB rows share each v[c] slot a lane loads; small problems (few slots x rows) take a smaller RB so that the grid still
    // covers the chip: the largest RB that leaves at least four workgroups per CU
    const size_t chunks = (c->degree + 255) / 256;
    int rb = 4;
    while (rb > 1 && chunks * ((nrows + rb - 1) / rb) < 4096) rb >>= 1;
    const size_t blocks = chunks * ((nrows + rb - 1) / rb);
    if (blocks > 0x7FFFFFFFull) return fail(SR_E_INVALID, "matvec: too many rows for one launch");
    ProfScope ps(c, st, K_OTHER);
    S *py = reinterpret_cast<S *>(y);
    const S *pm = reinterpret_cast<const S *>(m), *pv = reinterpret_cast<const S *>(v);
    const dim3 g((unsigned)blocks), b(256);
    if (rb == 4) hipLaunchKernelGGL((sr::matvec_kernel<F, 4>), g, b, 0, st, py, pm, pv, nrows, ncols, c->k);
    else if (rb == 2) hipLaunchKernelGGL((sr::matvec_kernel<F, 2>), g, b, 0, st, py, pm, pv, nrows, ncols, c->k);
    else hipLaunchKernelGGL((sr::matvec_kernel<F, 1>), g, b, 0, st, py, pm, pv, nrows, ncols, c->k);
    HIP_TRY(hipGetLastError());
    return SR_OK;
}
template <class F>
int spmv_dev(sr_ctx *c, uint64_t *y, const uint64_t *vals, const uint32_t *cols, const uint64_t *row_ptr, const uint64_t *v,
             size_t nrows, size_t ncols, hipStream_t st) {
    using S = typename F::storage;
    if (nrows == 0) return SR_OK;
    const size_t blocks = ((c->degree + 255) / 256) * nrows;
    if (blocks > 0x7FFFFFFFull) return fail(SR_E_INVALID, "spmv: too many rows for one launch");
    ProfScope ps(c, st, K_OTHER);
    hipLaunchKernelGGL((sr::spmv_kernel<F>), dim3((unsigned)blocks), dim3(256), 0, st,
                       reinterpret_cast<S *>(y), reinterpret_cast<const S *>(vals), cols, row_ptr, reinterpret_cast<const S *>(v),
                       ncols, c->k, c->d_counter + 1);
    HIP_TRY(hipGetLastError());
    return SR_OK;
}
template <class F>
int matmul_dev(sr_ctx *c, uint64_t *y, const uint64_t *a, const uint64_t *b, size_t n, size_t m, size_t p, hipStream_t st) {
    using S = typename F::storage;
    if (n == 0 || p == 0) return SR_OK;
    // register block of outputs per lane: RB + CB operand loads feed RB * CB multiply-adds.  BabyBear's accumulators are one
    // register each (8 x 4); Goldilocks' 96-bit sums and Stark's nine limbs cost 12 and 10 (4 x 2).
    constexpr bool bb = std::is_same<F, sr::BabyBear>::value;
    constexpr int RB = bb ? 8 : 4, CB = bb ? 4 : 2;
    const size_t blocks = ((c->degree + 255) / 256) * ((n + RB - 1) / RB) * ((p + CB - 1) / CB);
    if (blocks > 0x7FFFFFFFull) return fail(SR_E_INVALID, "matmul: too many rows or columns for one launch");
    ProfScope ps(c, st, K_OTHER);
    hipLaunchKernelGGL((sr::matmul_kernel<F, RB, CB>), dim3((unsigned)blocks),
                       dim3(256), 0, st, reinterpret_cast<S *>(y), reinterpret_cast<const S *>(a), reinterpret_cast<const S *>(b),
                       n, m, p, c->k);
    HIP_TRY(hipGetLastError());
    return SR_OK;
}
// remembers that a call arrived on a capturing stream (sr_ctx::scratch_frozen); true while `st` is being captured
bool note_capture(sr_ctx *c, hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (st && hipStreamIsCapturing(st, &cs) == hipSuccess && cs == hipStreamCaptureStatusActive) {
        c->scratch_frozen = true;
        return true;
    }
    (void)hipGetLastError();
    return false;
}
// Grows buffer b of the context to at least `bytes` (0 counts as 8, so that a temporary is never null); nothing is allocated or freed
// once warm.  st = the stream of the call that needs it (the null stream is a caller's stream like any other); reserving = the call is
// sr_ctx_reserve_scratch, the one place that may grow a graph-held buffer after a capture has been seen.  A hipMalloc here is why the
// very first call of a given size is not graph-capturable.
int grow(sr_ctx *c, Buf b, size_t bytes, hipStream_t st = nullptr, bool reserving = false) {
    if (bytes == 0) bytes = 8;
    const bool capturing = kBufs[b].graph && !reserving && note_capture(c, st);
    if (c->buf_bytes[b] >= bytes) return SR_OK;
    if (capturing || (kBufs[b].graph && !reserving && c->scratch_frozen))
        return fail(SR_E_INVALID, std::string("context buffer ") + kBufs[b].name +
                                      " would have to grow, but a stream capture has used it (a captured graph holds its address): call "
                                      "sr_ctx_reserve_scratch for the largest batch BEFORE capturing (include/stark_rings_hip.h)");
    if (c->buf[b]) {
        HIP_TRY(hipDeviceSynchronize());  // a _dev call on another stream may still be using the smaller buffer
        HIP_TRY(hipFree(c->buf[b]));
        c->buf[b] = nullptr;
        c->buf_bytes[b] = 0;
    }
    hipError_t e = hipMalloc(&c->buf[b], bytes);
    if (e != hipSuccess) {
        c->buf[b] = nullptr;
        return fail(SR_E_ALLOC, std::string("hipMalloc ") + kBufs[b].name + ": " + hipGetErrorString(e));
    }
    c->buf_bytes[b] = bytes;
    return SR_OK;
}
// One use of the graph-held buffers by a call on stream st (callers hold the context's mutex, so the bookkeeping itself is serialised).
// The release (an event recorded on st, which the next user on another stream waits for) happens on EVERY exit path once acquire()
// succeeded -- also after a failed launch, when earlier launches of the same call may still be using the buffers.
struct ScratchUse {
    sr_ctx *c;
    hipStream_t st;
    bool held = false;
    ScratchUse(sr_ctx *ctx, hipStream_t s) : c(ctx), st(s) {}
    int acquire() {
        note_capture(c, st);
        if (!c->scratch_free) HIP_TRY(hipEventCreateWithFlags(&c->scratch_free, hipEventDisableTiming));
        if (c->scratch_used && c->scratch_stream != st) HIP_TRY(hipStreamWaitEvent(st, c->scratch_free, 0));
        held = true;
        return SR_OK;
    }
    int release() {
        held = false;
        if (!c->scratch_free) HIP_TRY(hipEventCreateWithFlags(&c->scratch_free, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(c->scratch_free, st));
        c->scratch_stream = st;
        c->scratch_used = true;
        return SR_OK;
    }
    ~ScratchUse() {
        if (held) (void)release();
    }
};
// ring elements of elem_bytes each the operand scratch may hold for a batch (plan cap; at least one element)
size_t scratch_polys(const sr_ctx *c, size_t batch, size_t elem_bytes) {
    const size_t cap = c->plan.scratch_limit_bytes ? (size_t)c->plan.scratch_limit_bytes : ((size_t)16 << 30);
    size_t n = cap / elem_bytes;
    if (n == 0) n = 1;
    if (c->plan.chunk_polys && n > c->plan.chunk_polys) n = c->plan.chunk_polys;
    return n < batch ? n : batch;
}
// lanes the context runs its chunked products on: the plan's explicit choice, else what the probe settled on (two until it has run)
int effective_lanes(const sr_ctx *c) { return c->plan.lanes ? (int)c->plan.lanes : (c->lanes_choice ? c->lanes_choice : 2); }
// Small batches are the other regime: a set of launches over fewer elements than one lane chunk (64 MiB of coefficients) no longer fills
// the chip, so a batch is never cut below that -- 64 Goldilocks elements of degree 2^16 as eight chunks of eight took 0.339 ms, as ONE
// set of launches 0.085 ms; 128: 0.378 against 0.147 (tools/bench_small_batches.py).
size_t lane_chunk_default(const sr_ctx *c, size_t elem_bytes) {
    (void)c;
    const size_t n = ((size_t)64 << 20) / elem_bytes;
    return n ? n : 1;
}
// tuned Goldilocks path: a large batch runs as eight chunks of launches (unless the plan fixes chunk_polys) -- measured on config 2:
// 18.6 ms as one set of launches, 18.27 / 18.3 / 18.5 ms in chunks of 2048 / 4096 / 1024 ring elements (the inverse column pass
// finds part of the rows kernel's output still in the Infinity Cache), and the operand scratch is an eighth of the batch
size_t gl_chunk_polys(const sr_ctx *c, size_t batch) {
    if (c->probe_chunk) return c->probe_chunk < batch ? c->probe_chunk : batch;  // the probe times ONE set of launches of the real chunk size
    size_t chunk = scratch_polys(c, batch, (size_t)8 << c->k);
    const size_t eighth = (batch + 7) / 8;
    if (!c->plan.chunk_polys && eighth >= lane_chunk_default(c, (size_t)8 << c->k) && chunk > eighth) chunk = eighth;
    return chunk;
}
// bytes of one ring element in the scratch of the two-lane plans: packed words on the register-tiled BabyBear path, else 8-byte words
size_t lane_elem_bytes(const sr_ctx *c) { return (size_t)(c->path == RT_BABYBEAR ? 4 : 8) << c->k; }
// Two-lane plans of the tuned Goldilocks product (cols256) and of the register-tiled path: chunk of a lane in ring elements -- 64 MiB
// of words per scratch buffer by default, so that the four buffers of the two lanes are the 256 MiB of the Infinity Cache -- capped by
// the plan's scratch limit (four buffers) and by sr_plan.chunk_polys when set.
size_t lane_chunk(const sr_ctx *c) {
    const size_t elem = lane_elem_bytes(c);
    size_t chunk = c->plan.chunk_polys ? (size_t)c->plan.chunk_polys : (((size_t)64 << 20) / elem);
    const size_t cap = c->plan.scratch_limit_bytes ? (size_t)c->plan.scratch_limit_bytes : ((size_t)16 << 30);
    if (chunk > cap / (4 * elem)) chunk = cap / (4 * elem);
    return chunk ? chunk : 1;
}
// Two lanes pay from three and a half chunks on: below, one set of launches on the caller's stream is faster -- Goldilocks degree 2^16:
// 256 elements 0.256 against 0.273 ms, 288 0.287 against 0.338, 384 0.385 against 0.413, 448 level, 512 0.522 against 0.498, 640 0.655
// against 0.633; degree 2^20: 24 elements 0.491 against 0.533, 40 level; BabyBear 2^16: 768 0.513 against 0.532, 1 280 0.887 against
// 0.858 (tools/bench_small_batches.py).  (Three chunks on two lanes are two on one and one on the other.)  A plan that fixes
// chunk_polys gets its chunks on the lanes as soon as there are two.
bool lanes_pay(const sr_ctx *c, size_t batch, size_t lane_chunk) {
    return c->plan.chunk_polys ? batch > lane_chunk : 2 * batch >= 7 * lane_chunk;
}
// The stand-alone transforms (two launches per chunk, in place) need more chunks before the lanes pay: at four chunks one set of
// launches on the caller's stream is a quarter faster (512 Goldilocks elements of degree 2^16: 0.169 against 0.222 ms; 32 of degree
// 2^20: 0.210 against 0.268; 1 024 BabyBear: 0.251 against 0.294), at eight the two are level (tools/bench_small_transforms.py).
bool lanes_pay_transform(const sr_ctx *c, size_t batch, size_t lane_chunk) {
    return c->plan.chunk_polys ? batch > lane_chunk : batch >= 8 * lane_chunk;
}
// A call of the tuned Goldilocks path (cols256 plans only) or of the register-tiled path takes the lanes when the plan allows them
// (sr_plan.lanes != 1), the batch has enough chunks for them to pay, and the call is not on the lanes themselves: the host-pointer
// pipeline drives the device calls on the very streams the lanes are (and is bound by PCIe anyway).
bool use_lanes(const sr_ctx *c, size_t batch, hipStream_t st, bool transform) {
    if (effective_lanes(c) == 1 || c->k <= 12 || st == c->stream || st == c->out_stream) return false;
    if (c->path == GL_FAST && !c->gl_fast.cols256) return false;
    return transform ? lanes_pay_transform(c, batch, lane_chunk(c)) : lanes_pay(c, batch, lane_chunk(c));
}
int gl_lanes_init(sr_ctx *c) {
    sr::GlLanes &L = c->gl_lanes;
    if (L.n) return SR_OK;
    HIP_TRY(hipEventCreateWithFlags(&L.fork, hipEventDisableTiming));
    // The runtime multiplexes streams onto a few hardware queues (GPU_MAX_HW_QUEUES, 4 by default) and two streams that share
    // one run one after the other -- measured inside a PyTorch process: 20.4 ms per config-2 batch with two NEW streams for the
    // lanes (the fifth stream of the process landed on a lane's queue), 16.3 ms with a queue each.  Different stream priorities
    // do separate the queues but starve the lower lane (17.9 ms).  So the lanes are the two streams the context owns anyway (the
    // host-pointer pipeline's; idle during a device call, and any earlier work on them simply runs first); a process that holds
    // more streams than hardware queues should raise GPU_MAX_HW_QUEUES (bench.py does).
    L.st[0] = c->stream;
    L.st[1] = c->out_stream;
    for (int i = 0; i < 2; i++) HIP_TRY(hipEventCreateWithFlags(&L.join[i], hipEventDisableTiming));
    L.n = 2;
    return SR_OK;
}
// A batch on the two lanes with per-lane scratch: lane i gets buffers 2i and 2i + 1 of four chunk-sized buffers in OPERAND_A, and
// body(first, n, s0, s1, lane stream) enqueues the launches of elements [first, first + n).  `what`: the error of a failed launch.
template <class Body>
int on_lanes(sr_ctx *c, size_t batch, hipStream_t st, const char *what, Body body) {
    const size_t chunk = lane_chunk(c), bytes = chunk * lane_elem_bytes(c);
    if (int rc = grow(c, OPERAND_A, 4 * bytes, st)) return rc;
    if (int rc = gl_lanes_init(c)) return rc;
    ScratchUse su(c, st);
    if (int rc = su.acquire()) return rc;
    char *base = static_cast<char *>(c->buf[OPERAND_A]);
    const int rc = sr::for_each_lane_chunk(c->gl_lanes, batch, chunk, st, [&](int i, size_t first, size_t n, hipStream_t lane) {
        return body(first, n, (void *)(base + (size_t)(2 * i) * bytes), (void *)(base + (size_t)(2 * i + 1) * bytes), lane);
    });
    if (int r2 = su.release()) return r2;
    return rc ? fail(SR_E_HIP, what) : SR_OK;
}
template <class F>
int ring_mul_dev(sr_ctx *c, uint64_t *out, const uint64_t *a, const uint64_t *b, size_t batch, hipStream_t st) {
    using S = typename F::storage;
    if (batch == 0) return SR_OK;
    if constexpr (!sr::Lazy<F>::value) {  // (a lazy field is never selected for D = 1)
        if (c->k == 0) {  // D = 1: the ring is Fp itself
            if (out != a) HIP_TRY(hipMemcpyAsync(out, a, batch * sizeof(S), hipMemcpyDeviceToDevice, st));
            return pointwise_dev<F>(c, out, b, batch, st);
        }
    }
    if (c->k > c->log_tile) {
        // first (strided) forward stages of both operands: a's go straight to out, b's into the operand scratch, so that
        // neither operand is written (coeff_form.rs:250-258); batches beyond the scratch cap run in chunks
        const size_t elem = sizeof(S) << c->k;
        const size_t chunk = scratch_polys(c, batch, elem);
        if (int rc = grow(c, OPERAND_A, chunk * elem, st)) return rc;
        ScratchUse su(c, st);
        if (int rc = su.acquire()) return rc;
        S *sb = reinterpret_cast<S *>(c->buf[OPERAND_A]);
        for (size_t e = 0; e < batch; e += chunk) {
            const size_t n = batch - e < chunk ? batch - e : chunk;
            S *o = reinterpret_cast<S *>(out) + (e << c->k);
            int rc = launch_cols<F, sr::MODE_FWD>(c, o, reinterpret_cast<const S *>(a) + (e << c->k), n, true, st);
            if (rc) return rc;
            rc = launch_cols<F, sr::MODE_FWD>(c, sb, reinterpret_cast<const S *>(b) + (e << c->k), n, true, st);
            if (rc) return rc;
            rc = launch_rows<F, sr::MODE_MUL>(c, o, sb, o, n, true, st);
            if (rc) return rc;
            rc = launch_cols<F, sr::MODE_INV>(c, o, o, n, true, st);
            if (rc) return rc;
        }
        return su.release();
    }
    return launch_rows<F, sr::MODE_MUL>(c, reinterpret_cast<S *>(const_cast<uint64_t *>(a)),
                                        reinterpret_cast<const S *>(b), reinterpret_cast<S *>(out), batch, true, st);
}
template <class F>
int reduce_dev(sr_ctx *c, const uint64_t *in, size_t in_len, uint64_t *out, size_t batch, hipStream_t st) {
    if (in_len > 2 * c->degree) return fail(SR_E_INVALID, "reduce: in_len_per_elem > 2D");
    if (batch == 0) return SR_OK;
    size_t n = batch << c->k;
    const unsigned blocks = sr::stream_blocks<F>(n);
    ProfScope ps(c, st, K_OTHER);
    hipLaunchKernelGGL(sr::reduce_pow2_kernel<F>, dim3((unsigned)blocks), dim3(256), 0, st,
                       reinterpret_cast<const typename F::storage *>(in), in_len,
                       reinterpret_cast<typename F::storage *>(out), c->k, batch);
    HIP_TRY(hipGetLastError());
    return SR_OK;
}
template <class F>
int fill_dev(sr_ctx *c, uint64_t seed, uint64_t first, size_t n, uint64_t *out, hipStream_t st) {
    if (n == 0) return SR_OK;
    size_t blocks = (n + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    ProfScope ps(c, st, K_OTHER);
    hipLaunchKernelGGL(sr::fill_uniform_kernel<F>, dim3((unsigned)blocks), dim3(256), 0, st, seed, first, n, out);
    HIP_TRY(hipGetLastError());
    return SR_OK;
}
template <class F>
int count_dev(sr_ctx *c, const uint64_t *d, size_t n, uint64_t *host_count, hipStream_t st) {
    HIP_TRY(hipMemsetAsync(c->d_counter, 0, sizeof(unsigned long long), st));
    if (n) {
        size_t blocks = (n + 255) / 256;
        if (blocks > 8192) blocks = 8192;
        hipLaunchKernelGGL(sr::count_noncanonical_kernel<F>, dim3((unsigned)blocks), dim3(256), 0, st,
                           reinterpret_cast<const typename F::storage *>(d), n, c->d_counter);
        HIP_TRY(hipGetLastError());
    }
    unsigned long long v = 0;
    HIP_TRY(hipMemcpyAsync(&v, c->d_counter, sizeof v, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *host_count = v;
    return SR_OK;
}

template <class F>
sr::rt::Params<F> make_rt_params(const sr_ctx *c, bool fused) {
    using E = typename F::elem;
    sr::rt::Params<F> p;
    p.k = c->k;
    p.c = c->k - 12;
    p.tw = (const E *)c->tables;
    p.itw = p.tw + c->degree;
    memcpy(&p.scale0, fused ? c->mul_scale0 : c->inv_scale0, sizeof(E));
    memcpy(&p.scale1, fused ? c->mul_scale1 : c->inv_scale1, sizeof(E));
    p.no_cols256 = (c->plan.flags & SR_PLAN_RT_NO_COLS256) != 0;
    return p;
}
// a large batch runs as eight chunks of launches (unless the plan fixes chunk_polys), like the tuned Goldilocks path: measured on
// config 3 (BabyBear D = 2^16, batch 2^14): 11.68 ms as one set of launches, 11.38 / 11.41 / 11.56 ms in chunks of 2048 / 4096 / 1024
// ring elements, 12.4 ms and worse below 512 -- and the packed scratch is an eighth of the batch
size_t rt_chunk_polys(const sr_ctx *c, size_t batch) {
    if (c->probe_chunk) return c->probe_chunk < batch ? c->probe_chunk : batch;
    if (c->plan.chunk_polys) return c->plan.chunk_polys < batch ? c->plan.chunk_polys : batch;
    const size_t eighth = (batch + 7) / 8;   // never below one lane chunk of packed words (see gl_chunk_polys): 128 BabyBear elements of
    return eighth >= lane_chunk_default(c, lane_elem_bytes(c)) ? eighth : batch;   // degree 2^16 took 0.196 ms in eight chunks, 0.095 as one
}
// VB: the view of the caller's words -- sr::rt::Boundary (the reference's 8-byte limbs) or sr::rt::PackedStream (the packed-u32 entry
// points).  DIR 0 forward, 1 inverse.
template <class F, int DIR, class VB = sr::rt::Boundary>
int rt_transform(sr_ctx *c, void *d, size_t batch, hipStream_t st) {
    using E = typename F::elem;
    using S = typename sr::rt::View<F, VB>::T;
    const auto p = make_rt_params<F>(c, false);
    auto run = [&](S *dc, size_t n, void *scratch, hipStream_t s) {
        return DIR == 0 ? sr::rt::fwd<F, VB>(c->rt_hooks, dc, n, p, (E *)scratch, s) : sr::rt::inv<F, VB>(c->rt_hooks, dc, n, p, (E *)scratch, s);
    };
    // chunks on the two lanes, each with its own packed scratch (the product's: one allocation serves both)
    if (use_lanes(c, batch, st, true))
        return on_lanes(c, batch, st, "register-tiled launch failed", [&](size_t first, size_t n, void *s0, void *, hipStream_t lane) {
            return run(reinterpret_cast<S *>(d) + (first << c->k), n, s0, lane);
        });
    if (c->k > 12 && batch)
        if (int rc = grow(c, OPERAND_A, (batch << c->k) * sizeof(E), st)) return rc;
    ScratchUse su(c, st);
    if (int rc = su.acquire()) return rc;
    if (run(reinterpret_cast<S *>(d), batch, c->buf[OPERAND_A], st)) return fail(SR_E_HIP, "register-tiled launch failed");
    return su.release();
}
template <class F, class VB = sr::rt::Boundary>
int rt_ring_mul(sr_ctx *c, void *out, const void *a, const void *b, size_t batch, hipStream_t st) {
    using S = typename sr::rt::View<F, VB>::T;
    using E = typename F::elem;
    if (batch == 0) return SR_OK;
    const auto p = make_rt_params<F>(c, true);
    auto run = [&](size_t first, size_t n, void *s0, void *s1, hipStream_t s) {
        const size_t off = first << c->k;
        return sr::rt::ring_mul<F, VB>(c->rt_hooks, reinterpret_cast<S *>(out) + off, reinterpret_cast<const S *>(a) + off,
                                       reinterpret_cast<const S *>(b) + off, n, p, (E *)s0, (E *)s1, s);
    };
    if (use_lanes(c, batch, st, false)) return on_lanes(c, batch, st, "register-tiled launch failed", run);
    const size_t chunk = c->k > 12 ? rt_chunk_polys(c, batch) : batch;
    if (c->k > 12) {
        if (int rc = grow(c, OPERAND_A, (chunk << c->k) * sizeof(E), st)) return rc;
        if (int rc = grow(c, OPERAND_B, (chunk << c->k) * sizeof(E), st)) return rc;
    }
    ScratchUse su(c, st);
    if (int rc = su.acquire()) return rc;
    for (size_t e = 0; e < batch; e += chunk)
        if (run(e, batch - e < chunk ? batch - e : chunk, c->buf[OPERAND_A], c->buf[OPERAND_B], st))
            return fail(SR_E_HIP, "register-tiled launch failed");
    return su.release();
}

// ---- Stark rings, k >= 4: ntt_stark.hpp ----
int st_fwd(sr_ctx *c, uint64_t *d, size_t batch, hipStream_t st) {
    if (batch == 0) return SR_OK;
    auto p = make_params<sr::StarkL>(c, false);
    auto *a = reinterpret_cast<sr::U256Storage *>(d);
    auto hook = [&](bool begin) { begin ? gl_prof_begin(c, 0, st) : gl_prof_end(c, st); };
    if (sr::st::fwd_cols(a, a, batch, p, c->stark_one_tile, st, hook)) return fail(SR_E_HIP, "stark strided launch failed");
    ProfScope ps(c, st, K_ROWS);
    if (sr::st::launch_rows<sr::MODE_FWD>(a, nullptr, a, batch, p, c->stark_one_tile, st)) return fail(SR_E_HIP, "stark rows launch failed");
    return SR_OK;
}
int st_inv(sr_ctx *c, uint64_t *d, size_t batch, hipStream_t st) {
    if (batch == 0) return SR_OK;
    auto p = make_params<sr::StarkL>(c, false);
    auto *a = reinterpret_cast<sr::U256Storage *>(d);
    {
        ProfScope ps(c, st, K_ROWS);
        if (sr::st::launch_rows<sr::MODE_INV>(a, nullptr, a, batch, p, c->stark_one_tile, st)) return fail(SR_E_HIP, "stark rows launch failed");
    }
    auto hook = [&](bool begin) { begin ? gl_prof_begin(c, 2, st) : gl_prof_end(c, st); };
    if (sr::st::inv_cols(a, batch, p, c->stark_one_tile, st, hook)) return fail(SR_E_HIP, "stark strided launch failed");
    return SR_OK;
}
int st_ring_mul(sr_ctx *c, uint64_t *out, const uint64_t *a, const uint64_t *b, size_t batch, hipStream_t st) {
    if (batch == 0) return SR_OK;
    using S = sr::U256Storage;
    auto p = make_params<sr::StarkL>(c, true);
    if (c->stark_one_tile) {  // the ring element is one tile: one launch, a and b only read
        ProfScope ps(c, st, K_ROWS);
        if (sr::st::launch_rows<sr::MODE_MUL>(reinterpret_cast<S *>(const_cast<uint64_t *>(a)), reinterpret_cast<const S *>(b),
                                              reinterpret_cast<S *>(out), batch, p, true, st))
            return fail(SR_E_HIP, "stark rows launch failed");
        return SR_OK;
    }
    // strided stages of both operands first: a's go straight to out, b's into the operand scratch (neither is written)
    const size_t elem = sizeof(S) << c->k;
    const size_t chunk = scratch_polys(c, batch, elem);
    if (int rc = grow(c, OPERAND_A, chunk * elem, st)) return rc;
    ScratchUse su(c, st);
    if (int rc = su.acquire()) return rc;
    S *sb = reinterpret_cast<S *>(c->buf[OPERAND_A]);
    auto hook_f = [&](bool begin) { begin ? gl_prof_begin(c, 0, st) : gl_prof_end(c, st); };
    auto hook_i = [&](bool begin) { begin ? gl_prof_begin(c, 2, st) : gl_prof_end(c, st); };
    for (size_t e = 0; e < batch; e += chunk) {
        const size_t n = batch - e < chunk ? batch - e : chunk;
        S *o = reinterpret_cast<S *>(out) + (e << c->k);
        if (sr::st::fwd_cols(o, reinterpret_cast<const S *>(a) + (e << c->k), n, p, false, st, hook_f)) return fail(SR_E_HIP, "stark strided launch failed");
        if (sr::st::fwd_cols(sb, reinterpret_cast<const S *>(b) + (e << c->k), n, p, false, st, hook_f)) return fail(SR_E_HIP, "stark strided launch failed");
        {
            ProfScope ps(c, st, K_ROWS);
            if (sr::st::launch_rows<sr::MODE_MUL>(o, sb, o, n, p, false, st)) return fail(SR_E_HIP, "stark rows launch failed");
        }
        if (sr::st::inv_cols(o, n, p, false, st, hook_i)) return fail(SR_E_HIP, "stark strided launch failed");
    }
    return su.release();
}

bool is_pow2_ring(int ring) { return ring >= SR_RING_GOLDILOCKS_POW2 && ring <= SR_RING_STARK_POW2; }

// dispatch over the field of a pow2 ring
#define DISPATCH_POW2(c, CALL)                                                      \
    switch ((c)->ring) {                                                            \
        case SR_RING_GOLDILOCKS_POW2: { using F = sr::Goldilocks; return CALL; }    \
        case SR_RING_BABYBEAR_POW2: { using F = sr::BabyBear; return CALL; }        \
        case SR_RING_STARK_POW2: { using F = sr::Stark; return CALL; }              \
        default: return fail(SR_E_INVALID, "not a power-of-two ring");              \
    }

// dispatch over the coefficient field of any ring (the small rings' coefficients are Goldilocks / BabyBear elements)
#define DISPATCH_FIELD(c, CALL)                                                                          \
    switch ((c)->ring) {                                                                                 \
        case SR_RING_GOLDILOCKS_POW2: case SR_RING_GOLDILOCKS_24: { using F = sr::Goldilocks; return CALL; } \
        case SR_RING_BABYBEAR_POW2: case SR_RING_BABYBEAR_72: { using F = sr::BabyBear; return CALL; }   \
        case SR_RING_STARK_POW2: { using F = sr::Stark; return CALL; }                                   \
        case SR_RING_FROG_16: { using F = sr::Frog; return CALL; }                                       \
        default: return fail(SR_E_INVALID, "unknown ring");                                              \
    }

extern "C++" {
template <class F>
int decompose_dev(sr_ctx *c, uint64_t *out, const uint64_t *in, uint64_t b, size_t k, size_t batch, hipStream_t st) {
    using S = typename F::storage;
    const size_t n = batch * c->degree;
    if (n == 0 || k == 0) return SR_OK;
    const unsigned blocks = sr::stream_blocks<F>(n);
    ProfScope ps(c, st, K_OTHER);
    hipLaunchKernelGGL((sr::dec::decompose_kernel<F>), dim3((unsigned)blocks), dim3(256), 0, st, reinterpret_cast<S *>(out),
                       reinterpret_cast<const S *>(in), c->degree, batch, b, sr::dec::exact_log2(b), k, c->d_counter + 2);
    HIP_TRY(hipGetLastError());
    return SR_OK;
}
template <class F>
int recompose_dev(sr_ctx *c, uint64_t *out, const uint64_t *in, uint64_t b, size_t k, size_t batch_out, hipStream_t st) {
    using S = typename F::storage;
    const size_t n = batch_out * c->degree;
    if (n == 0) return SR_OK;
    const unsigned blocks = sr::stream_blocks<F>(n);
    ProfScope ps(c, st, K_OTHER);
    hipLaunchKernelGGL((sr::dec::recompose_kernel<F>), dim3((unsigned)blocks), dim3(256), 0, st, reinterpret_cast<S *>(out),
                       reinterpret_cast<const S *>(in), c->degree, batch_out, b, k);
    HIP_TRY(hipGetLastError());
    return SR_OK;
}
}
extern "C++" {
template <class F>
int rot_dev(sr_ctx *c, uint64_t *out, const uint64_t *in, size_t batch, hipStream_t st) {
    using S = typename F::storage;
    const size_t n = batch * c->degree;
    if (n == 0) return SR_OK;
    const unsigned blocks = sr::stream_blocks<F>(n);
    const size_t half = (c->ring == SR_RING_GOLDILOCKS_24 || c->ring == SR_RING_BABYBEAR_72) ? c->degree / 2 : 0;
    ProfScope ps(c, st, K_OTHER);
    hipLaunchKernelGGL((sr::rot_kernel<F>), dim3((unsigned)blocks), dim3(256), 0, st, reinterpret_cast<S *>(out),
                       reinterpret_cast<const S *>(in), c->degree, half, batch);
    HIP_TRY(hipGetLastError());
    return SR_OK;
}
}
extern "C++" {
template <class F>
int wire_dev(sr_ctx *c, bool ser, void *out, const void *in, const uint64_t *offsets, size_t batch, hipStream_t st) {
    using S = typename F::storage;
    const size_t n = batch * c->degree;
    if (n == 0) return SR_OK;
    const unsigned blocks = sr::stream_blocks<F>(n);
    ProfScope ps(c, st, K_OTHER);
    if (ser)
        hipLaunchKernelGGL((sr::wire::serialize_kernel<F>), dim3((unsigned)blocks), dim3(256), 0, st, (uint8_t *)out,
                           reinterpret_cast<const S *>(in), c->degree, batch, offsets, c->d_counter + 3);
    else
        hipLaunchKernelGGL((sr::wire::deserialize_kernel<F>), dim3((unsigned)blocks), dim3(256), 0, st, reinterpret_cast<S *>(out),
                           (const uint8_t *)in, c->degree, batch, offsets, c->d_counter + 3);
    HIP_TRY(hipGetLastError());
    return SR_OK;
}
template <class F>
size_t wire_width() {
    return sr::wire::Codec<F>::W;
}
}
int dev_wire(sr_ctx *c, bool ser, void *out, const void *in, const uint64_t *offsets, size_t batch, hipStream_t st) {
    DISPATCH_FIELD(c, (wire_dev<F>(c, ser, out, in, offsets, batch, st)));
}
size_t wire_coeff_bytes(const sr_ctx *c) {
    switch (c->ring) {
        case SR_RING_BABYBEAR_POW2: case SR_RING_BABYBEAR_72: return wire_width<sr::BabyBear>();
        case SR_RING_STARK_POW2: return wire_width<sr::Stark>();
        case SR_RING_FROG_16: return wire_width<sr::Frog>();
        default: return wire_width<sr::Goldilocks>();
    }
}
int dev_rot(sr_ctx *c, uint64_t *out, const uint64_t *in, size_t batch, hipStream_t st) {
    DISPATCH_FIELD(c, (rot_dev<F>(c, out, in, batch, st)));
}
int check_basis(uint64_t b) {
    if (b < 2) return fail(SR_E_INVALID, "cannot decompose in basis 0 or 1");              // mod.rs:63-66
    if (b & 1) return fail(SR_E_INVALID, "decomposition basis must be even");              // mod.rs:69
    return SR_OK;
}
int dev_decompose(sr_ctx *c, uint64_t *out, const uint64_t *in, uint64_t b, size_t k, size_t batch, hipStream_t st) {
    DISPATCH_FIELD(c, (decompose_dev<F>(c, out, in, b, k, batch, st)));
}
int dev_recompose(sr_ctx *c, uint64_t *out, const uint64_t *in, uint64_t b, size_t k, size_t batch_out, hipStream_t st) {
    DISPATCH_FIELD(c, (recompose_dev<F>(c, out, in, b, k, batch_out, st)));
}
uint64_t field_modulus64(const sr_ctx *c) {
    switch (c->ring) {
        case SR_RING_GOLDILOCKS_POW2: case SR_RING_GOLDILOCKS_24: return sr::Goldilocks::P;
        case SR_RING_BABYBEAR_POW2: case SR_RING_BABYBEAR_72: return sr::BabyBear::P;
        default: return sr::Frog::P;
    }
}
// basis = hi * 2^64 + lo with hi != 0 (the reference takes a u128).  One-limb fields: |x| <= (p - 1) / 2 < 2^63 < basis / 2, so digit 0
// is the coefficient itself and every other digit is zero -- a strided copy; Stark: 128-bit restoring division (decompose.hpp).
int dev_decompose_wide(sr_ctx *c, uint64_t *out, const uint64_t *in, uint64_t lo, uint64_t hi, size_t k, size_t batch, hipStream_t st) {
    if (batch == 0 || k == 0) return SR_OK;
    const size_t w = c->degree * c->limbs * 8;
    ProfScope ps(c, st, K_OTHER);
    if (c->ring == SR_RING_STARK_POW2) {
        const size_t n = batch * c->degree;
        hipLaunchKernelGGL(sr::dec::decompose_wide_kernel, dim3(sr::stream_blocks<sr::Stark>(n)), dim3(256), 0, st,
                           reinterpret_cast<sr::U256Storage *>(out), reinterpret_cast<const sr::U256Storage *>(in), c->degree, batch,
                           sr::dec::U128{lo, hi}, k, c->d_counter + 2);
        HIP_TRY(hipGetLastError());
        return SR_OK;
    }
    HIP_TRY(hipMemsetAsync(out, 0, batch * k * w, st));
    HIP_TRY(hipMemcpy2DAsync(out, k * w, in, w, w, batch, hipMemcpyDeviceToDevice, st));
    return SR_OK;
}
int dev_recompose_wide(sr_ctx *c, uint64_t *out, const uint64_t *in, uint64_t lo, uint64_t hi, size_t k, size_t batch_out, hipStream_t st) {
    if (batch_out == 0) return SR_OK;
    if (c->ring == SR_RING_STARK_POW2) {
        const size_t n = batch_out * c->degree;
        ProfScope ps(c, st, K_OTHER);
        hipLaunchKernelGGL(sr::dec::recompose_wide_kernel, dim3(sr::stream_blocks<sr::Stark>(n)), dim3(256), 0, st,
                           reinterpret_cast<sr::U256Storage *>(out), reinterpret_cast<const sr::U256Storage *>(in), c->degree, batch_out,
                           sr::dec::U128{lo, hi}, k);
        HIP_TRY(hipGetLastError());
        return SR_OK;
    }
    const unsigned __int128 b = ((unsigned __int128)hi << 64) | lo;  // R::from(b): b mod p, then the narrow Horner kernel
    return dev_recompose(c, out, in, (uint64_t)(b % field_modulus64(c)), k, batch_out, st);
}
int check_basis_wide(uint64_t lo, uint64_t hi) {
    if (hi == 0) return check_basis(lo);
    // decompose_balanced_in_place casts `b as i128` (mod.rs:73): 2^127 and above would be a negative basis there
    if (hi >> 63) return fail(SR_E_INVALID, "decomposition basis >= 2^127 (negative after the reference's cast to i128)");
    if (lo & 1) return fail(SR_E_INVALID, "decomposition basis must be even");
    return SR_OK;
}
int dev_decompose_any(sr_ctx *c, uint64_t *out, const uint64_t *in, uint64_t lo, uint64_t hi, size_t k, size_t batch, hipStream_t st) {
    return hi ? dev_decompose_wide(c, out, in, lo, hi, k, batch, st) : dev_decompose(c, out, in, lo, k, batch, st);
}
int dev_recompose_any(sr_ctx *c, uint64_t *out, const uint64_t *in, uint64_t lo, uint64_t hi, size_t k, size_t batch_out, hipStream_t st) {
    return hi ? dev_recompose_wide(c, out, in, lo, hi, k, batch_out, st) : dev_recompose(c, out, in, lo, k, batch_out, st);
}

// element counts are bounded so that no byte count or shift below can wrap (64 TiB of ring elements is far past any device)
int check_count(const sr_ctx *c, size_t n_elems, size_t per_elem = 1) {
    const size_t cap = ((size_t)1 << 46) / (c->degree * (size_t)c->limbs * 8);
    if (n_elems > cap || (per_elem > 1 && n_elems && per_elem > cap / n_elems)) return fail(SR_E_INVALID, "element count too large");
    return SR_OK;
}
// the first checks of an entry point: the context, then its buffers, then n_elems ring elements of per_elem each (check_count)
int check(const sr_ctx *c, std::initializer_list<const void *> bufs, size_t n_elems = 0, size_t per_elem = 1) {
    if (!c) return fail(SR_E_INVALID, "null context");
    for (const void *p : bufs)
        if (!p) return fail(SR_E_INVALID, "null buffer");
    return check_count(c, n_elems, per_elem);
}
// the ring and degree checks of every *_plan entry point and of sr_ctx_create_ex: host arithmetic, no context
int check_plan_ring(int ring, int log2_degree) {
    if (ring < SR_RING_GOLDILOCKS_POW2 || ring > SR_RING_FROG_16) return fail(SR_E_INVALID, "unknown ring id");
    if (is_pow2_ring(ring) && (log2_degree < 0 || log2_degree > 24)) return fail(SR_E_INVALID, "log2_degree out of range");
    return SR_OK;
}

// ---- per-ring device dispatch (pow2 rings and the reference-native small rings) --------------
int lanes_autoselect(sr_ctx *c, size_t batch);  // sr_plan.lanes = 0: measure once which plan this process's queues favour (below)
// one launch on the reference's own rings (frog_ring.hpp, small_rings.hpp): op = sr::FROG_CRT .. sr::FROG_REDUCE, numbered like the
// SMALL_G24_* and SMALL_B72_* operations
static_assert(sr::SMALL_G24_REDUCE - sr::SMALL_G24_CRT == sr::FROG_REDUCE && sr::SMALL_B72_REDUCE - sr::SMALL_B72_CRT == sr::FROG_REDUCE,
              "small-ring operations numbered alike");
int small_ring_launch(sr_ctx *c, int op, const uint64_t *a, const uint64_t *b, size_t in_len, uint64_t *out, size_t batch, hipStream_t st) {
    if (c->path == FROG) return sr::frog_launch(c->frog, op, a, b, in_len, out, batch, st) ? fail(SR_E_HIP, "frog-ring launch failed") : SR_OK;
    const int first = c->path == SMALL_G24 ? sr::SMALL_G24_CRT : sr::SMALL_B72_CRT;
    return sr::small_launch(c->small, first + op, a, b, in_len, out, batch, st) ? fail(SR_E_HIP, "small-ring launch failed") : SR_OK;
}
// the tuned Goldilocks transforms: in chunks on the two lanes (in place: no scratch, no ScratchUse), else one set of launches
template <int DIR>
int gl_transform(sr_ctx *c, uint64_t *d, size_t batch, hipStream_t st) {
    int rc;
    if (use_lanes(c, batch, st, true)) {
        if (int r = gl_lanes_init(c)) return r;
        rc = sr::for_each_lane_chunk(c->gl_lanes, batch, lane_chunk(c), st, [&](int, size_t first, size_t n, hipStream_t lane) {
            return sr::gl_fast_transform_chunk<DIR>(c->gl_fast, d + (first << c->k), n, lane);
        });
    } else {
        rc = DIR == 0 ? sr::gl_fast_fwd(c->gl_fast, d, batch, st) : sr::gl_fast_inv(c->gl_fast, d, batch, st);
    }
    return rc ? fail(SR_E_HIP, "goldilocks fast-path launch failed") : SR_OK;
}
int dev_fwd(sr_ctx *c, uint64_t *d, size_t batch, hipStream_t st) {
    switch (c->path) {
        case FROG: case SMALL_G24: case SMALL_B72: return small_ring_launch(c, sr::FROG_CRT, d, nullptr, 0, d, batch, st);
        case RT_BABYBEAR: return rt_transform<sr::BabyBear, 0>(c, d, batch, st);
        case RT_GOLDILOCKS: return rt_transform<sr::Goldilocks, 0>(c, d, batch, st);
        case GL_FAST: return gl_transform<0>(c, d, batch, st);
        case STARK_TUNED: return st_fwd(c, d, batch, st);
        case STARK_LAZY: return fwd_dev<sr::StarkL>(c, d, batch, st);
        default: DISPATCH_POW2(c, (fwd_dev<F>(c, d, batch, st)));
    }
}
int dev_inv(sr_ctx *c, uint64_t *d, size_t batch, hipStream_t st) {
    switch (c->path) {
        case FROG: case SMALL_G24: case SMALL_B72: return small_ring_launch(c, sr::FROG_ICRT, d, nullptr, 0, d, batch, st);
        case RT_BABYBEAR: return rt_transform<sr::BabyBear, 1>(c, d, batch, st);
        case RT_GOLDILOCKS: return rt_transform<sr::Goldilocks, 1>(c, d, batch, st);
        case GL_FAST: return gl_transform<1>(c, d, batch, st);
        case STARK_TUNED: return st_inv(c, d, batch, st);
        case STARK_LAZY: return inv_dev<sr::StarkL>(c, d, batch, st);
        default: DISPATCH_POW2(c, (inv_dev<F>(c, d, batch, st)));
    }
}
int dev_pointwise(sr_ctx *c, uint64_t *l, const uint64_t *r, size_t batch, hipStream_t st) {
    switch (c->path) {
        case FROG: case SMALL_G24: case SMALL_B72: return small_ring_launch(c, sr::FROG_MUL, l, r, 0, l, batch, st);
        default: DISPATCH_POW2(c, (pointwise_dev<F>(c, l, r, batch << c->k, st)));
    }
}
// every element of the batch *= ONE ring element r, slot-wise (CRT / NTT form): Matrix<R> *= &R, SparseMatrix<R> *= &R
int dev_mul_elem(sr_ctx *c, uint64_t *l, const uint64_t *r, size_t batch, hipStream_t st) {
    switch (c->path) {
        case FROG: return sr::frog_launch(c->frog, sr::FROG_MULB, l, r, 0, l, batch, st) ? fail(SR_E_HIP, "frog-ring launch failed") : SR_OK;
        case SMALL_G24: case SMALL_B72:
            return sr::small_launch_mul_bcast(c->small, c->path == SMALL_B72, l, r, batch, st) ? fail(SR_E_HIP, "small-ring launch failed") : SR_OK;
        default: DISPATCH_POW2(c, (pointwise_bcast_dev<F>(c, l, r, batch << c->k, st)));
    }
}
int dev_addsub(sr_ctx *c, uint64_t *l, const uint64_t *r, size_t batch, bool sub, hipStream_t st) {
    const size_t n = batch * c->degree;
    switch (c->ring) {
        case SR_RING_GOLDILOCKS_POW2:
        case SR_RING_GOLDILOCKS_24: return addsub_dev<sr::Goldilocks>(c, l, r, n, sub, st);
        case SR_RING_BABYBEAR_POW2:
        case SR_RING_BABYBEAR_72: return addsub_dev<sr::BabyBear>(c, l, r, n, sub, st);
        case SR_RING_FROG_16: return addsub_dev<sr::Frog>(c, l, r, n, sub, st);
        default: return addsub_dev<sr::Stark>(c, l, r, n, sub, st);
    }
}
// ---- unary word-wise operators of RqPoly / RqNTT: Neg, Mul<scalar>, Add<scalar> (every ring id, either form) -------------------
#define DISPATCH_BASE_FIELD(c, CALL)                                                       \
    switch ((c)->ring) {                                                                   \
        case SR_RING_GOLDILOCKS_POW2:                                                      \
        case SR_RING_GOLDILOCKS_24: { using F = sr::Goldilocks; return CALL; }             \
        case SR_RING_BABYBEAR_POW2:                                                        \
        case SR_RING_BABYBEAR_72: { using F = sr::BabyBear; return CALL; }                 \
        case SR_RING_FROG_16: { using F = sr::Frog; return CALL; }                         \
        default: { using F = sr::Stark; return CALL; }                                     \
    }
extern "C++" {
template <class F>
int neg_dev(sr_ctx *c, uint64_t *d, size_t n_words, hipStream_t st) {
    if (n_words == 0) return SR_OK;
    ProfScope ps(c, st, K_POINTWISE);
    hipLaunchKernelGGL(sr::neg_kernel<F>, dim3(sr::stream_blocks<F>(n_words)), dim3(256), 0, st, reinterpret_cast<typename F::storage *>(d), n_words);
    HIP_TRY(hipGetLastError());
    return SR_OK;
}
template <class F>
int load_scalar(const uint64_t *scalar, typename F::storage *out) {
    typename F::storage s, back;
    memcpy(&s, scalar, sizeof(s));
    const typename F::elem e = F::load(&s);
    F::store(&back, e);  // a BabyBear limb with bits above the low word is no field element's image either
    if (!F::valid(e) || memcmp(&back, &s, sizeof(s)) != 0) return fail(SR_E_INVALID, "scalar is not a canonical Montgomery image (>= p)");
    *out = s;
    return SR_OK;
}
template <class F>
int scale_dev(sr_ctx *c, uint64_t *d, const uint64_t *scalar, size_t n_words, hipStream_t st) {
    typename F::storage s;
    if (int rc = load_scalar<F>(scalar, &s)) return rc;
    if (n_words == 0) return SR_OK;
    ProfScope ps(c, st, K_POINTWISE);
    hipLaunchKernelGGL(sr::scale_kernel<F>, dim3(sr::stream_blocks<F>(n_words)), dim3(256), 0, st, reinterpret_cast<typename F::storage *>(d), n_words, s);
    HIP_TRY(hipGetLastError());
    return SR_OK;
}
template <class F>
int add_scalar_dev(sr_ctx *c, uint64_t *d, const uint64_t *scalar, size_t count, size_t stride, hipStream_t st) {
    typename F::storage s;
    if (int rc = load_scalar<F>(scalar, &s)) return rc;
    if (count == 0) return SR_OK;
    size_t blocks = (count + 255) / 256;
    if (blocks > 0xFFFFFFull) blocks = 0xFFFFFFull;
    ProfScope ps(c, st, K_POINTWISE);
    hipLaunchKernelGGL(sr::add_scalar_kernel<F>, dim3((unsigned)blocks), dim3(256), 0, st, reinterpret_cast<typename F::storage *>(d), count, stride, s);
    HIP_TRY(hipGetLastError());
    return SR_OK;
}
}  // extern "C++"
// base-field words per NTT slot: the extension degree of BaseCRTField (1 for the power-of-two rings)
size_t slot_words(const sr_ctx *c) {
    switch (c->ring) {
        case SR_RING_GOLDILOCKS_24: return 3;
        case SR_RING_BABYBEAR_72: return 9;
        case SR_RING_FROG_16: return 4;
        default: return 1;
    }
}
int dev_neg(sr_ctx *c, uint64_t *d, size_t batch, hipStream_t st) { DISPATCH_BASE_FIELD(c, (neg_dev<F>(c, d, batch * c->degree, st))); }
int dev_scale(sr_ctx *c, uint64_t *d, const uint64_t *scalar, size_t batch, hipStream_t st) {
    DISPATCH_BASE_FIELD(c, (scale_dev<F>(c, d, scalar, batch * c->degree, st)));
}
int dev_add_scalar(sr_ctx *c, uint64_t *d, const uint64_t *scalar, bool ntt_form, size_t batch, hipStream_t st) {
    const size_t stride = ntt_form ? slot_words(c) : c->degree, count = batch * c->degree / stride;
    DISPATCH_BASE_FIELD(c, (add_scalar_dev<F>(c, d, scalar, count, stride, st)));
}
// ---- Sum / Product over a slice of ring elements (coeff_form.rs:507-537, ntt_form.rs:640-670) --------------------------------------
// partial elements one stage of the word-wise fold leaves: about 2^20 lanes in flight, at least 32 elements per lane, one element
// once 32 or fewer remain
size_t fold_parts(size_t n, size_t w) {
    if (n <= 32) return 1;
    size_t r = (n + 31) / 32, cap = ((size_t)1 << 20) / w;
    if (cap < 1) cap = 1;
    return r < cap ? r : cap;
}
size_t fold_tmp_words(size_t w) { return w > ((size_t)1 << 20) ? w : ((size_t)1 << 20); }  // r * w <= max(w, 2^20)
extern "C++" {
template <class F, bool MUL>
int fold_dev(sr_ctx *c, uint64_t *out, const uint64_t *in, size_t n, hipStream_t st) {
    using S = typename F::storage;
    const size_t w = c->degree;  // storage words (coefficients) per ring element
    ScratchUse su(c, st);
    const S *src = reinterpret_cast<const S *>(in);
    bool tmp_used = false;
    int flip = 0;
    while (true) {
        const size_t r = fold_parts(n, w);
        S *dst = reinterpret_cast<S *>(out);
        if (r > 1) {
            const Buf t = flip ? FOLD_1 : FOLD_0;
            if (int rc = grow(c, t, fold_tmp_words(w) * sizeof(S), st)) return rc;
            if (!tmp_used) {
                if (int rc = su.acquire()) return rc;
                tmp_used = true;
            }
            dst = reinterpret_cast<S *>(c->buf[t]);
            flip ^= 1;
        }
        const size_t lanes = r * w;
        {
            ProfScope ps(c, st, K_OTHER);
            hipLaunchKernelGGL((sr::fold_stage_kernel<F, MUL>), dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, dst, src, w, n, r);
            HIP_TRY(hipGetLastError());
        }
        if (r == 1) break;
        src = dst;
        n = r;
    }
    return tmp_used ? su.release() : SR_OK;
}
// the Montgomery memory image of the base field's 1 (R mod p = mul_boundary(1, R^2))
template <class F>
void mont_one_image(uint64_t out[4]) {
    typename F::storage s;
    F::store(&s, F::mul_boundary(sr::dec::Consts<F>::one(), sr::dec::Consts<F>::r2()));
    memset(out, 0, 32);
    memcpy(out, &s, sizeof(s));
}
}  // extern "C++"
// n == 0: zero() / one() (one(): component 0 of every slot is the base field's 1)
int fold_empty(sr_ctx *c, uint64_t *out, bool mul, hipStream_t st) {
    const size_t bytes = c->degree * c->limbs * 8;
    HIP_TRY(hipMemsetAsync(out, 0, bytes, st));
    if (!mul) return SR_OK;
    uint64_t one[4];
    switch (c->ring) {
        case SR_RING_GOLDILOCKS_POW2: case SR_RING_GOLDILOCKS_24: mont_one_image<sr::Goldilocks>(one); break;
        case SR_RING_BABYBEAR_POW2: case SR_RING_BABYBEAR_72: mont_one_image<sr::BabyBear>(one); break;
        case SR_RING_FROG_16: mont_one_image<sr::Frog>(one); break;
        default: mont_one_image<sr::Stark>(one); break;
    }
    return dev_add_scalar(c, out, one, true, 1, st);
}
int dev_sum(sr_ctx *c, uint64_t *out, const uint64_t *in, size_t n, hipStream_t st) {
    if (n == 0) return fold_empty(c, out, false, st);
    DISPATCH_BASE_FIELD(c, (fold_dev<F, false>(c, out, in, n, st)));
}
int dev_product(sr_ctx *c, uint64_t *out, const uint64_t *in, size_t n, hipStream_t st) {
    if (n == 0) return fold_empty(c, out, true, st);
    if (is_pow2_ring(c->ring)) {  // fully split: the slot product is the base field's product on the memory images
        DISPATCH_POW2(c, (fold_dev<F, true>(c, out, in, n, st)));
    }
    // Fq3 / Fq9 / Fq4 slots: a halving tree of the rings' own slot-product kernels.  First level out of place (the input is only
    // read): tmp[i] = in[i] * in[m + i] for i < h = n / 2, m = n - h, the middle element of an odd n copied; then in place.
    const size_t w = c->degree, bytes = w * 8;
    if (n == 1) {
        HIP_TRY(hipMemcpyAsync(out, in, bytes, hipMemcpyDeviceToDevice, st));
        return SR_OK;
    }
    size_t h = n / 2, m = n - h;
    if (int rc = grow(c, FOLD_0, m * bytes, st)) return rc;
    ScratchUse su(c, st);
    if (int rc = su.acquire()) return rc;
    uint64_t *tmp = (uint64_t *)c->buf[FOLD_0];
    {
        ProfScope ps(c, st, K_POINTWISE);
        if (int rc = small_ring_launch(c, sr::FROG_MUL, in, in + m * w, 0, tmp, h, st)) return rc;
    }
    if (m > h) HIP_TRY(hipMemcpyAsync(tmp + h * w, in + h * w, bytes, hipMemcpyDeviceToDevice, st));
    n = m;
    while (n > 1) {
        h = n / 2;
        m = n - h;
        ProfScope ps(c, st, K_POINTWISE);
        if (int rc = small_ring_launch(c, sr::FROG_MUL, tmp, tmp + m * w, 0, tmp, h, st)) return rc;
        n = m;
    }
    HIP_TRY(hipMemcpyAsync(out, tmp, bytes, hipMemcpyDeviceToDevice, st));
    return su.release();
}
// the three reference-native rings: one slot (Fq3 / Fq9 / Fq4) per lane, small_linalg.hpp
#define DISPATCH_SLOT(c, CALL)                                                                                   \
    switch ((c)->ring) {                                                                                         \
        case SR_RING_GOLDILOCKS_24: { using SL = sr::SlotG24; const auto &K = (c)->small; return (CALL) ? fail(SR_E_HIP, "small-ring launch failed") : SR_OK; } \
        case SR_RING_BABYBEAR_72: { using SL = sr::SlotB72; const auto &K = (c)->small; return (CALL) ? fail(SR_E_HIP, "small-ring launch failed") : SR_OK; }   \
        default: { using SL = sr::SlotFrog; const auto &K = (c)->frog; return (CALL) ? fail(SR_E_HIP, "frog-ring launch failed") : SR_OK; }                       \
    }
int dev_spmv(sr_ctx *c, uint64_t *y, const uint64_t *vals, const uint32_t *cols, const uint64_t *row_ptr, const uint64_t *v,
             size_t nrows, size_t ncols, hipStream_t st) {
    if (!is_pow2_ring(c->ring)) {
        ProfScope ps(c, st, K_OTHER);
        DISPATCH_SLOT(c, (sr::slot_spmv<SL>(K, y, vals, cols, row_ptr, v, nrows, ncols, c->d_counter + 1, st)));
    }
    if (on_stark_lazy(c->path)) return spmv_dev<sr::StarkL>(c, y, vals, cols, row_ptr, v, nrows, ncols, st);  // sums of products on 28-bit lazy limbs (stark_lazy.hpp)
    DISPATCH_POW2(c, (spmv_dev<F>(c, y, vals, cols, row_ptr, v, nrows, ncols, st)));
}
int dev_matmul(sr_ctx *c, uint64_t *y, const uint64_t *a, const uint64_t *b, size_t n, size_t m, size_t p, hipStream_t st) {
    if (!is_pow2_ring(c->ring)) {
        ProfScope ps(c, st, K_OTHER);
        DISPATCH_SLOT(c, (sr::slot_matmul<SL>(K, y, a, b, n, m, p, st)));
    }
    if (on_stark_lazy(c->path)) return matmul_dev<sr::StarkL>(c, y, a, b, n, m, p, st);  // sums of products on 28-bit lazy limbs (stark_lazy.hpp)
    DISPATCH_POW2(c, (matmul_dev<F>(c, y, a, b, n, m, p, st)));
}
int dev_matvec(sr_ctx *c, uint64_t *y, const uint64_t *m, const uint64_t *v, size_t nrows, size_t ncols, hipStream_t st) {
    if (!is_pow2_ring(c->ring)) {
        ProfScope ps(c, st, K_OTHER);
        // few rows: every row is cut into parts (one workgroup each) whose sums meet in a context-owned buffer (small_linalg.hpp)
        const int groups = c->ring == SR_RING_FROG_16 ? 64 : 32;
        const unsigned nsplit = sr::slot_matvec_splits(nrows, ncols, groups);
        uint64_t *part = nullptr;
        // `part` is one buffer per context while _dev calls may come in on any stream: its users are ordered like those of the
        // operand scratch (an event recorded at release, awaited by the next user on another stream)
        ScratchUse su(c, st);
        if (nsplit > 1) {
            if (int rc = grow(c, MATVEC_PARTS, nrows * nsplit * c->degree * 8, st)) return rc;
            part = (uint64_t *)c->buf[MATVEC_PARTS];
            if (int rc = su.acquire()) return rc;
        }
        DISPATCH_SLOT(c, (sr::slot_matvec<SL>(K, y, m, v, nrows, ncols, part, nsplit, st)));
    }
    if (on_stark_lazy(c->path)) return matvec_dev<sr::StarkL>(c, y, m, v, nrows, ncols, st);  // sums of products on 28-bit lazy limbs (stark_lazy.hpp)
    DISPATCH_POW2(c, (matvec_dev<F>(c, y, m, v, nrows, ncols, st)));
}
// ---- plan selection: sr_plan.lanes = 0 means "measure once, keep the winner" ------------------------------------------------
// The two-lane plans (tuned Goldilocks cols256 product, register-tiled product) only pay when the HIP runtime gives each of the
// context's two streams its own hardware queue; which queue a stream gets is decided when the stream is created (GPU_MAX_HW_QUEUES,
// the streams the process already holds), so a host that runs RCCL or a framework beside this library can end up with both lanes
// on one queue -- and then the one-stream plan is the faster one (20.4 against 17.9 ms per config-2 batch).  The library
// therefore times both plans itself, once per context, on the context's real lanes, with a private non-blocking stream standing in
// for the caller's, on device-generated uniform operands in temporary buffers.
//   What is timed (round 4; the round-3 probe timed 16 chunks once, cold, and needed a 7 % fudge): each plan exactly as it will run,
//   on n = up to 32 lane chunks -- after four warm-up calls, four calls back to back, the mean.  Two lanes: every call forks and
//   joins like a real one (its last chunk runs alone on its lane: 1 / 32 of the call here, 1 / 128 of a config-2 batch -- the probe
//   reads about 1 % against the lanes); one stream: sets of launches of the REAL batch's set size, back to back.  The faster plan
//   wins, no margin.
//   Where it runs: ONLY inside sr_ctx_reserve_scratch (a blocking call by contract: it allocates).  A context whose host never
//   reserves runs two lanes, unmeasured -- an asynchronous _dev call never probes (it may be under stream capture, and its latency
//   belongs to the caller).  sr_ctx_plan_in_use reports the outcome.
int dev_ring_mul(sr_ctx *c, uint64_t *out, const uint64_t *a, const uint64_t *b, size_t batch, hipStream_t st);
bool lanes_candidate(const sr_ctx *c, size_t batch) {
    switch (c->path) {
        case RT_BABYBEAR: case RT_GOLDILOCKS: break;
        case GL_FAST: if (c->gl_fast.cols256) break; return false;
        default: return false;
    }
    return c->k > 12 && batch > lane_chunk(c);
}
int lanes_autoselect(sr_ctx *c, size_t batch) {
    if (c->plan.lanes || c->lanes_choice || c->probing || !lanes_candidate(c, batch)) return SR_OK;
    const size_t chunk = lane_chunk(c);
    if (batch < 8 * chunk) return SR_OK;  // too small for a steady state: two lanes, unmeasured (effective_lanes)
    // up to 32 chunks per call (2 GiB per buffer)
    size_t nch = batch / chunk;
    if (nch > 32) nch = 32;
    const size_t n = nch * chunk;
    const size_t elem = c->degree * c->limbs * 8, bytes = n * elem;
    void *buf[3] = {nullptr, nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipStream_t st = nullptr;
    c->probing = true;
    const bool prof_was = c->prof.on;
    c->prof.on = false;
    bool ok = hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess;
    for (auto &p : buf) ok = ok && hipMalloc(&p, bytes) == hipSuccess;
    for (auto &e : ev) ok = ok && hipEventCreate(&e) == hipSuccess;
    double t_plan[2] = {0, 0};  // milliseconds per call of n elements: [0] two lanes, [1] one stream
    constexpr int kWarm = 4, kCalls = 4;
    if (ok) {
        const size_t words = n * c->degree;
        auto fill = [&](void *p, uint64_t seed) {
            switch (c->ring) {
                case SR_RING_GOLDILOCKS_POW2: return fill_dev<sr::Goldilocks>(c, seed, 0, words, (uint64_t *)p, st);
                default: return fill_dev<sr::BabyBear>(c, seed, 0, words, (uint64_t *)p, st);
            }
        };
        ok = fill(buf[1], 0x9E3779B97F4A7C15ull) == SR_OK && fill(buf[2], 0xD1B54A32D192ED03ull) == SR_OK;
        // `calls` products of n elements back to back; the clock the chip holds under this load settles within the warm-up (the step
        // runs at the socket's power cap: a cold 2 ms sample reads 3-4 % fast)
        auto timed = [&](int calls, double &per_call) {
            float ms = 0;
            ok = ok && hipEventRecord(ev[0], st) == hipSuccess;
            for (int i = 0; i < calls; i++)
                ok = ok && dev_ring_mul(c, (uint64_t *)buf[0], (const uint64_t *)buf[1], (const uint64_t *)buf[2], n, st) == SR_OK;
            ok = ok && hipEventRecord(ev[1], st) == hipSuccess && hipEventSynchronize(ev[1]) == hipSuccess &&
                 hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess;
            if (ok) per_call = ms / calls;
        };
        for (int plan = 0; plan < 2 && ok; plan++) {
            c->lanes_choice = plan == 0 ? 2 : 1;
            c->probe_chunk = 0;
            if (plan == 1) {  // one stream: sets of launches of the size the REAL batch will run in (an eighth of it by default)
                const size_t real = c->path == GL_FAST ? gl_chunk_polys(c, batch) : rt_chunk_polys(c, batch);
                c->probe_chunk = real < n ? real : n;
            }
            double warm = 0;
            timed(kWarm, warm);  // allocates the plan's scratch, warms the caches and settles the clock
            timed(kCalls, t_plan[plan]);
        }
        ok = ok && hipStreamSynchronize(st) == hipSuccess;
    }
    // every launch of the probe was joined onto st and st has been waited for: the temporaries are idle (hipFree synchronises by itself)
    if (!ok && st) (void)hipStreamSynchronize(st);
    for (auto &p : buf)
        if (p) (void)hipFree(p);
    for (auto &e : ev)
        if (e) (void)hipEventDestroy(e);
    if (st) (void)hipStreamDestroy(st);
    // the probe sized the operand scratch for ITS one-stream run: drop it, the plan that won allocates what it needs
    for (Buf b : {OPERAND_A, OPERAND_B}) {
        if (c->buf[b]) (void)hipFree(c->buf[b]);
        c->buf[b] = nullptr;
        c->buf_bytes[b] = 0;
    }
    c->scratch_used = false;
    c->probe_chunk = 0;
    c->probing = false;
    c->prof.on = prof_was;
    if (ok && t_plan[0] > 0 && t_plan[1] > 0) {
        c->lanes_probe_ms[0] = t_plan[0];
        c->lanes_probe_ms[1] = t_plan[1];
        c->lanes_probe_elems = n;
        c->lanes_choice = t_plan[1] < t_plan[0] ? 1 : 2;
    } else {
        // no memory for the probe's temporaries (or a launch failed: the real call will report that): keep the default, unmeasured
        (void)hipGetLastError();
        c->lanes_choice = 2;
        g_err.clear();
    }
    return SR_OK;
}

// the tuned Goldilocks product: chunks on two internal streams, intermediates in per-lane scratch pairs; else one stream, b's column
// stages through the operand scratch
int gl_ring_mul(sr_ctx *c, uint64_t *out, const uint64_t *a, const uint64_t *b, size_t batch, hipStream_t st) {
    if (use_lanes(c, batch, st, false))
        return on_lanes(c, batch, st, "goldilocks fast-path launch failed", [&](size_t first, size_t n, void *sa, void *sb, hipStream_t lane) {
            const size_t off = first << c->k;
            return sr::gl_fast_ring_mul_chunk(c->gl_fast, out + off, a + off, b + off, (uint64_t *)sa, (uint64_t *)sb, n, lane);
        });
    uint64_t *scratch = nullptr;
    size_t chunk = 0;
    ScratchUse su(c, st);
    if (c->k > 12 && batch) {
        chunk = gl_chunk_polys(c, batch);
        if (int rc = grow(c, OPERAND_A, chunk * ((size_t)8 << c->k), st)) return rc;
        if (int rc = su.acquire()) return rc;
        scratch = reinterpret_cast<uint64_t *>(c->buf[OPERAND_A]);
    }
    if (sr::gl_fast_ring_mul(c->gl_fast, out, a, b, scratch, chunk, batch, st)) return fail(SR_E_HIP, "goldilocks fast-path launch failed");
    return scratch ? su.release() : SR_OK;
}
int dev_ring_mul(sr_ctx *c, uint64_t *out, const uint64_t *a, const uint64_t *b, size_t batch, hipStream_t st) {
    switch (c->path) {
        case FROG: case SMALL_G24: case SMALL_B72: return small_ring_launch(c, sr::FROG_RINGMUL, a, b, 0, out, batch, st);
        case RT_BABYBEAR: return rt_ring_mul<sr::BabyBear>(c, out, a, b, batch, st);
        case RT_GOLDILOCKS: return rt_ring_mul<sr::Goldilocks>(c, out, a, b, batch, st);
        case GL_FAST: return gl_ring_mul(c, out, a, b, batch, st);
        case STARK_TUNED: return st_ring_mul(c, out, a, b, batch, st);
        case STARK_LAZY: return ring_mul_dev<sr::StarkL>(c, out, a, b, batch, st);
        default: DISPATCH_POW2(c, (ring_mul_dev<F>(c, out, a, b, batch, st)));
    }
}
// out = icrt(crt(a) (.) b_ntt): forward transform, slot product and inverse transform on out, one after the other (the
// Goldilocks tuned path fuses them: gl_fast_ring_mul_rhs, on the lanes gl_fast_ring_mul_rhs_chunk)
int dev_ring_mul_ntt_rhs(sr_ctx *c, uint64_t *out, const uint64_t *a, const uint64_t *b_ntt, size_t batch, hipStream_t st) {
    if (batch == 0) return SR_OK;
    if (c->path == GL_FAST) {
        if (use_lanes(c, batch, st, false))
            return on_lanes(c, batch, st, "goldilocks fast-path launch failed", [&](size_t first, size_t n, void *sa, void *, hipStream_t lane) {
                const size_t off = first << c->k;
                return sr::gl_fast_ring_mul_rhs_chunk(c->gl_fast, out + off, a + off, b_ntt + off, (uint64_t *)sa, n, lane);
            });
        return sr::gl_fast_ring_mul_rhs(c->gl_fast, out, a, b_ntt, batch, st) ? fail(SR_E_HIP, "goldilocks fast-path launch failed") : SR_OK;
    }
    if (out != a) HIP_TRY(hipMemcpyAsync(out, a, batch * c->degree * c->limbs * 8, hipMemcpyDeviceToDevice, st));
    if (int rc = dev_fwd(c, out, batch, st)) return rc;
    if (int rc = dev_pointwise(c, out, b_ntt, batch, st)) return rc;
    return dev_inv(c, out, batch, st);
}
int dev_reduce(sr_ctx *c, const uint64_t *in, size_t in_len, uint64_t *out, size_t batch, hipStream_t st) {
    switch (c->path) {
        case FROG: case SMALL_G24: case SMALL_B72:
            if (in_len > 2 * c->degree) return fail(SR_E_INVALID, "reduce: in_len_per_elem > 2D");
            return small_ring_launch(c, sr::FROG_REDUCE, in, nullptr, in_len, out, batch, st);
        default: DISPATCH_POW2(c, (reduce_dev<F>(c, in, in_len, out, batch, st)));
    }
}

// ---- dense multilinear extensions (csrc/mle.hpp): every launch under K_POINTWISE, nothing allocated, no context scratch -------------
int mle_launch(sr_ctx *c, int j, uint64_t *out, const uint64_t *in, const uint64_t *pt, size_t n_out, size_t n_in, size_t sb, size_t st,
               hipStream_t s) {
    ProfScope ps(c, s, K_POINTWISE);
    hipError_t e;
    switch (c->ring) {
        case SR_RING_GOLDILOCKS_POW2: e = sr::mle::launch_fold<sr::Goldilocks>(j, out, in, pt, n_out, n_in, sb, st, c->k, s); break;
        case SR_RING_BABYBEAR_POW2: e = sr::mle::launch_fold<sr::BabyBear>(j, out, in, pt, n_out, n_in, sb, st, c->k, s); break;
        case SR_RING_STARK_POW2: e = sr::mle::launch_fold<sr::Stark>(j, out, in, pt, n_out, n_in, sb, st, c->k, s); break;
        case SR_RING_GOLDILOCKS_24: e = sr::mle::launch_slot_fold<sr::SlotG24>(c->small, j, out, in, pt, n_out, n_in, sb, st, s); break;
        case SR_RING_BABYBEAR_72: e = sr::mle::launch_slot_fold<sr::SlotB72>(c->small, j, out, in, pt, n_out, n_in, sb, st, s); break;
        default: e = sr::mle::launch_slot_fold<sr::SlotFrog>(c->frog, j, out, in, pt, n_out, n_in, sb, st, s); break;
    }
    if (e != hipSuccess) return fail(SR_E_HIP, std::string("mle fold launch: ") + hipGetErrorString(e));
    return SR_OK;
}
// The launches of sr::mle::plan, one after the other on `st`.  Trailing order: out == evals folds in place; otherwise the first
// intermediate table goes to `work` and is folded there in place.  Leading order alternates between the two regions of `work`.
// An intermediate launch writes only the elements that can be non-zero and hands their count on as the next launch's n_in; the
// last launch writes every element of `out`.
int dev_mle_fix(sr_ctx *c, uint64_t *out, const uint64_t *evals, size_t n_evals, size_t num_vars, const uint64_t *point, size_t n_fixed,
                int order, uint64_t *work, hipStream_t st) {
    sr::mle::Plan p;
    if (!sr::mle::plan(c->ring, num_vars, n_fixed, order, &p)) return fail(SR_E_INVALID, "mle_fix_variables: no plan for these arguments");
    const size_t w = (size_t)c->degree * c->limbs;
    const bool trailing = order == sr::mle::ORDER_TRAILING, in_place = out == evals;
    const uint64_t *src = evals;
    size_t n_in = n_evals, m = num_vars, done = 0;
    for (int l = 0; l < p.launches; l++) {
        const int j = p.j[l];
        const bool last = l == p.launches - 1;
        const size_t table = (size_t)1 << (m - j);  // elements of this launch's output table
        const size_t sb = trailing ? 1 : (size_t)1 << j, stride = trailing ? table : 1;
        const size_t n_valid = trailing ? (n_in < table ? n_in : table) : (n_in + sb - 1) >> j;
        // bit i of a group index is variable m - j + i (trailing: point entry m - j + i - (num_vars - n_fixed)) or done + i (leading)
        const uint64_t *pt = point + (trailing ? m - j - (num_vars - n_fixed) : done) * w;
        uint64_t *dst = last ? out : trailing ? (in_place ? out : work) : (l % 2 == 0 ? work : work + (((size_t)1 << (num_vars - p.j[0])) * w));
        const size_t n_out = last ? table : n_valid;
        if (n_out)
            if (int rc = mle_launch(c, j, dst, src, j ? pt : nullptr, n_out, n_in, sb, stride, st)) return rc;
        src = dst;
        n_in = n_valid;
        m -= j;
        done += j;
    }
    return SR_OK;
}
// acc[e] += r x[e], e < batch
int dev_mul_elem_add(sr_ctx *c, uint64_t *acc, const uint64_t *x, const uint64_t *r, size_t batch, hipStream_t st) {
    if (batch == 0) return SR_OK;
    ProfScope ps(c, st, K_POINTWISE);
    if (!is_pow2_ring(c->ring)) DISPATCH_SLOT(c, (sr::mle::launch_slot_mul_elem_add<SL>(K, acc, x, r, batch, st) != hipSuccess));
    DISPATCH_POW2(c, ([&] {
                      using S = typename F::storage;
                      const size_t n = batch << c->k;
                      hipLaunchKernelGGL(sr::mle::mul_elem_add_kernel<F>, dim3(sr::stream_blocks<F>(n)), dim3(256), 0, st, reinterpret_cast<S *>(acc),
                                         reinterpret_cast<const S *>(x), reinterpret_cast<const S *>(r), n, (size_t)c->degree - 1);
                      return hipGetLastError() == hipSuccess ? (int)SR_OK : fail(SR_E_HIP, "mul_elem_add launch failed");
                  }()));
}
bool ranges_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return a_bytes && b_bytes && pa < pb + b_bytes && pb < pa + a_bytes;
}
// the argument checks the two forms of sr_mle_fix_variables share; *out_elems = 2^(num_vars - n_fixed), *need = workspace elements
int check_mle(sr_ctx *c, const void *out, const void *evals, size_t n_evals, size_t num_vars, const void *point, size_t n_fixed, int order,
              size_t *out_elems, size_t *need) {
    if (!c) return fail(SR_E_INVALID, "null context");
    if (order != SR_MLE_LEADING && order != SR_MLE_TRAILING) return fail(SR_E_INVALID, "mle_fix_variables: unknown order");
    if (num_vars >= 48) return fail(SR_E_INVALID, "mle_fix_variables: num_vars must be below 48");
    if (n_fixed > num_vars) return fail(SR_E_INVALID, "mle_fix_variables: n_fixed exceeds num_vars");
    if (n_evals > (size_t)1 << num_vars) return fail(SR_E_INVALID, "mle_fix_variables: n_evals exceeds 2^num_vars");
    if (!out || (n_evals && !evals) || (n_fixed && !point)) return fail(SR_E_INVALID, "mle_fix_variables: null buffer");
    *out_elems = (size_t)1 << (num_vars - n_fixed);
    if (int rc = check_count(c, *out_elems)) return rc;
    if (int rc = check_count(c, n_evals)) return rc;
    sr::mle::Plan p;
    sr::mle::plan(c->ring, num_vars, n_fixed, order, &p);
    *need = p.work_elems;
    return check_count(c, p.work_elems);
}

// ---- sum-check round messages (csrc/sumcheck.hpp, sumcheck_fold.hpp, sumcheck_vpoly.hpp, sumcheck_vpoly_fold.hpp, sumcheck_weighted.hpp,
// range_check.hpp): every launch under K_POINTWISE, nothing allocated, no context scratch.  Seven families and one record of operands
// (RoundCall); the argument check, the aliasing rule, the launches and (with the host-pointer entry points, below) the staging each
// exist once and read that record.
struct RoundFamily {
    const char *name;  // the prefix of every message
    int max_tables;
    bool terms, fold;       // a sum of products (n_terms, degree); a fold as well (an order, no SR_MLE_ROUND_SUM, two variables)
    bool weighted = false;  // a per-pair weight (csrc/sumcheck_weighted.hpp): an order, no SR_MLE_ROUND_SUM
    bool range = false;     // a bound in place of terms and one coefficient per table (csrc/range_check.hpp); d_coeffs may alias a table
    bool index = false;     // the last n_index slots are integer columns (csrc/sumcheck_index.hpp)
    // log2 of the weights' element count: one per pair of the tables the message is over (of a fold: the folded ones)
    size_t weight_log2(size_t num_vars) const { return num_vars - (fold ? 2 : 1); }
};
const RoundFamily kMleRound{"mle_round", SR_MLE_ROUND_MAX_TABLES, false, false}, kVpolyRound{"vpoly_round", SR_VPOLY_MAX_TABLES, true, false},
    kMleRoundFold{"mle_round_fold", SR_MLE_ROUND_MAX_TABLES, false, true}, kVpolyRoundFold{"vpoly_round_fold", SR_VPOLY_MAX_TABLES, true, true},
    kVpolyWround{"vpoly_wround", SR_VPOLY_MAX_TABLES, true, false, true}, kVpolyWroundFold{"vpoly_wround_fold", SR_VPOLY_MAX_TABLES, true, true, true},
    kRangeWround{"range_wround", SR_RANGE_MAX_TABLES, false, false, true, true},
    kVpolyIwround{"vpoly_iwround", SR_VPOLY_MAX_TABLES, true, false, true, false, true},
    kVpolyIwroundFold{"vpoly_iwround_fold", SR_VPOLY_MAX_TABLES, true, true, true, false, true};
// Every operand of a round call.  The first seven exist in every family; an operand that a family does not have stays null (0).
// With integer columns (f.index) a slot is a table or a column: tables, n_evals and n_tables speak of all slots, the last n_index of
// which are the columns -- there tables[s] is null and n_evals[s] the column's stored length (a progression: 2^num_vars).
struct RoundCall {
    const RoundFamily &f;
    uint64_t *out;
    const uint64_t *const *tables;
    const size_t *n_evals;
    int n_tables;
    size_t num_vars;
    int mode;                               // an order where the family takes no SR_MLE_ROUND_SUM
    uint64_t *const *out_tables = nullptr;  // folds: the folded tables, the elements written to each, the challenge
    size_t *n_evals_out = nullptr;
    const uint64_t *r = nullptr;
    const uint64_t *weights = nullptr;      // weighted: 2^weight_log2 elements
    const sr_vpoly_term *terms = nullptr;   // sums of products
    int n_terms = 0;
    int bound = 0;                          // range
    const uint64_t *coef = nullptr;         // n_coef() elements, or null for one() everywhere
    uint64_t *work = nullptr;               // the *_evals_dev forms: the caller's workspace
    size_t work_elems = 0;
    const sr_index_column *columns = nullptr;  // integer columns: slots n_tables - n_index .. n_tables - 1
    int n_index = 0;
    sr::sumcheck::Plan plan{};              // check_round sets it
    int n_coef() const { return f.range ? n_tables : n_terms; }
    int first_column() const { return n_tables - n_index; }
};
extern "C++" {
template <class T> struct FamilyType {
    using type = T;
};
// fn(the family type of the context's ring, its constants) enqueues the launches of a call of family f
template <class Fn>
int round_dispatch(sr_ctx *c, hipStream_t st, const RoundFamily &f, Fn fn) {
    ProfScope ps(c, st, K_POINTWISE);
    const sr::sumcheck::NoConsts none;
    hipError_t e;
    switch (c->ring) {
        case SR_RING_GOLDILOCKS_POW2: e = fn(FamilyType<sr::Goldilocks>{}, none); break;
        case SR_RING_BABYBEAR_POW2: e = fn(FamilyType<sr::BabyBear>{}, none); break;
        case SR_RING_STARK_POW2: e = fn(FamilyType<sr::Stark>{}, none); break;
        case SR_RING_GOLDILOCKS_24: e = fn(FamilyType<sr::SlotG24>{}, c->small); break;
        case SR_RING_BABYBEAR_72: e = fn(FamilyType<sr::SlotB72>{}, c->small); break;
        default: e = fn(FamilyType<sr::SlotFrog>{}, c->frog); break;
    }
    if (e == hipSuccess) return SR_OK;
    std::string what(f.name);  // "mle round fold launch: ..."
    for (char &ch : what) ch = ch == '_' ? ' ' : ch;
    return fail(SR_E_HIP, what + " launch: " + hipGetErrorString(e));
}
}  // extern "C++"
// The launches of a checked call on `st`.  aligned: every operand the kernels touch starts on a 16-byte boundary (the workspace only
// where the plan has more than one record group to sum).
int dev_round(sr_ctx *c, const RoundCall &a, hipStream_t st) {
    const RoundFamily &f = a.f;
    const sr::sumcheck::Plan &p = a.plan;
    const int nt = a.n_tables, k = c->k;
    sr::vpoly::Tables tb{};
    sr::vpoly_fold::Folded fo{};
    sr::vpoly::Term tm[SR_VPOLY_MAX_TERMS];
    uintptr_t bits = (uintptr_t)a.out | (uintptr_t)a.weights | (uintptr_t)a.coef | (uintptr_t)a.r | (p.groups > 1 ? (uintptr_t)a.work : 0);
    for (int j = 0; j < nt; j++) {
        tb.p[j] = a.tables[j];
        tb.n[j] = a.n_evals[j];
        bits |= (uintptr_t)a.tables[j];
        if (!f.fold) continue;
        fo.p[j] = a.out_tables[j];
        bits |= (uintptr_t)a.out_tables[j];
    }
    for (int i = 0; i < a.n_terms; i++) {
        tm[i].n_factors = a.terms[i].n_factors;
        for (int s = 0; s < SR_VPOLY_MAX_FACTORS; s++) tm[i].table[s] = a.terms[i].table[s];
    }
    const bool aligned = (bits & 15u) == 0;
    // a product of at most four tables takes the narrower records of sumcheck.hpp
    const bool product = !f.terms && !f.range;
    sr::sumcheck::Tables tb4{};
    sr::sumcheck_fold::Folded fo4{};
    for (int j = 0; product && j < nt; j++) {
        tb4.p[j] = tb.p[j];
        tb4.n[j] = tb.n[j];
        fo4.p[j] = fo.p[j];
    }
    // One round_dispatch per header's launch, in the order the families were written: a launch is instantiated for every ring where
    // its dispatch stands, and that order is the order of the kernels in the code object.
    if (product && !f.fold)
        return round_dispatch(c, st, f, [&](auto t, const auto &kc) {
            return sr::sumcheck::launch<typename decltype(t)::type>(kc, p, a.mode, a.out, tb4, nt, a.num_vars, k, aligned, a.work, st);
        });
    if (f.terms && !f.weighted && !f.fold)
        return round_dispatch(c, st, f, [&](auto t, const auto &kc) {
            return sr::vpoly::launch<typename decltype(t)::type>(kc, p, a.mode, a.out, tb, nt, tm, a.n_terms, a.coef, a.num_vars, k, aligned, a.work,
                                                                 st);
        });
    if (product)
        return round_dispatch(c, st, f, [&](auto t, const auto &kc) {
            return sr::sumcheck_fold::launch<typename decltype(t)::type>(kc, p, a.mode, a.out, tb4, fo4, a.r, nt, a.num_vars, a.n_evals_out, k, aligned,
                                                                         a.work, st);
        });
    if (!f.weighted)
        return round_dispatch(c, st, f, [&](auto t, const auto &kc) {
            return sr::vpoly_fold::launch<typename decltype(t)::type>(kc, p, a.mode, a.out, tb, fo, a.r, nt, tm, a.n_terms, a.coef, a.num_vars,
                                                                      a.n_evals_out, k, aligned, a.work, st);
        });
    if (!f.range && !f.index && !f.fold)
        return round_dispatch(c, st, f, [&](auto t, const auto &kc) {
            return sr::wsumcheck::launch<typename decltype(t)::type>(kc, p, a.mode, a.out, a.weights, tb, nt, tm, a.n_terms, a.coef, a.num_vars, k,
                                                                     aligned, a.work, st);
        });
    if (!f.range && !f.index)
        return round_dispatch(c, st, f, [&](auto t, const auto &kc) {
            return sr::wsumcheck::launch_fold<typename decltype(t)::type>(kc, p, a.mode, a.out, a.weights, tb, fo, a.r, nt, tm, a.n_terms, a.coef,
                                                                          a.num_vars, a.n_evals_out, k, aligned, a.work, st);
        });
    if (f.range)
        return round_dispatch(c, st, f, [&](auto t, const auto &kc) {
            return sr::range::launch<typename decltype(t)::type>(kc, p, a.mode, a.out, a.weights, tb, nt, a.bound, a.coef, a.num_vars, k, aligned,
                                                                 a.work, st);
        });
    // integer columns: the index arrays are 8-byte accesses and take no part in `aligned`
    sr::isumcheck::ColumnArgs ca{};
    ca.n = a.n_index;
    for (int j = 0; j < a.n_index; j++) {
        ca.values[j] = a.columns[j].values;
        ca.start[j] = a.columns[j].start;
    }
    const int first = a.first_column();
    if (!f.fold)
        return round_dispatch(c, st, f, [&](auto t, const auto &kc) {
            return sr::isumcheck::launch<typename decltype(t)::type>(kc, p, a.mode, a.out, a.weights, tb, first, ca, tm, a.n_terms, a.coef, a.num_vars,
                                                                     k, aligned, a.work, st);
        });
    return round_dispatch(c, st, f, [&](auto t, const auto &kc) {
        return sr::isumcheck::launch_fold<typename decltype(t)::type>(kc, p, a.mode, a.out, a.weights, tb, fo, a.r, first, ca, tm, a.n_terms, a.coef,
                                                                      a.num_vars, a.n_evals_out, k, aligned, a.work, st);
    });
}
// a refusal of family f: the message is assembled here, on the failing path only
int refuse(const RoundFamily &f, const std::string &what) { return fail(SR_E_INVALID, std::string(f.name) + ": " + what); }
// the shape checks the *_plan call and the two forms of the *_evals call of a family share (n_terms, degree: families with terms;
// bound: the range check)
int round_plan_for(const RoundFamily &f, int ring, int k, size_t num_vars, int n_tables, int n_terms, int degree, int bound, int mode,
                   sr::sumcheck::Plan *p) {
    const bool ordered = f.fold || f.weighted;
    if (n_tables < 1 || n_tables > f.max_tables) return refuse(f, "n_tables must be 1 .. " + std::to_string(f.max_tables));
    if (f.terms) {
        if (n_terms < 1 || n_terms > SR_VPOLY_MAX_TERMS) return refuse(f, "n_terms must be 1 .. 8");
        if (degree < 1 || degree > SR_VPOLY_MAX_FACTORS) return refuse(f, "degree (the largest n_factors) must be 1 .. 4");
    }
    if (f.range && (bound < 2 || bound > SR_RANGE_MAX_BOUND)) return refuse(f, "bound must be 2 .. " + std::to_string(SR_RANGE_MAX_BOUND));
    if (f.weighted && !f.fold && !f.range && mode == SR_MLE_ROUND_SUM)
        return refuse(f, "SR_MLE_ROUND_SUM takes no weights (a weight of a plain sum is just a table)");
    if (mode != SR_MLE_LEADING && mode != SR_MLE_TRAILING && (ordered || mode != SR_MLE_ROUND_SUM))
        return refuse(f, ordered ? "unknown order" : "unknown mode");
    if (num_vars >= 48) return refuse(f, "num_vars must be below 48");
    if (f.fold && num_vars < 2) return refuse(f, "num_vars >= 2 (the folded tables need a variable for the next round)");
    if (num_vars == 0 && mode != SR_MLE_ROUND_SUM)
        return refuse(f, f.range ? "a round needs num_vars >= 1" : "a round needs num_vars >= 1 (only SR_MLE_ROUND_SUM takes 0)");
    const bool ok = f.range      ? sr::range::plan(ring, k, num_vars, n_tables, bound, mode, p)
                    : f.weighted ? (f.fold ? sr::wsumcheck::fold_plan(ring, k, num_vars, n_tables, degree, mode, p)
                                           : sr::wsumcheck::plan(ring, k, num_vars, n_tables, degree, mode, p))
                    : f.fold     ? (f.terms ? sr::vpoly_fold::plan(ring, k, num_vars, n_tables, degree, mode, p)
                                            : sr::sumcheck_fold::plan(ring, k, num_vars, n_tables, mode, p))
                    : f.terms    ? sr::vpoly::plan(ring, k, num_vars, n_tables, degree, mode, p)
                                 : sr::sumcheck::plan(ring, k, num_vars, n_tables, mode, p);
    return ok ? (int)SR_OK : refuse(f, "no plan for these arguments");
}
// the body of the seven *_plan entry points
int round_plan_entry(const RoundFamily &f, int ring, int log2_degree, size_t num_vars, int n_tables, int n_terms, int degree, int bound, int mode,
                     size_t *work_elems, int *launches) {
    if (int rc = check_plan_ring(ring, log2_degree)) return rc;
    if (!work_elems || !launches) return fail(SR_E_INVALID, std::string(f.name) + "_plan: null result pointer");
    sr::sumcheck::Plan p;
    if (int rc = round_plan_for(f, ring, log2_degree, num_vars, n_tables, n_terms, degree, bound, mode, &p)) return rc;
    *work_elems = p.work_elems;
    *launches = p.launches;
    return SR_OK;
}
// elements the fold of a table of n stored elements writes
size_t round_fold_n_out(size_t n, size_t num_vars, int order) {
    const size_t half = (size_t)1 << (num_vars - 1);
    return order == SR_MLE_LEADING ? (n + 1) / 2 : (n < half ? n : half);
}
// The aliasing rule of the *_evals_dev forms.  What a call writes -- d_out, d_work, every folded table -- overlaps no other operand,
// another folded table included; the one exception is a trailing-order fold in place, d_out_tables[j] == d_tables[j], where that
// table appears once among the inputs.  Of what a call only reads, d_r, d_coeffs and the tables are disjoint from each other, except
// that tables may alias tables (and, in the range check, d_coeffs a table); d_weights may alias any of them.
int check_round_aliasing(const sr_ctx *c, const RoundCall &a) {
    const RoundFamily &f = a.f;
    const size_t w = (size_t)c->degree * c->limbs * 8;
    // a refusal names its two operands in this order; a column's array may overlap whatever the call only reads
    enum Kind { WRITTEN, FOLDED, READ, TABLE, WEIGHTS, COLUMN };
    struct {
        const void *p;
        size_t bytes;
        const char *name;
        Kind kind;
        int j;
    } ops[5 + 2 * SR_VPOLY_MAX_TABLES];
    int n = 0;
    ops[n++] = {a.out, a.plan.np_total * w, "d_out", WRITTEN, 0};
    ops[n++] = {a.work, a.plan.work_elems * w, "d_work", WRITTEN, 0};
    ops[n++] = {a.r, a.r ? w : 0, "d_r", READ, 0};
    ops[n++] = {a.coef, a.coef ? a.n_coef() * w : 0, "d_coeffs", READ, 0};
    for (int j = 0; f.fold && j < a.n_tables; j++)
        ops[n++] = {a.out_tables[j], round_fold_n_out(a.n_evals[j], a.num_vars, a.mode) * w, "a folded table", FOLDED, j};
    for (int j = 0; j < a.first_column(); j++) ops[n++] = {a.tables[j], a.n_evals[j] * w, "a table", TABLE, j};
    ops[n++] = {a.weights, a.weights ? w << f.weight_log2(a.num_vars) : 0, "d_weights", WEIGHTS, 0};
    for (int j = 0; j < a.n_index; j++)
        ops[n++] = {a.columns[j].values, a.columns[j].values ? a.columns[j].n_evals * 8 : 0, "a column", COLUMN, a.first_column() + j};
    for (int x = 0; x < n; x++)
        for (int y = x + 1; y < n; y++) {
            const auto &p = ops[x], &q = ops[y];
            if (!ranges_overlap(p.p, p.bytes, q.p, q.bytes)) continue;
            if (p.kind == FOLDED && q.kind == FOLDED) return refuse(f, "two folded tables overlap");
            if (p.kind == FOLDED && q.kind == TABLE) {
                // in place: the table's own output only, trailing order only, and no other input may be that table (it would be folded twice)
                if (a.mode != SR_MLE_TRAILING || p.p != a.tables[p.j])
                    return refuse(f,
                                  "a folded table overlaps an input table (only a trailing-order fold may run in place, with "
                                  "d_out_tables[j] == d_tables[j])");
                if (q.j != p.j) return refuse(f, "an input table that appears twice cannot be folded in place");
                continue;
            }
            const bool written = p.kind <= FOLDED || q.kind == FOLDED;
            const bool inputs = p.kind == READ && (q.kind == READ || (q.kind == TABLE && !f.range));
            if (written || inputs) return refuse(f, std::string(p.name) + " overlaps " + q.name);
        }
    return SR_OK;
}
// The argument checks of every family.  dev: the *_evals_dev form, which names its weights d_weights (as both forms of the range check
// do) and brings a workspace and device pointers that may alias.  Sets a.plan.
int check_round(sr_ctx *c, RoundCall &a, bool dev) {
    const RoundFamily &f = a.f;
    if (f.weighted && !a.weights) return refuse(f, dev || f.range ? "null pointer (d_weights)" : "null pointer (weights)");
    if (!c) return fail(SR_E_INVALID, "null context");
    if (!a.out || !a.tables || !a.n_evals || (f.terms && !a.terms) || (f.fold && (!a.out_tables || !a.n_evals_out || !a.r)))
        return refuse(f, "null pointer");
    int degree = 0;
    if (f.terms) {  // the counts that bound the scan of the terms, ahead of round_plan_for
        if (a.n_tables < 1 || a.n_tables > f.max_tables) return refuse(f, "n_tables must be 1 .. " + std::to_string(f.max_tables));
        if (a.n_terms < 1 || a.n_terms > SR_VPOLY_MAX_TERMS) return refuse(f, "n_terms must be 1 .. 8");
        unsigned used = 0;
        for (int i = 0; i < a.n_terms; i++) {
            const sr_vpoly_term &t = a.terms[i];
            if (t.n_factors < 1 || t.n_factors > SR_VPOLY_MAX_FACTORS) return refuse(f, "n_factors must be 1 .. 4 (term " + std::to_string(i) + ")");
            degree = t.n_factors > degree ? t.n_factors : degree;
            for (int s = 0; s < t.n_factors; s++) {
                if (t.table[s] < 0 || t.table[s] >= a.n_tables)
                    return refuse(f, "table index outside 0 .. n_tables - 1 (term " + std::to_string(i) + ")");
                used |= 1u << t.table[s];
            }
        }
        if ((used | ~((1u << a.first_column()) - 1)) != ~0u) return refuse(f, "a table that no term uses");
        if (used != (1u << a.n_tables) - 1) return refuse(f, "a column that no term uses");
    }
    if (int rc = round_plan_for(f, c->ring, c->k, a.num_vars, a.n_tables, a.n_terms, degree, a.bound, a.mode, &a.plan)) return rc;
    for (int j = 0; j < a.n_tables; j++) {
        if (a.n_evals[j] > (size_t)1 << a.num_vars) return refuse(f, "n_evals exceeds 2^num_vars");
        const bool column = j >= a.first_column();  // its values are a progression's when null
        if (a.n_evals[j] && column && f.fold && !a.out_tables[j]) return refuse(f, "null pointer (the folded table of a column)");
        if (a.n_evals[j] && ((!column && !a.tables[j]) || (f.fold && !a.out_tables[j]))) return refuse(f, "null pointer (a table)");
        if (int rc = check_count(c, a.n_evals[j])) return rc;
    }
    if (!dev) return SR_OK;
    if (a.plan.work_elems && !a.work) return refuse(f, "null pointer (d_work)");
    if (a.work_elems < a.plan.work_elems)
        return refuse(f, "workspace too small (sr_" + std::string(f.name) + "_plan asks for " + std::to_string(a.plan.work_elems) + " elements)");
    return check_round_aliasing(c, a);
}
// a *_evals_dev entry point: the checks, then the device guard, the mutex and the caller's stream, then the launches
int round_dev(sr_ctx *c, RoundCall &a, void *stream) {
    if (int rc = check_round(c, a, true)) return rc;
    const Call call(c, stream);
    return dev_round(c, a, call.st);
}

// ---- sparse multilinear extensions (csrc/sparse_mle.hpp): nothing allocated, no context scratch ----------------------------------
sr::smle::One smle_one(const sr_ctx *c) {
    sr::smle::One one;
    switch (c->ring) {
        case SR_RING_GOLDILOCKS_POW2: case SR_RING_GOLDILOCKS_24: mont_one_image<sr::Goldilocks>(one.w); break;
        case SR_RING_BABYBEAR_POW2: case SR_RING_BABYBEAR_72: mont_one_image<sr::BabyBear>(one.w); break;
        case SR_RING_FROG_16: mont_one_image<sr::Frog>(one.w); break;
        default: mont_one_image<sr::Stark>(one.w); break;
    }
    return one;
}
extern "C++" {
template <class O, int J> struct SmleKind {
    using Ops = O;
    static constexpr int kJ = J;
};
// fn(kind, constants, log2 of the units per element) for the unit the context's ring and these buffers allow; `aligned`: every
// buffer of the call starts on a 16-byte boundary
template <class Fn>
int smle_dispatch(sr_ctx *c, bool aligned, Fn fn) {
    namespace sm = sr::smle;
    const bool pair = aligned && c->k >= 1;
    switch (c->ring) {
        case SR_RING_GOLDILOCKS_POW2:
            return pair ? fn(SmleKind<sm::PowOps<sr::Goldilocks, sr::Goldilocks, 2>, sm::kEqJ<sr::Goldilocks>>{}, 0, c->k - 1)
                        : fn(SmleKind<sm::PowOps<sr::Goldilocks, sr::Goldilocks, 1>, sm::kEqJ<sr::Goldilocks>>{}, 0, c->k);
        case SR_RING_BABYBEAR_POW2:
            return pair ? fn(SmleKind<sm::PowOps<sr::BabyBear, sr::BabyBear, 2>, sm::kEqJ<sr::BabyBear>>{}, 0, c->k - 1)
                        : fn(SmleKind<sm::PowOps<sr::BabyBear, sr::BabyBear, 1>, sm::kEqJ<sr::BabyBear>>{}, 0, c->k);
        case SR_RING_STARK_POW2:  // the sums of products run on 28-bit lazy limbs where the context's transforms do (stark_lazy.hpp)
            return on_stark_lazy(c->path) ? fn(SmleKind<sm::PowOps<sr::Stark, sr::StarkL, 4>, sm::kEqJ<sr::Stark>>{}, 0, c->k)
                                          : fn(SmleKind<sm::PowOps<sr::Stark, sr::Stark, 4>, sm::kEqJ<sr::Stark>>{}, 0, c->k);
        case SR_RING_GOLDILOCKS_24: return fn(SmleKind<sm::SlotOps<sr::SlotG24>, sm::kSlotEqJ<sr::SlotG24>>{}, c->small, 3);
        case SR_RING_BABYBEAR_72: return fn(SmleKind<sm::SlotOps<sr::SlotB72>, sm::kSlotEqJ<sr::SlotB72>>{}, c->small, 3);
        default: return fn(SmleKind<sm::SlotOps<sr::SlotFrog>, sm::kSlotEqJ<sr::SlotFrog>>{}, c->frog, 2);
    }
}
}  // extern "C++"
bool aligned16(std::initializer_list<const void *> ps) {
    uintptr_t x = 0;
    for (const void *p : ps) x |= (uintptr_t)p;
    return (x & 15u) == 0;
}
int dev_eq_table(sr_ctx *c, uint64_t *out, const uint64_t *point, size_t n_vars, hipStream_t st) {
    ProfScope ps(c, st, K_POINTWISE);
    const sr::smle::One one = smle_one(c);
    return smle_dispatch(c, aligned16({out, point}), [&](auto kind, const auto &k, int lu) {
        using Kind = decltype(kind);
        const hipError_t e = sr::smle::launch_eq<typename Kind::Ops, Kind::kJ>(k, one, out, point, (unsigned)n_vars, (unsigned)n_vars, 1, lu, st);
        return e == hipSuccess ? (int)SR_OK : fail(SR_E_HIP, std::string("eq table launch: ") + hipGetErrorString(e));
    });
}
// the fold of a checked call (nnz >= 1, p from smle_plan_for)
int dev_smle_fix(sr_ctx *c, const sr::smle::Plan &p, uint64_t *out, const uint64_t *vals, const uint64_t *idx, size_t nnz, const uint64_t *seg,
                 size_t n_out, const uint64_t *point, size_t n_fixed, uint64_t *work, hipStream_t st) {
    const size_t w = (size_t)c->degree * c->limbs;
    if (p.copy) {
        HIP_TRY(hipMemcpyAsync(out, vals, nnz * w * 8, hipMemcpyDeviceToDevice, st));
        return SR_OK;
    }
    ProfScope ps(c, st, K_POINTWISE);
    const sr::smle::One one = smle_one(c);
    return smle_dispatch(c, aligned16({out, vals, point, work}), [&](auto kind, const auto &k, int lu) {
        using Kind = decltype(kind);
        const hipError_t e = sr::smle::launch_fold<typename Kind::Ops, Kind::kJ>(k, one, p, out, vals, idx, seg, n_out, nnz, point, (unsigned)n_fixed,
                                                                               work, lu, w, st);
        return e == hipSuccess ? (int)SR_OK : fail(SR_E_HIP, std::string("sparse mle launch: ") + hipGetErrorString(e));
    });
}
// the shape checks sr_smle_plan and the two forms of sr_smle_fix_variables share
int smle_plan_for(int ring, int k, size_t nnz, size_t n_out, size_t n_fixed, sr::smle::Plan *p) {
    if (n_fixed >= 64) return fail(SR_E_INVALID, "smle: n_fixed must be below 64");
    if (n_out > nnz) return fail(SR_E_INVALID, "smle: n_out exceeds nnz");
    if (nnz && !n_out) return fail(SR_E_INVALID, "smle: n_out is zero but entries are stored");
    if (!sr::smle::plan(ring, k, nnz, n_out, n_fixed, p)) return fail(SR_E_INVALID, "smle: no plan for these arguments");
    return SR_OK;
}

// ---- norms of coefficient slices (csrc/norms.hpp): nothing allocated, no context scratch ------------------------------------------------
template <class F>
int norm_launch(sr_ctx *c, const sr::norms::Plan &p, int which, uint64_t *out, const uint64_t *coeffs, uint64_t *work, hipStream_t st) {
    ProfScope ps(c, st, K_OTHER);
    const hipError_t e = sr::norms::launch<F>(p, which, out, coeffs, work, st);
    return e == hipSuccess ? (int)SR_OK : fail(SR_E_HIP, std::string("norm launch: ") + hipGetErrorString(e));
}
int dev_norm(sr_ctx *c, const sr::norms::Plan &p, int which, uint64_t *out, const uint64_t *coeffs, uint64_t *work, hipStream_t st) {
    DISPATCH_BASE_FIELD(c, (norm_launch<F>(c, p, which, out, coeffs, work, st)));
}
// the argument checks sr_norm_plan and the two forms of sr_norm_batch share (limbs: 1 or 4 words per coefficient)
int check_norm(int limbs, size_t n_coeffs, size_t group, int which, sr::norms::Plan *p) {
    if (which < 1 || which > 3) return fail(SR_E_INVALID, "norm: `which` must be SR_NORM_LINF, SR_NORM_L2SQ or both");
    if (group == 0) return fail(SR_E_INVALID, "norm: group must be at least 1");
    if (n_coeffs % group != 0) return fail(SR_E_INVALID, "norm: group must divide n_coeffs");
    if (n_coeffs == 0 && (which & SR_NORM_LINF)) return fail(SR_E_INVALID, "norm: linf of an empty slice is undefined (the reference panics)");
    if (n_coeffs > ((size_t)1 << 46) / ((size_t)limbs * 8)) return fail(SR_E_INVALID, "norm: coefficient count too large");
    if (!sr::norms::plan(limbs, n_coeffs, group, which, p)) return fail(SR_E_INVALID, "norm: no plan for these arguments");
    return SR_OK;
}
// dst (+)= src on the host: max of the linf words, sum with carry of the l2sq words
void norm_combine_host(uint64_t *dst, const uint64_t *src, int nl, int ns) {
    for (int i = nl - 1; i >= 0; i--)
        if (src[i] != dst[i]) {
            if (src[i] > dst[i]) memcpy(dst, src, (size_t)nl * 8);
            break;
        }
    uint64_t carry = 0;
    for (int i = nl; i < nl + ns; i++) {
        const uint64_t t = dst[i] + carry, u = t + src[i];
        carry = (uint64_t)(t < carry) + (uint64_t)(u < t);
        dst[i] = u;
    }
}

// ---- symmetric matrices (csrc/symmetric.hpp): nothing allocated, no context scratch --------------------------------------------------
int dev_gram(sr_ctx *c, const sr::symm::GramPlan &p, uint64_t *out, const uint64_t *a, size_t n, size_t m, uint64_t *work, hipStream_t st) {
    namespace sy = sr::symm;
    ProfScope ps(c, st, K_OTHER);
    hipError_t e;
    switch (c->ring) {
        case SR_RING_GOLDILOCKS_POW2: e = sy::launch_gram<sr::Goldilocks, sr::Goldilocks>(p, out, a, n, m, c->k, work, st); break;
        case SR_RING_BABYBEAR_POW2: e = sy::launch_gram<sr::BabyBear, sr::BabyBear>(p, out, a, n, m, c->k, work, st); break;
        case SR_RING_STARK_POW2:  // sums of products on 28-bit lazy limbs where the context's transforms run on them (stark_lazy.hpp)
            e = on_stark_lazy(c->path) ? sy::launch_gram<sr::Stark, sr::StarkL>(p, out, a, n, m, c->k, work, st)
                                       : sy::launch_gram<sr::Stark, sr::Stark>(p, out, a, n, m, c->k, work, st);
            break;
        case SR_RING_GOLDILOCKS_24: e = sy::launch_slot_gram<sr::SlotG24>(c->small, p, out, a, n, m, work, st); break;
        case SR_RING_BABYBEAR_72: e = sy::launch_slot_gram<sr::SlotB72>(c->small, p, out, a, n, m, work, st); break;
        default: e = sy::launch_slot_gram<sr::SlotFrog>(c->frog, p, out, a, n, m, work, st); break;
    }
    return e == hipSuccess ? (int)SR_OK : fail(SR_E_HIP, std::string("gram launch: ") + hipGetErrorString(e));
}
int dev_symm_recompose(sr_ctx *c, const sr::symm::RecomposePlan &p, uint64_t *out, const uint64_t *mat, const uint64_t *powers, size_t n, size_t d,
                       uint64_t *work, hipStream_t st) {
    namespace sy = sr::symm;
    ProfScope ps(c, st, K_OTHER);
    const bool al = aligned16({out, mat, work});
    hipError_t e;
    switch (c->ring) {
        case SR_RING_GOLDILOCKS_POW2: e = sy::launch_recompose<sr::Goldilocks, sr::Goldilocks>(p, out, mat, powers, n, d, c->k, work, al, st); break;
        case SR_RING_BABYBEAR_POW2: e = sy::launch_recompose<sr::BabyBear, sr::BabyBear>(p, out, mat, powers, n, d, c->k, work, al, st); break;
        case SR_RING_STARK_POW2:
            e = on_stark_lazy(c->path) ? sy::launch_recompose<sr::Stark, sr::StarkL>(p, out, mat, powers, n, d, c->k, work, al, st)
                                       : sy::launch_recompose<sr::Stark, sr::Stark>(p, out, mat, powers, n, d, c->k, work, al, st);
            break;
        case SR_RING_GOLDILOCKS_24: e = sy::launch_slot_recompose<sr::SlotG24>(c->small, p, out, mat, powers, n, d, work, st); break;
        case SR_RING_BABYBEAR_72: e = sy::launch_slot_recompose<sr::SlotB72>(c->small, p, out, mat, powers, n, d, work, st); break;
        default: e = sy::launch_slot_recompose<sr::SlotFrog>(c->frog, p, out, mat, powers, n, d, work, st); break;
    }
    return e == hipSuccess ? (int)SR_OK : fail(SR_E_HIP, std::string("symmetric recompose launch: ") + hipGetErrorString(e));
}
int gram_plan_for(int ring, int k, size_t n, size_t m, sr::symm::GramPlan *p) {
    if (!sr::symm::gram_plan(ring, k, n, m, p)) return fail(SR_E_INVALID, "gram: n (n + 1) / 2 overflows or the grid exceeds one launch");
    return SR_OK;
}
int recompose_plan_for(int ring, int k, size_t n, size_t d, sr::symm::RecomposePlan *p) {
    if (d == 0) return fail(SR_E_INVALID, "symm_recompose: d == 0 (the reference divides by the number of powers)");
    if (!sr::symm::recompose_plan(ring, k, n, d, p)) return fail(SR_E_INVALID, "symm_recompose: a size overflows or the grid exceeds one launch");
    return SR_OK;
}
// the argument checks the two forms of sr_gram_ntt share
int check_gram(sr_ctx *c, const void *out, const void *a, size_t n, size_t m, sr::symm::GramPlan *p) {
    if (!c) return fail(SR_E_INVALID, "null context");
    if (int rc = gram_plan_for(c->ring, c->k, n, m, p)) return rc;
    if (n && (!out || (m && !a))) return fail(SR_E_INVALID, "gram: null buffer");
    if (int rc = check_count(c, p->packed)) return rc;
    if (int rc = check_count(c, n, m)) return rc;
    return check_count(c, p->work_elems);
}
int check_symm_recompose(sr_ctx *c, const void *out, const void *mat, size_t n, size_t d, const void *powers, sr::symm::RecomposePlan *p) {
    if (!c) return fail(SR_E_INVALID, "null context");
    if (int rc = recompose_plan_for(c->ring, c->k, n, d, p)) return rc;
    if (n && (!out || !mat || !powers)) return fail(SR_E_INVALID, "symm_recompose: null buffer");
    if (int rc = check_count(c, p->packed_in)) return rc;
    return check_count(c, p->work_elems);
}

// ---- sparse matrices (csrc/sparse_matrix.hpp): nothing allocated, no context scratch --------------------------------------------------
// out[t] = in[perm[t]] (perm != null) or the dense transpose of the nrows x ncols matrix `in`; n_out output elements
int dev_move(sr_ctx *c, uint64_t *out, const uint64_t *in, const uint32_t *perm, size_t n_out, size_t n_in, size_t nrows, size_t ncols,
             hipStream_t st) {
    int v;
    size_t units, blocks;
    if (!sr::spm::move_grid(n_out, (size_t)c->degree * c->limbs, aligned16({out, in}), &v, &units, &blocks))
        return fail(SR_E_INVALID, "gather / transpose: the grid exceeds one launch");
    if (n_out == 0) return SR_OK;
    ProfScope ps(c, st, K_OTHER);
    const hipError_t e = sr::spm::launch_move(out, in, perm, n_in, nrows, ncols, v, units, blocks, c->d_counter + 1, st);
    return e == hipSuccess ? (int)SR_OK : fail(SR_E_HIP, std::string("gather / transpose launch: ") + hipGetErrorString(e));
}
int dev_spgemm(sr_ctx *c, const sr::spm::SpgemmArgs &g, hipStream_t st) {
    namespace sp = sr::spm;
    ProfScope ps(c, st, K_OTHER);
    hipError_t e;
    switch (c->ring) {
        case SR_RING_GOLDILOCKS_POW2: e = sp::launch_spgemm<sr::Goldilocks>(g, c->k, st); break;
        case SR_RING_BABYBEAR_POW2: e = sp::launch_spgemm<sr::BabyBear>(g, c->k, st); break;
        case SR_RING_STARK_POW2:  // sums of products on 28-bit lazy limbs where the context's transforms run on them (stark_lazy.hpp)
            e = on_stark_lazy(c->path) ? sp::launch_spgemm<sr::StarkL>(g, c->k, st) : sp::launch_spgemm<sr::Stark>(g, c->k, st);
            break;
        case SR_RING_GOLDILOCKS_24: e = sp::launch_slot_spgemm<sr::SlotG24>(c->small, g, st); break;
        case SR_RING_BABYBEAR_72: e = sp::launch_slot_spgemm<sr::SlotB72>(c->small, g, st); break;
        default: e = sp::launch_slot_spgemm<sr::SlotFrog>(c->frog, g, st); break;
    }
    return e == hipSuccess ? (int)SR_OK : fail(SR_E_HIP, std::string("spgemm launch: ") + hipGetErrorString(e));
}
// the checks the two forms of the sparse product share: the grid of n_out entries, the element counts
int check_spgemm(sr_ctx *c, size_t nnz_a, size_t nnz_b, size_t n_out, size_t n_pairs) {
    if (!c) return fail(SR_E_INVALID, "null context");
    size_t work;
    int launches;
    if (!sr::spm::spgemm_plan(c->ring, c->k, n_out, n_pairs, &work, &launches)) return fail(SR_E_INVALID, "spgemm: the grid exceeds one launch");
    if (nnz_a > 0xFFFFFFFFull || nnz_b > 0xFFFFFFFFull) return fail(SR_E_INVALID, "spgemm: 2^32 or more stored entries (positions are 32-bit)");
    if (n_pairs > ((size_t)1 << 60)) return fail(SR_E_INVALID, "spgemm: pair count too large");
    if (int rc = check_count(c, nnz_a)) return rc;
    if (int rc = check_count(c, nnz_b)) return rc;
    return check_count(c, n_out);
}

int check_fold(sr_ctx *c, const uint64_t *out, const uint64_t *in, size_t n) {
    if (int rc = check(c, {out, n ? (const void *)in : (const void *)1}, n)) return rc;
    const uintptr_t w = (uintptr_t)c->degree * c->limbs * 8, po = (uintptr_t)out, pi = (uintptr_t)in;
    if (n && po + w > pi && pi + n * w > po) return fail(SR_E_INVALID, "sum / product: out must not overlap the input elements");
    return SR_OK;
}
// ---- grand products (csrc/prod_tree.hpp): every launch under K_POINTWISE, nothing allocated, no context scratch ----------------------
// The launches of sr::ptree::plan, one after the other on `st`: launch l reads the last layer launch l - 1 wrote (the leaves for the
// first) and writes its levels behind it.  Every layer is written in full, so only the first launch sees a truncated input.
int dev_prod_tree(sr_ctx *c, uint64_t *layers, const uint64_t *leaves, size_t n_leaves, size_t num_vars, int order, hipStream_t st) {
    sr::ptree::Plan p;
    if (!sr::ptree::plan(c->ring, num_vars, order, &p)) return fail(SR_E_INVALID, "prod_tree: no plan for these arguments");
    const size_t w = (size_t)c->degree * c->limbs;
    const bool tr = order == sr::mle::ORDER_TRAILING;
    const sr::smle::One one = smle_one(c);
    const uint64_t *src = leaves;
    size_t n_in = n_leaves, done = 0;
    for (int l = 0; l < p.launches; l++) {
        const int j = p.j[l], m = (int)(num_vars - done);
        uint64_t *dst = layers + sr::ptree::layer_offset(num_vars, done + 1) * w;
        ProfScope ps(c, st, K_POINTWISE);
        hipError_t e;
        switch (c->ring) {
            case SR_RING_GOLDILOCKS_POW2: e = sr::ptree::launch_tree<sr::Goldilocks>(j, dst, src, one, n_in, m, tr, c->k, st); break;
            case SR_RING_BABYBEAR_POW2: e = sr::ptree::launch_tree<sr::BabyBear>(j, dst, src, one, n_in, m, tr, c->k, st); break;
            case SR_RING_STARK_POW2: e = sr::ptree::launch_tree<sr::Stark>(j, dst, src, one, n_in, m, tr, c->k, st); break;
            case SR_RING_GOLDILOCKS_24: e = sr::ptree::launch_slot_tree<sr::SlotG24>(c->small, j, dst, src, one, n_in, m, tr, st); break;
            case SR_RING_BABYBEAR_72: e = sr::ptree::launch_slot_tree<sr::SlotB72>(c->small, j, dst, src, one, n_in, m, tr, st); break;
            default: e = sr::ptree::launch_slot_tree<sr::SlotFrog>(c->frog, j, dst, src, one, n_in, m, tr, st); break;
        }
        if (e != hipSuccess) return fail(SR_E_HIP, std::string("prod_tree launch: ") + hipGetErrorString(e));
        done += j;
        src = layers + sr::ptree::layer_offset(num_vars, done) * w;  // the last level of this launch
        n_in = (size_t)1 << (num_vars - done);
    }
    return SR_OK;
}
// the argument checks the two forms of sr_prod_tree share
int check_prod_tree(sr_ctx *c, const void *layers, const void *leaves, size_t n_leaves, size_t num_vars, int order) {
    if (!c) return fail(SR_E_INVALID, "null context");
    if (order != SR_MLE_LEADING && order != SR_MLE_TRAILING) return fail(SR_E_INVALID, "prod_tree: unknown order");
    if (num_vars >= 48) return fail(SR_E_INVALID, "prod_tree: num_vars must be below 48");
    if (n_leaves > (size_t)1 << num_vars) return fail(SR_E_INVALID, "prod_tree: n_leaves exceeds 2^num_vars");
    if (int rc = check_count(c, (size_t)1 << num_vars)) return rc;
    if ((num_vars && !layers) || (n_leaves && !leaves)) return fail(SR_E_INVALID, "prod_tree: null buffer");
    const size_t w = (size_t)c->degree * c->limbs * 8;
    if (ranges_overlap(layers, (((size_t)1 << num_vars) - 1) * w, leaves, n_leaves * w))
        return fail(SR_E_INVALID, "prod_tree: d_layers overlaps d_leaves");
    return SR_OK;
}
// ---- fraction trees (csrc/frac_tree.hpp): every launch under K_POINTWISE, nothing allocated, no context scratch ----------------------
// The launches of sr::ftree::plan, as in dev_prod_tree, on the two planar outputs at once.  Only the first launch sees truncated leaves
// or absent numerators (HP = false); every later one reads the full layers the one before it wrote.
extern "C++" {
template <bool HP>
hipError_t launch_frac_tree(sr_ctx *c, int j, uint64_t *pd, uint64_t *qd, const uint64_t *ps, const uint64_t *qs, const sr::smle::One &one,
                            size_t n_in, int m, bool tr, hipStream_t st) {
    switch (c->ring) {
        case SR_RING_GOLDILOCKS_POW2: return sr::ftree::launch_tree<sr::Goldilocks, HP>(j, pd, qd, ps, qs, one, n_in, m, tr, c->k, st);
        case SR_RING_BABYBEAR_POW2: return sr::ftree::launch_tree<sr::BabyBear, HP>(j, pd, qd, ps, qs, one, n_in, m, tr, c->k, st);
        case SR_RING_STARK_POW2: return sr::ftree::launch_tree<sr::Stark, HP>(j, pd, qd, ps, qs, one, n_in, m, tr, c->k, st);
        case SR_RING_GOLDILOCKS_24: return sr::ftree::launch_slot_tree<sr::SlotG24, HP>(c->small, j, pd, qd, ps, qs, one, n_in, m, tr, st);
        case SR_RING_BABYBEAR_72: return sr::ftree::launch_slot_tree<sr::SlotB72, HP>(c->small, j, pd, qd, ps, qs, one, n_in, m, tr, st);
        default: return sr::ftree::launch_slot_tree<sr::SlotFrog, HP>(c->frog, j, pd, qd, ps, qs, one, n_in, m, tr, st);
    }
}
}  // extern "C++"
int dev_frac_tree(sr_ctx *c, uint64_t *p_layers, uint64_t *q_layers, const uint64_t *p_leaves, const uint64_t *q_leaves, size_t n_leaves,
                  size_t num_vars, int order, hipStream_t st) {
    sr::ftree::Plan p;
    if (!sr::ftree::plan(c->ring, num_vars, order, &p)) return fail(SR_E_INVALID, "frac_tree: no plan for these arguments");
    const size_t w = (size_t)c->degree * c->limbs;
    const bool tr = order == sr::mle::ORDER_TRAILING;
    const sr::smle::One one = smle_one(c);
    const uint64_t *ps = p_leaves, *qs = q_leaves;
    size_t n_in = n_leaves, done = 0;
    for (int l = 0; l < p.launches; l++) {
        const int j = p.j[l], m = (int)(num_vars - done);
        const size_t off = sr::ftree::layer_offset(num_vars, done + 1) * w;
        ProfScope prof(c, st, K_POINTWISE);
        const hipError_t e = (l == 0 && !p_leaves) ? launch_frac_tree<false>(c, j, p_layers + off, q_layers + off, ps, qs, one, n_in, m, tr, st)
                                                   : launch_frac_tree<true>(c, j, p_layers + off, q_layers + off, ps, qs, one, n_in, m, tr, st);
        if (e != hipSuccess) return fail(SR_E_HIP, std::string("frac_tree launch: ") + hipGetErrorString(e));
        done += j;
        const size_t last = sr::ftree::layer_offset(num_vars, done) * w;  // the last level of this launch
        ps = p_layers + last;
        qs = q_layers + last;
        n_in = (size_t)1 << (num_vars - done);
    }
    return SR_OK;
}
// the argument checks the two forms of sr_frac_tree share
int check_frac_tree(sr_ctx *c, const void *p_layers, const void *q_layers, const void *p_leaves, const void *q_leaves, size_t n_leaves,
                    size_t num_vars, int order) {
    if (!c) return fail(SR_E_INVALID, "null context");
    if (order != SR_MLE_LEADING && order != SR_MLE_TRAILING) return fail(SR_E_INVALID, "frac_tree: unknown order");
    if (num_vars >= 48) return fail(SR_E_INVALID, "frac_tree: num_vars must be below 48");
    if (n_leaves > (size_t)1 << num_vars) return fail(SR_E_INVALID, "frac_tree: n_leaves exceeds 2^num_vars");
    if (int rc = check_count(c, (size_t)1 << num_vars)) return rc;
    if (num_vars && (!p_layers || !q_layers)) return fail(SR_E_INVALID, "frac_tree: null output buffer");
    if (n_leaves && !q_leaves) return fail(SR_E_INVALID, "frac_tree: null denominator leaves");
    const size_t w = (size_t)c->degree * c->limbs * 8, out = (((size_t)1 << num_vars) - 1) * w, in = n_leaves * w;
    if (ranges_overlap(p_layers, out, q_layers, out)) return fail(SR_E_INVALID, "frac_tree: d_p_layers overlaps d_q_layers");
    if (ranges_overlap(p_layers, out, q_leaves, in)) return fail(SR_E_INVALID, "frac_tree: d_p_layers overlaps d_q_leaves");
    if (ranges_overlap(q_layers, out, q_leaves, in)) return fail(SR_E_INVALID, "frac_tree: d_q_layers overlaps d_q_leaves");
    if (p_leaves && ranges_overlap(p_layers, out, p_leaves, in)) return fail(SR_E_INVALID, "frac_tree: d_p_layers overlaps d_p_leaves");
    if (p_leaves && ranges_overlap(q_layers, out, p_leaves, in)) return fail(SR_E_INVALID, "frac_tree: d_q_layers overlaps d_p_leaves");
    return SR_OK;
}
// ---- batch inversion (csrc/inverse.hpp): one launch under K_POINTWISE, nothing allocated, no context scratch ------------------------
// out[e] = num[e] / den[e] slot by slot (num == nullptr: one()); zero slots come back zero and are counted in d_counter[5]
int dev_inverse(sr_ctx *c, uint64_t *out, const uint64_t *num, const uint64_t *den, size_t n, hipStream_t st) {
    if (n == 0) return SR_OK;
    const bool aligned = ((((uintptr_t)out | (uintptr_t)num | (uintptr_t)den)) & 15u) == 0;
    const sr::smle::One one = smle_one(c);
    unsigned long long *zeros = c->d_counter + 5;
    ProfScope prof(c, st, K_POINTWISE);
    hipError_t e;
    switch (c->ring) {
        case SR_RING_GOLDILOCKS_POW2: e = sr::inverse::launch<sr::Goldilocks>({}, out, num, den, one, n, c->k, aligned, zeros, st); break;
        case SR_RING_BABYBEAR_POW2: e = sr::inverse::launch<sr::BabyBear>({}, out, num, den, one, n, c->k, aligned, zeros, st); break;
        case SR_RING_STARK_POW2: e = sr::inverse::launch<sr::Stark>({}, out, num, den, one, n, c->k, aligned, zeros, st); break;
        case SR_RING_GOLDILOCKS_24: e = sr::inverse::launch<sr::SlotG24>(c->small, out, num, den, one, n, 0, aligned, zeros, st); break;
        case SR_RING_BABYBEAR_72: e = sr::inverse::launch<sr::SlotB72>(c->small, out, num, den, one, n, 0, aligned, zeros, st); break;
        default: e = sr::inverse::launch<sr::SlotFrog>(c->frog, out, num, den, one, n, 0, aligned, zeros, st); break;
    }
    if (e != hipSuccess) return fail(SR_E_HIP, std::string("inverse launch: ") + hipGetErrorString(e));
    return SR_OK;
}
// the argument checks the two forms of sr_inverse_batch share
int check_inverse(sr_ctx *c, const void *out, const void *num, const void *den, size_t n) {
    if (!c) return fail(SR_E_INVALID, "null context");
    if (!out) return fail(SR_E_INVALID, "inverse: null output buffer");
    if (!den) return fail(SR_E_INVALID, "inverse: null denominators");
    if (int rc = check_count(c, n)) return rc;
    const size_t bytes = n * (size_t)c->degree * c->limbs * 8;
    if (out != den && ranges_overlap(out, bytes, den, bytes)) return fail(SR_E_INVALID, "inverse: d_out overlaps d_den (in place needs d_out == d_den)");
    if (num && out != num && ranges_overlap(out, bytes, num, bytes))
        return fail(SR_E_INVALID, "inverse: d_out overlaps d_num (in place needs d_out == d_num)");
    return SR_OK;
}
// ---- linear combinations (csrc/lincomb.hpp): every launch under K_POINTWISE, nothing allocated, no context scratch -------------------
// The launches of sr::lincomb::plan: outputs m0 .. m0 + outputs_per_launch - 1 each, every launch over all the tables.
int dev_lincomb(sr_ctx *c, uint64_t *const *outs, int n_outputs, const uint64_t *const *tables, const size_t *n_evals, int n_tables,
                const uint64_t *coef, const uint32_t *uses, size_t n, hipStream_t st) {
    if (n == 0) return SR_OK;
    sr::lincomb::Plan p;
    if (!sr::lincomb::plan(c->ring, n_tables, n_outputs, &p)) return fail(SR_E_INVALID, "lincomb: no plan for these arguments");
    const size_t w = (size_t)c->degree * c->limbs;
    uintptr_t all = (uintptr_t)coef;
    for (int k = 0; k < n_tables; k++) all |= (uintptr_t)tables[k];
    for (int m = 0; m < n_outputs; m++) all |= (uintptr_t)outs[m];
    const bool aligned = (all & 15u) == 0;
    for (int m0 = 0; m0 < n_outputs; m0 += p.outputs_per_launch) {
        const int mm = n_outputs - m0 < p.outputs_per_launch ? n_outputs - m0 : p.outputs_per_launch;
        const bool reg = p.launches == 1 && n_tables <= sr::lincomb::kRegTables;
        sr::lincomb::Args a{};
        for (int k = 0; k < n_tables; k++) {
            a.t[k] = tables[k];
            a.ne[k] = n_evals ? n_evals[k] : n;
        }
        for (int m = 0; m < mm; m++) {
            a.out[m] = outs[m0 + m];
            a.uses[m] = uses[m0 + m];
        }
        a.coef = coef + (size_t)m0 * (n_tables + 1) * w;
        ProfScope prof(c, st, K_POINTWISE);
        hipError_t e;
        switch (c->ring) {
            case SR_RING_GOLDILOCKS_POW2: e = sr::lincomb::launch<sr::Goldilocks>({}, reg && mm <= sr::lincomb::kRegOutputs<sr::Goldilocks>, mm, a, n_tables, n, c->k, aligned, st); break;
            case SR_RING_BABYBEAR_POW2: e = sr::lincomb::launch<sr::BabyBear>({}, reg && mm <= sr::lincomb::kRegOutputs<sr::BabyBear>, mm, a, n_tables, n, c->k, aligned, st); break;
            case SR_RING_STARK_POW2: e = sr::lincomb::launch<sr::Stark>({}, reg && mm <= sr::lincomb::kRegOutputs<sr::Stark>, mm, a, n_tables, n, c->k, aligned, st); break;
            case SR_RING_GOLDILOCKS_24: e = sr::lincomb::launch<sr::SlotG24>(c->small, reg && mm <= sr::lincomb::kRegOutputs<sr::SlotG24>, mm, a, n_tables, n, 0, aligned, st); break;
            case SR_RING_BABYBEAR_72: e = sr::lincomb::launch<sr::SlotB72>(c->small, false, mm, a, n_tables, n, 0, aligned, st); break;
            default: e = sr::lincomb::launch<sr::SlotFrog>(c->frog, false, mm, a, n_tables, n, 0, aligned, st); break;
        }
        if (e != hipSuccess) return fail(SR_E_HIP, std::string("lincomb launch: ") + hipGetErrorString(e));
    }
    return SR_OK;
}
// ---- linear combinations with integer columns, multiplicities (csrc/lincomb_index.hpp): as above, nothing allocated -----------------
// n_index == 0 is dev_lincomb, bit for bit
int dev_lincomb_index(sr_ctx *c, uint64_t *const *outs, int n_outputs, const uint64_t *const *tables, const size_t *n_evals, int n_tables,
                      const sr_index_column *cols, int n_index, const uint64_t *coef, const uint32_t *uses, size_t n, hipStream_t st) {
    namespace li = sr::lincomb_index;
    if (n_index == 0) return dev_lincomb(c, outs, n_outputs, tables, n_evals, n_tables, coef, uses, n, st);
    if (n == 0) return SR_OK;
    sr::lincomb::Plan p;
    if (!li::plan(c->ring, n_tables, n_index, n_outputs, &p)) return fail(SR_E_INVALID, "lincomb_index: no plan for these arguments");
    const size_t w = (size_t)c->degree * c->limbs;
    const int terms = n_tables + n_index;
    uintptr_t all = (uintptr_t)coef;
    for (int k = 0; k < n_tables; k++) all |= (uintptr_t)tables[k];
    for (int m = 0; m < n_outputs; m++) all |= (uintptr_t)outs[m];
    const bool aligned = (all & 15u) == 0;
    const bool reg = p.launches == 1 && terms <= li::kRegTerms;
    for (int m0 = 0; m0 < n_outputs; m0 += p.outputs_per_launch) {
        const int mm = n_outputs - m0 < p.outputs_per_launch ? n_outputs - m0 : p.outputs_per_launch;
        li::Args a{};
        for (int k = 0; k < n_tables; k++) {
            a.t[k] = tables[k];
            a.ne[k] = n_evals ? n_evals[k] : n;
        }
        for (int j = 0; j < n_index; j++) {
            a.col[j] = cols[j].values;
            a.cne[j] = cols[j].values ? cols[j].n_evals : 0;
            a.start[j] = cols[j].start;
        }
        for (int m = 0; m < mm; m++) {
            a.out[m] = outs[m0 + m];
            a.uses[m] = uses[m0 + m];
        }
        a.coef = coef + (size_t)m0 * (terms + 1) * w;
        ProfScope prof(c, st, K_POINTWISE);
        hipError_t e;
        switch (c->ring) {
            case SR_RING_GOLDILOCKS_POW2: e = li::launch<sr::Goldilocks>({}, reg, mm, a, n_tables, n_index, n, c->k, aligned, st); break;
            case SR_RING_BABYBEAR_POW2: e = li::launch<sr::BabyBear>({}, reg, mm, a, n_tables, n_index, n, c->k, aligned, st); break;
            case SR_RING_STARK_POW2: e = li::launch<sr::Stark>({}, reg, mm, a, n_tables, n_index, n, c->k, aligned, st); break;
            case SR_RING_GOLDILOCKS_24: e = li::launch<sr::SlotG24>(c->small, reg, mm, a, n_tables, n_index, n, 0, aligned, st); break;
            case SR_RING_BABYBEAR_72: e = li::launch<sr::SlotB72>(c->small, false, mm, a, n_tables, n_index, n, 0, aligned, st); break;
            default: e = li::launch<sr::SlotFrog>(c->frog, false, mm, a, n_tables, n_index, n, 0, aligned, st); break;
        }
        if (e != hipSuccess) return fail(SR_E_HIP, std::string("lincomb_index launch: ") + hipGetErrorString(e));
    }
    return SR_OK;
}
// Which call the shared checks and the shared staging speak for.  sr_lincomb is sr_lincomb_index without index columns: its terms
// are its tables, so there is at least one.
struct LincombCall {
    const char *name, *n_terms;  // the prefix of every message; what the message calls the term count
    int min_tables;
};
const LincombCall kLincomb{"lincomb", "n_tables", 1}, kLincombIndex{"lincomb_index", "n_tables + n_index", 0};
// entry: "" or "_plan"
int refuse(const LincombCall &who, const char *entry, const std::string &what) {
    return fail(SR_E_INVALID, std::string(who.name) + entry + ": " + what);
}
// the counts the *_plan call and the two forms of the call share
int check_lincomb_counts(const LincombCall &who, const char *entry, int n_tables, int n_index, int n_outputs) {
    if (n_tables < who.min_tables || n_tables > SR_LINCOMB_MAX_TABLES)
        return refuse(who, entry, "n_tables outside " + std::to_string(who.min_tables) + " .. 16");
    if (n_index < 0 || n_index > SR_LINCOMB_MAX_INDEX_COLUMNS) return refuse(who, entry, "n_index outside 0 .. 8");
    if (n_tables + n_index < 1 || n_tables + n_index > SR_LINCOMB_MAX_TABLES) return refuse(who, entry, std::string(who.n_terms) + " outside 1 .. 16");
    if (n_outputs < 1 || n_outputs > SR_LINCOMB_MAX_OUTPUTS) return refuse(who, entry, "n_outputs outside 1 .. 4");
    return SR_OK;
}
// the body of the two *_plan entry points
int lincomb_plan_entry(const LincombCall &who, int ring, int log2_degree, int n_tables, int n_index, int n_outputs, int *launches,
                       int *outputs_per_launch) {
    if (int rc = check_plan_ring(ring, log2_degree)) return rc;
    if (!launches || !outputs_per_launch) return refuse(who, "_plan", "null result pointer");
    if (int rc = check_lincomb_counts(who, "_plan", n_tables, n_index, n_outputs)) return rc;
    sr::lincomb::Plan p;
    if (!sr::lincomb_index::plan(ring, n_tables, n_index, n_outputs, &p)) return refuse(who, "_plan", "no plan for these arguments");
    *launches = p.launches;
    *outputs_per_launch = p.outputs_per_launch;
    return SR_OK;
}
// the argument checks the two forms of sr_lincomb and of sr_lincomb_index share; everything here is host arithmetic on the arguments
int check_lincomb_index(const LincombCall &who, sr_ctx *c, uint64_t *const *outs, int n_outputs, const uint64_t *const *tables,
                        const size_t *n_evals, int n_tables, const sr_index_column *cols, int n_index, const uint64_t *coef, const uint32_t *uses,
                        size_t n) {
    if (!c) return fail(SR_E_INVALID, "null context");
    if (int rc = check_lincomb_counts(who, "", n_tables, n_index, n_outputs)) return rc;
    const int terms = n_tables + n_index;
    if (!outs || (n_tables && !tables) || (n_index && !cols) || !coef || !uses) return refuse(who, "", "null argument");
    uint32_t any = 0;
    for (int m = 0; m < n_outputs; m++) {
        if (uses[m] == 0) return refuse(who, "", "an output with an empty mask");
        if (uses[m] >> (terms + 1)) return refuse(who, "", std::string("a mask bit above ") + who.n_terms);
        any |= uses[m];
    }
    for (int k = 0; k < n_tables; k++)
        if (!((any >> k) & 1u)) return refuse(who, "", "a table that no output uses");
    for (int j = 0; j < n_index; j++)
        if (!((any >> (n_tables + j)) & 1u)) return refuse(who, "", "a column that no output uses");
    if (n >= (size_t)1 << 48) return refuse(who, "", "n must be below 2^48");
    for (int k = 0; k < n_tables; k++)
        if (n_evals && n_evals[k] > n) return refuse(who, "", "n_evals exceeds n");
    for (int j = 0; j < n_index; j++) {
        if (cols[j].values) {
            if (cols[j].n_evals > n) return refuse(who, "", "a column's n_evals exceeds n");
            if (cols[j].start != 0) return refuse(who, "", "a stored column with a non-zero start");
        } else if (n && cols[j].start > UINT64_MAX - (uint64_t)(n - 1)) {
            return refuse(who, "", "a progression wraps past 2^64 - 1");
        }
    }
    for (int k = 0; k < n_tables; k++)
        if (!tables[k]) return refuse(who, "", "null table");
    for (int m = 0; m < n_outputs; m++)
        if (!outs[m]) return refuse(who, "", "null output");
    if (int rc = check_count(c, n)) return rc;  // everything above is decided without reading the context
    const size_t w = (size_t)c->degree * c->limbs * 8;
    for (int m = 0; m < n_outputs; m++) {
        for (int j = 0; j < m; j++)
            if (ranges_overlap(outs[m], n * w, outs[j], n * w)) return refuse(who, "", "two outputs overlap");
        if (ranges_overlap(outs[m], n * w, coef, (size_t)n_outputs * (terms + 1) * w)) return refuse(who, "", "an output overlaps the coefficients");
        for (int j = 0; j < n_index; j++)
            if (cols[j].values && ranges_overlap(outs[m], n * w, cols[j].values, cols[j].n_evals * 8))
                return refuse(who, "", "an output overlaps a column");
        for (int k = 0; k < n_tables; k++) {
            if (!ranges_overlap(outs[m], n * w, tables[k], (n_evals ? n_evals[k] : n) * w)) continue;
            if (outs[m] != tables[k]) return refuse(who, "", "an output overlaps a table");
            if (n_outputs != 1) return refuse(who, "", "in place needs n_outputs == 1");
        }
    }
    return SR_OK;
}
// the *_dev form of the two calls
int lincomb_dev(const LincombCall &who, sr_ctx *c, uint64_t *const *outs, int n_outputs, const uint64_t *const *tables, const size_t *n_evals,
                int n_tables, const sr_index_column *cols, int n_index, const uint64_t *coef, const uint32_t *uses, size_t n, void *stream) {
    if (int rc = check_lincomb_index(who, c, outs, n_outputs, tables, n_evals, n_tables, cols, n_index, coef, uses, n)) return rc;
    const Call call(c, stream);
    return dev_lincomb_index(c, outs, n_outputs, tables, n_evals, n_tables, cols, n_index, coef, uses, n, call.st);
}
// counts[t] = #{ i : idx[i] == t }: the clear and one launch on the stream; an index >= n_bins goes to d_counter[1] (gather's, spmv's)
int dev_index_count(sr_ctx *c, uint64_t *counts, const uint64_t *idx, size_t n, size_t n_bins, hipStream_t st) {
    if (n_bins) HIP_TRY(hipMemsetAsync(counts, 0, n_bins * 8, st));
    if (n == 0) return SR_OK;
    ProfScope ps(c, st, K_OTHER);
    const hipError_t e = sr::lincomb_index::launch_count(counts, idx, n, n_bins, c->d_counter + 1, st);
    return e == hipSuccess ? (int)SR_OK : fail(SR_E_HIP, std::string("index_count launch: ") + hipGetErrorString(e));
}
int check_index_count(sr_ctx *c, const uint64_t *counts, const uint64_t *idx, size_t n, size_t n_bins) {
    if (!c) return fail(SR_E_INVALID, "null context");
    if (n >= (size_t)1 << 48) return fail(SR_E_INVALID, "index_count: n must be below 2^48");
    if (n_bins >= (size_t)1 << 48) return fail(SR_E_INVALID, "index_count: n_bins must be below 2^48");
    if (n_bins && !counts) return fail(SR_E_INVALID, "index_count: null counts");
    if (n && !idx) return fail(SR_E_INVALID, "index_count: null indices");
    if (ranges_overlap(counts, n_bins * 8, idx, n * 8)) return fail(SR_E_INVALID, "index_count: counts overlaps the indices");
    return SR_OK;
}
// d_counter[i] (sr_ctx_create_ex) to the host, then cleared
int read_counter(sr_ctx *c, int i, unsigned long long *out, hipStream_t st) {
    HIP_TRY(hipMemcpyAsync(out, c->d_counter + i, sizeof *out, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemsetAsync(c->d_counter + i, 0, sizeof *out, st));
    HIP_TRY(hipStreamSynchronize(st));
    return SR_OK;
}

// ---- host-pointer entry points: stage, run, copy back ----
// One operand of a one-shot host-pointer call: `bytes` in its HOST_* slot, uploaded from `up` and / or downloaded to `down`
struct Staged {
    const void *up;
    void *down;
    size_t bytes;
};
// Operand i lives in HOST_i.  The slots grow to fit, the uploads are enqueued on the context's stream, body(device pointers, HOST_0
// first) enqueues the work, the downloads follow and the stream is synchronised: the calls hold the context's mutex, so every HOST_*
// slot is free again when the next one starts.  A failed body downloads nothing.  Zero-byte copies are skipped (an empty operand
// may have no host buffer).
template <size_t N, class Body>
int staged(sr_ctx *c, const Staged (&ops)[N], Body body) {
    static_assert(N <= HOST_4 - HOST_0 + 1, "one HOST_* slot per operand");
    for (size_t i = 0; i < N; i++)
        if (int rc = grow(c, Buf(HOST_0 + i), ops[i].bytes)) return rc;
    for (size_t i = 0; i < N; i++)
        if (ops[i].up && ops[i].bytes) HIP_TRY(hipMemcpyAsync(c->buf[HOST_0 + i], ops[i].up, ops[i].bytes, hipMemcpyHostToDevice, c->stream));
    if (int rc = body(c->buf + HOST_0)) {
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    for (size_t i = 0; i < N; i++)
        if (ops[i].down && ops[i].bytes) HIP_TRY(hipMemcpyAsync(ops[i].down, c->buf[HOST_0 + i], ops[i].bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SR_OK;
}
// The tables of a host-pointer call in one HOST_* slot: one behind the other, each on a 16-byte boundary
struct TableSlot {
    size_t off[SR_VPOLY_MAX_TABLES], total = 0;
    TableSlot(const size_t *n, int n_tables, size_t w) {
        for (int j = 0; j < n_tables; j++) {
            off[j] = total;
            total += (n[j] * w + 15) & ~(size_t)15;
        }
    }
    // d[j]: table j of the slot at `base`
    void at(void *base, int n_tables, uint64_t **d) const {
        for (int j = 0; j < n_tables; j++) d[j] = (uint64_t *)((char *)base + off[j]);
    }
};
// the host tables to their places d[j], on the context's stream
int upload_tables(sr_ctx *c, uint64_t *const *d, const uint64_t *const *tables, const size_t *n, int n_tables, size_t w) {
    for (int j = 0; j < n_tables; j++)
        if (n[j]) HIP_TRY(hipMemcpyAsync(d[j], tables[j], n[j] * w, hipMemcpyHostToDevice, c->stream));
    return SR_OK;
}
// A host-pointer round call (the families of RoundCall, above): the checks, then the operands to their slots -- HOST_0: the tables;
// HOST_1: the message; HOST_2: the workspace; HOST_3: the folded tables; HOST_4: r, the coefficients and the weights, each on a 16-byte
// boundary (an absent operand takes no room) -- and the same call on the device copies.  A fold's tables come back by the counts
// the launch left in n_evals_out.
int round_host(sr_ctx *c, RoundCall &a) {
    if (int rc = check_round(c, a, false)) return rc;
    const RoundFamily &f = a.f;
    const Call call(c);
    const size_t w = (size_t)c->degree * c->limbs * 8;
    const int nt = a.n_tables, nf = f.fold ? nt : 0;
    size_t n_out[SR_VPOLY_MAX_TABLES];
    for (int j = 0; j < nf; j++) n_out[j] = round_fold_n_out(a.n_evals[j], a.num_vars, a.mode);
    const uint64_t *const rest[3] = {a.r, a.coef, a.weights};
    const size_t rest_bytes[3] = {a.r ? w : 0, a.coef ? a.n_coef() * w : 0, a.weights ? w << f.weight_log2(a.num_vars) : 0};
    // a slot's host source and its bytes: a table's elements, a stored column's integers, nothing for a progression
    const uint64_t *src[SR_VPOLY_MAX_TABLES];
    size_t src_bytes[SR_VPOLY_MAX_TABLES];
    for (int j = 0; j < nt; j++) {
        const sr_index_column *col = j >= a.first_column() ? a.columns + (j - a.first_column()) : nullptr;
        src[j] = col ? col->values : a.tables[j];
        src_bytes[j] = col ? (col->values ? col->n_evals * 8 : 0) : a.n_evals[j] * w;
    }
    const TableSlot in(src_bytes, nt, 1), folded(n_out, nf, w), aux(rest_bytes, 3, 1);
    return staged(c, {{nullptr, nullptr, in.total}, {nullptr, a.out, a.plan.np_total * w}, {nullptr, nullptr, a.plan.work_elems * w},
                      {nullptr, nullptr, folded.total}, {nullptr, nullptr, aux.total}},
                  [&](void *const *d) -> int {
                      uint64_t *dt[SR_VPOLY_MAX_TABLES], *df[SR_VPOLY_MAX_TABLES], *ds[3];
                      in.at(d[0], nt, dt);
                      folded.at(d[3], nf, df);
                      aux.at(d[4], 3, ds);
                      if (int rc = upload_tables(c, dt, src, src_bytes, nt, 1)) return rc;
                      if (int rc = upload_tables(c, ds, rest, rest_bytes, 3, 1)) return rc;
                      RoundCall dev = a;
                      sr_index_column dc[SR_LINCOMB_MAX_INDEX_COLUMNS];
                      for (int j = 0; j < a.n_index; j++) {
                          dc[j] = a.columns[j];
                          if (dc[j].values) dc[j].values = dt[a.first_column() + j];
                      }
                      dev.columns = a.n_index ? dc : nullptr;
                      dev.out = (uint64_t *)d[1], dev.work = (uint64_t *)d[2], dev.tables = dt, dev.out_tables = nf ? df : nullptr;
                      dev.r = a.r ? ds[0] : nullptr, dev.coef = a.coef ? ds[1] : nullptr, dev.weights = a.weights ? ds[2] : nullptr;
                      if (int rc = dev_round(c, dev, c->stream)) return rc;
                      for (int j = 0; j < nf; j++)
                          if (a.n_evals_out[j])
                              HIP_TRY(hipMemcpyAsync(a.out_tables[j], df[j], a.n_evals_out[j] * w, hipMemcpyDeviceToHost, c->stream));
                      return SR_OK;
                  });
}
// The weighted calls with integer columns.  Without columns they ARE the weighted calls (family kVpolyWround / kVpolyWroundFold);
// otherwise the slots of the call -- the tables, then the columns -- are laid out for RoundCall here, after the checks that only the
// columns have.
const RoundFamily &iwround_family(bool fold) { return fold ? kVpolyIwroundFold : kVpolyIwround; }
int check_iwround_counts(const RoundFamily &f, int n_tables, int n_index) {
    if (n_index < 0 || n_index > SR_LINCOMB_MAX_INDEX_COLUMNS) return refuse(f, "n_index must be 0 .. 8");
    if (n_index == 0) return SR_OK;  // the weighted call checks its own n_tables
    if (n_tables < 0 || n_tables + n_index > SR_VPOLY_MAX_TABLES) return refuse(f, "n_tables + n_index must be 1 .. 8");
    return SR_OK;
}
int iwround_call(bool fold, bool dev, sr_ctx *c, uint64_t *out, uint64_t *const *out_tables, size_t *n_evals_out, const uint64_t *weights,
                 const uint64_t *const *tables, const size_t *n_evals, int n_tables, const sr_index_column *columns, int n_index,
                 const sr_vpoly_term *terms, int n_terms, const uint64_t *coef, size_t num_vars, const uint64_t *r, int order, uint64_t *work,
                 size_t work_elems, void *stream) {
    const RoundFamily &f = iwround_family(fold);
    if (int rc = check_iwround_counts(f, n_tables, n_index)) return rc;
    const uint64_t *slot_tables[SR_VPOLY_MAX_TABLES];
    size_t slot_evals[SR_VPOLY_MAX_TABLES];
    if (n_index) {
        if (!columns) return refuse(f, "null pointer (columns)");
        if (n_tables && (!tables || !n_evals)) return refuse(f, "null pointer");
        if (num_vars >= 48) return refuse(f, "num_vars must be below 48");
        const size_t full = (size_t)1 << num_vars;
        for (int j = 0; j < n_tables; j++) {
            slot_tables[j] = tables[j];
            slot_evals[j] = n_evals[j];
        }
        for (int j = 0; j < n_index; j++) {
            const sr_index_column &col = columns[j];
            if (col.values) {
                if (col.start != 0) return refuse(f, "a stored column with a non-zero start");
                if (col.n_evals > full) return refuse(f, "a column's n_evals exceeds 2^num_vars");
            } else if (col.start > UINT64_MAX - (uint64_t)(full - 1)) {
                return refuse(f, "a progression wraps past 2^64 - 1");
            }
            slot_tables[n_tables + j] = nullptr;
            slot_evals[n_tables + j] = col.values ? col.n_evals : full;
        }
    }
    RoundCall a{n_index ? f : (fold ? kVpolyWroundFold : kVpolyWround), out, n_index ? slot_tables : tables, n_index ? slot_evals : n_evals,
                n_tables + n_index, num_vars, order};
    a.out_tables = out_tables, a.n_evals_out = n_evals_out, a.r = r;
    a.weights = weights, a.terms = terms, a.n_terms = n_terms, a.coef = coef;
    a.work = work, a.work_elems = work_elems;
    a.columns = n_index ? columns : nullptr, a.n_index = n_index;
    return dev ? round_dev(c, a, stream) : round_host(c, a);
}
// The host-pointer form of sr_lincomb and sr_lincomb_index.  HOST_0: the stored parts of the tables, one behind the other on 16-byte
// boundaries; HOST_1: the outputs; HOST_2: the coefficients; HOST_3: the stored parts of the index arrays, copied as they are
int lincomb_host(const LincombCall &who, sr_ctx *c, uint64_t *const *outs, int n_outputs, const uint64_t *const *tables, const size_t *n_evals,
                 int n_tables, const sr_index_column *columns, int n_index, const uint64_t *coef, const uint32_t *uses, size_t n) {
    if (int rc = check_lincomb_index(who, c, outs, n_outputs, tables, n_evals, n_tables, columns, n_index, coef, uses, n)) return rc;
    if (n == 0) return SR_OK;
    const Call call(c);
    const size_t w = (size_t)c->degree * c->limbs * 8, ob = (n * w + 15) & ~(size_t)15;
    size_t off[SR_LINCOMB_MAX_TABLES], total = 0, coff[SR_LINCOMB_MAX_INDEX_COLUMNS], ctotal = 0;
    for (int k = 0; k < n_tables; k++) {
        off[k] = total;
        total += ((n_evals ? n_evals[k] : n) * w + 15) & ~(size_t)15;
    }
    for (int j = 0; j < n_index; j++) {
        coff[j] = ctotal;
        ctotal += 16 + (((columns[j].values ? columns[j].n_evals * 8 : 0) + 15) & ~(size_t)15);  // never empty: a stored column keeps a non-null pointer
    }
    return staged(c, {{nullptr, nullptr, total}, {nullptr, nullptr, ob * n_outputs}, {coef, nullptr, (size_t)n_outputs * (n_tables + n_index + 1) * w},
                      {nullptr, nullptr, ctotal}},
                  [&](void *const *d) -> int {
                      const uint64_t *dt[SR_LINCOMB_MAX_TABLES];
                      uint64_t *dout[SR_LINCOMB_MAX_OUTPUTS];
                      sr_index_column dc[SR_LINCOMB_MAX_INDEX_COLUMNS];
                      for (int k = 0; k < n_tables; k++) {
                          dt[k] = (const uint64_t *)((char *)d[0] + off[k]);
                          const size_t b = (n_evals ? n_evals[k] : n) * w;
                          if (b) HIP_TRY(hipMemcpyAsync((void *)dt[k], tables[k], b, hipMemcpyHostToDevice, c->stream));
                      }
                      for (int j = 0; j < n_index; j++) {
                          dc[j] = columns[j];
                          if (!columns[j].values) continue;
                          dc[j].values = (const uint64_t *)((char *)d[3] + coff[j]);
                          const size_t b = columns[j].n_evals * 8;
                          if (b) HIP_TRY(hipMemcpyAsync((void *)dc[j].values, columns[j].values, b, hipMemcpyHostToDevice, c->stream));
                      }
                      for (int m = 0; m < n_outputs; m++) dout[m] = (uint64_t *)((char *)d[1] + ob * m);
                      if (int r = dev_lincomb_index(c, dout, n_outputs, dt, n_evals, n_tables, dc, n_index, (const uint64_t *)d[2], uses, n, c->stream))
                          return r;
                      for (int m = 0; m < n_outputs; m++) HIP_TRY(hipMemcpyAsync(outs[m], dout[m], n * w, hipMemcpyDeviceToHost, c->stream));
                      return SR_OK;
                  });
}
// Sum / Product on host buffers: the n elements go to a device temporary as a whole (like the linear-algebra calls)
int host_fold(sr_ctx *c, uint64_t *out, const uint64_t *in, size_t n, bool mul) {
    if (int rc = check_fold(c, out, in, n)) return rc;
    const Call call(c);
    const size_t w = (size_t)c->degree * c->limbs * 8;
    return staged(c, {{in, nullptr, n * w}, {nullptr, out, w}}, [&](void *const *d) {
        const uint64_t *di = (const uint64_t *)d[0];
        uint64_t *dout = (uint64_t *)d[1];
        return mul ? dev_product(c, dout, di, n, c->stream) : dev_sum(c, dout, di, n, c->stream);
    });
}
// Host-pointer batches: results = compute(a[, b]) element-wise over the batch, through device staging buffers.
// Small batches: copy in, compute, copy out on the context's stream.  Large batches are cut into chunks (default 128 MiB per
// operand, SR_HOST_CHUNK_MB) that alternate between two sets of staging buffers: the calling thread copies chunk i in and
// launches it while a helper thread copies chunk i-1 out on a second stream, so the two PCIe directions overlap and the device
// memory needed no longer grows with the batch.  compute(s0, s1, n, stream) works in place on s0 (n elements).
// unit_bytes != 0: the batch counts units of that many bytes instead of ring elements (the norms count coefficients).  out == nullptr:
// a read-only pass -- nothing is copied back, compute() keeps what it needs, and a lane's buffer is free for chunk i + 2 by stream order.
int host_pipeline(sr_ctx *c, uint64_t *out, const uint64_t *a, const uint64_t *b, size_t batch,
                  const std::function<int(uint64_t *, uint64_t *, size_t, hipStream_t)> &compute, size_t unit_bytes = 0) {
    const size_t elem_bytes = unit_bytes ? unit_bytes : c->degree * c->limbs * 8;
    const size_t bytes = batch * elem_bytes;
    if (bytes == 0) return SR_OK;
    // The caller's buffers are ordinary (pageable) host memory -- a Rust Vec -- and stay that way: round 3 registered them with the
    // HIP runtime for the duration of the call (hipHostRegister), which measured inside the noise (69.8-78.3 against 66.9-73.0 GB/s:
    // the pipeline is PCIe-bound either way) and had two lifetime hazards (a read-only operand shared by two contexts on two
    // threads was unregistered by whichever call returned first while the other GPU's DMA still read it; an early error return
    // unregistered pages under an in-flight copy).  Removed in round 4; SR_PLAN_NO_HOST_PIN is accepted and has no effect.
    const size_t chunk_mb = c->plan.host_chunk_mb ? c->plan.host_chunk_mb : 128;
    size_t chunk = (chunk_mb << 20) / elem_bytes;
    if (chunk == 0) chunk = 1;
    if (batch <= 2 * chunk) {  // one shot
        auto run = [&](void *const *d) { return compute((uint64_t *)d[0], (uint64_t *)d[1], batch, c->stream); };
        return b ? staged(c, {{a, out, bytes}, {b, nullptr, bytes}}, run) : staged(c, {{a, out, bytes}}, run);
    }
    const size_t chunk_bytes = chunk * elem_bytes;
    for (int i = 0; i < 4; i++)
        if (b || (i & 1) == 0)
            if (int rc = grow(c, Buf(HOST_0 + i), chunk_bytes)) return rc;
    hipEvent_t ready[2];
    for (auto &e : ready) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    struct Job {
        const void *src;
        uint64_t *dst;
        size_t bytes;
    } jobs[2];
    std::mutex m;
    std::condition_variable cv;
    size_t submitted = 0, done = 0;
    bool stop = false;
    hipError_t worker_err = hipSuccess;
    const int device = c->device;
    hipStream_t out_stream = c->out_stream;
    std::thread worker([&] {
        (void)hipSetDevice(device);
        for (;;) {
            Job j;
            int lane;
            {
                std::unique_lock<std::mutex> lk(m);
                cv.wait(lk, [&] { return done < submitted || stop; });
                if (done == submitted) return;
                lane = (int)(done & 1);
                j = jobs[lane];
            }
            hipError_t e = hipStreamWaitEvent(out_stream, ready[lane], 0);
            if (e == hipSuccess) e = hipMemcpyAsync(j.dst, j.src, j.bytes, hipMemcpyDeviceToHost, out_stream);
            if (e == hipSuccess) e = hipStreamSynchronize(out_stream);
            {
                std::lock_guard<std::mutex> lk(m);
                if (e != hipSuccess && worker_err == hipSuccess) worker_err = e;
                done++;
            }
            cv.notify_all();
        }
    });
    int rc = SR_OK;
    hipError_t main_err = hipSuccess;
    const size_t nchunks = (batch + chunk - 1) / chunk;
    for (size_t i = 0; i < nchunks && rc == SR_OK && main_err == hipSuccess; i++) {
        const int lane = (int)(i & 1);
        const size_t first = i * chunk, n = batch - first < chunk ? batch - first : chunk;
        if (out) {
            std::unique_lock<std::mutex> lk(m);  // the lane's buffers are free once chunk i - 2 has been copied out
            cv.wait(lk, [&] { return i < 2 || done + 1 >= i; });
        }
        uint64_t *s0 = (uint64_t *)c->buf[HOST_0 + 2 * lane], *s1 = (uint64_t *)c->buf[HOST_1 + 2 * lane];
        main_err = hipMemcpyAsync(s0, a + first * (elem_bytes / 8), n * elem_bytes, hipMemcpyHostToDevice, c->stream);
        if (main_err == hipSuccess && b)
            main_err = hipMemcpyAsync(s1, b + first * (elem_bytes / 8), n * elem_bytes, hipMemcpyHostToDevice, c->stream);
        if (main_err != hipSuccess) break;
        rc = compute(s0, s1, n, c->stream);
        if (rc != SR_OK) break;
        if (!out) continue;
        main_err = hipEventRecord(ready[lane], c->stream);
        if (main_err != hipSuccess) break;
        {
            std::lock_guard<std::mutex> lk(m);
            jobs[lane] = Job{s0, out + first * (elem_bytes / 8), n * elem_bytes};
            submitted++;
        }
        cv.notify_all();
    }
    {
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return done == submitted; });
        stop = true;
    }
    cv.notify_all();
    worker.join();
    (void)hipStreamSynchronize(c->stream);
    for (auto &e : ready) (void)hipEventDestroy(e);
    if (rc != SR_OK) return rc;
    if (main_err != hipSuccess) return fail(SR_E_HIP, std::string("host pipeline: ") + hipGetErrorString(main_err));
    if (worker_err != hipSuccess) return fail(SR_E_HIP, std::string("host pipeline (copy out): ") + hipGetErrorString(worker_err));
    return SR_OK;
}
int host_inplace(sr_ctx *c, uint64_t *data, size_t batch, bool fwd) {
    if (int rc = check(c, {data}, batch)) return rc;
    const Call call(c);
    return host_pipeline(c, data, data, nullptr, batch, [&](uint64_t *s0, uint64_t *, size_t n, hipStream_t st) {
        return fwd ? dev_fwd(c, s0, n, st) : dev_inv(c, s0, n, st);
    });
}
// the unary operators on host buffers: op 0 neg, 1 scale, 2 add scalar (coefficient form), 3 add scalar (NTT form)
int host_unary(sr_ctx *c, uint64_t *data, const uint64_t *scalar, size_t batch, int op) {
    if (int rc = check(c, {data, op ? (const void *)scalar : (const void *)1}, batch)) return rc;
    const Call call(c);
    return host_pipeline(c, data, data, nullptr, batch, [&](uint64_t *s0, uint64_t *, size_t n, hipStream_t st) {
        return op == 0 ? dev_neg(c, s0, n, st) : op == 1 ? dev_scale(c, s0, scalar, n, st) : dev_add_scalar(c, s0, scalar, op == 3, n, st);
    });
}
enum { HB_POINTWISE = 0, HB_RING_MUL = 1, HB_ADD = 2, HB_SUB = 3, HB_RING_MUL_NTT_RHS = 4 };
int host_binary(sr_ctx *c, uint64_t *out, const uint64_t *a, const uint64_t *b, size_t batch, int op) {
    if (int rc = check(c, {out, a, b}, batch)) return rc;
    const Call call(c);
    return host_pipeline(c, out, a, b, batch, [&](uint64_t *s0, uint64_t *s1, size_t n, hipStream_t st) {
        return op == HB_RING_MUL ? dev_ring_mul(c, s0, s0, s1, n, st)
               : op == HB_RING_MUL_NTT_RHS ? dev_ring_mul_ntt_rhs(c, s0, s0, s1, n, st)
               : op == HB_POINTWISE ? dev_pointwise(c, s0, s1, n, st)
                                    : dev_addsub(c, s0, s1, n, op == HB_SUB, st);
    });
}
// ---- packed-u32 boundary (BabyBear power-of-two rings; csrc/packed32.hpp) ----------------------------------------------------
// check() of a packed-u32 entry point: the ring is tested between the buffers and the element count
int check_packed(sr_ctx *c, std::initializer_list<const void *> bufs, size_t batch) {
    if (int rc = check(c, bufs)) return rc;
    if (c->ring != SR_RING_BABYBEAR_POW2) return fail(SR_E_INVALID, "packed32 entry points: BabyBear power-of-two rings only");
    return check_count(c, batch);
}
int launch_pack32(sr_ctx *c, uint32_t *out, const uint64_t *in, size_t n, hipStream_t st) {
    if (n == 0) return SR_OK;
    ProfScope ps(c, st, K_OTHER);
    hipLaunchKernelGGL(sr::p32::pack32_kernel, dim3(sr::p32::blocks_for(n)), dim3(256), 0, st, out, in, n);
    HIP_TRY(hipGetLastError());
    return SR_OK;
}
int launch_unpack32(sr_ctx *c, uint64_t *out, const uint32_t *in, size_t n, hipStream_t st) {
    if (n == 0) return SR_OK;
    ProfScope ps(c, st, K_OTHER);
    hipLaunchKernelGGL(sr::p32::unpack32_kernel, dim3(sr::p32::blocks_for(n)), dim3(256), 0, st, out, in, n);
    HIP_TRY(hipGetLastError());
    return SR_OK;
}
// D < 4096 has no register-tiled path: such (small) batches are widened into the context's staging buffers, run through the 8-byte
// kernels and narrowed again -- same values, only the traffic advantage is lost where it does not matter
template <class Fn>
int packed_via_wide(sr_ctx *c, uint32_t *out, const uint32_t *a, const uint32_t *b, size_t batch, hipStream_t st, Fn run) {
    const size_t n = batch << c->k;
    if (int rc = grow(c, WIDE_A, n * 8, st)) return rc;
    if (b)
        if (int rc = grow(c, WIDE_B, n * 8, st)) return rc;
    ScratchUse su(c, st);  // the staging buffers belong to the context, the call may arrive on any stream: ordered like the operand scratch
    if (int rc = su.acquire()) return rc;
    uint64_t *wa = (uint64_t *)c->buf[WIDE_A], *wb = (uint64_t *)c->buf[WIDE_B];
    if (int rc = launch_unpack32(c, wa, a, n, st)) return rc;
    if (b)
        if (int rc = launch_unpack32(c, wb, b, n, st)) return rc;
    if (int rc = run(wa, wb)) return rc;
    return launch_pack32(c, out, wa, n, st);
}
int packed_elementwise(sr_ctx *c, uint32_t *l, const uint32_t *r, size_t batch, void *stream, int op) {
    if (int rc = check_packed(c, {l, r}, batch)) return rc;
    const Call call(c, stream);
    const size_t n = batch << c->k;
    if (n == 0) return SR_OK;
    ProfScope ps(c, call.st, K_POINTWISE);
    const dim3 gr(sr::p32::blocks_for(n)), bl(256);
    if (op == 0) hipLaunchKernelGGL(sr::p32::elementwise32_kernel<0>, gr, bl, 0, call.st, l, r, n);
    else if (op == 1) hipLaunchKernelGGL(sr::p32::elementwise32_kernel<1>, gr, bl, 0, call.st, l, r, n);
    else hipLaunchKernelGGL(sr::p32::elementwise32_kernel<2>, gr, bl, 0, call.st, l, r, n);
    HIP_TRY(hipGetLastError());
    return SR_OK;
}
// ---- host-side self-test hook: runs the SAME __host__ __device__ field routines the kernels use,
// on the host, one scalar operation per call.  Lets the CPU test-suite check fields.hpp without a
// GPU.  Not a compute path: no batch entry point routes through it.
// op: 0 add, 1 sub, 2 mul_boundary (a*b*R_b^-1 on in-memory images), 3 mul_tw, 4 tw_from_u64(a[0])
// tools/ubench/field_ops_device.hip runs the same operations in kernels and takes the field ids of sr_selftest_field_op
// (0 Goldilocks, 1 BabyBear, 2 Stark, 3 Frog, 4 StarkL) and the op numbers of selftest_op / selftest_lazy below (its own
// additions start at 16): keep the two equal.
template <class F>
int selftest_op(int op, const uint64_t *a, const uint64_t *b, uint64_t *out) {
    using S = typename F::storage;
    typename F::elem x = F::load(reinterpret_cast<const S *>(a)), y = F::load(reinterpret_cast<const S *>(b)), r;
    switch (op) {
        case 0: r = F::add(x, y); break;
        case 1: r = F::sub(x, y); break;
        case 2: r = F::mul_boundary(x, y); break;
        case 3: r = F::mul_tw(x, y); break;
        case 4: r = F::tw_from_u64(a[0]); break;
        default: return fail(SR_E_INVALID, "selftest: unknown op");
    }
    F::store(reinterpret_cast<S *>(out), r);
    return SR_OK;
}
// StarkL (stark_lazy.hpp): 0 add, 1 sub, 3 mul_tw, 4 table form, 5 a chain of six lazy additions and subtractions feeding
// mul_tw and mul_data, 6 repeated quadrupling with weak reductions, 7 / 8 signed combinations -- results leave through the
// canonicalising store
int selftest_lazy(int op, const uint64_t *a, const uint64_t *b, uint64_t *out) {
    using F = sr::StarkL;
    using S = F::storage;
    F::elem x = F::load(reinterpret_cast<const S *>(a)), y = F::load(reinterpret_cast<const S *>(b)), r;
    switch (op) {
        case 0: r = F::add(x, y); break;
        case 1: r = F::sub(x, y); break;
        case 3: r = F::mul_tw(x, y); break;
        case 4: r = F::tw_from_u64(a[0]); break;
        case 5: {
            F::elem s = x, d = x;
            for (int i = 0; i < 6; i++) {
                s = F::add(s, y);
                d = F::sub(d, y);
            }
            r = F::add(F::mul_tw(s, y), F::mul_data(d, s));
            break;
        }
        case 6: {
            r = x;
            for (int i = 0; i < 4; i++) r = F::weak_reduce(F::add(F::add(r, r), F::add(r, r)));  // 256 a, reduced weakly on the way
            break;
        }
        case 7: {  // 3 a - 5 b and, case 8, 7 a - 2 b without any carry in between: canonical() on signed lazy states
            r = F::sub(F::add(F::add(x, x), x), F::add(F::add(F::add(y, y), F::add(y, y)), y));
            break;
        }
        case 8: {
            F::elem x2 = F::add(x, x), x4 = F::add(x2, x2);
            r = F::sub(F::add(F::add(x4, x2), x), F::add(y, y));
            break;
        }
        default: return fail(SR_E_INVALID, "selftest: unknown op");
    }
    F::store(reinterpret_cast<S *>(out), r);
    return SR_OK;
}
// op 5, field 0: the compile-time shift product of the tuned Goldilocks path, gl::mul_pow2<E>(a[0]) with E = b[0] in [1, 95]
template <int... Es>
uint64_t mul_pow2_any(uint64_t x, int e, std::integer_sequence<int, Es...>) {
    uint64_t r = 0;
    ((e == Es + 1 ? (r = sr::gl::mul_pow2<Es + 1>(x), 0) : 0), ...);
    return r;
}
}  // namespace

// ===============================================================================================
extern "C" {

const char *sr_last_error_string(void) { return g_err.c_str(); }
const char *sr_version(void) { return "stark-rings-amd 0.1 (gfx950)"; }

int sr_ctx_create(int ring, int log2_degree, int device, sr_ctx **out) {
    return sr_ctx_create_ex(ring, log2_degree, device, nullptr, out);
}
int sr_ctx_create_ex(int ring, int log2_degree, int device, const sr_plan *plan, sr_ctx **out) {
    if (!out) return fail(SR_E_INVALID, "null out pointer");
    *out = nullptr;
    if (plan) {
        if (plan->flags >> 9) return fail(SR_E_INVALID, "sr_plan: unknown flag bits");
        if (plan->log_tile && (plan->log_tile < 8 || plan->log_tile > 12)) return fail(SR_E_INVALID, "sr_plan: log_tile must be 0 or 8..12");
        if (plan->stark_whole_max && (plan->stark_whole_max < 9 || plan->stark_whole_max > 12))
            return fail(SR_E_INVALID, "sr_plan: stark_whole_max must be 0 or 9..12");
        if (plan->lanes > 2) return fail(SR_E_INVALID, "sr_plan: lanes must be 0 (default), 1 or 2");
    }
    if (int rc = check_plan_ring(ring, log2_degree)) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(SR_E_NO_DEVICE, "no HIP device available (this backend has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(SR_E_NO_DEVICE, "device index out of range");
    DeviceGuard g(device);
    if (!g.ok) return fail(SR_E_HIP, "hipSetDevice failed");
    sr_ctx *c = new sr_ctx();
    c->ring = ring;
    c->device = device;
    if (plan) c->plan = *plan;
    const uint32_t pf = c->plan.flags;
    int rc = SR_OK;
    auto bail = [&](int code) {
        sr_ctx_destroy(c);
        return code;
    };
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) return bail(fail(SR_E_HIP, "hipStreamCreate failed"));
    if (hipStreamCreateWithFlags(&c->out_stream, hipStreamNonBlocking) != hipSuccess) return bail(fail(SR_E_HIP, "hipStreamCreate failed"));
    // six words: [0] scratch counter of count_noncanonical, [1] out-of-range column indices seen by spmv and out-of-range positions
    // seen by the gather, [2] coefficients that needed more digits than padding_size in a decomposition, [3] wire coefficients >= p /
    // misaligned wire offsets, [4] structural entries of a sparse product none of whose products was non-zero, [5] zero slots met by the batch inversion
    // ([1]..[5] sticky until read)
    if (hipMalloc(&c->d_counter, 6 * sizeof(unsigned long long)) != hipSuccess) return bail(fail(SR_E_ALLOC, "hipMalloc counter failed"));
    if (hipMemset(c->d_counter, 0, 6 * sizeof(unsigned long long)) != hipSuccess) return bail(fail(SR_E_HIP, "hipMemset counter failed"));
    if (is_pow2_ring(ring)) {
        const int k = log2_degree;
        c->k = k;
        c->degree = (size_t)1 << k;
        c->limbs = ring == SR_RING_STARK_POW2 ? 4 : 1;
        // SR_PLAN_STARK_NO_LAZY keeps the Stark transforms on the 8 x 32-bit-limb arithmetic (differential tests); D = 1 has none
        const bool stark_lazy = ring == SR_RING_STARK_POW2 && !(pf & SR_PLAN_STARK_NO_LAZY) && k >= 1;
        const bool stark_tuned = stark_lazy && !(pf & (SR_PLAN_STARK_GENERIC_ON_LAZY | SR_PLAN_GENERIC_KERNELS)) && sr::st::supported(k);
        const bool regtile = k >= 12 && k <= 24;
        switch (ring) {
            case SR_RING_GOLDILOCKS_POW2:
                c->gl_fast.prof_user = c;
                c->gl_fast.prof_begin = gl_prof_begin;
                c->gl_fast.prof_end = gl_prof_end;
                rc = init_pow2<sr::Goldilocks>(c);
                break;
            case SR_RING_BABYBEAR_POW2: rc = init_pow2<sr::BabyBear>(c); break;
            default:
                c->stark_one_tile = sr::st::whole(k, sr::st::whole_max(c->plan.stark_whole_max));
                rc = stark_lazy ? init_pow2<sr::StarkL>(c, stark_tuned) : init_pow2<sr::Stark>(c);
                break;
        }
        if (rc) return bail(rc);
        switch (ring) {
            case SR_RING_GOLDILOCKS_POW2:
                c->path = (pf & SR_PLAN_GL_REGTILE) && regtile ? RT_GOLDILOCKS
                          : !(pf & SR_PLAN_GENERIC_KERNELS) && sr::gl_fast_supported(c->gl_fast) ? GL_FAST
                                                                                                 : GENERIC;
                break;
            case SR_RING_BABYBEAR_POW2: c->path = !(pf & SR_PLAN_GENERIC_KERNELS) && regtile ? RT_BABYBEAR : GENERIC; break;
            default: c->path = stark_tuned ? STARK_TUNED : stark_lazy ? STARK_LAZY : GENERIC; break;
        }
        c->rt_hooks.user = c;
        c->rt_hooks.begin = gl_prof_begin;
        c->rt_hooks.end = gl_prof_end;
    } else if (ring == SR_RING_FROG_16) {
        c->path = FROG;
        c->k = 0;
        c->degree = 16;
        c->limbs = 1;
        sr::frog_init(c->frog);
    } else {
        c->path = ring == SR_RING_GOLDILOCKS_24 ? SMALL_G24 : SMALL_B72;
        c->k = 0;
        c->degree = ring == SR_RING_GOLDILOCKS_24 ? 24 : 72;
        c->limbs = 1;
        if (sr::small_init(c->small, ring == SR_RING_GOLDILOCKS_24)) return bail(fail(SR_E_HIP, "small-ring init failed"));
    }
    *out = c;
    return SR_OK;
}

int sr_ctx_destroy(sr_ctx *c) {
    if (!c) return SR_OK;
    DeviceGuard g(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (auto &p : c->prof.pending) {
        (void)hipEventDestroy(p.a);
        (void)hipEventDestroy(p.b);
    }
    sr::gl_fast_destroy(c->gl_fast);
    sr::small_destroy(c->small);
    if (c->tables) (void)hipFree(c->tables);
    for (void *p : c->buf)
        if (p) (void)hipFree(p);
    if (c->out_stream) (void)hipStreamDestroy(c->out_stream);
    if (c->scratch_free) (void)hipEventDestroy(c->scratch_free);
    if (c->gl_lanes.n) {
        for (int i = 0; i < 2; i++)
            if (c->gl_lanes.join[i]) (void)hipEventDestroy(c->gl_lanes.join[i]);  // the streams are the context's own
        if (c->gl_lanes.fork) (void)hipEventDestroy(c->gl_lanes.fork);
    }
    if (c->d_counter) (void)hipFree(c->d_counter);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return SR_OK;
}

int sr_ctx_degree(const sr_ctx *c, size_t *degree) {
    if (!c || !degree) return fail(SR_E_INVALID, "null argument");
    *degree = c->degree;
    return SR_OK;
}
int sr_ctx_limbs(const sr_ctx *c, int *limbs) {
    if (!c || !limbs) return fail(SR_E_INVALID, "null argument");
    *limbs = c->limbs;
    return SR_OK;
}
int sr_ctx_twiddle_block(sr_ctx *c, void **dev_ptr, size_t *bytes) {
    if (!c || !dev_ptr || !bytes) return fail(SR_E_INVALID, "null argument");
    if (!is_pow2_ring(c->ring)) return fail(SR_E_INVALID, "small rings keep their constants in kernel arguments");
    *dev_ptr = c->tables;
    *bytes = c->table_bytes;
    return SR_OK;
}
int sr_ctx_twiddles_updated(sr_ctx *c) {
    if (!c) return fail(SR_E_INVALID, "null context");
    const Call call(c);
    HIP_TRY(hipDeviceSynchronize());  // every table (generic and tuned) lives in the one block: nothing to rebuild
    return SR_OK;
}

// One context per device of a node, twiddles built ONCE: device_ids[0] builds the block, every other context's block is
// overwritten with a peer copy of it (over xGMI between the GPUs of one node) -- the single-process form of the one-shot
// twiddle broadcast of SURVEY 8e (processes use RCCL: stark_rings_amd/sharding.py).  No data-path traffic afterwards.
int sr_ctx_create_group(int ring, int log2_degree, const int *device_ids, int n, const sr_plan *plan, sr_ctx **out) {
    if (!device_ids || !out || n <= 0) return fail(SR_E_INVALID, "create_group: null argument or n <= 0");
    for (int i = 0; i < n; i++) out[i] = nullptr;
    auto undo = [&](int rc) {
        for (int i = 0; i < n; i++) {
            if (out[i]) sr_ctx_destroy(out[i]);
            out[i] = nullptr;
        }
        return rc;
    };
    for (int i = 0; i < n; i++)
        if (int rc = sr_ctx_create_ex(ring, log2_degree, device_ids[i], plan, &out[i])) return undo(rc);
    if (!is_pow2_ring(ring)) return SR_OK;  // the small rings keep their constants in kernel arguments
    for (int i = 1; i < n; i++) {
        if (out[i]->table_bytes != out[0]->table_bytes) return undo(fail(SR_E_INVALID, "create_group: table sizes differ"));
        // poison first, so that a failed copy cannot leave a locally built (and therefore plausible) table behind
        DeviceGuard g(out[i]->device);
        if (hipMemset(out[i]->tables, 0xFF, out[i]->table_bytes) != hipSuccess) return undo(fail(SR_E_HIP, "create_group: hipMemset failed"));
        if (hipMemcpyPeer(out[i]->tables, out[i]->device, out[0]->tables, out[0]->device, out[0]->table_bytes) != hipSuccess)
            return undo(fail(SR_E_HIP, "create_group: hipMemcpyPeer of the twiddle block failed"));
        if (int rc = sr_ctx_twiddles_updated(out[i])) return undo(rc);
    }
    return SR_OK;
}
// contiguous, balanced split of `batch` ring elements over n contexts: part i gets [*first, *first + *count)
int sr_shard_range(size_t batch, int n, int i, size_t *first, size_t *count) {
    if (!first || !count || n <= 0 || i < 0 || i >= n) return fail(SR_E_INVALID, "shard_range: bad argument");
    const size_t q = batch / (size_t)n, r = batch % (size_t)n;
    *first = (size_t)i * q + ((size_t)i < r ? (size_t)i : r);
    *count = q + ((size_t)i < r ? 1 : 0);
    return SR_OK;
}

// ---- device-resident entry points ----
int sr_ntt_fwd_batch_dev(sr_ctx *c, uint64_t *d, size_t batch, void *stream) {
    if (int rc = check(c, {d}, batch)) return rc;
    const Call call(c, stream);
    return dev_fwd(c, d, batch, call.st);
}
int sr_ntt_inv_batch_dev(sr_ctx *c, uint64_t *d, size_t batch, void *stream) {
    if (int rc = check(c, {d}, batch)) return rc;
    const Call call(c, stream);
    return dev_inv(c, d, batch, call.st);
}
int sr_pointwise_mul_batch_dev(sr_ctx *c, uint64_t *l, const uint64_t *r, size_t batch, void *stream) {
    if (int rc = check(c, {l, r}, batch)) return rc;
    const Call call(c, stream);
    return dev_pointwise(c, l, r, batch, call.st);
}
int sr_mul_elem_batch_dev(sr_ctx *c, uint64_t *d, const uint64_t *elem, size_t batch, void *stream) {
    if (int rc = check(c, {d, elem}, batch)) return rc;
    const uintptr_t w = (uintptr_t)c->degree * c->limbs * 8, pe = (uintptr_t)elem, pd = (uintptr_t)d;
    if (pe + w > pd && pd + batch * w > pe) return fail(SR_E_INVALID, "mul_elem: the element must not lie inside the batch it multiplies");
    const Call call(c, stream);
    return dev_mul_elem(c, d, elem, batch, call.st);
}
int sr_mle_plan(int ring, int log2_degree, size_t num_vars, size_t n_fixed, int order, size_t *work_elems, int *launches) {
    if (int rc = check_plan_ring(ring, log2_degree)) return rc;
    if (!work_elems || !launches) return fail(SR_E_INVALID, "mle_plan: null result pointer");
    if (num_vars >= 48) return fail(SR_E_INVALID, "mle_plan: num_vars must be below 48");
    sr::mle::Plan p;
    if (!sr::mle::plan(ring, num_vars, n_fixed, order, &p))
        return fail(SR_E_INVALID, n_fixed > num_vars ? "mle_plan: n_fixed exceeds num_vars" : "mle_plan: unknown order");
    *work_elems = p.work_elems;
    *launches = p.launches;
    return SR_OK;
}
int sr_mle_fix_variables_dev(sr_ctx *c, uint64_t *out, const uint64_t *evals, size_t n_evals, size_t num_vars, const uint64_t *point,
                             size_t n_fixed, int order, uint64_t *work, size_t work_elems, void *stream) {
    size_t out_elems = 0, need = 0;
    if (int rc = check_mle(c, out, evals, n_evals, num_vars, point, n_fixed, order, &out_elems, &need)) return rc;
    const size_t w = (size_t)c->degree * c->limbs * 8;
    const bool in_place = order == SR_MLE_TRAILING && n_evals && out == evals;
    if (in_place) need = 0;  // an in-place trailing fold keeps its intermediate tables where they are and ignores d_work
    if (need && !work) return fail(SR_E_INVALID, "mle_fix_variables: null buffer");
    if (work_elems < need)
        return fail(SR_E_INVALID, "mle_fix_variables: workspace too small (sr_mle_plan asks for " + std::to_string(need) + " elements)");
    if (!in_place && ranges_overlap(out, out_elems * w, evals, n_evals * w))
        return fail(SR_E_INVALID, "mle_fix_variables: d_out overlaps d_evals (only a trailing-order fold may run in place, with d_out == d_evals)");
    if (ranges_overlap(out, out_elems * w, point, n_fixed * w)) return fail(SR_E_INVALID, "mle_fix_variables: d_out overlaps d_point");
    if (ranges_overlap(evals, n_evals * w, point, n_fixed * w)) return fail(SR_E_INVALID, "mle_fix_variables: d_evals overlaps d_point");
    if (ranges_overlap(out, out_elems * w, work, need * w)) return fail(SR_E_INVALID, "mle_fix_variables: d_out overlaps d_work");
    if (ranges_overlap(evals, n_evals * w, work, need * w)) return fail(SR_E_INVALID, "mle_fix_variables: d_evals overlaps d_work");
    if (ranges_overlap(point, n_fixed * w, work, need * w)) return fail(SR_E_INVALID, "mle_fix_variables: d_point overlaps d_work");
    const Call call(c, stream);
    return dev_mle_fix(c, out, evals, n_evals, num_vars, point, n_fixed, order, work, call.st);
}
int sr_mle_fix_variables(sr_ctx *c, uint64_t *out, const uint64_t *evals, size_t n_evals, size_t num_vars, const uint64_t *point,
                         size_t n_fixed, int order) {
    size_t out_elems = 0, need = 0;
    if (int rc = check_mle(c, out, evals, n_evals, num_vars, point, n_fixed, order, &out_elems, &need)) return rc;
    const Call call(c);
    const size_t w = (size_t)c->degree * c->limbs * 8;
    return staged(c, {{evals, nullptr, n_evals * w}, {point, nullptr, n_fixed * w}, {nullptr, out, out_elems * w}, {nullptr, nullptr, need * w}},
                  [&](void *const *d) {
                      return dev_mle_fix(c, (uint64_t *)d[2], (const uint64_t *)d[0], n_evals, num_vars, (const uint64_t *)d[1], n_fixed, order,
                                         (uint64_t *)d[3], c->stream);
                  });
}
int sr_prod_tree_plan(int ring, int log2_degree, size_t num_vars, int order, size_t *layer_elems, int *launches) {
    if (int rc = check_plan_ring(ring, log2_degree)) return rc;
    if (!layer_elems || !launches) return fail(SR_E_INVALID, "prod_tree_plan: null result pointer");
    if (num_vars >= 48) return fail(SR_E_INVALID, "prod_tree_plan: num_vars must be below 48");
    sr::ptree::Plan p;
    if (!sr::ptree::plan(ring, num_vars, order, &p)) return fail(SR_E_INVALID, "prod_tree_plan: unknown order");
    *layer_elems = p.layer_elems;
    *launches = p.launches;
    return SR_OK;
}
int sr_prod_tree_dev(sr_ctx *c, uint64_t *layers, const uint64_t *leaves, size_t n_leaves, size_t num_vars, int order, void *stream) {
    if (int rc = check_prod_tree(c, layers, leaves, n_leaves, num_vars, order)) return rc;
    const Call call(c, stream);
    return dev_prod_tree(c, layers, leaves, n_leaves, num_vars, order, call.st);
}
int sr_prod_tree(sr_ctx *c, uint64_t *layers, const uint64_t *leaves, size_t n_leaves, size_t num_vars, int order) {
    if (int rc = check_prod_tree(c, layers, leaves, n_leaves, num_vars, order)) return rc;
    const Call call(c);
    const size_t w = (size_t)c->degree * c->limbs * 8;
    return staged(c, {{leaves, nullptr, n_leaves * w}, {nullptr, layers, (((size_t)1 << num_vars) - 1) * w}}, [&](void *const *d) {
        return dev_prod_tree(c, (uint64_t *)d[1], (const uint64_t *)d[0], n_leaves, num_vars, order, c->stream);
    });
}
int sr_frac_tree_plan(int ring, int log2_degree, size_t num_vars, int order, size_t *layer_elems, int *launches) {
    if (int rc = check_plan_ring(ring, log2_degree)) return rc;
    if (!layer_elems || !launches) return fail(SR_E_INVALID, "frac_tree_plan: null result pointer");
    if (num_vars >= 48) return fail(SR_E_INVALID, "frac_tree_plan: num_vars must be below 48");
    sr::ftree::Plan p;
    if (!sr::ftree::plan(ring, num_vars, order, &p)) return fail(SR_E_INVALID, "frac_tree_plan: unknown order");
    *layer_elems = p.layer_elems;
    *launches = p.launches;
    return SR_OK;
}
int sr_frac_tree_dev(sr_ctx *c, uint64_t *p_layers, uint64_t *q_layers, const uint64_t *p_leaves, const uint64_t *q_leaves, size_t n_leaves,
                     size_t num_vars, int order, void *stream) {
    if (int rc = check_frac_tree(c, p_layers, q_layers, p_leaves, q_leaves, n_leaves, num_vars, order)) return rc;
    const Call call(c, stream);
    return dev_frac_tree(c, p_layers, q_layers, p_leaves, q_leaves, n_leaves, num_vars, order, call.st);
}
int sr_frac_tree(sr_ctx *c, uint64_t *p_layers, uint64_t *q_layers, const uint64_t *p_leaves, const uint64_t *q_leaves, size_t n_leaves,
                 size_t num_vars, int order) {
    if (int rc = check_frac_tree(c, p_layers, q_layers, p_leaves, q_leaves, n_leaves, num_vars, order)) return rc;
    const Call call(c);
    const size_t w = (size_t)c->degree * c->limbs * 8, out = (((size_t)1 << num_vars) - 1) * w;
    return staged(c, {{q_leaves, nullptr, n_leaves * w}, {p_leaves, nullptr, p_leaves ? n_leaves * w : 0}, {nullptr, p_layers, out}, {nullptr, q_layers, out}},
                  [&](void *const *d) {
                      return dev_frac_tree(c, (uint64_t *)d[2], (uint64_t *)d[3], p_leaves ? (const uint64_t *)d[1] : nullptr, (const uint64_t *)d[0],
                                           n_leaves, num_vars, order, c->stream);
                  });
}
int sr_lincomb_plan(int ring, int log2_degree, int n_tables, int n_outputs, int *launches, int *outputs_per_launch) {
    return lincomb_plan_entry(kLincomb, ring, log2_degree, n_tables, 0, n_outputs, launches, outputs_per_launch);
}
int sr_lincomb_dev(sr_ctx *c, uint64_t *const *outs, int n_outputs, const uint64_t *const *tables, const size_t *n_evals, int n_tables,
                   const uint64_t *coef, const uint32_t *uses, size_t n, void *stream) {
    return lincomb_dev(kLincomb, c, outs, n_outputs, tables, n_evals, n_tables, nullptr, 0, coef, uses, n, stream);
}
int sr_lincomb(sr_ctx *c, uint64_t *const *outs, int n_outputs, const uint64_t *const *tables, const size_t *n_evals, int n_tables,
               const uint64_t *coef, const uint32_t *uses, size_t n) {
    return lincomb_host(kLincomb, c, outs, n_outputs, tables, n_evals, n_tables, nullptr, 0, coef, uses, n);
}
int sr_lincomb_index_plan(int ring, int log2_degree, int n_tables, int n_index, int n_outputs, int *launches, int *outputs_per_launch) {
    return lincomb_plan_entry(kLincombIndex, ring, log2_degree, n_tables, n_index, n_outputs, launches, outputs_per_launch);
}
int sr_lincomb_index_dev(sr_ctx *c, uint64_t *const *outs, int n_outputs, const uint64_t *const *tables, const size_t *n_evals, int n_tables,
                         const sr_index_column *columns, int n_index, const uint64_t *coef, const uint32_t *uses, size_t n, void *stream) {
    return lincomb_dev(kLincombIndex, c, outs, n_outputs, tables, n_evals, n_tables, columns, n_index, coef, uses, n, stream);
}
int sr_lincomb_index(sr_ctx *c, uint64_t *const *outs, int n_outputs, const uint64_t *const *tables, const size_t *n_evals, int n_tables,
                     const sr_index_column *columns, int n_index, const uint64_t *coef, const uint32_t *uses, size_t n) {
    return lincomb_host(kLincombIndex, c, outs, n_outputs, tables, n_evals, n_tables, columns, n_index, coef, uses, n);
}
int sr_inverse_plan(int ring, int log2_degree, size_t n, int has_num, size_t *work_elems, int *launches, size_t *chunk_elems) {
    if (int rc = check_plan_ring(ring, log2_degree)) return rc;
    if (!work_elems || !launches || !chunk_elems) return fail(SR_E_INVALID, "inverse_plan: null result pointer");
    if (n > (size_t)1 << 46) return fail(SR_E_INVALID, "inverse_plan: element count too large");
    sr::inverse::Plan p;
    if (!sr::inverse::plan(ring, n, has_num != 0, &p)) return fail(SR_E_INVALID, "inverse_plan: no plan for these arguments");
    *work_elems = p.work_elems;
    *launches = p.launches;
    *chunk_elems = p.chunk_elems;
    return SR_OK;
}
int sr_inverse_batch_dev(sr_ctx *c, uint64_t *out, const uint64_t *num, const uint64_t *den, size_t n, uint64_t *work, size_t work_elems,
                         void *stream) {
    if (int rc = check_inverse(c, out, num, den, n)) return rc;
    sr::inverse::Plan p;
    if (!sr::inverse::plan(c->ring, n, num != nullptr, &p)) return fail(SR_E_INVALID, "inverse: no plan for these arguments");
    if (p.work_elems && (!work || work_elems < p.work_elems)) return fail(SR_E_INVALID, "inverse: d_work is smaller than sr_inverse_plan asks for");
    const Call call(c, stream);
    return dev_inverse(c, out, num, den, n, call.st);
}
int sr_inverse_batch(sr_ctx *c, uint64_t *out, const uint64_t *num, const uint64_t *den, size_t n) {
    if (int rc = check_inverse(c, out, num, den, n)) return rc;
    const Call call(c);
    // in place on the staged denominators; a staging chunk is a whole number of elements, and a lane's chunk never crosses it
    return host_pipeline(c, out, den, num, n, [&](uint64_t *s0, uint64_t *s1, size_t m, hipStream_t st) {
        return dev_inverse(c, s0, num ? s1 : nullptr, s0, m, st);
    });
}
int sr_inverse_zero_count(sr_ctx *c, unsigned long long *out, void *stream) {
    if (int rc = check(c, {out})) return rc;
    const Call call(c, stream);
    return read_counter(c, 5, out, call.st);
}
int sr_index_count_dev(sr_ctx *c, uint64_t *counts, const uint64_t *idx, size_t n, size_t n_bins, void *stream) {
    if (int rc = check_index_count(c, counts, idx, n, n_bins)) return rc;
    const Call call(c, stream);
    return dev_index_count(c, counts, idx, n, n_bins, call.st);
}
int sr_index_count(sr_ctx *c, uint64_t *counts, const uint64_t *idx, size_t n, size_t n_bins) {
    if (int rc = check_index_count(c, counts, idx, n, n_bins)) return rc;
    for (size_t i = 0; i < n; i++)
        if (idx[i] >= n_bins) return fail(SR_E_INVALID, "index_count: an index is not below n_bins");
    if (n_bins == 0) return SR_OK;
    const Call call(c);
    return staged(c, {{idx, nullptr, n * 8}, {nullptr, counts, n_bins * 8}},
                  [&](void *const *d) { return dev_index_count(c, (uint64_t *)d[1], (const uint64_t *)d[0], n, n_bins, c->stream); });
}
int sr_mle_round_plan(int ring, int log2_degree, size_t num_vars, int n_tables, int mode, size_t *work_elems, int *launches) {
    return round_plan_entry(kMleRound, ring, log2_degree, num_vars, n_tables, 0, 0, 0, mode, work_elems, launches);
}
int sr_mle_round_evals_dev(sr_ctx *c, uint64_t *out, const uint64_t *const *tables, const size_t *n_evals, int n_tables, size_t num_vars,
                           int mode, uint64_t *work, size_t work_elems, void *stream) {
    RoundCall a{kMleRound, out, tables, n_evals, n_tables, num_vars, mode};
    a.work = work, a.work_elems = work_elems;
    return round_dev(c, a, stream);
}
int sr_mle_round_evals(sr_ctx *c, uint64_t *out, const uint64_t *const *tables, const size_t *n_evals, int n_tables, size_t num_vars, int mode) {
    RoundCall a{kMleRound, out, tables, n_evals, n_tables, num_vars, mode};
    return round_host(c, a);
}
int sr_vpoly_round_plan(int ring, int log2_degree, size_t num_vars, int n_tables, int n_terms, int degree, int mode, size_t *work_elems,
                        int *launches) {
    return round_plan_entry(kVpolyRound, ring, log2_degree, num_vars, n_tables, n_terms, degree, 0, mode, work_elems, launches);
}
int sr_vpoly_round_evals_dev(sr_ctx *c, uint64_t *out, const uint64_t *const *tables, const size_t *n_evals, int n_tables,
                             const sr_vpoly_term *terms, int n_terms, const uint64_t *coef, size_t num_vars, int mode, uint64_t *work,
                             size_t work_elems, void *stream) {
    RoundCall a{kVpolyRound, out, tables, n_evals, n_tables, num_vars, mode};
    a.terms = terms, a.n_terms = n_terms, a.coef = coef;
    a.work = work, a.work_elems = work_elems;
    return round_dev(c, a, stream);
}
int sr_vpoly_round_evals(sr_ctx *c, uint64_t *out, const uint64_t *const *tables, const size_t *n_evals, int n_tables, const sr_vpoly_term *terms,
                         int n_terms, const uint64_t *coef, size_t num_vars, int mode) {
    RoundCall a{kVpolyRound, out, tables, n_evals, n_tables, num_vars, mode};
    a.terms = terms, a.n_terms = n_terms, a.coef = coef;
    return round_host(c, a);
}
int sr_mle_round_fold_plan(int ring, int log2_degree, size_t num_vars, int n_tables, int order, size_t *work_elems, int *launches) {
    return round_plan_entry(kMleRoundFold, ring, log2_degree, num_vars, n_tables, 0, 0, 0, order, work_elems, launches);
}
int sr_mle_round_fold_evals_dev(sr_ctx *c, uint64_t *out, uint64_t *const *out_tables, size_t *n_evals_out, const uint64_t *const *tables,
                                const size_t *n_evals, int n_tables, size_t num_vars, const uint64_t *r, int order, uint64_t *work,
                                size_t work_elems, void *stream) {
    RoundCall a{kMleRoundFold, out, tables, n_evals, n_tables, num_vars, order};
    a.out_tables = out_tables, a.n_evals_out = n_evals_out, a.r = r;
    a.work = work, a.work_elems = work_elems;
    return round_dev(c, a, stream);
}
int sr_mle_round_fold_evals(sr_ctx *c, uint64_t *out, uint64_t *const *out_tables, size_t *n_evals_out, const uint64_t *const *tables,
                            const size_t *n_evals, int n_tables, size_t num_vars, const uint64_t *r, int order) {
    RoundCall a{kMleRoundFold, out, tables, n_evals, n_tables, num_vars, order};
    a.out_tables = out_tables, a.n_evals_out = n_evals_out, a.r = r;
    return round_host(c, a);
}
int sr_vpoly_round_fold_plan(int ring, int log2_degree, size_t num_vars, int n_tables, int n_terms, int degree, int order, size_t *work_elems,
                             int *launches) {
    return round_plan_entry(kVpolyRoundFold, ring, log2_degree, num_vars, n_tables, n_terms, degree, 0, order, work_elems, launches);
}
int sr_vpoly_round_fold_evals_dev(sr_ctx *c, uint64_t *out, uint64_t *const *out_tables, size_t *n_evals_out, const uint64_t *const *tables,
                                  const size_t *n_evals, int n_tables, const sr_vpoly_term *terms, int n_terms, const uint64_t *coef,
                                  size_t num_vars, const uint64_t *r, int order, uint64_t *work, size_t work_elems, void *stream) {
    RoundCall a{kVpolyRoundFold, out, tables, n_evals, n_tables, num_vars, order};
    a.out_tables = out_tables, a.n_evals_out = n_evals_out, a.r = r;
    a.terms = terms, a.n_terms = n_terms, a.coef = coef;
    a.work = work, a.work_elems = work_elems;
    return round_dev(c, a, stream);
}
int sr_vpoly_round_fold_evals(sr_ctx *c, uint64_t *out, uint64_t *const *out_tables, size_t *n_evals_out, const uint64_t *const *tables,
                              const size_t *n_evals, int n_tables, const sr_vpoly_term *terms, int n_terms, const uint64_t *coef, size_t num_vars,
                              const uint64_t *r, int order) {
    RoundCall a{kVpolyRoundFold, out, tables, n_evals, n_tables, num_vars, order};
    a.out_tables = out_tables, a.n_evals_out = n_evals_out, a.r = r;
    a.terms = terms, a.n_terms = n_terms, a.coef = coef;
    return round_host(c, a);
}
int sr_vpoly_wround_plan(int ring, int log2_degree, size_t num_vars, int n_tables, int n_terms, int degree, int order, size_t *work_elems,
                         int *launches) {
    return round_plan_entry(kVpolyWround, ring, log2_degree, num_vars, n_tables, n_terms, degree, 0, order, work_elems, launches);
}
int sr_vpoly_wround_evals_dev(sr_ctx *c, uint64_t *out, const uint64_t *weights, const uint64_t *const *tables, const size_t *n_evals,
                              int n_tables, const sr_vpoly_term *terms, int n_terms, const uint64_t *coef, size_t num_vars, int order,
                              uint64_t *work, size_t work_elems, void *stream) {
    RoundCall a{kVpolyWround, out, tables, n_evals, n_tables, num_vars, order};
    a.weights = weights, a.terms = terms, a.n_terms = n_terms, a.coef = coef;
    a.work = work, a.work_elems = work_elems;
    return round_dev(c, a, stream);
}
int sr_vpoly_wround_evals(sr_ctx *c, uint64_t *out, const uint64_t *weights, const uint64_t *const *tables, const size_t *n_evals, int n_tables,
                          const sr_vpoly_term *terms, int n_terms, const uint64_t *coef, size_t num_vars, int order) {
    RoundCall a{kVpolyWround, out, tables, n_evals, n_tables, num_vars, order};
    a.weights = weights, a.terms = terms, a.n_terms = n_terms, a.coef = coef;
    return round_host(c, a);
}
int sr_vpoly_wround_fold_plan(int ring, int log2_degree, size_t num_vars, int n_tables, int n_terms, int degree, int order, size_t *work_elems,
                              int *launches) {
    return round_plan_entry(kVpolyWroundFold, ring, log2_degree, num_vars, n_tables, n_terms, degree, 0, order, work_elems, launches);
}
int sr_vpoly_wround_fold_evals_dev(sr_ctx *c, uint64_t *out, uint64_t *const *out_tables, size_t *n_evals_out, const uint64_t *weights,
                                   const uint64_t *const *tables, const size_t *n_evals, int n_tables, const sr_vpoly_term *terms, int n_terms,
                                   const uint64_t *coef, size_t num_vars, const uint64_t *r, int order, uint64_t *work, size_t work_elems,
                                   void *stream) {
    RoundCall a{kVpolyWroundFold, out, tables, n_evals, n_tables, num_vars, order};
    a.out_tables = out_tables, a.n_evals_out = n_evals_out, a.r = r;
    a.weights = weights, a.terms = terms, a.n_terms = n_terms, a.coef = coef;
    a.work = work, a.work_elems = work_elems;
    return round_dev(c, a, stream);
}
int sr_vpoly_wround_fold_evals(sr_ctx *c, uint64_t *out, uint64_t *const *out_tables, size_t *n_evals_out, const uint64_t *weights,
                               const uint64_t *const *tables, const size_t *n_evals, int n_tables, const sr_vpoly_term *terms, int n_terms,
                               const uint64_t *coef, size_t num_vars, const uint64_t *r, int order) {
    RoundCall a{kVpolyWroundFold, out, tables, n_evals, n_tables, num_vars, order};
    a.out_tables = out_tables, a.n_evals_out = n_evals_out, a.r = r;
    a.weights = weights, a.terms = terms, a.n_terms = n_terms, a.coef = coef;
    return round_host(c, a);
}
int sr_vpoly_iwround_plan(int ring, int log2_degree, size_t num_vars, int n_tables, int n_index, int n_terms, int degree, int order, int fold,
                          size_t *work_elems, int *launches) {
    if (fold != 0 && fold != 1) return refuse(kVpolyIwround, "fold must be 0 or 1");
    const RoundFamily &f = iwround_family(fold);
    if (int rc = check_iwround_counts(f, n_tables, n_index)) return rc;
    if (n_index == 0)
        return round_plan_entry(fold ? kVpolyWroundFold : kVpolyWround, ring, log2_degree, num_vars, n_tables, n_terms, degree, 0, order, work_elems,
                                launches);
    return round_plan_entry(f, ring, log2_degree, num_vars, n_tables + n_index, n_terms, degree, 0, order, work_elems, launches);
}
int sr_vpoly_iwround_evals_dev(sr_ctx *c, uint64_t *out, const uint64_t *weights, const uint64_t *const *tables, const size_t *n_evals,
                               int n_tables, const sr_index_column *columns, int n_index, const sr_vpoly_term *terms, int n_terms,
                               const uint64_t *coef, size_t num_vars, int order, uint64_t *work, size_t work_elems, void *stream) {
    return iwround_call(false, true, c, out, nullptr, nullptr, weights, tables, n_evals, n_tables, columns, n_index, terms, n_terms, coef, num_vars,
                        nullptr, order, work, work_elems, stream);
}
int sr_vpoly_iwround_evals(sr_ctx *c, uint64_t *out, const uint64_t *weights, const uint64_t *const *tables, const size_t *n_evals, int n_tables,
                           const sr_index_column *columns, int n_index, const sr_vpoly_term *terms, int n_terms, const uint64_t *coef,
                           size_t num_vars, int order) {
    return iwround_call(false, false, c, out, nullptr, nullptr, weights, tables, n_evals, n_tables, columns, n_index, terms, n_terms, coef, num_vars,
                        nullptr, order, nullptr, 0, nullptr);
}
int sr_vpoly_iwround_fold_evals_dev(sr_ctx *c, uint64_t *out, uint64_t *const *out_tables, size_t *n_evals_out, const uint64_t *weights,
                                    const uint64_t *const *tables, const size_t *n_evals, int n_tables, const sr_index_column *columns, int n_index,
                                    const sr_vpoly_term *terms, int n_terms, const uint64_t *coef, size_t num_vars, const uint64_t *r, int order,
                                    uint64_t *work, size_t work_elems, void *stream) {
    return iwround_call(true, true, c, out, out_tables, n_evals_out, weights, tables, n_evals, n_tables, columns, n_index, terms, n_terms, coef,
                        num_vars, r, order, work, work_elems, stream);
}
int sr_vpoly_iwround_fold_evals(sr_ctx *c, uint64_t *out, uint64_t *const *out_tables, size_t *n_evals_out, const uint64_t *weights,
                                const uint64_t *const *tables, const size_t *n_evals, int n_tables, const sr_index_column *columns, int n_index,
                                const sr_vpoly_term *terms, int n_terms, const uint64_t *coef, size_t num_vars, const uint64_t *r, int order) {
    return iwround_call(true, false, c, out, out_tables, n_evals_out, weights, tables, n_evals, n_tables, columns, n_index, terms, n_terms, coef,
                        num_vars, r, order, nullptr, 0, nullptr);
}
int sr_range_wround_plan(int ring, int log2_degree, size_t num_vars, int n_tables, int bound, int order, size_t *work_elems, int *launches) {
    return round_plan_entry(kRangeWround, ring, log2_degree, num_vars, n_tables, 0, 0, bound, order, work_elems, launches);
}
int sr_range_wround_evals_dev(sr_ctx *c, uint64_t *out, const uint64_t *weights, const uint64_t *const *tables, const size_t *n_evals,
                              int n_tables, int bound, const uint64_t *coef, size_t num_vars, int order, uint64_t *work, size_t work_elems,
                              void *stream) {
    RoundCall a{kRangeWround, out, tables, n_evals, n_tables, num_vars, order};
    a.weights = weights, a.bound = bound, a.coef = coef;
    a.work = work, a.work_elems = work_elems;
    return round_dev(c, a, stream);
}
int sr_range_wround_evals(sr_ctx *c, uint64_t *out, const uint64_t *weights, const uint64_t *const *tables, const size_t *n_evals, int n_tables,
                          int bound, const uint64_t *coef, size_t num_vars, int order) {
    RoundCall a{kRangeWround, out, tables, n_evals, n_tables, num_vars, order};
    a.weights = weights, a.bound = bound, a.coef = coef;
    return round_host(c, a);
}
int sr_eq_table_dev(sr_ctx *c, uint64_t *out, const uint64_t *point, size_t n_vars, void *stream) {
    if (int rc = check(c, {out, n_vars ? (const void *)point : (const void *)1})) return rc;
    if (n_vars >= 48) return fail(SR_E_INVALID, "eq_table: n_vars must be below 48");
    if (int rc = check_count(c, (size_t)1 << n_vars)) return rc;
    const size_t w = (size_t)c->degree * c->limbs * 8;
    if (ranges_overlap(out, w << n_vars, point, n_vars * w)) return fail(SR_E_INVALID, "eq_table: d_out overlaps d_point");
    const Call call(c, stream);
    return dev_eq_table(c, out, point, n_vars, call.st);
}
int sr_eq_table(sr_ctx *c, uint64_t *out, const uint64_t *point, size_t n_vars) {
    if (int rc = check(c, {out, n_vars ? (const void *)point : (const void *)1})) return rc;
    if (n_vars >= 48) return fail(SR_E_INVALID, "eq_table: n_vars must be below 48");
    if (int rc = check_count(c, (size_t)1 << n_vars)) return rc;
    const Call call(c);
    const size_t w = (size_t)c->degree * c->limbs * 8;
    return staged(c, {{point, nullptr, n_vars * w}, {nullptr, out, w << n_vars}},
                  [&](void *const *d) { return dev_eq_table(c, (uint64_t *)d[1], (const uint64_t *)d[0], n_vars, c->stream); });
}
int sr_smle_fix_pattern(const uint64_t *idx, size_t nnz, size_t num_vars, size_t n_fixed, uint64_t *out_idx, uint64_t *seg_ptr, size_t *n_out) {
    if (num_vars >= 64) return fail(SR_E_INVALID, "smle: num_vars must be below 64");
    if (n_fixed > num_vars) return fail(SR_E_INVALID, "smle: n_fixed exceeds num_vars");
    if (!n_out || !seg_ptr || (nnz && (!idx || !out_idx))) return fail(SR_E_INVALID, "smle: null buffer");
    const uint64_t limit = (uint64_t)1 << num_vars;
    size_t n = 0;
    for (size_t j = 0; j < nnz; j++) {
        if (idx[j] >= limit) return fail(SR_E_INVALID, "smle: index " + std::to_string(j) + " is not below 2^num_vars");
        if (j && idx[j] <= idx[j - 1]) return fail(SR_E_INVALID, "smle: indices must be strictly ascending (entry " + std::to_string(j) + ")");
        const uint64_t key = idx[j] >> n_fixed;
        if (!n || key != out_idx[n - 1]) {
            out_idx[n] = key;
            seg_ptr[n++] = j;
        }
    }
    seg_ptr[n] = nnz;
    *n_out = n;
    return SR_OK;
}
int sr_smle_plan(int ring, int log2_degree, size_t nnz, size_t n_out, size_t n_fixed, size_t *work_elems, int *launches) {
    if (int rc = check_plan_ring(ring, log2_degree)) return rc;
    if (!work_elems || !launches) return fail(SR_E_INVALID, "smle_plan: null result pointer");
    sr::smle::Plan p;
    if (int rc = smle_plan_for(ring, log2_degree, nnz, n_out, n_fixed, &p)) return rc;
    *work_elems = p.work_elems;
    *launches = p.launches;
    return SR_OK;
}
int sr_smle_fix_variables_dev(sr_ctx *c, uint64_t *out, const uint64_t *vals, const uint64_t *idx, size_t nnz, const uint64_t *seg, size_t n_out,
                              const uint64_t *point, size_t n_fixed, uint64_t *work, size_t work_elems, void *stream) {
    if (!c) return fail(SR_E_INVALID, "null context");
    sr::smle::Plan p;
    if (int rc = smle_plan_for(c->ring, c->k, nnz, n_out, n_fixed, &p)) return rc;
    if (nnz == 0) return SR_OK;
    if (!out || !vals || !idx || !seg || (n_fixed && !point) || (p.work_elems && !work)) return fail(SR_E_INVALID, "smle: null buffer");
    if (int rc = check_count(c, nnz)) return rc;
    if (int rc = check_count(c, p.work_elems)) return rc;
    if (work_elems < p.work_elems)
        return fail(SR_E_INVALID, "smle: workspace too small (sr_smle_plan asks for " + std::to_string(p.work_elems) + " elements)");
    const size_t w = (size_t)c->degree * c->limbs * 8;
    if (ranges_overlap(out, n_out * w, vals, nnz * w)) return fail(SR_E_INVALID, "smle: d_out_vals overlaps d_vals");
    if (ranges_overlap(out, n_out * w, point, n_fixed * w)) return fail(SR_E_INVALID, "smle: d_out_vals overlaps d_point");
    if (ranges_overlap(out, n_out * w, work, p.work_elems * w)) return fail(SR_E_INVALID, "smle: d_out_vals overlaps d_work");
    const Call call(c, stream);
    return dev_smle_fix(c, p, out, vals, idx, nnz, seg, n_out, point, n_fixed, work, call.st);
}
int sr_smle_fix_variables(sr_ctx *c, uint64_t *out_vals, uint64_t *out_idx, size_t *n_out, const uint64_t *vals, const uint64_t *idx, size_t nnz,
                          size_t num_vars, const uint64_t *point, size_t n_fixed) {
    if (!c) return fail(SR_E_INVALID, "null context");
    if (!n_out || (nnz && (!out_vals || !out_idx || !vals || !idx)) || (nnz && n_fixed && !point)) return fail(SR_E_INVALID, "smle: null buffer");
    if (int rc = check_count(c, nnz)) return rc;
    std::vector<uint64_t> meta(2 * nnz + 1);  // [idx | seg_ptr]: one staged operand
    if (int rc = sr_smle_fix_pattern(idx, nnz, num_vars, n_fixed, out_idx, meta.data() + nnz, n_out)) return rc;
    if (nnz == 0) return SR_OK;
    memcpy(meta.data(), idx, nnz * 8);
    sr::smle::Plan p;
    if (int rc = smle_plan_for(c->ring, c->k, nnz, *n_out, n_fixed, &p)) return rc;
    if (int rc = check_count(c, p.work_elems)) return rc;
    const Call call(c);
    const size_t w = (size_t)c->degree * c->limbs * 8, no = *n_out;
    return staged(c, {{vals, nullptr, nnz * w}, {meta.data(), nullptr, (nnz + no + 1) * 8}, {point, nullptr, n_fixed * w}, {nullptr, out_vals, no * w},
                      {nullptr, nullptr, p.work_elems * w}},
                  [&](void *const *d) {
                      const uint64_t *dm = (const uint64_t *)d[1];
                      return dev_smle_fix(c, p, (uint64_t *)d[3], (const uint64_t *)d[0], dm, nnz, dm + nnz, no, (const uint64_t *)d[2], n_fixed,
                                          (uint64_t *)d[4], c->stream);
                  });
}
int sr_norm_plan(int ring, size_t n_coeffs, size_t group, int which, size_t *out_words_per_group, size_t *work_words, int *launches) {
    if (int rc = check_plan_ring(ring, 0)) return rc;  // no degree: the norms count coefficients
    if (!out_words_per_group || !work_words || !launches) return fail(SR_E_INVALID, "norm_plan: null result pointer");
    sr::norms::Plan p;
    if (int rc = check_norm(ring == SR_RING_STARK_POW2 ? 4 : 1, n_coeffs, group, which, &p)) return rc;
    *out_words_per_group = p.words_per_group;
    *work_words = p.work_words;
    *launches = p.launches;
    return SR_OK;
}
int sr_norm_batch_dev(sr_ctx *c, uint64_t *out, const uint64_t *coeffs, size_t n_coeffs, size_t group, int which, uint64_t *work,
                      size_t work_words, void *stream) {
    if (int rc = check(c, {out, n_coeffs ? (const void *)coeffs : (const void *)1})) return rc;
    sr::norms::Plan p;
    if (int rc = check_norm(c->limbs, n_coeffs, group, which, &p)) return rc;
    if (p.work_words && !work) return fail(SR_E_INVALID, "norm: null buffer");
    if (work_words < p.work_words)
        return fail(SR_E_INVALID, "norm: workspace too small (sr_norm_plan asks for " + std::to_string(p.work_words) + " words)");
    const size_t out_bytes = p.n_groups * p.words_per_group * 8;
    if (ranges_overlap(out, out_bytes, coeffs, n_coeffs * c->limbs * 8)) return fail(SR_E_INVALID, "norm: d_out overlaps d_coeffs");
    if (ranges_overlap(out, out_bytes, work, p.work_words * 8)) return fail(SR_E_INVALID, "norm: d_out overlaps d_work");
    if (ranges_overlap(coeffs, n_coeffs * c->limbs * 8, work, p.work_words * 8)) return fail(SR_E_INVALID, "norm: d_coeffs overlaps d_work");
    const Call call(c, stream);
    return dev_norm(c, p, which, out, coeffs, work, call.st);
}
// Host pointers: the slice goes through host_pipeline in chunks of coefficients.  A chunk is [the rest of a group the previous chunk
// began][whole groups][the beginning of a group]: up to three device calls whose records are copied back and combined here.
int sr_norm_batch(sr_ctx *c, uint64_t *out, const uint64_t *coeffs, size_t n_coeffs, size_t group, int which) {
    if (int rc = check(c, {out, n_coeffs ? (const void *)coeffs : (const void *)1})) return rc;
    sr::norms::Plan whole;
    if (int rc = check_norm(c->limbs, n_coeffs, group, which, &whole)) return rc;
    const size_t wpg = whole.words_per_group, limbs = (size_t)c->limbs;
    const int nl = (which & SR_NORM_LINF) ? c->limbs : 0, ns = (int)wpg - nl;
    memset(out, 0, whole.n_groups * wpg * 8);
    if (n_coeffs == 0) return SR_OK;
    const Call call(c);
    // the chunk host_pipeline will use, hence the most records one chunk leaves; one workspace serves the calls of a chunk in turn
    const size_t chunk_mb = c->plan.host_chunk_mb ? c->plan.host_chunk_mb : 128;
    size_t chunk = (chunk_mb << 20) / (limbs * 8);
    if (chunk == 0) chunk = 1;
    const size_t largest = n_coeffs <= 2 * chunk ? n_coeffs : chunk, max_records = largest / group + 2;
    if (int rc = grow(c, HOST_1, max_records * wpg * 8)) return rc;
    if (int rc = grow(c, HOST_3, sr::norms::kMaxParts * wpg * 8)) return rc;
    uint64_t *d_rec = (uint64_t *)c->buf[HOST_1], *d_work = (uint64_t *)c->buf[HOST_3];
    struct Part {  // the records one chunk left: those of piece i belong to the groups g0[i] .. g0[i] + count[i] - 1
        size_t g0[3], count[3];
        int pieces;
        std::vector<uint64_t> words;
    };
    std::vector<Part> parts;
    size_t first = 0;  // of the next chunk: compute() is called once per chunk, in order
    const int rc = host_pipeline(
        c, nullptr, coeffs, nullptr, n_coeffs,
        [&](uint64_t *s0, uint64_t *, size_t n, hipStream_t st) {
            const size_t end = first + n;
            size_t pos = first, records = 0;
            Part pt{};
            auto piece = [&](size_t len, size_t grp) {
                sr::norms::Plan p;
                if (!sr::norms::plan(c->limbs, len, grp, which, &p)) return fail(SR_E_INVALID, "norm: no plan for a chunk");
                if (int r = dev_norm(c, p, which, d_rec + records * wpg, s0 + (pos - first) * limbs, d_work, st)) return r;
                pt.g0[pt.pieces] = pos / group;
                pt.count[pt.pieces++] = p.n_groups;
                records += p.n_groups;
                pos += len;
                return (int)SR_OK;
            };
            if (pos % group) {  // the rest of the group the previous chunk began, or as much of it as this chunk holds
                const size_t rest = group - pos % group, len = rest < end - pos ? rest : end - pos;
                if (int r = piece(len, len)) return r;
            }
            if ((end - pos) / group)
                if (int r = piece((end - pos) / group * group, group)) return r;
            if (pos < end)
                if (int r = piece(end - pos, end - pos)) return r;
            pt.words.resize(records * wpg);
            parts.push_back(std::move(pt));
            HIP_TRY(hipMemcpyAsync(parts.back().words.data(), d_rec, records * wpg * 8, hipMemcpyDeviceToHost, st));
            first = end;
            return (int)SR_OK;
        },
        limbs * 8);
    if (rc) return rc;
    for (const Part &pt : parts) {  // host_pipeline has synchronised the stream: the records are here
        const uint64_t *src = pt.words.data();
        for (int i = 0; i < pt.pieces; i++)
            for (size_t r = 0; r < pt.count[i]; r++, src += wpg) norm_combine_host(out + (pt.g0[i] + r) * wpg, src, nl, ns);
    }
    return SR_OK;
}
int sr_mul_elem_add_batch_dev(sr_ctx *c, uint64_t *acc, const uint64_t *x, const uint64_t *r, size_t batch, void *stream) {
    if (int rc = check(c, {acc, x, r}, batch)) return rc;
    const size_t w = (size_t)c->degree * c->limbs * 8;
    if (batch && (ranges_overlap(r, w, acc, batch * w) || ranges_overlap(r, w, x, batch * w)))
        return fail(SR_E_INVALID, "mul_elem_add: r must not lie inside acc or x");
    if (acc != x && ranges_overlap(acc, batch * w, x, batch * w))
        return fail(SR_E_INVALID, "mul_elem_add: acc and x must be the same buffer or disjoint");
    const Call call(c, stream);
    return dev_mul_elem_add(c, acc, x, r, batch, call.st);
}
int sr_mul_elem_add_batch(sr_ctx *c, uint64_t *acc, const uint64_t *x, const uint64_t *r, size_t batch) {
    if (int rc = check(c, {acc, x, r}, batch)) return rc;
    const Call call(c);
    const size_t w = (size_t)c->degree * c->limbs * 8;
    const bool same = acc == x;
    return staged(c, {{acc, acc, batch * w}, {r, nullptr, w}, {same ? nullptr : x, nullptr, same ? 0 : batch * w}}, [&](void *const *d) {
        return dev_mul_elem_add(c, (uint64_t *)d[0], (const uint64_t *)(same ? d[0] : d[2]), (const uint64_t *)d[1], batch, c->stream);
    });
}
int sr_sum_batch_dev(sr_ctx *c, uint64_t *out, const uint64_t *in, size_t n, void *stream) {
    if (int rc = check_fold(c, out, in, n)) return rc;
    const Call call(c, stream);
    return dev_sum(c, out, in, n, call.st);
}
int sr_product_batch_dev(sr_ctx *c, uint64_t *out, const uint64_t *in, size_t n, void *stream) {
    if (int rc = check_fold(c, out, in, n)) return rc;
    const Call call(c, stream);
    return dev_product(c, out, in, n, call.st);
}
int sr_add_batch_dev(sr_ctx *c, uint64_t *l, const uint64_t *r, size_t batch, void *stream) {
    if (int rc = check(c, {l, r}, batch)) return rc;
    const Call call(c, stream);
    return dev_addsub(c, l, r, batch, false, call.st);
}
int sr_sub_batch_dev(sr_ctx *c, uint64_t *l, const uint64_t *r, size_t batch, void *stream) {
    if (int rc = check(c, {l, r}, batch)) return rc;
    const Call call(c, stream);
    return dev_addsub(c, l, r, batch, true, call.st);
}
int sr_neg_batch_dev(sr_ctx *c, uint64_t *d, size_t batch, void *stream) {
    if (int rc = check(c, {d}, batch)) return rc;
    const Call call(c, stream);
    return dev_neg(c, d, batch, call.st);
}
int sr_scale_batch_dev(sr_ctx *c, uint64_t *d, const uint64_t *scalar, size_t batch, void *stream) {
    if (int rc = check(c, {d, scalar}, batch)) return rc;
    const Call call(c, stream);
    return dev_scale(c, d, scalar, batch, call.st);
}
int sr_add_scalar_batch_dev(sr_ctx *c, uint64_t *d, const uint64_t *scalar, int ntt_form, size_t batch, void *stream) {
    if (int rc = check(c, {d, scalar}, batch)) return rc;
    const Call call(c, stream);
    return dev_add_scalar(c, d, scalar, ntt_form != 0, batch, call.st);
}
int sr_matvec_ntt_dev(sr_ctx *c, uint64_t *y, const uint64_t *m, const uint64_t *v, size_t nrows, size_t ncols, void *stream) {
    if (int rc = check(c, {y, m, v}, nrows, ncols)) return rc;
    if (y == m || y == v) return fail(SR_E_INVALID, "matvec: y must not alias M or v");
    const Call call(c, stream);
    return dev_matvec(c, y, m, v, nrows, ncols, call.st);
}
int sr_spmv_ntt_dev(sr_ctx *c, uint64_t *y, const uint64_t *vals, const uint32_t *cols, const uint64_t *row_ptr, const uint64_t *v,
                    size_t nrows, size_t ncols, void *stream) {
    if (int rc = check(c, {y, row_ptr, v}, nrows)) return rc;
    if (int rc = check_count(c, ncols)) return rc;   // the dense product nrows * ncols is irrelevant here
    if (y == v || y == vals) return fail(SR_E_INVALID, "spmv: y must not alias the matrix or v");
    const Call call(c, stream);
    return dev_spmv(c, y, vals, cols, row_ptr, v, nrows, ncols, call.st);
}
int sr_spmv_bad_index_count(sr_ctx *c, unsigned long long *out, void *stream) {
    if (int rc = check(c, {out})) return rc;
    const Call call(c, stream);
    return read_counter(c, 1, out, call.st);
}
int sr_matmul_ntt_dev(sr_ctx *c, uint64_t *y, const uint64_t *a, const uint64_t *b, size_t n, size_t m, size_t p, void *stream) {
    if (int rc = check(c, {y, a, b}, n, m)) return rc;
    if (check_count(c, m, p) || check_count(c, n, p)) return SR_E_INVALID;
    if (y == a || y == b) return fail(SR_E_INVALID, "matmul: y must not alias A or B");
    const Call call(c, stream);
    return dev_matmul(c, y, a, b, n, m, p, call.st);
}

int sr_rot_batch_dev(sr_ctx *c, uint64_t *out, const uint64_t *in, size_t batch, void *stream) {
    if (int rc = check(c, {out, in}, batch)) return rc;
    if (out == in) return fail(SR_E_INVALID, "rot: out must not alias in");
    const Call call(c, stream);
    return dev_rot(c, out, in, batch, call.st);
}
int sr_rot_batch(sr_ctx *c, uint64_t *data, size_t batch) {
    if (int rc = check(c, {data}, batch)) return rc;
    const Call call(c);
    const size_t bytes = batch * c->degree * c->limbs * 8;
    if (bytes == 0) return SR_OK;
    return staged(c, {{data, nullptr, bytes}, {nullptr, data, bytes}}, [&](void *const *d) {
        return dev_rot(c, (uint64_t *)d[1], (const uint64_t *)d[0], batch, c->stream);
    });
}
size_t sr_wire_coeff_bytes(const sr_ctx *c) { return c ? wire_coeff_bytes(c) : 0; }
int sr_serialize_batch_dev(sr_ctx *c, uint8_t *wire, const uint64_t *in, const uint64_t *offsets, size_t batch, void *stream) {
    if (int rc = check(c, {wire, in}, batch)) return rc;
    if ((const void *)wire == (const void *)in) return fail(SR_E_INVALID, "serialize: wire must not alias in");
    const Call call(c, stream);
    return dev_wire(c, true, wire, in, offsets, batch, call.st);
}
int sr_deserialize_batch_dev(sr_ctx *c, uint64_t *out, const uint8_t *wire, const uint64_t *offsets, size_t batch, void *stream) {
    if (int rc = check(c, {out, wire}, batch)) return rc;
    if ((const void *)wire == (const void *)out) return fail(SR_E_INVALID, "deserialize: out must not alias wire");
    const Call call(c, stream);
    return dev_wire(c, false, out, wire, offsets, batch, call.st);
}
int sr_wire_invalid_count(sr_ctx *c, unsigned long long *out, void *stream) {
    if (int rc = check(c, {out})) return rc;
    const Call call(c, stream);
    return read_counter(c, 3, out, call.st);
}
int sr_decompose_balanced_batch_wide_dev(sr_ctx *c, uint64_t *out, const uint64_t *in, uint64_t basis_lo, uint64_t basis_hi,
                                         size_t padding_size, size_t batch, void *stream) {
    if (int rc = check(c, {out, in}, batch, padding_size)) return rc;
    if (int rc = check_basis_wide(basis_lo, basis_hi)) return rc;
    if (out == in) return fail(SR_E_INVALID, "decompose: out must not alias in");
    const Call call(c, stream);
    return dev_decompose_any(c, out, in, basis_lo, basis_hi, padding_size, batch, call.st);
}
int sr_decompose_balanced_batch_dev(sr_ctx *c, uint64_t *out, const uint64_t *in, uint64_t basis, size_t padding_size, size_t batch,
                                    void *stream) {
    return sr_decompose_balanced_batch_wide_dev(c, out, in, basis, 0, padding_size, batch, stream);
}
int sr_decompose_overflow_count(sr_ctx *c, unsigned long long *out, void *stream) {
    if (int rc = check(c, {out})) return rc;
    const Call call(c, stream);
    return read_counter(c, 2, out, call.st);
}
int sr_recompose_batch_wide_dev(sr_ctx *c, uint64_t *out, const uint64_t *in, uint64_t basis_lo, uint64_t basis_hi, size_t padding_size,
                                size_t batch_out, void *stream) {
    if (int rc = check(c, {out, in}, batch_out, padding_size)) return rc;
    if (out == in) return fail(SR_E_INVALID, "recompose: out must not alias in");
    const Call call(c, stream);
    return dev_recompose_any(c, out, in, basis_lo, basis_hi, padding_size, batch_out, call.st);
}
int sr_recompose_batch_dev(sr_ctx *c, uint64_t *out, const uint64_t *in, uint64_t basis, size_t padding_size, size_t batch_out,
                           void *stream) {
    return sr_recompose_batch_wide_dev(c, out, in, basis, 0, padding_size, batch_out, stream);
}

// ---- host-pointer variants of the linear-algebra entry points (convenience entry points for callers that hold Vec<..> on the
// host; resident data uses the _dev forms)
int sr_matmul_ntt(sr_ctx *c, uint64_t *y, const uint64_t *a, const uint64_t *b, size_t n, size_t m, size_t p) {
    if (int rc = check(c, {y, a, b}, n, m)) return rc;
    if (check_count(c, m, p) || check_count(c, n, p)) return SR_E_INVALID;
    const Call call(c);
    const size_t w = c->degree * c->limbs * 8;
    return staged(c, {{a, nullptr, n * m * w}, {b, nullptr, m * p * w}, {nullptr, y, n * p * w}}, [&](void *const *d) {
        return dev_matmul(c, (uint64_t *)d[2], (const uint64_t *)d[0], (const uint64_t *)d[1], n, m, p, c->stream);
    });
}
int sr_matvec_ntt(sr_ctx *c, uint64_t *y, const uint64_t *m, const uint64_t *v, size_t nrows, size_t ncols) {
    if (int rc = check(c, {y, m, v}, nrows, ncols)) return rc;
    const Call call(c);
    const size_t w = c->degree * c->limbs * 8;
    return staged(c, {{m, nullptr, nrows * ncols * w}, {v, nullptr, ncols * w}, {nullptr, y, nrows * w}}, [&](void *const *d) {
        return dev_matvec(c, (uint64_t *)d[2], (const uint64_t *)d[0], (const uint64_t *)d[1], nrows, ncols, c->stream);
    });
}
int sr_spmv_ntt(sr_ctx *c, uint64_t *y, const uint64_t *vals, const uint32_t *cols, const uint64_t *row_ptr, const uint64_t *v,
                size_t nrows, size_t ncols) {
    if (int rc = check(c, {y, row_ptr, v}, nrows)) return rc;
    if (int rc = check_count(c, ncols)) return rc;
    const size_t nnz = (size_t)row_ptr[nrows];
    if (nnz && (!vals || !cols)) return fail(SR_E_INVALID, "null buffer");
    for (size_t r = 0; r < nrows; r++)
        if (row_ptr[r] > row_ptr[r + 1]) return fail(SR_E_INVALID, "spmv: row_ptr is not monotone");
    for (size_t j = 0; j < nnz; j++)  // the reference indexes v[col] and panics when out of range (sparse_matrix.rs:208)
        if (cols[j] >= ncols) return fail(SR_E_INVALID, "spmv: column index out of range");
    const Call call(c);
    const size_t w = c->degree * c->limbs * 8;
    const Staged ops[] = {{vals, nullptr, nnz * w}, {cols, nullptr, nnz * 4}, {row_ptr, nullptr, (nrows + 1) * 8}, {v, nullptr, ncols * w},
                          {nullptr, y, nrows * w}};
    return staged(c, ops, [&](void *const *d) {
        return dev_spmv(c, (uint64_t *)d[4], (const uint64_t *)d[0], (const uint32_t *)d[1], (const uint64_t *)d[2], (const uint64_t *)d[3],
                        nrows, ncols, c->stream);
    });
}
int sr_gram_plan(int ring, int log2_degree, size_t n, size_t m, size_t *work_elems, int *launches) {
    if (int rc = check_plan_ring(ring, log2_degree)) return rc;
    if (!work_elems || !launches) return fail(SR_E_INVALID, "gram_plan: null result pointer");
    sr::symm::GramPlan p;
    if (int rc = gram_plan_for(ring, log2_degree, n, m, &p)) return rc;
    *work_elems = p.work_elems;
    *launches = p.launches;
    return SR_OK;
}
int sr_gram_ntt_dev(sr_ctx *c, uint64_t *out, const uint64_t *a, size_t n, size_t m, uint64_t *work, size_t work_elems, void *stream) {
    sr::symm::GramPlan p;
    if (int rc = check_gram(c, out, a, n, m, &p)) return rc;
    if (n == 0) return SR_OK;
    if (p.work_elems && !work) return fail(SR_E_INVALID, "gram: null buffer");
    if (work_elems < p.work_elems)
        return fail(SR_E_INVALID, "gram: workspace too small (sr_gram_plan asks for " + std::to_string(p.work_elems) + " elements)");
    const size_t w = (size_t)c->degree * c->limbs * 8;
    if (ranges_overlap(out, p.packed * w, a, n * m * w)) return fail(SR_E_INVALID, "gram: d_out overlaps d_a");
    if (ranges_overlap(out, p.packed * w, work, p.work_elems * w)) return fail(SR_E_INVALID, "gram: d_out overlaps d_work");
    if (ranges_overlap(a, n * m * w, work, p.work_elems * w)) return fail(SR_E_INVALID, "gram: d_a overlaps d_work");
    const Call call(c, stream);
    return dev_gram(c, p, out, a, n, m, work, call.st);
}
int sr_gram_ntt(sr_ctx *c, uint64_t *out, const uint64_t *a, size_t n, size_t m) {
    sr::symm::GramPlan p;
    if (int rc = check_gram(c, out, a, n, m, &p)) return rc;
    if (n == 0) return SR_OK;
    const Call call(c);
    const size_t w = (size_t)c->degree * c->limbs * 8;
    return staged(c, {{a, nullptr, n * m * w}, {nullptr, out, p.packed * w}, {nullptr, nullptr, p.work_elems * w}}, [&](void *const *d) {
        return dev_gram(c, p, (uint64_t *)d[1], (const uint64_t *)d[0], n, m, (uint64_t *)d[2], c->stream);
    });
}
int sr_symm_recompose_plan(int ring, int log2_degree, size_t n, size_t d, size_t *work_elems, int *launches) {
    if (int rc = check_plan_ring(ring, log2_degree)) return rc;
    if (!work_elems || !launches) return fail(SR_E_INVALID, "symm_recompose_plan: null result pointer");
    sr::symm::RecomposePlan p;
    if (int rc = recompose_plan_for(ring, log2_degree, n, d, &p)) return rc;
    *work_elems = p.work_elems;
    *launches = p.launches;
    return SR_OK;
}
int sr_symm_recompose_dev(sr_ctx *c, uint64_t *out, const uint64_t *mat, size_t n, size_t d, const uint64_t *powers, uint64_t *work,
                          size_t work_elems, void *stream) {
    sr::symm::RecomposePlan p;
    if (int rc = check_symm_recompose(c, out, mat, n, d, powers, &p)) return rc;
    if (n == 0) return SR_OK;
    if (!work) return fail(SR_E_INVALID, "symm_recompose: null buffer");
    if (work_elems < p.work_elems)
        return fail(SR_E_INVALID, "symm_recompose: workspace too small (sr_symm_recompose_plan asks for " + std::to_string(p.work_elems) + " elements)");
    const size_t w = (size_t)c->degree * c->limbs * 8;
    if (ranges_overlap(out, p.packed_out * w, mat, p.packed_in * w)) return fail(SR_E_INVALID, "symm_recompose: d_out overlaps d_mat");
    if (ranges_overlap(out, p.packed_out * w, powers, d * w)) return fail(SR_E_INVALID, "symm_recompose: d_out overlaps d_powers");
    if (ranges_overlap(out, p.packed_out * w, work, p.work_elems * w)) return fail(SR_E_INVALID, "symm_recompose: d_out overlaps d_work");
    if (ranges_overlap(mat, p.packed_in * w, work, p.work_elems * w)) return fail(SR_E_INVALID, "symm_recompose: d_mat overlaps d_work");
    if (ranges_overlap(powers, d * w, work, p.work_elems * w)) return fail(SR_E_INVALID, "symm_recompose: d_powers overlaps d_work");
    const Call call(c, stream);
    return dev_symm_recompose(c, p, out, mat, powers, n, d, work, call.st);
}
int sr_symm_recompose(sr_ctx *c, uint64_t *out, const uint64_t *mat, size_t n, size_t d, const uint64_t *powers) {
    sr::symm::RecomposePlan p;
    if (int rc = check_symm_recompose(c, out, mat, n, d, powers, &p)) return rc;
    if (n == 0) return SR_OK;
    const Call call(c);
    const size_t w = (size_t)c->degree * c->limbs * 8;
    return staged(c, {{mat, nullptr, p.packed_in * w}, {powers, nullptr, d * w}, {nullptr, out, p.packed_out * w}, {nullptr, nullptr, p.work_elems * w}},
                  [&](void *const *dv) {
                      return dev_symm_recompose(c, p, (uint64_t *)dv[2], (const uint64_t *)dv[0], (const uint64_t *)dv[1], n, d, (uint64_t *)dv[3],
                                                c->stream);
                  });
}
// ---- sparse matrices: transpose and sparse x sparse product (csrc/sparse_matrix.hpp) ---------------------------------------------------
int sr_sparse_transpose_pattern(const uint32_t *cols, const uint64_t *row_ptr, size_t nrows, size_t ncols, uint64_t *t_row_ptr, uint32_t *t_cols,
                                uint32_t *perm) {
    if (const char *e = sr::spm::transpose_pattern(cols, row_ptr, nrows, ncols, t_row_ptr, t_cols, perm))
        return fail(SR_E_INVALID, std::string("sparse_transpose_pattern: ") + e);
    return SR_OK;
}
int sr_spgemm_pattern(const uint32_t *a_cols, const uint64_t *a_row_ptr, size_t n, size_t m, const uint32_t *b_cols, const uint64_t *b_row_ptr,
                      size_t p, uint64_t *out_row_ptr, uint32_t *out_cols, uint64_t *pair_ptr, uint32_t *pair_a, uint32_t *pair_b, size_t *n_out,
                      size_t *n_pairs) {
    const bool fill = out_row_ptr || out_cols || pair_ptr || pair_a || pair_b;
    try {
        if (const char *e = sr::spm::spgemm_pattern(a_cols, a_row_ptr, n, m, b_cols, b_row_ptr, p, fill, out_row_ptr, out_cols, pair_ptr, pair_a,
                                                    pair_b, n_out, n_pairs))
            return fail(SR_E_INVALID, std::string("spgemm_pattern: ") + e);
    } catch (const std::exception &) {
        return fail(SR_E_ALLOC, "spgemm_pattern: out of host memory");
    }
    return SR_OK;
}
int sr_spgemm_plan(int ring, int log2_degree, size_t n_out, size_t n_pairs, size_t *work_elems, int *launches) {
    if (int rc = check_plan_ring(ring, log2_degree)) return rc;
    if (!work_elems || !launches) return fail(SR_E_INVALID, "spgemm_plan: null result pointer");
    if (!sr::spm::spgemm_plan(ring, is_pow2_ring(ring) ? log2_degree : 0, n_out, n_pairs, work_elems, launches))
        return fail(SR_E_INVALID, "spgemm: the grid exceeds one launch");
    return SR_OK;
}
int sr_gather_batch_dev(sr_ctx *c, uint64_t *out, const uint64_t *in, const uint32_t *perm, size_t n_out, size_t n_in, void *stream) {
    if (int rc = check(c, {}, n_out)) return rc;
    if (int rc = check_count(c, n_in)) return rc;
    if (n_out == 0) return SR_OK;
    if (!out || !perm || (n_in && !in)) return fail(SR_E_INVALID, "gather: null buffer");
    const size_t w = (size_t)c->degree * c->limbs * 8;
    if (ranges_overlap(out, n_out * w, in, n_in * w)) return fail(SR_E_INVALID, "gather: d_out overlaps d_in");
    if (ranges_overlap(out, n_out * w, perm, n_out * 4)) return fail(SR_E_INVALID, "gather: d_out overlaps d_perm");
    const Call call(c, stream);
    return dev_move(c, out, in, perm, n_out, n_in, 0, 0, call.st);
}
int sr_transpose_dev(sr_ctx *c, uint64_t *out, const uint64_t *in, size_t nrows, size_t ncols, void *stream) {
    if (int rc = check(c, {}, nrows, ncols)) return rc;
    if (nrows == 0 || ncols == 0) return SR_OK;
    if (!out || !in) return fail(SR_E_INVALID, "transpose: null buffer");
    const size_t bytes = nrows * ncols * c->degree * c->limbs * 8;
    if (ranges_overlap(out, bytes, in, bytes)) return fail(SR_E_INVALID, "transpose: d_out overlaps d_in");
    const Call call(c, stream);
    return dev_move(c, out, in, nullptr, nrows * ncols, nrows * ncols, nrows, ncols, call.st);
}
int sr_spgemm_ntt_dev(sr_ctx *c, uint64_t *out, uint32_t *live, const uint64_t *a, size_t nnz_a, const uint64_t *b, size_t nnz_b,
                      const uint64_t *pair_ptr, const uint32_t *pair_a, const uint32_t *pair_b, size_t n_out, size_t n_pairs, uint64_t *work,
                      size_t work_elems, void *stream) {
    if (int rc = check_spgemm(c, nnz_a, nnz_b, n_out, n_pairs)) return rc;
    (void)work_elems;  // sr_spgemm_plan asks for none
    if (n_out == 0) return SR_OK;
    if (!out || !live || !pair_ptr || (n_pairs && (!pair_a || !pair_b)) || (nnz_a && !a) || (nnz_b && !b)) return fail(SR_E_INVALID, "spgemm: null buffer");
    const size_t w = (size_t)c->degree * c->limbs * 8;
    const struct {
        const void *p;
        size_t bytes;
        const char *name;
    } in[] = {{a, nnz_a * w, "d_a_vals"},       {b, nnz_b * w, "d_b_vals"},       {pair_ptr, (n_out + 1) * 8, "d_pair_ptr"},
              {pair_a, n_pairs * 4, "d_pair_a"}, {pair_b, n_pairs * 4, "d_pair_b"}, {work, work_elems * w, "d_work"}};
    for (const auto &r : in) {
        if (ranges_overlap(out, n_out * w, r.p, r.bytes)) return fail(SR_E_INVALID, std::string("spgemm: d_out_vals overlaps ") + r.name);
        if (ranges_overlap(live, n_out * 4, r.p, r.bytes)) return fail(SR_E_INVALID, std::string("spgemm: d_live overlaps ") + r.name);
    }
    if (ranges_overlap(out, n_out * w, live, n_out * 4)) return fail(SR_E_INVALID, "spgemm: d_out_vals overlaps d_live");
    const Call call(c, stream);
    return dev_spgemm(c, {out, live, a, b, nnz_a, nnz_b, pair_ptr, pair_a, pair_b, n_out, n_pairs, c->d_counter + 4}, call.st);
}
int sr_spgemm_dead_count(sr_ctx *c, unsigned long long *out, void *stream) {
    if (int rc = check(c, {out})) return rc;
    const Call call(c, stream);
    return read_counter(c, 4, out, call.st);
}
int sr_sparse_transpose(sr_ctx *c, uint64_t *t_vals, uint32_t *t_cols, uint64_t *t_row_ptr, const uint64_t *vals, const uint32_t *cols,
                        const uint64_t *row_ptr, size_t nrows, size_t ncols) {
    if (!c) return fail(SR_E_INVALID, "null context");
    if (!row_ptr) return fail(SR_E_INVALID, "sparse_transpose: null buffer");
    std::vector<uint32_t> perm;
    try {
        perm.resize(row_ptr[nrows] <= 0xFFFFFFFFull ? (size_t)row_ptr[nrows] : 0);
    } catch (const std::exception &) {
        return fail(SR_E_ALLOC, "sparse_transpose: out of host memory");
    }
    if (int rc = sr_sparse_transpose_pattern(cols, row_ptr, nrows, ncols, t_row_ptr, t_cols, perm.data())) return rc;
    const size_t nnz = perm.size();
    if (int rc = check_count(c, nnz)) return rc;
    if (nnz == 0) return SR_OK;
    if (!vals || !t_vals) return fail(SR_E_INVALID, "sparse_transpose: null buffer");
    const Call call(c);
    const size_t w = (size_t)c->degree * c->limbs * 8;
    return staged(c, {{vals, nullptr, nnz * w}, {perm.data(), nullptr, nnz * 4}, {nullptr, t_vals, nnz * w}}, [&](void *const *d) {
        return dev_move(c, (uint64_t *)d[2], (const uint64_t *)d[0], (const uint32_t *)d[1], nnz, nnz, 0, 0, c->stream);
    });
}
int sr_transpose(sr_ctx *c, uint64_t *out, const uint64_t *in, size_t nrows, size_t ncols) {
    if (int rc = check(c, {}, nrows, ncols)) return rc;
    if (nrows == 0 || ncols == 0) return SR_OK;
    if (!out || !in) return fail(SR_E_INVALID, "transpose: null buffer");
    const Call call(c);
    const size_t bytes = nrows * ncols * c->degree * c->limbs * 8;
    return staged(c, {{in, nullptr, bytes}, {nullptr, out, bytes}}, [&](void *const *d) {
        return dev_move(c, (uint64_t *)d[1], (const uint64_t *)d[0], nullptr, nrows * ncols, nrows * ncols, nrows, ncols, c->stream);
    });
}
int sr_spgemm_ntt(sr_ctx *c, uint64_t *out_vals, uint32_t *out_cols, uint64_t *out_row_ptr, size_t *nnz_out, const uint64_t *a_vals,
                  const uint32_t *a_cols, const uint64_t *a_row_ptr, size_t n, size_t m, const uint64_t *b_vals, const uint32_t *b_cols,
                  const uint64_t *b_row_ptr, size_t p) {
    if (!c) return fail(SR_E_INVALID, "null context");
    if (!out_row_ptr || !nnz_out) return fail(SR_E_INVALID, "spgemm: null buffer");
    size_t n_out = 0, n_pairs = 0;
    if (int rc = sr_spgemm_pattern(a_cols, a_row_ptr, n, m, b_cols, b_row_ptr, p, nullptr, nullptr, nullptr, nullptr, nullptr, &n_out, &n_pairs)) return rc;
    *nnz_out = 0;
    if (n_out == 0) {
        for (size_t i = 0; i <= n; i++) out_row_ptr[i] = 0;
        return SR_OK;
    }
    const size_t nnz_a = (size_t)a_row_ptr[n], nnz_b = (size_t)b_row_ptr[m];
    if (!out_vals || !out_cols || !a_vals || !b_vals) return fail(SR_E_INVALID, "spgemm: null buffer");
    if (int rc = check_spgemm(c, nnz_a, nnz_b, n_out, n_pairs)) return rc;
    // one index block [pair_ptr | pair_a | pair_b] so that the five HOST_* slots suffice
    std::vector<uint64_t> idx, row_ptr;
    std::vector<uint32_t> cols, live;
    try {
        idx.resize(n_out + 1 + n_pairs);  // two 32-bit positions per pair: one 64-bit word
        row_ptr.resize(n + 1);
        cols.resize(n_out);
        live.resize(n_out);
    } catch (const std::exception &) {
        return fail(SR_E_ALLOC, "spgemm: out of host memory");
    }
    uint32_t *pa = reinterpret_cast<uint32_t *>(idx.data() + n_out + 1), *pb = pa + n_pairs;
    if (int rc = sr_spgemm_pattern(a_cols, a_row_ptr, n, m, b_cols, b_row_ptr, p, row_ptr.data(), cols.data(), idx.data(), pa, pb, &n_out, &n_pairs))
        return rc;
    const size_t w = (size_t)c->degree * c->limbs * 8;
    {
        const Call call(c);
        const Staged ops[] = {{a_vals, nullptr, nnz_a * w}, {b_vals, nullptr, nnz_b * w}, {idx.data(), nullptr, idx.size() * 8}, {nullptr, out_vals, n_out * w},
                              {nullptr, live.data(), n_out * 4}};
        if (int rc = staged(c, ops, [&](void *const *d) {
                const uint64_t *di = (const uint64_t *)d[2];
                const uint32_t *dpa = reinterpret_cast<const uint32_t *>(di + n_out + 1);
                return dev_spgemm(c, {(uint64_t *)d[3], (uint32_t *)d[4], (const uint64_t *)d[0], (const uint64_t *)d[1], nnz_a, nnz_b, di, dpa, dpa + n_pairs,
                                      n_out, n_pairs, nullptr}, c->stream);
            }))
            return rc;
    }
    // the reference's matrix: the entries none of whose products was non-zero are dropped, in place (kept <= e throughout)
    const size_t words = (size_t)c->degree * c->limbs;
    size_t kept = 0, e = 0;
    out_row_ptr[0] = 0;
    for (size_t i = 0; i < n; i++) {
        for (; e < row_ptr[i + 1]; e++) {
            if (!live[e]) continue;
            if (kept != e) std::memmove(out_vals + kept * words, out_vals + e * words, words * 8);
            out_cols[kept++] = cols[e];
        }
        out_row_ptr[i + 1] = kept;
    }
    *nnz_out = kept;
    return SR_OK;
}
int sr_sum_batch(sr_ctx *c, uint64_t *out, const uint64_t *in, size_t n) { return host_fold(c, out, in, n, false); }
int sr_product_batch(sr_ctx *c, uint64_t *out, const uint64_t *in, size_t n) { return host_fold(c, out, in, n, true); }
int sr_decompose_balanced_batch(sr_ctx *c, uint64_t *out, const uint64_t *in, uint64_t basis, size_t padding_size, size_t batch) {
    return sr_decompose_balanced_batch_wide(c, out, in, basis, 0, padding_size, batch);
}
int sr_decompose_balanced_batch_wide(sr_ctx *c, uint64_t *out, const uint64_t *in, uint64_t basis, uint64_t basis_hi, size_t padding_size,
                                     size_t batch) {
    if (int rc = check(c, {out, in}, batch, padding_size)) return rc;
    if (int rc = check_basis_wide(basis, basis_hi)) return rc;
    const Call call(c);
    const size_t w = c->degree * c->limbs * 8;
    if (batch == 0 || padding_size == 0) return SR_OK;
    int rc = staged(c, {{in, nullptr, batch * w}, {nullptr, out, batch * padding_size * w}}, [&](void *const *d) {
        HIP_TRY(hipMemsetAsync(c->d_counter + 2, 0, sizeof(unsigned long long), c->stream));
        return dev_decompose_any(c, (uint64_t *)d[1], (const uint64_t *)d[0], basis, basis_hi, padding_size, batch, c->stream);
    });
    unsigned long long over = 0;
    if (rc == SR_OK) rc = read_counter(c, 2, &over, c->stream);
    if (rc) return rc;
    // the digits are written; the reference indexes out[padding_size] and panics (mod.rs:81-91)
    if (over) return fail(SR_E_INVALID, "decompose: a coefficient needs more than padding_size digits");
    return SR_OK;
}
int sr_serialize_batch(sr_ctx *c, uint8_t *wire, const uint64_t *in, size_t batch) {
    if (int rc = check(c, {wire, in}, batch)) return rc;
    const Call call(c);
    const size_t n = batch * c->degree;
    if (n == 0) return SR_OK;
    return staged(c, {{in, nullptr, n * c->limbs * 8}, {nullptr, wire, n * wire_coeff_bytes(c)}}, [&](void *const *d) {
        return dev_wire(c, true, d[1], d[0], nullptr, batch, c->stream);
    });
}
int sr_deserialize_batch(sr_ctx *c, uint64_t *out, const uint8_t *wire, size_t batch) {
    if (int rc = check(c, {out, wire}, batch)) return rc;
    const Call call(c);
    const size_t n = batch * c->degree;
    if (n == 0) return SR_OK;
    return staged(c, {{nullptr, out, n * c->limbs * 8}, {wire, nullptr, n * wire_coeff_bytes(c)}}, [&](void *const *d) -> int {
        HIP_TRY(hipMemsetAsync(c->d_counter + 3, 0, sizeof(unsigned long long), c->stream));
        if (int rc = dev_wire(c, false, d[0], d[1], nullptr, batch, c->stream)) return rc;
        unsigned long long bad = 0;
        if (int rc = read_counter(c, 3, &bad, c->stream)) return rc;
        // Fp::deserialize_with_flags: from_bigint(..) is None for an integer >= p -> SerializationError::InvalidData (out not written)
        if (bad) return fail(SR_E_INVALID, "deserialize: a coefficient is not below the modulus (InvalidData)");
        return SR_OK;
    });
}
int sr_recompose_batch(sr_ctx *c, uint64_t *out, const uint64_t *in, uint64_t basis, size_t padding_size, size_t batch_out) {
    return sr_recompose_batch_wide(c, out, in, basis, 0, padding_size, batch_out);
}
int sr_recompose_batch_wide(sr_ctx *c, uint64_t *out, const uint64_t *in, uint64_t basis, uint64_t basis_hi, size_t padding_size,
                            size_t batch_out) {
    if (int rc = check(c, {out, in}, batch_out, padding_size)) return rc;
    const Call call(c);
    const size_t w = c->degree * c->limbs * 8;
    if (batch_out == 0) return SR_OK;
    return staged(c, {{in, nullptr, batch_out * padding_size * w}, {nullptr, out, batch_out * w}}, [&](void *const *d) {
        return dev_recompose_any(c, (uint64_t *)d[1], (const uint64_t *)d[0], basis, basis_hi, padding_size, batch_out, c->stream);
    });
}
int sr_ring_mul_batch_dev(sr_ctx *c, uint64_t *out, const uint64_t *a, const uint64_t *b, size_t batch, void *stream) {
    if (int rc = check(c, {out, a, b}, batch)) return rc;
    if (b == out) return fail(SR_E_INVALID, "ring_mul: b must not alias out");
    const Call call(c, stream);
    return dev_ring_mul(c, out, a, b, batch, call.st);
}
int sr_ring_mul_ntt_rhs_batch_dev(sr_ctx *c, uint64_t *out, const uint64_t *a, const uint64_t *b_ntt, size_t batch, void *stream) {
    if (int rc = check(c, {out, a, b_ntt}, batch)) return rc;
    if (b_ntt == out) return fail(SR_E_INVALID, "ring_mul_ntt_rhs: b_ntt must not alias out");
    const Call call(c, stream);
    return dev_ring_mul_ntt_rhs(c, out, a, b_ntt, batch, call.st);
}
int sr_ctx_reserve_scratch(sr_ctx *c, size_t batch) {
    if (int rc = check(c, {}, batch)) return rc;
    const Call call(c);
    if (batch == 0) return SR_OK;
    // the two partial-element buffers of sr_sum_batch_dev / sr_product_batch_dev (a few MiB; the small rings' product tree sizes FOLD_0
    // by the slice length on first use)
    for (Buf b : {FOLD_0, FOLD_1})
        if (int rc = grow(c, b, fold_tmp_words(c->degree) * c->limbs * 8, nullptr, true)) return rc;
    if (!is_pow2_ring(c->ring)) return SR_OK;  // the small rings need no operand scratch
    if (int rc = lanes_autoselect(c, batch)) return rc;      // sr_plan.lanes = 0: settle the plan now, then size the scratch for it
    const size_t elem = c->degree * c->limbs * 8;
    switch (c->path) {
        case RT_BABYBEAR: case RT_GOLDILOCKS: {
            // BOTH users of the packed scratch: the ring product (four lane chunks on two lanes, else two buffers of one chunk) and the
            // stand-alone transforms, whose lanes only start at eight chunks (lanes_pay_transform): below that they run on the caller's
            // stream through ONE buffer of the whole batch (a batch of 4 .. 8 lane chunks used to be reserved for the product
            // only, and the first transform afterwards synchronised the device and reallocated)
            const bool lanes = use_lanes(c, batch, nullptr, false), lanes_t = use_lanes(c, batch, nullptr, true);
            const size_t whole = batch * lane_elem_bytes(c), four = 4 * lane_chunk(c) * lane_elem_bytes(c);
            if (lanes || lanes_t)
                if (int rc = gl_lanes_init(c)) return rc;
            if (c->k <= 12) return SR_OK;
            size_t need0 = lanes ? four : rt_chunk_polys(c, batch) * lane_elem_bytes(c), need1 = lanes ? 0 : need0;
            const size_t transform = lanes_t ? four : whole;
            if (transform > need0) need0 = transform;
            if (int rc = grow(c, OPERAND_A, need0, nullptr, true)) return rc;
            return need1 ? grow(c, OPERAND_B, need1, nullptr, true) : SR_OK;
        }
        case GL_FAST:
            if (c->k <= 12) return SR_OK;
            if (use_lanes(c, batch, nullptr, false)) {
                if (int rc = gl_lanes_init(c)) return rc;
                return grow(c, OPERAND_A, 4 * lane_chunk(c) * elem, nullptr, true);
            }
            return grow(c, OPERAND_A, gl_chunk_polys(c, batch) * elem, nullptr, true);
        case STARK_TUNED:
            if (c->stark_one_tile) return SR_OK;
            break;
        default:
            if (c->k <= c->log_tile) return SR_OK;
            break;
    }
    return grow(c, OPERAND_A, scratch_polys(c, batch, elem) * elem, nullptr, true);
}
int sr_pack32_batch_dev(sr_ctx *c, uint32_t *d_out, const uint64_t *d_in, size_t batch, void *stream) {
    if (int rc = check_packed(c, {d_out, d_in}, batch)) return rc;
    const Call call(c, stream);
    return launch_pack32(c, d_out, d_in, batch << c->k, call.st);
}
int sr_unpack32_batch_dev(sr_ctx *c, uint64_t *d_out, const uint32_t *d_in, size_t batch, void *stream) {
    if (int rc = check_packed(c, {d_out, d_in}, batch)) return rc;
    const Call call(c, stream);
    return launch_unpack32(c, d_out, d_in, batch << c->k, call.st);
}
int sr_ntt_fwd_packed32_batch_dev(sr_ctx *c, uint32_t *d, size_t batch, void *stream) {
    if (int rc = check_packed(c, {d}, batch)) return rc;
    const Call call(c, stream);
    if (batch == 0) return SR_OK;
    if (c->path == RT_BABYBEAR) return rt_transform<sr::BabyBear, 0, sr::rt::PackedStream>(c, d, batch, call.st);
    return packed_via_wide(c, d, d, nullptr, batch, call.st, [&](uint64_t *wa, uint64_t *) { return dev_fwd(c, wa, batch, call.st); });
}
int sr_ntt_inv_packed32_batch_dev(sr_ctx *c, uint32_t *d, size_t batch, void *stream) {
    if (int rc = check_packed(c, {d}, batch)) return rc;
    const Call call(c, stream);
    if (batch == 0) return SR_OK;
    if (c->path == RT_BABYBEAR) return rt_transform<sr::BabyBear, 1, sr::rt::PackedStream>(c, d, batch, call.st);
    return packed_via_wide(c, d, d, nullptr, batch, call.st, [&](uint64_t *wa, uint64_t *) { return dev_inv(c, wa, batch, call.st); });
}
int sr_ring_mul_packed32_batch_dev(sr_ctx *c, uint32_t *d_out, const uint32_t *d_a, const uint32_t *d_b, size_t batch, void *stream) {
    if (int rc = check_packed(c, {d_out, d_a, d_b}, batch)) return rc;
    if (d_b == d_out) return fail(SR_E_INVALID, "ring_mul: b must not alias out");
    const Call call(c, stream);
    if (batch == 0) return SR_OK;
    if (c->path == RT_BABYBEAR) return rt_ring_mul<sr::BabyBear, sr::rt::PackedStream>(c, d_out, d_a, d_b, batch, call.st);
    return packed_via_wide(c, d_out, d_a, d_b, batch, call.st, [&](uint64_t *wa, uint64_t *wb) { return dev_ring_mul(c, wa, wa, wb, batch, call.st); });
}
int sr_pointwise_mul_packed32_batch_dev(sr_ctx *c, uint32_t *l, const uint32_t *r, size_t batch, void *stream) {
    return packed_elementwise(c, l, r, batch, stream, 0);
}
int sr_add_packed32_batch_dev(sr_ctx *c, uint32_t *l, const uint32_t *r, size_t batch, void *stream) {
    return packed_elementwise(c, l, r, batch, stream, 1);
}
int sr_sub_packed32_batch_dev(sr_ctx *c, uint32_t *l, const uint32_t *r, size_t batch, void *stream) {
    return packed_elementwise(c, l, r, batch, stream, 2);
}
int sr_ctx_plan_in_use(sr_ctx *c, sr_plan *plan, double probe_ms[2], size_t *probe_elems) {
    if (!c || !plan) return fail(SR_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    *plan = c->plan;
    if (!plan->lanes) plan->lanes = (uint32_t)c->lanes_choice;  // 0 = auto and not settled yet (no chunked product seen)
    if (probe_ms) {
        probe_ms[0] = c->lanes_probe_ms[0];
        probe_ms[1] = c->lanes_probe_ms[1];
    }
    if (probe_elems) *probe_elems = c->lanes_probe_elems;
    return SR_OK;
}
int sr_reduce_batch_dev(sr_ctx *c, const uint64_t *in, size_t in_len, uint64_t *out, size_t batch, void *stream) {
    if (int rc = check(c, {in, out}, batch)) return rc;
    const Call call(c, stream);
    return dev_reduce(c, in, in_len, out, batch, call.st);
}
int sr_fill_uniform_dev(sr_ctx *c, uint64_t seed, uint64_t first, size_t n, uint64_t *out, void *stream) {
    if (int rc = check(c, {out})) return rc;
    const Call call(c, stream);
    DISPATCH_BASE_FIELD(c, (fill_dev<F>(c, seed, first, n, out, call.st)));
}
int sr_count_noncanonical_dev(sr_ctx *c, const uint64_t *d, size_t n, uint64_t *host_count, void *stream) {
    if (int rc = check(c, {d, host_count})) return rc;
    const Call call(c, stream);
    DISPATCH_BASE_FIELD(c, (count_dev<F>(c, d, n, host_count, call.st)));
}

int sr_neg_batch(sr_ctx *c, uint64_t *data, size_t batch) { return host_unary(c, data, nullptr, batch, 0); }
int sr_scale_batch(sr_ctx *c, uint64_t *data, const uint64_t *scalar, size_t batch) { return host_unary(c, data, scalar, batch, 1); }
int sr_add_scalar_batch(sr_ctx *c, uint64_t *data, const uint64_t *scalar, int ntt_form, size_t batch) {
    return host_unary(c, data, scalar, batch, ntt_form ? 3 : 2);
}
// host buffers: the one element goes to ELEMENT, the batch through the staged pipeline
int sr_mul_elem_batch(sr_ctx *c, uint64_t *data, const uint64_t *elem, size_t batch) {
    if (int rc = check(c, {data, elem}, batch)) return rc;
    const Call call(c);
    const size_t bytes = (size_t)c->degree * c->limbs * 8;
    if (int rc = grow(c, ELEMENT, bytes)) return rc;
    const uint64_t *dr = (const uint64_t *)c->buf[ELEMENT];
    HIP_TRY(hipMemcpy(c->buf[ELEMENT], elem, bytes, hipMemcpyHostToDevice));
    return host_pipeline(c, data, data, nullptr, batch, [&](uint64_t *s0, uint64_t *, size_t n, hipStream_t st) {
        return dev_mul_elem(c, s0, dr, n, st);
    });
}
int sr_ntt_fwd_batch(sr_ctx *c, uint64_t *data, size_t batch) { return host_inplace(c, data, batch, true); }
int sr_ntt_inv_batch(sr_ctx *c, uint64_t *data, size_t batch) { return host_inplace(c, data, batch, false); }

int sr_pointwise_mul_batch(sr_ctx *c, uint64_t *lhs, const uint64_t *rhs, size_t batch) {
    return host_binary(c, lhs, lhs, rhs, batch, HB_POINTWISE);
}
int sr_add_batch(sr_ctx *c, uint64_t *lhs, const uint64_t *rhs, size_t batch) { return host_binary(c, lhs, lhs, rhs, batch, HB_ADD); }
int sr_sub_batch(sr_ctx *c, uint64_t *lhs, const uint64_t *rhs, size_t batch) { return host_binary(c, lhs, lhs, rhs, batch, HB_SUB); }
int sr_ring_mul_batch(sr_ctx *c, uint64_t *out, const uint64_t *a, const uint64_t *b, size_t batch) {
    return host_binary(c, out, a, b, batch, HB_RING_MUL);
}
int sr_ring_mul_ntt_rhs_batch(sr_ctx *c, uint64_t *out, const uint64_t *a, const uint64_t *b_ntt, size_t batch) {
    return host_binary(c, out, a, b_ntt, batch, HB_RING_MUL_NTT_RHS);
}
int sr_reduce_batch(sr_ctx *c, const uint64_t *in, size_t in_len, uint64_t *out, size_t batch) {
    if (int rc = check(c, {in, out}, batch)) return rc;
    if (in_len > 2 * c->degree) return fail(SR_E_INVALID, "reduce: in_len_per_elem > 2D");
    const Call call(c);
    const size_t in_bytes = batch * in_len * c->limbs * 8, out_bytes = batch * c->degree * c->limbs * 8;
    if (out_bytes == 0) return SR_OK;
    return staged(c, {{in, nullptr, in_bytes}, {nullptr, out, out_bytes}}, [&](void *const *d) {
        return dev_reduce(c, (const uint64_t *)d[0], in_len, (uint64_t *)d[1], batch, c->stream);
    });
}

int sr_selftest_field_op(int field, int op, const uint64_t *a, const uint64_t *b, uint64_t *out) {
    if (!a || !b || !out) return fail(SR_E_INVALID, "null argument");
    if (field == 0 && op == 5) {
        if (b[0] < 1 || b[0] > 95) return fail(SR_E_INVALID, "selftest: shift out of range");
        out[0] = mul_pow2_any(a[0], (int)b[0], std::make_integer_sequence<int, 95>{});
        return SR_OK;
    }
    alignas(16) uint64_t ta[4] = {0, 0, 0, 0}, tb[4] = {0, 0, 0, 0}, to[4] = {0, 0, 0, 0};
    int words = (field == 2 || field == 4) ? 4 : 1;
    memcpy(ta, a, words * 8);
    memcpy(tb, b, words * 8);
    int rc;
    switch (field) {
        case 0: rc = selftest_op<sr::Goldilocks>(op, ta, tb, to); break;
        case 1: rc = selftest_op<sr::BabyBear>(op, ta, tb, to); break;
        case 2: rc = selftest_op<sr::Stark>(op, ta, tb, to); break;
        case 3: rc = selftest_op<sr::Frog>(op, ta, tb, to); break;
        case 4: rc = selftest_lazy(op, ta, tb, to); break;
        default: return fail(SR_E_INVALID, "selftest: unknown field");
    }
    memcpy(out, to, words * 8);
    return rc;
}

// Representative-invariant counters of the checking build (fields.hpp: repcheck).  The product library counts nothing and says so.
int sr_selftest_rep_counters(uint64_t counters[8], int reset) {
    if (!counters) return fail(SR_E_INVALID, "null argument");
#if defined(SR_GL_CHECK_REPS)
    // g_counters is a __device__ symbol, i.e. one copy per device: visit every visible device (contexts of the sharded tests live on
    // devices other than the current one), sum the violation counts and take the high-water mark's maximum
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    for (int i = 0; i < 8; i++) counters[i] = 0;
    for (int dev = 0; dev < ndev; dev++) {
        DeviceGuard g(dev);
        if (!g.ok) return fail(SR_E_HIP, "hipSetDevice failed");
        unsigned long long h[8];
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpyFromSymbol(h, HIP_SYMBOL(sr::repcheck::g_counters), sizeof(h)));
        for (int i = 0; i < 7; i++) counters[i] += h[i];
        if (h[7] > counters[7]) counters[7] = h[7];
        if (reset) {
            memset(h, 0, sizeof(h));
            HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(sr::repcheck::g_counters), h, sizeof(h)));
        }
    }
    return SR_OK;
#else
    (void)reset;
    for (int i = 0; i < 8; i++) counters[i] = 0;
    return fail(SR_E_UNSUPPORTED, "this build does not check representatives (built without -DSR_GL_CHECK_REPS)");
#endif
}

// ---- profiling ----
int sr_ctx_profile_enable(sr_ctx *c, int on) {
    if (!c) return fail(SR_E_INVALID, "null context");
    std::lock_guard<std::mutex> lk(c->mu);
    c->prof.on = on != 0;
    c->prof.stride = on > 1 ? (unsigned)on : 1u;
    c->prof.tick = 0;
    return SR_OK;
}
int sr_ctx_profile_read(sr_ctx *c, double *ms_total, uint64_t *launches) { return sr_ctx_profile_read_sampled(c, ms_total, launches, nullptr); }
int sr_ctx_profile_read_sampled(sr_ctx *c, double *ms_total, uint64_t *launches, uint64_t *seen) {
    if (!c || !ms_total || !launches) return fail(SR_E_INVALID, "null argument");
    const Call call(c);
    for (auto &p : c->prof.pending) {
        HIP_TRY(hipEventSynchronize(p.b));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, p.a, p.b));
        c->prof.ms[p.tag] += ms;
        c->prof.launches[p.tag]++;
        (void)hipEventDestroy(p.a);
        (void)hipEventDestroy(p.b);
    }
    c->prof.pending.clear();
    for (int t = 0; t < K_NTAGS; t++) {
        ms_total[t] = c->prof.ms[t];
        launches[t] = c->prof.launches[t];
        if (seen) seen[t] = c->prof.seen[t];
        c->prof.ms[t] = 0;
        c->prof.launches[t] = 0;
        c->prof.seen[t] = 0;
    }
    return SR_OK;
}

}  // extern "C"
