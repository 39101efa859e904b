// Device build AND host build of the per-field arithmetic (fields.hpp, stark_lazy.hpp) on operands read from a file; the results of
// both go to a file and tests/test_device_fields_gpu.py compares them with exact integers.  This program compares nothing itself.
//
//   field_ops_device [--host-only] REQUESTS RESULTS
//
// REQUESTS: "SRFOPRQ1", u32 count, u32 0, then per request: u32 field, u32 op, u32 n, u32 0, n x (a, b), every operand 4 x u64 in
//   the memory image sr_selftest_field_op takes (one-word fields use word 0).
// RESULTS:  "SRFOPRS1", u32 count, u32 device arrays present, then per request: u32 field, u32 op, u32 n, u32 0 and the arrays
//   host plain, host divergent, [device plain, device divergent], n x 4 x u64 each.
// Field ids and op numbers are those of sr_selftest_field_op (capi.hip: selftest_op, selftest_lazy) -- keep them equal:
//   fields 0 Goldilocks, 1 BabyBear, 2 Stark, 3 Frog: 0 add, 1 sub, 2 mul_boundary, 3 mul_tw, 4 tw_from_u64(a[0]);
//   field 4 StarkL: 0 add, 1 sub, 3 mul_tw, 4 tw_from_u64(a[0]), 5 six lazy additions / subtractions feeding mul_tw and mul_data,
//     6 repeated quadrupling with weak reductions, 7 3a - 5b, 8 7a - 2b, all leaving through the canonicalising store.
// Ops the hook does not have start at 16:
//   16 neg(a) (fields 0..3), 17 mul_tw(a, a) with both operands the same object (every field), and for StarkL 18 mul_data(a, b),
//   19 weak_reduce(a) then store, 20 boundary_post(mul_boundary_pre(a, b)).
// Every request is launched twice, 256 lanes per workgroup: plain, lane i computes op(a[i], b[i]); divergent, lanes whose flag
// word (i & 1, read from memory) is set compute op(a[i], b[i]) in one arm of a branch and the others op(b[i], a[i]) in the other,
// so both arms run under complementary, partially set EXEC masks.  --host-only makes no HIP call at all.
// Exit status: 0, 1 for a usage / file error, 2 for a HIP error.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -o tools/ubench/field_ops_device tools/ubench/field_ops_device.hip
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>
#include "../../stark_rings_amd/csrc/fields.hpp"
#include "../../stark_rings_amd/csrc/stark_lazy.hpp"

using Img = sr::U256Storage;

template <class F, int OP>
SR_HD void plain_op(const Img &a, const Img &b, Img &o) {
    using S = typename F::storage;
    const typename F::elem x = F::load(reinterpret_cast<const S *>(&a)), y = F::load(reinterpret_cast<const S *>(&b));
    typename F::elem r;
    if constexpr (OP == 0) r = F::add(x, y);
    else if constexpr (OP == 1) r = F::sub(x, y);
    else if constexpr (OP == 2) r = F::mul_boundary(x, y);
    else if constexpr (OP == 3) r = F::mul_tw(x, y);
    else if constexpr (OP == 4) r = F::tw_from_u64(a.q[0]);
    else if constexpr (OP == 16) r = F::neg(x);
    else r = F::mul_tw(x, x);
    o.q[0] = o.q[1] = o.q[2] = o.q[3] = 0;
    F::store(reinterpret_cast<S *>(&o), r);
}

template <int OP>
SR_HD void lazy_op(const Img &a, const Img &b, Img &o) {
    using F = sr::StarkL;
    const F::elem x = F::load(&a), y = F::load(&b);
    F::elem r;
    if constexpr (OP == 0) r = F::add(x, y);
    else if constexpr (OP == 1) r = F::sub(x, y);
    else if constexpr (OP == 3) r = F::mul_tw(x, y);
    else if constexpr (OP == 4) r = F::tw_from_u64(a.q[0]);
    else if constexpr (OP == 5) {
        F::elem s = x, d = x;
        for (int i = 0; i < 6; i++) {
            s = F::add(s, y);
            d = F::sub(d, y);
        }
        r = F::add(F::mul_tw(s, y), F::mul_data(d, s));
    } else if constexpr (OP == 6) {
        r = x;
        for (int i = 0; i < 4; i++) r = F::weak_reduce(F::add(F::add(r, r), F::add(r, r)));
    } else if constexpr (OP == 7) {
        r = F::sub(F::add(F::add(x, x), x), F::add(F::add(F::add(y, y), F::add(y, y)), y));
    } else if constexpr (OP == 8) {
        const F::elem x2 = F::add(x, x), x4 = F::add(x2, x2);
        r = F::sub(F::add(F::add(x4, x2), x), F::add(y, y));
    } else if constexpr (OP == 17) r = F::mul_tw(x, x);
    else if constexpr (OP == 18) r = F::mul_data(x, y);
    else if constexpr (OP == 19) r = F::weak_reduce(x);
    else r = F::boundary_post(F::mul_boundary_pre(x, y));
    F::store(&o, r);
}

template <class F, int OP>
SR_HD void field_op(const Img &a, const Img &b, Img &o) {
    if constexpr (std::is_same<F, sr::StarkL>::value) lazy_op<OP>(a, b, o);
    else plain_op<F, OP>(a, b, o);
}

// The two arms differ only in their operands; the markers keep the compiler from merging them into one arm behind selects.
#define ARM(tag) asm volatile("; field_ops_device arm " tag ::: "memory")
template <class F, int OP, bool DIVERGENT>
__global__ void __launch_bounds__(256) op_kernel(const Img *a, const Img *b, const uint32_t *flag, Img *o, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Img x = a[i], y = b[i];
    Img r;
    if (!DIVERGENT) {
        field_op<F, OP>(x, y, r);
    } else if (flag[i]) {
        ARM("set: begin");
        field_op<F, OP>(x, y, r);
        ARM("set: end");
    } else {
        ARM("clear: begin");
        field_op<F, OP>(y, x, r);
        ARM("clear: end");
    }
    o[i] = r;
}

#define HIP_OK(call)                                                                                      \
    do {                                                                                                  \
        const hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess) {                                                                           \
            fprintf(stderr, "field_ops_device: %s: %s\n", #call, hipGetErrorString(e_));                  \
            return 2;                                                                                     \
        }                                                                                                 \
    } while (0)

struct Buffers {
    Img *a = nullptr, *b = nullptr, *o = nullptr;
    uint32_t *flag = nullptr;
    uint32_t cap = 0;
};

// host plain, host divergent, and with a device the same two from kernels; res holds 2 or 4 arrays of n images
template <class F, int OP>
int run(const Img *a, const Img *b, uint32_t n, Img *res, Buffers *dev) {
    for (uint32_t i = 0; i < n; i++) {
        field_op<F, OP>(a[i], b[i], res[i]);
        if (i & 1) field_op<F, OP>(a[i], b[i], res[n + i]);
        else field_op<F, OP>(b[i], a[i], res[n + i]);
    }
    if (!dev || n == 0) return 0;
    if (n > dev->cap) return 1;
    const size_t bytes = (size_t)n * sizeof(Img);
    const dim3 grid((n + 255) / 256), block(256);
    HIP_OK(hipMemcpy(dev->a, a, bytes, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dev->b, b, bytes, hipMemcpyHostToDevice));
    for (int mode = 0; mode < 2; mode++) {
        HIP_OK(hipMemset(dev->o, 0xA5, bytes));
        if (mode == 0) hipLaunchKernelGGL((op_kernel<F, OP, false>), grid, block, 0, 0, dev->a, dev->b, dev->flag, dev->o, n);
        else hipLaunchKernelGGL((op_kernel<F, OP, true>), grid, block, 0, 0, dev->a, dev->b, dev->flag, dev->o, n);
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(res + (size_t)(2 + mode) * n, dev->o, bytes, hipMemcpyDeviceToHost));
    }
    return 0;
}

template <class F>
int run_plain(uint32_t op, const Img *a, const Img *b, uint32_t n, Img *res, Buffers *dev) {
    switch (op) {
        case 0: return run<F, 0>(a, b, n, res, dev);
        case 1: return run<F, 1>(a, b, n, res, dev);
        case 2: return run<F, 2>(a, b, n, res, dev);
        case 3: return run<F, 3>(a, b, n, res, dev);
        case 4: return run<F, 4>(a, b, n, res, dev);
        case 16: return run<F, 16>(a, b, n, res, dev);
        case 17: return run<F, 17>(a, b, n, res, dev);
    }
    return 1;
}
int run_lazy(uint32_t op, const Img *a, const Img *b, uint32_t n, Img *res, Buffers *dev) {
    using F = sr::StarkL;
    switch (op) {
        case 0: return run<F, 0>(a, b, n, res, dev);
        case 1: return run<F, 1>(a, b, n, res, dev);
        case 3: return run<F, 3>(a, b, n, res, dev);
        case 4: return run<F, 4>(a, b, n, res, dev);
        case 5: return run<F, 5>(a, b, n, res, dev);
        case 6: return run<F, 6>(a, b, n, res, dev);
        case 7: return run<F, 7>(a, b, n, res, dev);
        case 8: return run<F, 8>(a, b, n, res, dev);
        case 17: return run<F, 17>(a, b, n, res, dev);
        case 18: return run<F, 18>(a, b, n, res, dev);
        case 19: return run<F, 19>(a, b, n, res, dev);
        case 20: return run<F, 20>(a, b, n, res, dev);
    }
    return 1;
}

struct Head {
    uint32_t field, op, n, zero;
};

static bool read_all(FILE *f, void *p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }
static bool write_all(FILE *f, const void *p, size_t bytes) { return bytes == 0 || fwrite(p, 1, bytes, f) == bytes; }

int main(int argc, char **argv) {
    bool host_only = false;
    const char *paths[2] = {nullptr, nullptr};
    int np = 0;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--host-only")) host_only = true;
        else if (np < 2) paths[np++] = argv[i];
        else np = 3;
    }
    if (np != 2) {
        fprintf(stderr, "usage: field_ops_device [--host-only] REQUESTS RESULTS\n");
        return 1;
    }
    FILE *in = fopen(paths[0], "rb");
    if (!in) {
        fprintf(stderr, "field_ops_device: cannot read %s\n", paths[0]);
        return 1;
    }
    char magic[8];
    uint32_t top[2];
    if (!read_all(in, magic, 8) || memcmp(magic, "SRFOPRQ1", 8) != 0 || !read_all(in, top, 8)) {
        fprintf(stderr, "field_ops_device: %s is not a request file\n", paths[0]);
        return 1;
    }
    const uint32_t count = top[0], kMaxN = 1u << 20;
    std::vector<Head> heads(count);
    std::vector<std::vector<Img>> as(count), bs(count);
    uint32_t max_n = 0;
    for (uint32_t r = 0; r < count; r++) {
        if (!read_all(in, &heads[r], sizeof(Head)) || heads[r].n > kMaxN) {
            fprintf(stderr, "field_ops_device: request %u: bad header\n", r);
            return 1;
        }
        const uint32_t n = heads[r].n;
        std::vector<Img> pairs(2 * (size_t)n);
        if (!read_all(in, pairs.data(), pairs.size() * sizeof(Img))) {
            fprintf(stderr, "field_ops_device: request %u: file ends early\n", r);
            return 1;
        }
        as[r].resize(n);
        bs[r].resize(n);
        for (uint32_t i = 0; i < n; i++) {
            as[r][i] = pairs[2 * (size_t)i];
            bs[r][i] = pairs[2 * (size_t)i + 1];
        }
        max_n = n > max_n ? n : max_n;
    }
    fclose(in);

    Buffers dev;
    if (!host_only && max_n) {
        const size_t bytes = (size_t)max_n * sizeof(Img);
        HIP_OK(hipMalloc(&dev.a, bytes));
        HIP_OK(hipMalloc(&dev.b, bytes));
        HIP_OK(hipMalloc(&dev.o, bytes));
        HIP_OK(hipMalloc(&dev.flag, (size_t)max_n * 4));
        std::vector<uint32_t> flag(max_n);
        for (uint32_t i = 0; i < max_n; i++) flag[i] = i & 1u;
        HIP_OK(hipMemcpy(dev.flag, flag.data(), (size_t)max_n * 4, hipMemcpyHostToDevice));
        dev.cap = max_n;
    }

    FILE *out = fopen(paths[1], "wb");
    if (!out) {
        fprintf(stderr, "field_ops_device: cannot write %s\n", paths[1]);
        return 1;
    }
    const uint32_t arrays = host_only ? 2 : 4, rtop[2] = {count, host_only ? 0u : 1u};
    bool ok = write_all(out, "SRFOPRS1", 8) && write_all(out, rtop, 8);
    for (uint32_t r = 0; r < count && ok; r++) {
        const Head h = heads[r];
        std::vector<Img> res((size_t)arrays * h.n);
        Buffers *d = host_only ? nullptr : &dev;
        int rc = 1;
        switch (h.field) {
            case 0: rc = run_plain<sr::Goldilocks>(h.op, as[r].data(), bs[r].data(), h.n, res.data(), d); break;
            case 1: rc = run_plain<sr::BabyBear>(h.op, as[r].data(), bs[r].data(), h.n, res.data(), d); break;
            case 2: rc = run_plain<sr::Stark>(h.op, as[r].data(), bs[r].data(), h.n, res.data(), d); break;
            case 3: rc = run_plain<sr::Frog>(h.op, as[r].data(), bs[r].data(), h.n, res.data(), d); break;
            case 4: rc = run_lazy(h.op, as[r].data(), bs[r].data(), h.n, res.data(), d); break;
        }
        if (rc == 1) fprintf(stderr, "field_ops_device: request %u: unknown field %u / op %u\n", r, h.field, h.op);
        if (rc) return rc;
        ok = write_all(out, &h, sizeof(Head)) && write_all(out, res.data(), res.size() * sizeof(Img));
    }
    if (fclose(out) != 0 || !ok) {
        fprintf(stderr, "field_ops_device: writing %s failed\n", paths[1]);
        return 1;
    }
    if (!host_only) {
        HIP_OK(hipFree(dev.a));
        HIP_OK(hipFree(dev.b));
        HIP_OK(hipFree(dev.o));
        HIP_OK(hipFree(dev.flag));
    }
    printf("field_ops_device: %u requests, %s\n", count, host_only ? "host only" : "host and device");
    return 0;
}
