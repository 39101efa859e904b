// The batch-inversion kernel of stark_rings_amd/csrc/inverse.hpp at the library's chunk length against the SAME kernel at chunk 1 -- a
// Fermat inversion per unit -- and at the neighbouring chunk lengths, reached through the launcher's template parameter: the product
// library has no switch for this.  tools/bench_inverse.py runs it per shape and keeps the lines.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -o build_tmp/inverse_bench tools/ubench/inverse_bench.hip
//   build_tmp/inverse_bench <goldilocks|babybear|stark|goldilocks24|babybear72|frog16> <log2 D> <log2 n> <reps>
// Tables hold canonical non-zero words.  The contenders alternate per repetition; one JSON line with every time of every contender.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../stark_rings_amd/csrc/decompose.hpp"
#include "../../stark_rings_amd/csrc/inverse.hpp"

using namespace sr;

#define CHECK(x)                                                                      \
    do {                                                                              \
        hipError_t e_ = (x);                                                          \
        if (e_ != hipSuccess) {                                                       \
            std::printf("%s: %s\n", #x, hipGetErrorString(e_));                       \
            std::exit(1);                                                             \
        }                                                                             \
    } while (0)

// word i of a table: below 2^63 (2^30 for BabyBear, whose upper half is zero; 2^58 in the top limb of a Stark coefficient), never 0
__global__ void fill_kernel(uint64_t *t, size_t words, uint64_t seed, uint64_t mask, uint64_t top_mask, int limbs) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < words; i += (size_t)gridDim.x * blockDim.x) {
        uint64_t x = (i + seed) * 0x9E3779B97F4A7C15ull;
        x ^= x >> 29;
        x *= 0xBF58476D1CE4E5B9ull;
        x ^= x >> 32;
        t[i] = (x & ((int)(i % limbs) == limbs - 1 ? top_mask : mask)) | 1;
    }
}

template <class F>
static smle::One one_of() {
    smle::One one;
    typename F::storage s;
    F::store(&s, F::mul_boundary(dec::Consts<F>::one(), dec::Consts<F>::r2()));
    std::memset(one.w, 0, 32);
    std::memcpy(one.w, &s, sizeof(s));
    return one;
}

struct Run {
    std::string name;
    bool has_num;
    std::vector<float> ms;
};

template <class T, int C>
static void add(std::vector<Run> &runs, std::vector<hipError_t (*)(const typename sumcheck::Family<T>::K &, uint64_t *, const uint64_t *, const uint64_t *,
                                                                  const smle::One &, size_t, int, bool, unsigned long long *, hipStream_t)> &fns,
                const char *label) {
    for (int hn = 0; hn < 2; hn++) {
        runs.push_back({std::string(label) + (hn ? "_num" : ""), hn != 0, {}});
        fns.push_back(&inverse::launch<T, C>);
    }
}

template <class T, class F>
static int bench(const typename sumcheck::Family<T>::K &kc, const char *name, int k, int log2n, int reps, int limbs, uint64_t mask, uint64_t top_mask) {
    const size_t n = (size_t)1 << log2n;
    const size_t w = sumcheck::kSlot<T> ? sumcheck::geometry_of<T>(0, true).words : ((size_t)limbs << k);
    const size_t words = n * w;
    uint64_t *den, *num, *out;
    unsigned long long *zeros, host_zeros = 0;
    CHECK(hipMalloc(&den, words * 8));
    CHECK(hipMalloc(&num, words * 8));
    CHECK(hipMalloc(&out, words * 8));
    CHECK(hipMalloc(&zeros, 8));
    CHECK(hipMemset(zeros, 0, 8));
    hipLaunchKernelGGL(fill_kernel, dim3(4096), dim3(256), 0, 0, den, words, 0x1111ull, mask, top_mask, limbs);
    hipLaunchKernelGGL(fill_kernel, dim3(4096), dim3(256), 0, 0, num, words, 0x7777777ull, mask, top_mask, limbs);
    CHECK(hipDeviceSynchronize());
    const smle::One one = one_of<F>();
    std::vector<Run> runs;
    std::vector<hipError_t (*)(const typename sumcheck::Family<T>::K &, uint64_t *, const uint64_t *, const uint64_t *, const smle::One &, size_t, int,
                               bool, unsigned long long *, hipStream_t)>
        fns;
    add<T, 0>(runs, fns, "chosen");
    add<T, 1>(runs, fns, "chunk1");
    add<T, 2>(runs, fns, "chunk2");
    if constexpr (!std::is_same<T, SlotB72>::value) add<T, 4>(runs, fns, "chunk4");
    if constexpr (std::is_same<T, Goldilocks>::value || std::is_same<T, BabyBear>::value) {
        add<T, 8>(runs, fns, "chunk8");
        add<T, 16>(runs, fns, "chunk16");
    }
    hipEvent_t a, b;
    CHECK(hipEventCreate(&a));
    CHECK(hipEventCreate(&b));
    for (int rep = -1; rep < reps; rep++) {  // rep -1: warm-up
        for (size_t i = 0; i < runs.size(); i++) {
            CHECK(hipEventRecord(a, 0));
            CHECK(fns[i](kc, out, runs[i].has_num ? num : nullptr, den, one, n, k, true, zeros, 0));
            CHECK(hipEventRecord(b, 0));
            CHECK(hipEventSynchronize(b));
            float ms = 0;
            CHECK(hipEventElapsedTime(&ms, a, b));
            if (rep >= 0) runs[i].ms.push_back(ms);
        }
    }
    CHECK(hipMemcpy(&host_zeros, zeros, 8, hipMemcpyDeviceToHost));
    std::printf("{\"tool\": \"inverse_bench\", \"ring\": \"%s\", \"log2_degree\": %d, \"log2_n\": %d, \"table_bytes\": %zu, \"reps\": %d, \"zero_units\": %llu, "
                "\"chunk\": %d, \"chunk_num\": %d, \"ms\": {",
                name, k, log2n, words * 8, reps, host_zeros, inverse::kChunk<T, false>, inverse::kChunk<T, true>);
    for (size_t i = 0; i < runs.size(); i++) {
        std::printf("%s\"%s\": [", i ? ", " : "", runs[i].name.c_str());
        for (size_t j = 0; j < runs[i].ms.size(); j++) std::printf("%s%.4f", j ? ", " : "", runs[i].ms[j]);
        std::printf("]");
    }
    std::printf("}}\n");
    CHECK(hipFree(den));
    CHECK(hipFree(num));
    CHECK(hipFree(out));
    CHECK(hipFree(zeros));
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 5) {
        std::printf("usage: inverse_bench <ring> <log2 D> <log2 n> <reps>\n");
        return 2;
    }
    const std::string ring = argv[1];
    const int k = std::atoi(argv[2]), log2n = std::atoi(argv[3]), reps = std::atoi(argv[4]);
    const uint64_t m63 = (1ull << 63) - 1;
    if (k < 0 || k > 24 || log2n < 0 || log2n > 30 || reps < 1) return 2;
    if (ring == "goldilocks") return bench<Goldilocks, Goldilocks>({}, "goldilocks", k, log2n, reps, 1, m63, m63);
    if (ring == "babybear") return bench<BabyBear, BabyBear>({}, "babybear", k, log2n, reps, 1, (1ull << 30) - 1, (1ull << 30) - 1);
    if (ring == "stark") return bench<Stark, Stark>({}, "stark", k, log2n, reps, 4, ~0ull, (1ull << 58) - 1);
    if (ring == "goldilocks24" || ring == "babybear72") {
        SmallRingConsts c{};
        if (ring == "goldilocks24") {
            small_consts_for<Goldilocks>(c);
            return bench<SlotG24, Goldilocks>(c, "goldilocks24", 0, log2n, reps, 1, m63, m63);
        }
        small_consts_for<BabyBear>(c);
        return bench<SlotB72, BabyBear>(c, "babybear72", 0, log2n, reps, 1, (1ull << 30) - 1, (1ull << 30) - 1);
    }
    if (ring == "frog16") {
        FrogConsts c{};
        frog_init(c);
        return bench<SlotFrog, Frog>(c, "frog16", 0, log2n, reps, 1, m63, m63);
    }
    return 2;
}
