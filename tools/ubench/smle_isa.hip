// The sparse multilinear-extension kernels alone (stark_rings_amd/csrc/sparse_mle.hpp), every instantiation the library dispatches
// to (smle_dispatch in capi.hip), so that `hipcc -S` takes seconds: tests/test_smle_isa.py reads the listing.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only -o smle.s tools/ubench/smle_isa.hip
#include "../../stark_rings_amd/csrc/stark_lazy.hpp"
#include "../../stark_rings_amd/csrc/sparse_mle.hpp"
using namespace sr;
#define SMLE(O, J)                                                                                                                          \
    template __global__ void smle::eq_kernel<O, J>(O::K, smle::One, uint64_t *, const uint64_t *, unsigned, unsigned, int);                   \
    template __global__ void smle::fold_kernel<O, true>(O::K, smle::One, uint64_t *, const uint64_t *, const uint64_t *, const uint64_t *,    \
                                                        size_t, size_t, const uint64_t *, unsigned, unsigned, size_t, size_t, uint64_t *, int); \
    template __global__ void smle::fold_kernel<O, false>(O::K, smle::One, uint64_t *, const uint64_t *, const uint64_t *, const uint64_t *,   \
                                                         size_t, size_t, const uint64_t *, unsigned, unsigned, size_t, size_t, uint64_t *, int); \
    template __global__ void smle::combine_kernel<O>(uint64_t *, const uint64_t *, size_t, size_t, size_t, const uint64_t *, int);
using GL2 = smle::PowOps<Goldilocks, Goldilocks, 2>;
using GL1 = smle::PowOps<Goldilocks, Goldilocks, 1>;
using BB2 = smle::PowOps<BabyBear, BabyBear, 2>;
using BB1 = smle::PowOps<BabyBear, BabyBear, 1>;
using STL = smle::PowOps<Stark, StarkL, 4>;
using ST = smle::PowOps<Stark, Stark, 4>;
using G24 = smle::SlotOps<SlotG24>;
using B72 = smle::SlotOps<SlotB72>;
using FRG = smle::SlotOps<SlotFrog>;
SMLE(GL2, 3) SMLE(GL1, 3) SMLE(BB2, 3) SMLE(BB1, 3) SMLE(STL, 2) SMLE(ST, 2) SMLE(G24, 3) SMLE(B72, 2) SMLE(FRG, 3)
