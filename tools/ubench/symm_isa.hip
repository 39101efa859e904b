// The symmetric-matrix kernels alone (stark_rings_amd/csrc/symmetric.hpp), every instantiation the library dispatches to, so that
// `hipcc -S` takes seconds: tests/test_symm_isa.py reads the listing.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only -o symm.s tools/ubench/symm_isa.hip
#include "../../stark_rings_amd/csrc/stark_lazy.hpp"
#include "../../stark_rings_amd/csrc/symmetric.hpp"
using namespace sr;
#define GRAM(F, RB, CB) template __global__ void symm::gram_kernel<F, RB, CB>(F::storage *, const F::storage *, size_t, size_t, int, unsigned, size_t);
GRAM(Goldilocks, 4, 2)
GRAM(BabyBear, 8, 4)
GRAM(Stark, 2, 1)
GRAM(StarkL, 2, 1)
#define SUM(F) template __global__ void symm::sum_parts_kernel<F>(F::storage *, const F::storage *, size_t, unsigned);
SUM(Goldilocks)
SUM(BabyBear)
SUM(Stark)
SUM(Frog)
#define WEIGHTS(F) template __global__ void symm::weights_kernel<F>(F::storage *, const F::storage *, size_t, int);
WEIGHTS(Goldilocks)
WEIGHTS(BabyBear)
WEIGHTS(Stark)
#define RECOMPOSE(F, FA) template __global__ void symm::recompose_kernel<F, FA>(uint64_t *, const uint64_t *, const uint64_t *, size_t, size_t, int, int);
RECOMPOSE(Goldilocks, Goldilocks)
RECOMPOSE(BabyBear, BabyBear)
RECOMPOSE(Stark, Stark)
RECOMPOSE(Stark, StarkL)
#define SLOT(SL)                                                                                                                   \
    template __global__ void symm::slot_gram_kernel<SL>(SL::K, uint64_t *, const uint64_t *, size_t, size_t, unsigned, size_t);   \
    template __global__ void symm::slot_weights_kernel<SL>(SL::K, uint64_t *, const uint64_t *, size_t);                          \
    template __global__ void symm::slot_recompose_kernel<SL>(SL::K, uint64_t *, const uint64_t *, const uint64_t *, size_t, size_t);
SLOT(SlotG24)
SLOT(SlotB72)
SLOT(SlotFrog)
