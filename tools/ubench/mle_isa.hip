// The multilinear-fold kernels alone (stark_rings_amd/csrc/mle.hpp), every instantiation the library dispatches to, so that
// `hipcc -S` takes seconds: tests/test_mle_isa.py reads the listing.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only -o mle.s tools/ubench/mle_isa.hip
#include "../../stark_rings_amd/csrc/mle.hpp"
using namespace sr;
#define FOLD(F, J) \
    template __global__ void mle::fold_kernel<F, J>(F::storage *, const F::storage *, const F::storage *, size_t, size_t, size_t, size_t, int);
#define FOLDS(F) FOLD(F, 0) FOLD(F, 1) FOLD(F, 2)
FOLDS(Goldilocks) FOLD(Goldilocks, 3)
FOLDS(BabyBear) FOLD(BabyBear, 3)
FOLDS(Stark)
#define SLOT(SL, J) \
    template __global__ void mle::slot_fold_kernel<SL, J>(SL::K, uint64_t *, const uint64_t *, const uint64_t *, size_t, size_t, size_t, size_t);
#define SLOTS(SL) SLOT(SL, 0) SLOT(SL, 1) SLOT(SL, 2)
SLOTS(SlotG24) SLOT(SlotG24, 3)
SLOTS(SlotB72)
SLOTS(SlotFrog) SLOT(SlotFrog, 3)
#define MEA(F) template __global__ void mle::mul_elem_add_kernel<F>(F::storage *, const F::storage *, const F::storage *, size_t, size_t);
MEA(Goldilocks)
MEA(BabyBear)
MEA(Stark)
#define SMEA(SL) template __global__ void mle::slot_mul_elem_add_kernel<SL>(SL::K, uint64_t *, const uint64_t *, const uint64_t *, size_t);
SMEA(SlotG24)
SMEA(SlotB72)
SMEA(SlotFrog)
