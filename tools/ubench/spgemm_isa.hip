// The sparse-matrix kernels alone (stark_rings_amd/csrc/sparse_matrix.hpp), every instantiation the library dispatches to, so that
// `hipcc -S` takes seconds: tests/test_spgemm_isa.py reads the listing.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only -o spgemm.s tools/ubench/spgemm_isa.hip
#include "../../stark_rings_amd/csrc/stark_lazy.hpp"
#include "../../stark_rings_amd/csrc/sparse_matrix.hpp"
using namespace sr;
#define MOVE(V) template __global__ void spm::move_kernel<V>(uint64_t *, const uint64_t *, const uint32_t *, size_t, size_t, size_t, size_t, unsigned long long *);
MOVE(1)
MOVE(2)
#define SPGEMM(F)                                                                                                                              \
    template __global__ void spm::spgemm_kernel<F>(F::storage *, uint32_t *, const F::storage *, size_t, const F::storage *, size_t, const uint64_t *, \
                                                   const uint32_t *, const uint32_t *, size_t, int);
SPGEMM(Goldilocks)
SPGEMM(BabyBear)
SPGEMM(Stark)
SPGEMM(StarkL)
#define SLOT(SL)                                                                                                                               \
    template __global__ void spm::slot_spgemm_kernel<SL>(SL::K, uint64_t *, uint32_t *, const uint64_t *, size_t, const uint64_t *, size_t,    \
                                                         const uint64_t *, const uint32_t *, const uint32_t *, size_t);
SLOT(SlotG24)
SLOT(SlotB72)
SLOT(SlotFrog)
// count_dead_kernel is not a template: the include instantiates it
