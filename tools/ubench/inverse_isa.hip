// The batch-inversion kernels alone (stark_rings_amd/csrc/inverse.hpp), every instantiation the library dispatches to, so that
// `hipcc -S` takes seconds: tests/test_inverse_isa.py reads the listing.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only -o inverse.s tools/ubench/inverse_isa.hip
// -DINVERSE_ISA_ALL adds the other chunk lengths that were considered (the counts behind kChunk), which the launcher does not dispatch.
#include "../../stark_rings_amd/csrc/inverse.hpp"
using namespace sr;
#define POW2(F, C, HN)                                                                                                                      \
    template __global__ void inverse::inverse_kernel<F, C, HN>(uint64_t *, const uint64_t *, const uint64_t *, smle::One, size_t, size_t, int, \
                                                               int, unsigned long long *);
#define SLOT(SL, C, HN)                                                                                                                     \
    template __global__ void inverse::slot_inverse_kernel<SL, C, HN>(SL::K, uint64_t *, const uint64_t *, const uint64_t *, smle::One, size_t, \
                                                                     size_t, unsigned long long *);
#define BOTH(M, T, C) M(T, C, false) M(T, C, true)
#define CHOSEN(M, T) M(T, (inverse::kChunk<T, false>), false) M(T, (inverse::kChunk<T, true>), true)
CHOSEN(POW2, Goldilocks) CHOSEN(POW2, BabyBear) CHOSEN(POW2, Stark)
CHOSEN(SLOT, SlotG24) CHOSEN(SLOT, SlotB72) CHOSEN(SLOT, SlotFrog)
#ifdef INVERSE_ISA_ALL
POW2(Goldilocks, 8, true) BOTH(POW2, Goldilocks, 16)
BOTH(POW2, BabyBear, 16)
POW2(Stark, 4, true) BOTH(POW2, Stark, 8)
BOTH(SLOT, SlotG24, 8)
BOTH(SLOT, SlotB72, 4)
BOTH(SLOT, SlotFrog, 8)
#endif
