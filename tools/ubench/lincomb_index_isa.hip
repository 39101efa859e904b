// The kernels of stark_rings_amd/csrc/lincomb_index.hpp alone, every instantiation the library dispatches to, so that `hipcc -S` takes
// seconds: tests/test_lincomb_index_isa.py reads the listing.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only -o lincomb_index.s tools/ubench/lincomb_index_isa.hip
// -DLINCOMB_INDEX_ISA_ALL adds the kernels one output above each family's bounds, which the launcher does not dispatch (the counts
// behind kRegOutputs / kRunOutputs).
#include "../../stark_rings_amd/csrc/lincomb_index.hpp"
using namespace sr;
#define POW2(F, M, REG) \
    template __global__ void lincomb_index::lincomb_index_kernel<F, M, REG>(lincomb_index::Args, int, int, size_t, int, int, size_t);
#define SLOT(SL, M, REG) \
    template __global__ void lincomb_index::slot_lincomb_index_kernel<SL, M, REG>(SL::K, lincomb_index::Args, int, int, size_t, size_t);
POW2(Goldilocks, 1, true) POW2(Goldilocks, 2, true)
POW2(Goldilocks, 1, false) POW2(Goldilocks, 2, false) POW2(Goldilocks, 3, false)
POW2(BabyBear, 1, true) POW2(BabyBear, 2, true)
POW2(BabyBear, 1, false) POW2(BabyBear, 2, false) POW2(BabyBear, 3, false) POW2(BabyBear, 4, false)
POW2(Stark, 1, false)
SLOT(SlotG24, 1, true) SLOT(SlotG24, 1, false)
SLOT(SlotB72, 1, false)
SLOT(SlotFrog, 1, false)
template __global__ void lincomb_index::index_count_kernel<true>(unsigned long long *, const uint64_t *, size_t, size_t, unsigned long long *);
template __global__ void lincomb_index::index_count_kernel<false>(unsigned long long *, const uint64_t *, size_t, size_t, unsigned long long *);
#ifdef LINCOMB_INDEX_ISA_ALL
POW2(Goldilocks, 4, false)
POW2(Stark, 1, true) POW2(Stark, 2, false)
SLOT(SlotG24, 2, true) SLOT(SlotG24, 2, false)
SLOT(SlotB72, 2, false)
SLOT(SlotFrog, 1, true) SLOT(SlotFrog, 2, false)
#endif
