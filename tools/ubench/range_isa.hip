// The range-check round kernels alone (stark_rings_amd/csrc/range_check.hpp), so that `hipcc -S` takes minutes rather than the whole
// library: tests/test_range_isa.py reads the listing.  The launcher itself is instantiated, so the listing holds exactly the kernels
// the dispatcher can reach -- one per family, of points_of points -- and nothing it cannot.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only -o range.s tools/ubench/range_isa.hip
#include "../../stark_rings_amd/csrc/stark_lazy.hpp"
#include "../../stark_rings_amd/csrc/range_check.hpp"
using namespace sr;
#define LAUNCHER(T)                                                                                                                     \
    template hipError_t range::launch<T>(const sumcheck::Family<T>::K &, const range::Plan &, int, uint64_t *, const uint64_t *,            \
                                         const range::Tables &, int, int, const uint64_t *, size_t, int, bool, uint64_t *, hipStream_t);
#define POW2(F) LAUNCHER(F)
POW2(Goldilocks)
POW2(BabyBear)
POW2(Stark)
#define SLOT(SL) LAUNCHER(SL)
SLOT(SlotG24)
SLOT(SlotB72)
SLOT(SlotFrog)
