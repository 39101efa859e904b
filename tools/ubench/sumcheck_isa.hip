// The sum-check round kernels alone (stark_rings_amd/csrc/sumcheck.hpp), so that `hipcc -S` takes a minute rather than the whole
// library: tests/test_sumcheck_isa.py reads the listing.  The launchers themselves are instantiated, so the listing holds exactly the
// kernels the dispatcher can reach -- every (field, d, points per launch) -- and nothing it cannot.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only -o sumcheck.s tools/ubench/sumcheck_isa.hip
#include "../../stark_rings_amd/csrc/stark_lazy.hpp"
#include "../../stark_rings_amd/csrc/sumcheck.hpp"
using namespace sr;
#define LAUNCHER(T)                                                                                                                   \
    template hipError_t sumcheck::launch<T>(const sumcheck::Family<T>::K &, const sumcheck::Plan &, int, uint64_t *, const sumcheck::Tables &, int, \
                                            size_t, int, bool, uint64_t *, hipStream_t);
#define POW2(F) LAUNCHER(F)
POW2(Goldilocks)
POW2(BabyBear)
POW2(Stark)
#define SLOT(SL) LAUNCHER(SL)
SLOT(SlotG24)
SLOT(SlotB72)
SLOT(SlotFrog)
