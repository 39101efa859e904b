// The fused fold-and-round kernels alone (stark_rings_amd/csrc/sumcheck_fold.hpp), so that `hipcc -S` takes a minute rather than the
// whole library: tests/test_sumcheck_fold_isa.py reads the listing.  The launchers themselves are instantiated, so the listing holds
// exactly the kernels the dispatcher can reach -- every (field, d) -- and nothing it cannot.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only -o sumcheck_fold.s tools/ubench/sumcheck_fold_isa.hip
#include "../../stark_rings_amd/csrc/stark_lazy.hpp"
#include "../../stark_rings_amd/csrc/sumcheck_fold.hpp"
using namespace sr;
#define LAUNCHER(T)                                                                                                                       \
    template hipError_t sumcheck_fold::launch<T>(const sumcheck::Family<T>::K &, const sumcheck_fold::Plan &, int, uint64_t *, const sumcheck::Tables &, \
                                                 sumcheck_fold::Folded, const uint64_t *, int, size_t, size_t *, int, bool, uint64_t *, hipStream_t);
#define POW2(F) LAUNCHER(F)
POW2(Goldilocks)
POW2(BabyBear)
POW2(Stark)
#define SLOT(SL) LAUNCHER(SL)
SLOT(SlotG24)
SLOT(SlotB72)
SLOT(SlotFrog)
