// The fused fold-and-round kernels of a sum of products alone (stark_rings_amd/csrc/sumcheck_vpoly_fold.hpp), so that `hipcc -S` takes
// minutes rather than the whole library: tests/test_vpoly_fold_isa.py reads the listing.  The launchers themselves are instantiated, so
// the listing holds exactly the kernels the dispatcher can reach -- every (field, table slots) -- and nothing it cannot.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only -o vpoly_fold.s tools/ubench/vpoly_fold_isa.hip
#include "../../stark_rings_amd/csrc/stark_lazy.hpp"
#include "../../stark_rings_amd/csrc/sumcheck_vpoly_fold.hpp"
using namespace sr;
#define LAUNCHER(T)                                                                                                                      \
    template hipError_t vpoly_fold::launch<T>(const sumcheck::Family<T>::K &, const vpoly_fold::Plan &, int, uint64_t *, const vpoly::Tables &,    \
                                              vpoly_fold::Folded, const uint64_t *, int, const vpoly::Term *, int, const uint64_t *, size_t,      \
                                              size_t *, int, bool, uint64_t *, hipStream_t);
#define POW2(F) LAUNCHER(F)
POW2(Goldilocks)
POW2(BabyBear)
POW2(Stark)
#define SLOT(SL) LAUNCHER(SL)
SLOT(SlotG24)
SLOT(SlotB72)
SLOT(SlotFrog)
