// The weighted round kernels and the weighted fused fold-and-round kernels alone (stark_rings_amd/csrc/sumcheck_weighted.hpp), so that
// `hipcc -S` takes minutes rather than the whole library: tests/test_wsumcheck_isa.py reads the listing.  The launchers themselves are
// instantiated, so the listing holds exactly the kernels the dispatcher can reach -- every (field, table slots) -- and nothing it cannot.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only -o wsumcheck.s tools/ubench/wsumcheck_isa.hip
#include "../../stark_rings_amd/csrc/stark_lazy.hpp"
#include "../../stark_rings_amd/csrc/sumcheck_weighted.hpp"
using namespace sr;
#define LAUNCHER(T)                                                                                                                          \
    template hipError_t wsumcheck::launch<T>(const sumcheck::Family<T>::K &, const wsumcheck::Plan &, int, uint64_t *, const uint64_t *,          \
                                             const vpoly::Tables &, int, const vpoly::Term *, int, const uint64_t *, size_t, int, bool,           \
                                             uint64_t *, hipStream_t);                                                                            \
    template hipError_t wsumcheck::launch_fold<T>(const sumcheck::Family<T>::K &, const wsumcheck::Plan &, int, uint64_t *, const uint64_t *,     \
                                                  const vpoly::Tables &, vpoly_fold::Folded, const uint64_t *, int, const vpoly::Term *, int,     \
                                                  const uint64_t *, size_t, size_t *, int, bool, uint64_t *, hipStream_t);
#define POW2(F) LAUNCHER(F)
POW2(Goldilocks)
POW2(BabyBear)
POW2(Stark)
#define SLOT(SL) LAUNCHER(SL)
SLOT(SlotG24)
SLOT(SlotB72)
SLOT(SlotFrog)
