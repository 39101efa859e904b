// The weighted round kernels and fused fold-and-round kernels with integer-column operands alone
// (stark_rings_amd/csrc/sumcheck_index.hpp), so that `hipcc -S` takes minutes rather than the whole library:
// tests/test_isumcheck_isa.py reads the listing.  The launchers themselves are instantiated, so the listing holds exactly the kernels
// of namespace isumcheck the dispatcher can reach -- every (field, operand slots) -- and nothing it cannot.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only -o isumcheck.s tools/ubench/isumcheck_isa.hip
#include "../../stark_rings_amd/csrc/stark_lazy.hpp"
#include "../../stark_rings_amd/csrc/sumcheck_index.hpp"
using namespace sr;
#define LAUNCHER(T)                                                                                                                          \
    template hipError_t isumcheck::launch<T>(const sumcheck::Family<T>::K &, const isumcheck::Plan &, int, uint64_t *, const uint64_t *,          \
                                             const vpoly::Tables &, int, const isumcheck::ColumnArgs &, const vpoly::Term *, int,                \
                                             const uint64_t *, size_t, int, bool, uint64_t *, hipStream_t);                                       \
    template hipError_t isumcheck::launch_fold<T>(const sumcheck::Family<T>::K &, const isumcheck::Plan &, int, uint64_t *, const uint64_t *,     \
                                                  const vpoly::Tables &, vpoly_fold::Folded, const uint64_t *, int,                               \
                                                  const isumcheck::ColumnArgs &, const vpoly::Term *, int, const uint64_t *, size_t, size_t *,    \
                                                  int, bool, uint64_t *, hipStream_t);
#define POW2(F) LAUNCHER(F)
POW2(Goldilocks)
POW2(BabyBear)
POW2(Stark)
#define SLOT(SL) LAUNCHER(SL)
SLOT(SlotG24)
SLOT(SlotB72)
SLOT(SlotFrog)
