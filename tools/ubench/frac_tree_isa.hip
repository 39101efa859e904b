// The fraction-tree kernels alone (stark_rings_amd/csrc/frac_tree.hpp), every instantiation the library dispatches to, so that
// `hipcc -S` takes seconds: tests/test_frac_tree_isa.py reads the listing.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only -o frac_tree.s tools/ubench/frac_tree_isa.hip
// -DFRAC_TREE_ISA_ALL adds the kernels one level above each family's bound, which the launcher does not dispatch (the counts behind
// kMaxJ / kSlotMaxJ).
#include "../../stark_rings_amd/csrc/frac_tree.hpp"
using namespace sr;
#define TREE1(F, J, HP)                                                                                                                    \
    template __global__ void ftree::tree_kernel<F, J, HP>(F::storage *, F::storage *, const F::storage *, const F::storage *, smle::One, size_t, \
                                                          int, int, int);
#define SLOT1(SL, J, HP)                                                                                                                   \
    template __global__ void ftree::slot_tree_kernel<SL, J, HP>(SL::K, uint64_t *, uint64_t *, const uint64_t *, const uint64_t *, smle::One,   \
                                                                size_t, int, int);
#define TREE(F, J) TREE1(F, J, true) TREE1(F, J, false)
#define SLOT(SL, J) SLOT1(SL, J, true) SLOT1(SL, J, false)
TREE(Goldilocks, 1) TREE(Goldilocks, 2)
TREE(BabyBear, 1) TREE(BabyBear, 2) TREE(BabyBear, 3)
TREE(Stark, 1) TREE(Stark, 2)
SLOT(SlotG24, 1) SLOT(SlotG24, 2)
SLOT(SlotB72, 1)
SLOT(SlotFrog, 1) SLOT(SlotFrog, 2)
#ifdef FRAC_TREE_ISA_ALL
TREE(Goldilocks, 3)
TREE(Stark, 3)
SLOT(SlotG24, 3)
SLOT(SlotB72, 2)
SLOT(SlotFrog, 3)
#endif
