// The product-tree kernels alone (stark_rings_amd/csrc/prod_tree.hpp), every instantiation the library dispatches to, so that
// `hipcc -S` takes seconds: tests/test_prod_tree_isa.py reads the listing.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only -o prod_tree.s tools/ubench/prod_tree_isa.hip
// -DPROD_TREE_ISA_ALL adds the babybear72 J = 3 kernel the launcher does not dispatch (the count behind kSlotMaxJ).
#include "../../stark_rings_amd/csrc/prod_tree.hpp"
using namespace sr;
#define TREE(F, J) template __global__ void ptree::tree_kernel<F, J>(F::storage *, const F::storage *, smle::One, size_t, int, int, int);
#define SLOT(SL, J) template __global__ void ptree::slot_tree_kernel<SL, J>(SL::K, uint64_t *, const uint64_t *, smle::One, size_t, int, int);
#define TREES(F) TREE(F, 1) TREE(F, 2)
#define SLOTS(SL) SLOT(SL, 1) SLOT(SL, 2)
TREES(Goldilocks) TREE(Goldilocks, 3)
TREES(BabyBear) TREE(BabyBear, 3)
TREES(Stark) TREE(Stark, 3)
SLOTS(SlotG24) SLOT(SlotG24, 3)
SLOTS(SlotB72)
SLOTS(SlotFrog) SLOT(SlotFrog, 3)
#ifdef PROD_TREE_ISA_ALL
SLOT(SlotB72, 3)
#endif
