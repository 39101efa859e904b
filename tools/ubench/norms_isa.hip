// The norm kernels alone (stark_rings_amd/csrc/norms.hpp), every instantiation the launcher dispatches to, so that `hipcc -S` takes
// seconds: tests/test_norms_isa.py reads the listing.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only -o norms.s tools/ubench/norms_isa.hip
#include <hip/hip_runtime.h>

#include "../../stark_rings_amd/csrc/norms.hpp"
using namespace sr;
#define NORM(F, W)                                                                                                      \
    template __global__ void norms::wide_kernel<F, W>(uint64_t *, const uint64_t *, size_t, size_t, size_t);           \
    template __global__ void norms::narrow_kernel<F, W>(uint64_t *, const uint64_t *, size_t, size_t, int);            \
    template __global__ void norms::fold_kernel<F, W>(uint64_t *, const uint64_t *, size_t, size_t, int);
#define NORMS(F) NORM(F, 1) NORM(F, 2) NORM(F, 3)
NORMS(Goldilocks)
NORMS(BabyBear)
NORMS(Frog)
NORMS(Stark)
