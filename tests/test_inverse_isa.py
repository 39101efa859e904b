"""Static budget of the batch-inversion kernels (no GPU): hipcc -S of tools/ubench/inverse_isa.hip, which instantiates every kernel the
launcher dispatches to (csrc/inverse.hpp: kChunk per family, with and without numerators), and the resource metadata of the listing:
the register count that keeps four waves per SIMD, and no scratch.  The chunk lengths were chosen by these figures; a kernel that grows
past them costs a wave or spills, which the parity tests cannot see."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "ubench", "inverse_isa.hip")
OUT = os.path.join(ROOT, "build_tmp", "inverse_isa_budget.s")
CSRC = os.path.join(ROOT, "stark_rings_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("inverse.hpp", "lincomb.hpp", "sparse_mle.hpp", "sumcheck.hpp", "mle.hpp", "fields.hpp",
                                                "ntt_generic.hpp", "small_rings.hpp", "small_linalg.hpp", "frog_ring.hpp")]
sys.path.insert(0, os.path.join(ROOT, "tools"))
import model_inverse as MI  # noqa: E402

# every kernel is __launch_bounds__(256): four waves per workgroup.  128 VGPRs keep four waves on each SIMD (512 registers per lane).
MAX_VGPR = 128
# kernel (mangled-name fragment: the family, Li<C>: the chunk, Lb<has numerators>) -> VGPRs when the kernel was written
WRITTEN = {
    "inverse_kernelINS_10GoldilocksELi8ELb0E": 128, "inverse_kernelINS_10GoldilocksELi4ELb1E": 82,
    "inverse_kernelINS_8BabyBearELi8ELb0E": 94, "inverse_kernelINS_8BabyBearELi8ELb1E": 94,
    "inverse_kernelINS_5StarkELi4ELb0E": 124, "inverse_kernelINS_5StarkELi2ELb1E": 96,
    "slot_inverse_kernelINS_7SlotG24ELi4ELb0E": 92, "slot_inverse_kernelINS_7SlotG24ELi4ELb1E": 96,
    "slot_inverse_kernelINS_7SlotB72ELi2ELb0E": 125, "slot_inverse_kernelINS_7SlotB72ELi2ELb1E": 128,
    "slot_inverse_kernelINS_8SlotFrogELi4ELb0E": 120, "slot_inverse_kernelINS_8SlotFrogELi4ELb1E": 120,
}
FAMILY = {"GoldilocksE": "goldilocks", "BabyBearE": "babybear", "StarkE": "stark", "SlotG24E": "goldilocks24", "SlotB72E": "babybear72",
          "SlotFrogE": "frog16"}


def _listing():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    if not hipcc:
        pytest.skip("hipcc not found")
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in DEPS):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", OUT, SRC], check=True,
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    return open(OUT).read()


def _kernels(s):
    for m in re.finditer(r"\.amdhsa_kernel (_ZN2sr7inverse\w+)\n(.*?)\.end_amdhsa_kernel", s, flags=re.S):
        yield m.group(1), m.group(2)


def test_every_dispatched_kernel_keeps_four_waves_and_has_no_scratch():
    seen = set()
    for name, meta in _kernels(_listing()):
        frags = [f for f in WRITTEN if f in name]
        assert len(frags) == 1, "no entry for %s" % name
        seen.add(frags[0])
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", meta).group(1))
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", meta).group(1))
        print("%-46s VGPR %3d (written %3d)  scratch %d" % (frags[0], vgpr, WRITTEN[frags[0]], scratch))
        assert scratch == 0, "%s: %d bytes of scratch (spills)" % (name, scratch)
        assert vgpr <= MAX_VGPR, "%s: %d VGPRs (budget %d: four waves per SIMD)" % (name, vgpr, MAX_VGPR)
    assert seen == set(WRITTEN), "kernels not found in the listing: %s" % (set(WRITTEN) - seen)


def test_the_table_holds_exactly_the_chunks_the_plan_reports():
    """one kernel per (family, with / without numerators), at the chunk csrc/inverse.hpp: kChunk, tools/model_inverse.py: CHOSEN and
    sr_inverse_plan all name"""
    import ctypes

    from stark_rings_amd import _lib

    lib = _lib.load()
    for frag in WRITTEN:
        fam = FAMILY[[f for f in FAMILY if "INS_%d%s" % (len(f) - 1, f) in frag][0]]
        c, hn = (int(x) for x in re.search(r"ELi(\d+)ELb([01])E$", frag).groups())
        assert MI.CHOSEN[fam][hn] == c, frag
        work, launches, chunk = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_size_t()
        assert lib.sr_inverse_plan(MI.RING_IDS[fam], 4 if MI.RING_IDS[fam] <= 2 else 0, 5, hn, ctypes.byref(work), ctypes.byref(launches),
                                   ctypes.byref(chunk)) == 0
        assert (work.value, launches.value, chunk.value) == (0, 1, c), frag
    assert len(WRITTEN) == 2 * len(FAMILY)
