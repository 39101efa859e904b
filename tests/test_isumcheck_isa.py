"""Static budget of the weighted round kernels and fused fold-and-round kernels with integer-column operands (no GPU): hipcc -S of
tools/ubench/isumcheck_isa.hip, which instantiates the launchers of csrc/sumcheck_index.hpp and with them every kernel of namespace
isumcheck the dispatcher can reach.  Every such kernel is in the listing, has no scratch and stays within its family's register bound;
the plan dispatches nothing the listing lacks.  Only the .amdhsa_* metadata of those kernels is read."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from stark_rings_amd import _lib
from test_vpoly_isa import MAX_VGPR
from test_wsumcheck_isa import FUSED, POINTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "ubench", "isumcheck_isa.hip")
OUT = os.path.join(ROOT, "build_tmp", "isumcheck_isa_budget.s")
CSRC = os.path.join(ROOT, "stark_rings_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("sumcheck_index.hpp", "lincomb_index.hpp", "lincomb.hpp", "decompose.hpp", "sumcheck_weighted.hpp",
                                                "sumcheck_vpoly_fold.hpp", "sumcheck_vpoly.hpp", "sumcheck_fold.hpp", "sumcheck.hpp", "mle.hpp",
                                                "fields.hpp", "ntt_generic.hpp", "small_rings.hpp", "small_linalg.hpp", "frog_ring.hpp",
                                                "stark_lazy.hpp")]
RING_ID = {"Goldilocks": 0, "BabyBear": 1, "Stark": 2, "SlotG24": 3, "SlotB72": 4, "SlotFrog": 5}
# The kernels hold the points of their weighted siblings (the launchers of csrc/sumcheck_index.hpp instantiate them at
# wsumcheck::points_of / fused_points_of): a column slot is embedded into the registers a table slot is loaded into.


def _listing():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    if not hipcc:
        pytest.skip("hipcc not found")
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in DEPS):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", OUT, SRC], check=True,
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1800)
    return open(OUT).read()


def _kernels(s):
    """(kernel, field, slots, points) -> (VGPRs, scratch bytes) of every kernel of namespace isumcheck in the listing"""
    found = {}
    for m in re.finditer(r"\.amdhsa_kernel _ZN2sr9isumcheck\d+(\w+?_kernel)INS_\d+([A-Za-z0-9]+?)ELi(\d)ELi(\d)E\w*(.*?)\.end_amdhsa_kernel", s, flags=re.S):
        meta = m.group(5)
        key = (m.group(1), m.group(2), int(m.group(3)), int(m.group(4)))
        assert key not in found, key
        found[key] = (int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", meta).group(1)),
                      int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", meta).group(1)))
    return found


def _want():
    want = set()
    for field in POINTS:
        slot = field.startswith("Slot")
        for slots in (4, 8):
            want.add(("slot_round_kernel" if slot else "round_kernel", field, slots, POINTS[field][slots]))
            want.add(("slot_fold_round_kernel" if slot else "fold_round_kernel", field, slots, FUSED[field][slots]))
    return want


def test_the_listing_holds_exactly_the_kernels_the_launcher_reaches():
    found = _kernels(_listing())
    assert set(found) == _want(), (set(found) - _want(), _want() - set(found))
    isa = open(SRC).read()
    for line in ("POW2(Goldilocks)", "POW2(BabyBear)", "POW2(Stark)", "SLOT(SlotG24)", "SLOT(SlotB72)", "SLOT(SlotFrog)"):
        assert line in isa, line


def test_every_kernel_has_no_scratch_and_stays_within_its_family_register_bound():
    for key, (vgpr, scratch) in sorted(_kernels(_listing()).items()):
        print("%-24s %-10s slots %d points %d  VGPR %3d  scratch %d" % (key + (vgpr, scratch)))
        assert scratch == 0, "%s: %d bytes of scratch (spills, or a register array indexed at run time)" % (key, scratch)
        assert vgpr <= MAX_VGPR[key[1]], "%s: %d VGPRs (family bound %d)" % (key, vgpr, MAX_VGPR[key[1]])


def test_the_plan_dispatches_nothing_the_listing_lacks():
    """the launches a plan counts are those of kernels with the listing's points: one launch per chunk of the message's points, the fused
    launch and the weighted round kernels for the rest, plus the sum over the records where there are several"""
    found, lib = _kernels(_listing()), _lib.load()
    work, launches = ctypes.c_size_t(), ctypes.c_int()
    for field, ring in RING_ID.items():
        slot = field.startswith("Slot")
        for K, J in ((1, 1), (0, 4), (3, 5), (0, 8)):
            slots = 4 if K + J <= 4 else 8
            per = [p for (kern, f, s, p) in found if f == field and s == slots and kern == ("slot_round_kernel" if slot else "round_kernel")]
            fused = [p for (kern, f, s, p) in found if f == field and s == slots and kern.endswith("fold_round_kernel")]
            assert len(per) == 1 and len(fused) == 1, (field, slots)
            for degree in (1, 2, 3, 4):
                for nv in (2, 12):
                    assert lib.sr_vpoly_iwround_plan(ring, 0 if slot else 4, nv, K, J, 2, degree, 0, 0, ctypes.byref(work), ctypes.byref(launches)) == 0
                    chunks = -(-(degree + 1) // min(per[0], degree + 1))
                    assert launches.value == chunks + (1 if work.value else 0), (field, K, J, degree, nv)
                    assert lib.sr_vpoly_iwround_plan(ring, 0 if slot else 4, nv, K, J, 2, degree, 0, 1, ctypes.byref(work), ctypes.byref(launches)) == 0
                    rest = degree + 1 - min(fused[0], degree + 1)
                    chunks = 1 + -(-rest // min(POINTS[field][slots], degree + 1))
                    assert launches.value == chunks + (1 if work.value else 0), (field, K, J, degree, nv)
