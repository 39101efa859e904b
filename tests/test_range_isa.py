"""Static budget of the range-check round kernels (no GPU): hipcc -S of tools/ubench/range_isa.hip, which instantiates the launcher of
csrc/range_check.hpp and with it every kernel the dispatcher can reach, and a count of what the listing holds.  A spill -- the points of
a launch are unrolled, each with its own lazy sums -- or a register count beyond the family's bound is a regression the parity tests
cannot see.  Only the .amdhsa_* metadata is read and v_ lines are counted."""
import os
import re
import shutil
import subprocess

import pytest

from test_vpoly_isa import MAX_VGPR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "ubench", "range_isa.hip")
OUT = os.path.join(ROOT, "build_tmp", "range_isa_budget.s")
CSRC = os.path.join(ROOT, "stark_rings_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("range_check.hpp", "lincomb.hpp", "decompose.hpp", "sumcheck_weighted.hpp", "sumcheck_vpoly_fold.hpp",
                                                "sumcheck_vpoly.hpp", "sumcheck_fold.hpp", "sumcheck.hpp", "mle.hpp", "fields.hpp",
                                                "ntt_generic.hpp", "small_rings.hpp", "small_linalg.hpp", "frog_ring.hpp", "stark_lazy.hpp")]

# kernel (mangled-name fragment: kernel, field, points of a launch) -> (max VALU instructions in the listing: what the compiler produced
# when the kernel was written plus 2 per cent; the VGPR count it gave, pinned).  The one-limb kernels hold the 16-byte path and the
# one-coefficient fallback, both counted.
BUDGET = {
    "round_kernelINS_10GoldilocksELi7E":      (5126, 248),
    "round_kernelINS_8BabyBearELi8E":         (2610,  90),
    "round_kernelINS_5StarkELi3E":            (4452, 246),
    "slot_round_kernelINS_7SlotG24ELi2E":     (3015, 220),
    "slot_round_kernelINS_7SlotB72ELi2E":     (4698, 214),
    "slot_round_kernelINS_8SlotFrogELi2E":    (8661, 244),
}
# points per launch: points_of of csrc/range_check.hpp -- per family the largest number within the bound without scratch
POINTS = {"Goldilocks": 7, "BabyBear": 8, "Stark": 3, "SlotG24": 2, "SlotB72": 2, "SlotFrog": 2}


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


def _kernels(s, namespace):
    for m in re.finditer(r"^(_ZN2sr%s\w+):.*?\n(.*?)\.Lfunc_end" % namespace, s, flags=re.S | re.M):
        name, body = m.group(1), m.group(2)
        meta = s[s.index(".amdhsa_kernel " + name):]
        yield name, body, meta[:meta.index(".end_amdhsa_kernel")]


def _fragment(name):
    frags = [f for f in BUDGET if "%d%s" % (len(f.split("INS_")[0]), f) in name]
    assert len(frags) == 1, "no budget entry for %s" % name
    return frags[0]


def _field(frag):
    return re.search(r"INS_\d+([A-Za-z0-9]+?)E", frag).group(1)


def test_every_range_kernel_stays_within_its_register_and_instruction_budget():
    seen = set()
    for name, body, meta in _kernels(_listing(), "5range"):
        frag = _fragment(name)
        seen.add(frag)
        valu = sum(1 for line in body.split("\n") if re.match(r"\s+v_[a-z0-9_]+\s", line))
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", meta).group(1))
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", meta).group(1))
        budget, pinned = BUDGET[frag]
        print("%-44s VALU %5d (budget %5d)  VGPR %3d  scratch %d" % (frag, valu, budget, vgpr, scratch))
        assert scratch == 0, "%s: %d bytes of scratch (spills, or a register array indexed at run time)" % (name, scratch)
        assert vgpr == pinned, "%s: %d VGPRs (pinned %d)" % (name, vgpr, pinned)
        assert vgpr <= MAX_VGPR[_field(frag)], "%s: %d VGPRs (family bound %d)" % (name, vgpr, MAX_VGPR[_field(frag)])
        assert valu <= budget, "%s: %d VALU instructions (budget %d)" % (name, valu, budget)
    assert seen == set(BUDGET), "kernels not found in the listing: %s" % (set(BUDGET) - seen)


def test_no_kernel_of_the_listing_uses_scratch():
    """the sum over the records and zero_kernel as well; no other sum-check kernel is in the listing"""
    n = 0
    for name, _, meta in _kernels(_listing(), "(?:5range|8sumcheck)"):
        n += 1
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", meta).group(1)) == 0, name
    assert n > len(BUDGET)
    assert not list(_kernels(_listing(), "(?:5vpoly|10vpoly_fold|9wsumcheck|7lincomb)")), "another family's kernel is reached from the range launcher"


def test_the_listing_holds_exactly_what_the_dispatcher_reaches():
    """A family reaches one kernel, of points_of points (fewer are a run-time argument of the same kernel, and so are the bound and the
    number of tables).  The instantiation file instantiates the launcher, so the two cannot drift; the table in the header file is
    pinned here."""
    src = open(os.path.join(CSRC, "range_check.hpp")).read()
    for text in ("if (std::is_same<T, Goldilocks>::value) return 7;", "if (std::is_same<T, BabyBear>::value) return 8;",
                 "if (std::is_same<T, Stark>::value) return 3;", "return 2;  // goldilocks24"):
        assert text in src, text
    want = {("slot_round_kernel" if f.startswith("Slot") else "round_kernel", f, n) for f, n in POINTS.items()}
    got = set()
    for frag in BUDGET:
        m = re.match(r"(\w+?_kernel)INS_\d+(\w+?)ELi(\d+)E", frag)
        got.add((m.group(1), m.group(2), int(m.group(3))))
    assert got == want, (got - want, want - got)
    isa = open(SRC).read()
    for line in ("POW2(Goldilocks)", "POW2(BabyBear)", "POW2(Stark)", "SLOT(SlotG24)", "SLOT(SlotB72)", "SLOT(SlotFrog)"):
        assert line in isa, line
