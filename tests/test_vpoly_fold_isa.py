"""Static budget of the fused fold-and-round kernels of a sum of products (no GPU): hipcc -S of tools/ubench/vpoly_fold_isa.hip, which
instantiates the launchers of csrc/sumcheck_vpoly_fold.hpp and with them every kernel the dispatcher can reach, and a count of what the
listing holds.  A spill -- the term walk selects registers with a run-time index and the fold unrolls over the table slots, which is
exactly how one happens -- or a register count that costs a wave is a regression the parity tests cannot see.  Only the .amdhsa_*
metadata is read and v_ lines are counted."""
import os
import re
import shutil
import subprocess

import pytest

from test_vpoly_isa import MAX_VGPR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "ubench", "vpoly_fold_isa.hip")
OUT = os.path.join(ROOT, "build_tmp", "vpoly_fold_isa_budget.s")
CSRC = os.path.join(ROOT, "stark_rings_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("sumcheck_vpoly_fold.hpp", "sumcheck_vpoly.hpp", "sumcheck_fold.hpp", "sumcheck.hpp", "mle.hpp",
                                                "fields.hpp", "ntt_generic.hpp", "small_rings.hpp", "small_linalg.hpp", "frog_ring.hpp",
                                                "stark_lazy.hpp")]

# fused kernel (mangled-name fragment: kernel, field, table slots, points of the fused launch) -> (max VALU instructions in the listing:
# what the compiler produced when the kernel was written plus 2 per cent; the VGPR count it gave, pinned).  The one-limb kernels hold
# the 16-byte path and the one-coefficient fallback, both counted.  The kernels of the remaining points, the sum over the records and
# zero_kernel are in the listing too; tests/test_vpoly_isa.py holds them.
BUDGET = {
    "fold_round_kernelINS_10GoldilocksELi4ELi5E":        ( 5447, 222),
    "fold_round_kernelINS_10GoldilocksELi8ELi4E":        ( 6143, 230),
    "fold_round_kernelINS_8BabyBearELi4ELi5E":           ( 2812, 107),
    "fold_round_kernelINS_8BabyBearELi8ELi3E":           ( 3168, 128),
    "fold_round_kernelINS_5StarkELi4ELi2E":              ( 7342, 242),
    "fold_round_kernelINS_5StarkELi8ELi1E":              ( 8754, 239),
    "slot_fold_round_kernelINS_7SlotG24ELi4ELi2E":       ( 5987, 216),
    "slot_fold_round_kernelINS_7SlotG24ELi8ELi1E":       ( 6602, 183),
    "slot_fold_round_kernelINS_7SlotB72ELi4ELi1E":       ( 7223, 212),
    "slot_fold_round_kernelINS_7SlotB72ELi8ELi0E":       ( 8925, 169),
    "slot_fold_round_kernelINS_8SlotFrogELi4ELi1E":      (13562, 186),
    "slot_fold_round_kernelINS_8SlotFrogELi8ELi1E":      (22037, 235),
}
# points of the fused launch of (field, table slots): fused_points_of of csrc/sumcheck_vpoly_fold.hpp
FUSED = {"Goldilocks": {4: 5, 8: 4}, "BabyBear": {4: 5, 8: 3}, "Stark": {4: 2, 8: 1}, "SlotG24": {4: 2, 8: 1}, "SlotB72": {4: 1, 8: 0},
         "SlotFrog": {4: 1, 8: 1}}


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
    frags = [f for f in BUDGET if "%d%sE" % (len(f.split("INS_")[0]), f) in name]
    assert len(frags) == 1, "no budget entry for %s" % name
    return frags[0]


def _field(frag):
    return re.search(r"INS_\d+([A-Za-z0-9]+?)E", frag).group(1)


def test_every_fused_kernel_stays_within_its_register_and_instruction_budget():
    seen = set()
    for name, body, meta in _kernels(_listing(), "10vpoly_fold"):
        frag = _fragment(name)
        seen.add(frag)
        valu = sum(1 for line in body.split("\n") if re.match(r"\s+v_[a-z0-9_]+\s", line))
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", meta).group(1))
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", meta).group(1))
        budget, pinned = BUDGET[frag]
        print("%-52s VALU %5d (budget %5d)  VGPR %3d  scratch %d" % (frag, valu, budget, vgpr, scratch))
        assert scratch == 0, "%s: %d bytes of scratch (spills, or a register array indexed at run time)" % (name, scratch)
        assert vgpr == pinned, "%s: %d VGPRs (pinned %d)" % (name, vgpr, pinned)
        assert vgpr <= MAX_VGPR[_field(frag)], "%s: %d VGPRs (family bound %d)" % (name, vgpr, MAX_VGPR[_field(frag)])
        assert valu <= budget, "%s: %d VALU instructions (budget %d)" % (name, valu, budget)
    assert seen == set(BUDGET), "kernels not found in the listing: %s" % (set(BUDGET) - seen)


def test_no_kernel_of_the_listing_uses_scratch():
    """the round kernels of the remaining points, the sum over the records and zero_kernel as well"""
    n = 0
    for name, _, meta in _kernels(_listing(), "(?:10vpoly_fold|5vpoly|8sumcheck)"):
        n += 1
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", meta).group(1)) == 0, name
    assert n > len(BUDGET)


def test_the_listing_holds_exactly_what_the_dispatcher_reaches():
    """A (field, table slots) pair reaches one fused kernel, of fused_points_of points (the points of a low degree are a run-time
    argument of the same kernel), and for the remaining points the round kernel of sumcheck_vpoly.hpp's points_of.  The instantiation
    file instantiates the launchers, so the two cannot drift."""
    src = open(os.path.join(CSRC, "sumcheck_vpoly_fold.hpp")).read()
    for text in ("if (std::is_same<T, Goldilocks>::value) return slots == 4 ? 5 : 4;",
                 "if (std::is_same<T, BabyBear>::value) return slots == 4 ? 5 : 3;",
                 "if (std::is_same<T, SlotB72>::value) return slots == 4 ? 1 : 0;",
                 "return vpoly::points_of<T>(slots);"):
        assert text in src, text
    want = set()
    for field, per in FUSED.items():
        kernel = "slot_fold_round_kernel" if field.startswith("Slot") else "fold_round_kernel"
        for slots, p in per.items():
            want.add((kernel, field, slots, p))
    got = set()
    for frag in BUDGET:
        m = re.match(r"(\w+?_kernel)INS_\d+(\w+?)ELi(\d)ELi(\d)E", frag)
        got.add((m.group(1), m.group(2), int(m.group(3)), int(m.group(4))))
    assert got == want, (got - want, want - got)
    isa = open(SRC).read()
    for line in ("POW2(Goldilocks)", "POW2(BabyBear)", "POW2(Stark)", "SLOT(SlotG24)", "SLOT(SlotB72)", "SLOT(SlotFrog)"):
        assert line in isa, line
    # the kernels of the remaining points: the round kernels with pairs where the fused launch can leave a point, nothing else of vpoly
    from test_vpoly_isa import POINTS
    rest = set()
    for name, _, _ in _kernels(_listing(), "5vpoly"):
        m = re.search(r"(\w*round_kernel)INS_\d+(\w+?)ELi(\d)ELi(\d)ELb([01])E", name)
        rest.add((m.group(2), int(m.group(3)), int(m.group(4)), int(m.group(5))))
    assert rest == {(field, slots, p, 1) for field, per in POINTS.items() for slots, p in per.items() if FUSED[field][slots] < 5}, rest
