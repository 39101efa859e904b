"""Static budget of the weighted round kernels and the weighted fused fold-and-round kernels (no GPU): hipcc -S of
tools/ubench/wsumcheck_isa.hip, which instantiates the launchers of csrc/sumcheck_weighted.hpp and with them every kernel the dispatcher
can reach, and a count of what the listing holds.  A spill -- the term walk selects registers with a run-time index, the fold unrolls
over the table slots and the weight is live across both -- or a register count that costs a wave is a regression the parity tests
cannot see.  Only the .amdhsa_* metadata is read and v_ lines are counted."""
import os
import re
import shutil
import subprocess

import pytest

from test_vpoly_isa import MAX_VGPR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "ubench", "wsumcheck_isa.hip")
OUT = os.path.join(ROOT, "build_tmp", "wsumcheck_isa_budget.s")
CSRC = os.path.join(ROOT, "stark_rings_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("sumcheck_weighted.hpp", "sumcheck_vpoly_fold.hpp", "sumcheck_vpoly.hpp", "sumcheck_fold.hpp",
                                                "sumcheck.hpp", "mle.hpp", "fields.hpp", "ntt_generic.hpp", "small_rings.hpp",
                                                "small_linalg.hpp", "frog_ring.hpp", "stark_lazy.hpp")]

# kernel (mangled-name fragment: kernel, field, table slots, points of a launch) -> (max VALU instructions in the listing: what the
# compiler produced when the kernel was written plus 2 per cent; the VGPR count it gave, pinned).  The one-limb kernels hold the
# 16-byte path and the one-coefficient fallback, both counted.
BUDGET = {
    "round_kernelINS_10GoldilocksELi4ELi5E":             ( 4901, 203),
    "round_kernelINS_10GoldilocksELi8ELi5E":             ( 5796, 235),
    "fold_round_kernelINS_10GoldilocksELi4ELi5E":        ( 5679, 221),
    "fold_round_kernelINS_10GoldilocksELi8ELi4E":        ( 6304, 232),
    "round_kernelINS_8BabyBearELi4ELi5E":                ( 2382,  77),
    "round_kernelINS_8BabyBearELi8ELi5E":                ( 3000, 105),
    "fold_round_kernelINS_8BabyBearELi4ELi5E":           ( 2930, 106),
    "fold_round_kernelINS_8BabyBearELi8ELi3E":           ( 3377, 128),
    "round_kernelINS_5StarkELi4ELi4E":                   ( 8843, 224),
    "round_kernelINS_5StarkELi8ELi1E":                   ( 3301, 202),
    "fold_round_kernelINS_5StarkELi4ELi2E":              ( 7704, 248),
    "fold_round_kernelINS_5StarkELi8ELi1E":              ( 9500, 237),
    "slot_round_kernelINS_7SlotG24ELi4ELi3E":            ( 6167, 254),
    "slot_round_kernelINS_7SlotG24ELi8ELi1E":            ( 2416, 169),
    "slot_fold_round_kernelINS_7SlotG24ELi4ELi2E":       ( 6446, 217),
    "slot_fold_round_kernelINS_7SlotG24ELi8ELi1E":       ( 6821, 183),
    "slot_round_kernelINS_7SlotB72ELi4ELi1E":            ( 3538, 190),
    "slot_round_kernelINS_7SlotB72ELi8ELi1E":            ( 4086, 252),
    "slot_fold_round_kernelINS_7SlotB72ELi4ELi1E":       ( 7634, 222),
    "slot_fold_round_kernelINS_7SlotB72ELi8ELi0E":       ( 8926, 169),
    "slot_round_kernelINS_8SlotFrogELi4ELi1E":           ( 6466, 169),
    "slot_round_kernelINS_8SlotFrogELi8ELi1E":           ( 6878, 208),
    "slot_fold_round_kernelINS_8SlotFrogELi4ELi1E":      (14483, 188),
    "slot_fold_round_kernelINS_8SlotFrogELi8ELi1E":      (22945, 237),
}
# points per launch of the weighted round kernels / of the fused launch of (field, table slots): points_of and fused_points_of of
# csrc/sumcheck_weighted.hpp -- per family and slot count the largest number within the bound without scratch
POINTS = {"Goldilocks": {4: 5, 8: 5}, "BabyBear": {4: 5, 8: 5}, "Stark": {4: 4, 8: 1}, "SlotG24": {4: 3, 8: 1}, "SlotB72": {4: 1, 8: 1},
          "SlotFrog": {4: 1, 8: 1}}
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


def test_every_weighted_kernel_stays_within_its_register_and_instruction_budget():
    seen = set()
    for name, body, meta in _kernels(_listing(), "9wsumcheck"):
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
    """the sum over the records and zero_kernel as well; no unweighted sum-check kernel is in the listing"""
    n = 0
    for name, _, meta in _kernels(_listing(), "(?:9wsumcheck|8sumcheck)"):
        n += 1
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", meta).group(1)) == 0, name
    assert n > len(BUDGET)
    assert not list(_kernels(_listing(), "(?:5vpoly|10vpoly_fold)")), "an unweighted kernel is reached from the weighted launchers"


def test_the_listing_holds_exactly_what_the_dispatcher_reaches():
    """A (field, table slots) pair reaches one weighted round kernel, of points_of points (fewer are a run-time argument of the same
    kernel), and one fused kernel, of fused_points_of points.  The instantiation file instantiates the launchers, so the two cannot
    drift; the tables in the header file are pinned here."""
    src = open(os.path.join(CSRC, "sumcheck_weighted.hpp")).read()
    for text in ("if (std::is_same<T, Stark>::value) return slots == 4 ? 4 : 1;", "if (std::is_same<T, SlotG24>::value) return slots == 4 ? 3 : 1;",
                 "return vpoly::points_of<T>(slots);", "return vpoly_fold::fused_points_of<T>(slots);"):
        assert text in src, text
    want = set()
    for field in POINTS:
        slot = field.startswith("Slot")
        for slots in (4, 8):
            want.add(("slot_round_kernel" if slot else "round_kernel", field, slots, POINTS[field][slots]))
            want.add(("slot_fold_round_kernel" if slot else "fold_round_kernel", field, slots, FUSED[field][slots]))
    got = set()
    for frag in BUDGET:
        m = re.match(r"(\w+?_kernel)INS_\d+(\w+?)ELi(\d)ELi(\d)E", frag)
        got.add((m.group(1), m.group(2), int(m.group(3)), int(m.group(4))))
    assert got == want, (got - want, want - got)
    isa = open(SRC).read()
    for line in ("POW2(Goldilocks)", "POW2(BabyBear)", "POW2(Stark)", "SLOT(SlotG24)", "SLOT(SlotB72)", "SLOT(SlotFrog)"):
        assert line in isa, line
