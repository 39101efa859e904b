"""Static budget of the sum-of-products round kernels (no GPU): hipcc -S of tools/ubench/vpoly_isa.hip, which instantiates the launchers
of csrc/sumcheck_vpoly.hpp and with them every kernel the dispatcher can reach, and a count of what the listing holds.  A spill -- the
term walk selects registers with a runtime index, which is exactly how one happens -- or a register count that costs a wave is a
regression the parity tests cannot see.  Only the .amdhsa_* metadata is read, v_ lines are counted, and the 16-byte non-temporal
loads of the one-limb kernels."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "ubench", "vpoly_isa.hip")
OUT = os.path.join(ROOT, "build_tmp", "vpoly_isa_budget.s")
CSRC = os.path.join(ROOT, "stark_rings_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("sumcheck_vpoly.hpp", "sumcheck.hpp", "mle.hpp", "fields.hpp", "ntt_generic.hpp",
                                                "small_rings.hpp", "small_linalg.hpp", "frog_ring.hpp", "stark_lazy.hpp")]

# Every kernel is __launch_bounds__(256): four waves per workgroup, 512 registers per lane on a SIMD.  Bound per family:
#   BabyBear            128: four waves per SIMD with all five points over eight table slots
#   every other field   256: two waves per SIMD (lo / hi of four or eight table slots beside the lazy sums of the launch's points)
MAX_VGPR = {"BabyBear": 128, "Goldilocks": 256, "Stark": 256, "SlotG24": 256, "SlotB72": 256, "SlotFrog": 256, "Frog": 256, None: 32}
# kernel (mangled-name fragment: kernel, field, table slots, points per launch, round / plain sum) -> (max VALU instructions in the
# listing: what the compiler produced when the kernel was written plus 2 per cent; the VGPR count it gave, pinned).  The one-limb round
# kernels hold the 16-byte path and the one-coefficient fallback, both counted.
BUDGET = {
    "zero_kernel":                                       (   12,   6),
    "round_kernelINS_10GoldilocksELi4ELi1ELb0E":         (  965,  70),
    "round_kernelINS_10GoldilocksELi4ELi5ELb1E":         ( 4668, 201),
    "round_kernelINS_10GoldilocksELi8ELi1ELb0E":         ( 1112,  87),
    "round_kernelINS_10GoldilocksELi8ELi5ELb1E":         ( 5556, 233),
    "sum_groups_kernelINS_10GoldilocksE":                (   78,  34),
    "round_kernelINS_8BabyBearELi4ELi1ELb0E":            (  501,  44),
    "round_kernelINS_8BabyBearELi4ELi5ELb1E":            ( 2275,  75),
    "round_kernelINS_8BabyBearELi8ELi1ELb0E":            (  587,  52),
    "round_kernelINS_8BabyBearELi8ELi5ELb1E":            ( 2872, 102),
    "sum_groups_kernelINS_8BabyBearE":                   (   63,  23),
    "round_kernelINS_5StarkELi4ELi1ELb0E":               ( 1698, 106),
    "round_kernelINS_5StarkELi4ELi2ELb1E":               ( 4275, 180),
    "round_kernelINS_5StarkELi8ELi1ELb0E":               ( 1853, 138),
    "round_kernelINS_5StarkELi8ELi1ELb1E":               ( 3104, 194),
    "sum_groups_kernelINS_5StarkE":                      (  705, 118),
    "slot_round_kernelINS_7SlotG24ELi4ELi1ELb0E":        ( 1790, 126),
    "slot_round_kernelINS_7SlotG24ELi4ELi2ELb1E":        ( 3707, 202),
    "slot_round_kernelINS_7SlotG24ELi8ELi1ELb0E":        ( 1912, 158),
    "slot_round_kernelINS_7SlotG24ELi8ELi1ELb1E":        ( 2180, 158),
    "slot_round_kernelINS_7SlotB72ELi4ELi1ELb0E":        ( 2770, 156),
    "slot_round_kernelINS_7SlotB72ELi4ELi1ELb1E":        ( 3116, 156),
    "slot_round_kernelINS_7SlotB72ELi8ELi1ELb0E":        ( 2966, 228),
    "slot_round_kernelINS_7SlotB72ELi8ELi1ELb1E":        ( 3650, 228),
    "slot_round_kernelINS_8SlotFrogELi4ELi1ELb0E":       ( 5280, 164),
    "slot_round_kernelINS_8SlotFrogELi4ELi1ELb1E":       ( 5539, 166),
    "slot_round_kernelINS_8SlotFrogELi8ELi1ELb0E":       ( 5439, 204),
    "slot_round_kernelINS_8SlotFrogELi8ELi1ELb1E":       ( 5951, 206),
    "sum_groups_kernelINS_4FrogE":                       (   94,  32),
}
# points per launch of (field, table slots): points_of of csrc/sumcheck_vpoly.hpp
POINTS = {"Goldilocks": {4: 5, 8: 5}, "BabyBear": {4: 5, 8: 5}, "Stark": {4: 2, 8: 1}, "SlotG24": {4: 2, 8: 1}, "SlotB72": {4: 1, 8: 1},
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
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    return open(OUT).read()


def _kernels(s):
    """the kernels of the two namespaces the launchers reach: vpoly's own, and sum_groups_kernel / zero_kernel of sumcheck.hpp"""
    for m in re.finditer(r"^(_ZN2sr(?:5vpoly|8sumcheck)\w+):.*?\n(.*?)\.Lfunc_end", s, flags=re.S | re.M):
        name, body = m.group(1), m.group(2)
        meta = s[s.index(".amdhsa_kernel " + name):]
        yield name, body, meta[:meta.index(".end_amdhsa_kernel")]


def _fragment(name):
    frags = [f for f in BUDGET if "%d%sE" % (len(f.split("INS_")[0]), f) in name]
    assert len(frags) == 1, "no budget entry for %s" % name
    return frags[0]


def _field(frag):
    m = re.search(r"INS_\d+([A-Za-z0-9]+?)E", frag)
    return m.group(1) if m else None


def test_every_reachable_kernel_stays_within_its_register_and_instruction_budget():
    seen = set()
    for name, body, meta in _kernels(_listing()):
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


def test_the_listing_holds_exactly_what_the_dispatcher_reaches():
    """A (field, table slots) pair reaches the round kernel of points_of points and the plain-sum kernel, nothing else: the points of a
    short last launch are a run-time argument of the same kernel.  The instantiation file instantiates the launchers, so the two
    cannot drift."""
    src = open(os.path.join(CSRC, "sumcheck_vpoly.hpp")).read()
    for text in ("inline int table_slots(int n_tables) { return n_tables <= 4 ? 4 : 8; }",
                 "std::is_same<T, Goldilocks>::value) return 5;",
                 "std::is_same<T, BabyBear>::value) return 5;",
                 "std::is_same<T, Stark>::value) return slots == 4 ? 2 : 1;",
                 "std::is_same<T, SlotG24>::value) return slots == 4 ? 2 : 1;",
                 "return 1;  // SlotB72"):
        assert text in src, text
    want = set()
    for field, per in POINTS.items():
        kernel = "slot_round_kernel" if field.startswith("Slot") else "round_kernel"
        for slots, p in per.items():
            want.add((kernel, field, slots, 1, 0))
            want.add((kernel, field, slots, p, 1))
    got = set()
    for frag in BUDGET:
        m = re.match(r"(\w+?_kernel)INS_\d+(\w+?)ELi(\d)ELi(\d)ELb([01])E", frag)
        if m:
            got.add((m.group(1), m.group(2), int(m.group(3)), int(m.group(4)), int(m.group(5))))
    assert got == want, (got - want, want - got)
    isa = open(SRC).read()
    for line in ("POW2(Goldilocks)", "POW2(BabyBear)", "POW2(Stark)", "SLOT(SlotG24)", "SLOT(SlotB72)", "SLOT(SlotFrog)"):
        assert line in isa, line
    for kernel in set(re.findall(r"hipLaunchKernelGGL\(\(?(?:sumcheck::)?(\w+)[<,]", src)):
        assert any(f.startswith(kernel) for f in BUDGET), kernel


def test_one_limb_round_kernels_stream_the_tables_with_sixteen_byte_non_temporal_loads():
    n = 0
    for name, body, _ in _kernels(_listing()):
        if "12round_kernelINS_10Goldilocks" not in name and "12round_kernelINS_8BabyBear" not in name:
            continue
        n += 1
        slots = int(re.search(r"ELi(\d)ELi\dELb", name).group(1))
        loads = len(re.findall(r"global_load_dwordx4 .* nt\b", body))
        assert loads >= slots * (2 if "ELb1E" in name else 1), "%s: %d non-temporal 16-byte table loads" % (name, loads)
    assert n == 8, n
