"""Static budget of the sum-check round kernels (no GPU): hipcc -S of tools/ubench/sumcheck_isa.hip, which instantiates the launchers of
csrc/sumcheck.hpp and with them every kernel the dispatcher can reach, and a count of what the listing holds.  A spill, or a register
count that costs a wave, is a regression the parity tests cannot see."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "ubench", "sumcheck_isa.hip")
OUT = os.path.join(ROOT, "build_tmp", "sumcheck_isa_budget.s")
CSRC = os.path.join(ROOT, "stark_rings_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("sumcheck.hpp", "mle.hpp", "fields.hpp", "ntt_generic.hpp", "small_rings.hpp", "small_linalg.hpp",
                                                "frog_ring.hpp", "stark_lazy.hpp")]

# Every kernel is __launch_bounds__(256): four waves per workgroup, 512 registers per lane on a SIMD.  Bound per family:
#   BabyBear                      128: four waves per SIMD at every d
#   every other field             256: two waves per SIMD (d + 1 lazy sums of four 96-bit words beside 2 d operands; the points of
#                                 Stark d = 4, G24 d = 3, 4, B72 d = 3, 4 and Frog d = 2, 3, 4 go in several launches to stay there)
MAX_VGPR = {"BabyBear": 128, "Goldilocks": 256, "Stark": 256, "SlotG24": 256, "SlotB72": 256, "SlotFrog": 256, "Frog": 256, None: 32}
# kernel (mangled-name fragment: kernel, field, tables, points per launch, round / plain sum) -> (max VALU instructions in the listing:
# what the compiler produced when the kernel was written plus 2 per cent; the VGPR count it gave, pinned).  The one-limb round kernels
# hold the 16-byte path and the one-coefficient fallback, both counted.
BUDGET = {
    "zero_kernel":                                       (   12,   6),
    "round_kernelINS_10GoldilocksELi1ELi1ELb0E":         (   96,  22),
    "round_kernelINS_10GoldilocksELi1ELi2ELb1E":         (  192,  28),
    "round_kernelINS_10GoldilocksELi2ELi1ELb0E":         (  613,  58),
    "round_kernelINS_10GoldilocksELi2ELi3ELb1E":         ( 1826, 120),
    "round_kernelINS_10GoldilocksELi3ELi1ELb0E":         (  676,  68),
    "round_kernelINS_10GoldilocksELi3ELi4ELb1E":         ( 2695, 166),
    "round_kernelINS_10GoldilocksELi4ELi1ELb0E":         (  737,  70),
    "round_kernelINS_10GoldilocksELi4ELi5ELb1E":         ( 3705, 206),
    "sum_groups_kernelINS_10GoldilocksE":                (   78,  34),
    "round_kernelINS_8BabyBearELi1ELi1ELb0E":            (  196,  42),
    "round_kernelINS_8BabyBearELi1ELi2ELb1E":            (  366,  48),
    "round_kernelINS_8BabyBearELi2ELi1ELb0E":            (  274,  42),
    "round_kernelINS_8BabyBearELi2ELi3ELb1E":            (  802,  60),
    "round_kernelINS_8BabyBearELi3ELi1ELb0E":            (  307,  42),
    "round_kernelINS_8BabyBearELi3ELi4ELb1E":            ( 1201,  68),
    "round_kernelINS_8BabyBearELi4ELi1ELb0E":            (  337,  42),
    "round_kernelINS_8BabyBearELi4ELi5ELb1E":            ( 1672,  75),
    "sum_groups_kernelINS_8BabyBearE":                   (   63,  23),
    "round_kernelINS_5StarkELi1ELi1ELb0E":               (  218,  48),
    "round_kernelINS_5StarkELi1ELi2ELb1E":               (  632,  80),
    "round_kernelINS_5StarkELi2ELi1ELb0E":               (  663,  73),
    "round_kernelINS_5StarkELi2ELi3ELb1E":               ( 2517, 186),
    "round_kernelINS_5StarkELi3ELi1ELb0E":               (  924,  78),
    "round_kernelINS_5StarkELi3ELi4ELb1E":               ( 4697, 214),
    "round_kernelINS_5StarkELi4ELi1ELb0E":               ( 1184,  80),
    "round_kernelINS_5StarkELi4ELi2ELb1E":               ( 3291, 180),
    "round_kernelINS_5StarkELi4ELi1ELb1E":               ( 1811, 132),
    "sum_groups_kernelINS_5StarkE":                      (  705, 118),
    "slot_round_kernelINS_7SlotG24ELi1ELi1ELb0E":        (  179,  24),
    "slot_round_kernelINS_7SlotG24ELi1ELi2ELb1E":        (  389,  44),
    "slot_round_kernelINS_7SlotG24ELi2ELi1ELb0E":        (  952,  80),
    "slot_round_kernelINS_7SlotG24ELi2ELi3ELb1E":        ( 2895, 200),
    "slot_round_kernelINS_7SlotG24ELi3ELi1ELb0E":        ( 1196, 128),
    "slot_round_kernelINS_7SlotG24ELi3ELi2ELb1E":        ( 2490, 170),
    "slot_round_kernelINS_7SlotG24ELi4ELi1ELb0E":        ( 1438, 134),
    "slot_round_kernelINS_7SlotG24ELi4ELi3ELb1E":        ( 4451, 240),
    "slot_round_kernelINS_7SlotG24ELi4ELi2ELb1E":        ( 3015, 188),
    "slot_round_kernelINS_7SlotB72ELi1ELi1ELb0E":        (  182,  30),
    "slot_round_kernelINS_7SlotB72ELi1ELi2ELb1E":        (  457,  62),
    "slot_round_kernelINS_7SlotB72ELi2ELi1ELb0E":        ( 1246, 108),
    "slot_round_kernelINS_7SlotB72ELi2ELi3ELb1E":        ( 3918, 244),
    "slot_round_kernelINS_7SlotB72ELi3ELi1ELb0E":        ( 1694, 130),
    "slot_round_kernelINS_7SlotB72ELi3ELi2ELb1E":        ( 3668, 207),
    "slot_round_kernelINS_7SlotB72ELi4ELi1ELb0E":        ( 2133, 132),
    "slot_round_kernelINS_7SlotB72ELi4ELi2ELb1E":        ( 4650, 232),
    "slot_round_kernelINS_7SlotB72ELi4ELi1ELb1E":        ( 2471, 158),
    "slot_round_kernelINS_8SlotFrogELi1ELi1ELb0E":       (  447,  22),
    "slot_round_kernelINS_8SlotFrogELi1ELi2ELb1E":       (  961,  50),
    "slot_round_kernelINS_8SlotFrogELi2ELi1ELb0E":       ( 2262, 108),
    "slot_round_kernelINS_8SlotFrogELi2ELi2ELb1E":       ( 4575, 206),
    "slot_round_kernelINS_8SlotFrogELi2ELi1ELb1E":       ( 2392, 122),
    "slot_round_kernelINS_8SlotFrogELi3ELi1ELb0E":       ( 3218, 140),
    "slot_round_kernelINS_8SlotFrogELi3ELi2ELb1E":       ( 6569, 244),
    "slot_round_kernelINS_8SlotFrogELi4ELi1ELb0E":       ( 4172, 150),
    "slot_round_kernelINS_8SlotFrogELi4ELi1ELb1E":       ( 4427, 148),
    "sum_groups_kernelINS_4FrogE":                       (   94,  32),
}


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
    for m in re.finditer(r"^(_ZN2sr8sumcheck\w+):.*?\n(.*?)\.Lfunc_end", s, flags=re.S | re.M):
        name, body = m.group(1), m.group(2)
        meta = s[s.index(".amdhsa_kernel " + name):]
        yield name, body, meta[:meta.index(".end_amdhsa_kernel")]


def _fragment(name):
    frags = [f for f in BUDGET if "8sumcheck%d%sE" % (len(f.split("INS_")[0]), f) in name]
    assert len(frags) == 1, "no budget entry for %s" % name
    return frags[0]


def _field(frag):
    m = re.search(r"INS_\d+([A-Za-z0-9]+?)E", frag)
    return m.group(1) if m else None


def test_every_reachable_round_kernel_stays_within_its_register_and_instruction_budget():
    seen = set()
    for name, body, meta in _kernels(_listing()):
        frag = _fragment(name)
        seen.add(frag)
        valu = sum(1 for line in body.split("\n") if re.match(r"\s+v_[a-z0-9_]+\s", line))
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", meta).group(1))
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", meta).group(1))
        budget, pinned = BUDGET[frag]
        print("%-52s VALU %5d (budget %5d)  VGPR %3d  scratch %d" % (frag, valu, budget, vgpr, scratch))
        assert scratch == 0, "%s: %d bytes of scratch (spills)" % (name, scratch)
        assert vgpr == pinned, "%s: %d VGPRs (pinned %d)" % (name, vgpr, pinned)
        assert vgpr <= MAX_VGPR[_field(frag)], "%s: %d VGPRs (family bound %d)" % (name, vgpr, MAX_VGPR[_field(frag)])
        assert valu <= budget, "%s: %d VALU instructions (budget %d)" % (name, valu, budget)
    assert seen == set(BUDGET), "kernels not found in the listing: %s" % (set(BUDGET) - seen)


def test_the_listing_holds_exactly_what_the_dispatcher_reaches():
    """points_of (csrc/sumcheck.hpp) decides the points per launch; a (field, d) pair reaches that kernel, the kernel of the remaining
    points and the plain-sum kernel, nothing else.  The instantiation file instantiates the launchers, so the two cannot drift."""
    src = open(os.path.join(CSRC, "sumcheck.hpp")).read()
    points = {"Goldilocks": [2, 3, 4, 5], "BabyBear": [2, 3, 4, 5], "Stark": [2, 3, 4, 2], "SlotG24": [2, 3, 2, 3], "SlotB72": [2, 3, 2, 2],
              "SlotFrog": [2, 2, 2, 1]}
    for text in ("std::is_same<T, Stark>::value) return n_tables >= 4 ? 2 : n_tables + 1;",
                 "std::is_same<T, SlotG24>::value) return n_tables == 3 ? 2 : n_tables == 4 ? 3 : n_tables + 1;",
                 "std::is_same<T, SlotB72>::value) return n_tables >= 3 ? 2 : n_tables + 1;",
                 "std::is_same<T, SlotFrog>::value) return n_tables >= 4 ? 1 : n_tables >= 2 ? 2 : n_tables + 1;"):
        assert text in src, text
    want = set()
    for field, per in points.items():
        kernel = "slot_round_kernel" if field.startswith("Slot") else "round_kernel"
        for d, p in zip((1, 2, 3, 4), per):
            want.add((kernel, field, d, 1, 0))
            want.add((kernel, field, d, p, 1))
            if (d + 1) % p:
                want.add((kernel, field, d, (d + 1) % p, 1))
    got = set()
    for frag in BUDGET:
        m = re.match(r"(\w+?_kernel)INS_\d+(\w+?)ELi(\d)ELi(\d)ELb([01])E", frag)
        if m:
            got.add((m.group(1), m.group(2), int(m.group(3)), int(m.group(4)), int(m.group(5))))
    assert got == want, (got - want, want - got)
    isa = open(SRC).read()
    for line in ("POW2(Goldilocks)", "POW2(BabyBear)", "POW2(Stark)", "SLOT(SlotG24)", "SLOT(SlotB72)", "SLOT(SlotFrog)"):
        assert line in isa, line
    for kernel in set(re.findall(r"hipLaunchKernelGGL\(\(?(\w+)[<,]", src)):
        assert any(f.startswith(kernel) for f in BUDGET), kernel


def test_one_limb_round_kernels_stream_the_tables_with_sixteen_byte_non_temporal_loads():
    n = 0
    for name, body, _ in _kernels(_listing()):
        if "12round_kernelINS_10Goldilocks" not in name and "12round_kernelINS_8BabyBear" not in name:
            continue
        n += 1
        tables = int(re.search(r"ELi(\d)ELi\dELb", name).group(1))
        loads = len(re.findall(r"global_load_dwordx4 .* nt\b", body))
        assert loads >= tables * (2 if "ELb1E" in name else 1), "%s: %d non-temporal 16-byte table loads" % (name, loads)
    assert n == 16, n
