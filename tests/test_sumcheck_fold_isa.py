"""Static budget of the fused fold-and-round kernels (no GPU): hipcc -S of tools/ubench/sumcheck_fold_isa.hip, which instantiates the
launchers of csrc/sumcheck_fold.hpp and with them every kernel the dispatcher can reach, and a count of what the listing holds.  A
spill, or a register count that costs a wave, is a regression the parity tests cannot see.  Registers and instructions only."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "ubench", "sumcheck_fold_isa.hip")
OUT = os.path.join(ROOT, "build_tmp", "sumcheck_fold_isa_budget.s")
CSRC = os.path.join(ROOT, "stark_rings_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("sumcheck_fold.hpp", "sumcheck.hpp", "mle.hpp", "fields.hpp", "ntt_generic.hpp", "small_rings.hpp",
                                                "small_linalg.hpp", "frog_ring.hpp", "stark_lazy.hpp")]

# Every kernel is __launch_bounds__(256).  Bound per family, as for the round kernels (tests/test_sumcheck_isa.py): BabyBear 128 (four
# waves per SIMD at every d), every other field 256 (two waves per SIMD).
MAX_VGPR = {"BabyBear": 128, "Goldilocks": 256, "Stark": 256, "SlotG24": 256, "SlotB72": 256, "SlotFrog": 256}
# kernel (mangled-name fragment: kernel, field, tables, points in the launch) -> (max VALU instructions in the listing: what the compiler
# produced when the kernel was written plus 2 per cent; the VGPR count it gave, pinned).  The one-limb kernels hold the 16-byte path and
# the one-coefficient fallback, both counted.  The slot kernels ask for two waves per SIMD outright, so their d = 1 forms report the 169
# registers that leaves them rather than what they need.  Last: the round kernels of csrc/sumcheck.hpp at point counts that only the
# remaining launches of a fused plan reach (every other one is held by tests/test_sumcheck_isa.py).
BUDGET = {
    "fold_round_kernelINS_10GoldilocksELi1ELi2E":        (  422,  58),
    "fold_round_kernelINS_10GoldilocksELi2ELi3E":        ( 2229, 154),
    "fold_round_kernelINS_10GoldilocksELi3ELi4E":        ( 3276, 190),
    "fold_round_kernelINS_10GoldilocksELi4ELi5E":        ( 4463, 226),
    "fold_round_kernelINS_8BabyBearELi1ELi2E":           (  538,  54),
    "fold_round_kernelINS_8BabyBearELi2ELi3E":           ( 1102,  80),
    "fold_round_kernelINS_8BabyBearELi3ELi4E":           ( 1629,  94),
    "fold_round_kernelINS_8BabyBearELi4ELi5E":           ( 2232, 108),
    "fold_round_kernelINS_5StarkELi1ELi2E":              ( 1434, 115),
    "fold_round_kernelINS_5StarkELi2ELi3E":              ( 4066, 208),
    "fold_round_kernelINS_5StarkELi3ELi3E":              ( 5929, 248),
    "fold_round_kernelINS_5StarkELi4ELi2E":              ( 6356, 224),
    "slot_fold_round_kernelINS_7SlotG24ELi1ELi2E":       (  972, 169),
    "slot_fold_round_kernelINS_7SlotG24ELi2ELi3E":       ( 4034, 244),
    "slot_fold_round_kernelINS_7SlotG24ELi3ELi2E":       ( 4189, 218),
    "slot_fold_round_kernelINS_7SlotG24ELi4ELi2E":       ( 5276, 242),
    "slot_fold_round_kernelINS_7SlotB72ELi1ELi2E":       ( 1578, 169),
    "slot_fold_round_kernelINS_7SlotB72ELi2ELi2E":       ( 4859, 236),
    "slot_fold_round_kernelINS_7SlotB72ELi3ELi1E":       ( 4019, 196),
    "slot_fold_round_kernelINS_7SlotB72ELi4ELi1E":       ( 4354, 169),
    "slot_fold_round_kernelINS_8SlotFrogELi1ELi2E":      ( 3037, 169),
    "slot_fold_round_kernelINS_8SlotFrogELi2ELi1E":      ( 6416, 176),
    "slot_fold_round_kernelINS_8SlotFrogELi3ELi1E":      ( 9432, 196),
    "slot_fold_round_kernelINS_8SlotFrogELi4ELi1E":      (12449, 216),
    "round_kernelINS_5StarkELi3ELi1ELb1E":               ( 1394, 116),
    "slot_round_kernelINS_7SlotB72ELi2ELi1ELb1E":        ( 1420, 122),
    "slot_round_kernelINS_7SlotB72ELi3ELi1ELb1E":        ( 1951, 140),
    "slot_round_kernelINS_8SlotFrogELi3ELi1ELb1E":       ( 3410, 138),
}
# points of the fused launch for d = 1 .. 4 (fused_points_of) and points per launch of the round kernels (sumcheck::points_of)
FUSED = {"Goldilocks": [2, 3, 4, 5], "BabyBear": [2, 3, 4, 5], "Stark": [2, 3, 3, 2], "SlotG24": [2, 3, 2, 2], "SlotB72": [2, 2, 1, 1],
         "SlotFrog": [2, 1, 1, 1]}
PER_LAUNCH = {"Goldilocks": [2, 3, 4, 5], "BabyBear": [2, 3, 4, 5], "Stark": [2, 3, 4, 2], "SlotG24": [2, 3, 2, 3], "SlotB72": [2, 3, 2, 2],
              "SlotFrog": [2, 2, 2, 1]}


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
    """the fused kernels and the round kernels next to them: (name, body, metadata)"""
    for m in re.finditer(r"^(_ZN2sr(?:13sumcheck_fold|8sumcheck)\d+\w*round_kernel\w+):.*?\n(.*?)\.Lfunc_end", s, flags=re.S | re.M):
        name, body = m.group(1), m.group(2)
        meta = s[s.index(".amdhsa_kernel " + name):]
        yield name, body, meta[:meta.index(".end_amdhsa_kernel")]


def _fragment(name):
    frags = [f for f in BUDGET if re.search(r"(13sumcheck_fold|8sumcheck)%d%s" % (len(f.split("INS_")[0]), f), name)]
    return frags[0] if len(frags) == 1 else None


def _field(frag):
    return re.search(r"INS_\d+([A-Za-z0-9]+?)E", frag).group(1)


def test_every_reachable_fused_kernel_stays_within_its_register_and_instruction_budget():
    seen = set()
    for name, body, meta in _kernels(_listing()):
        frag = _fragment(name)
        if frag is None:  # a round kernel that sr_mle_round_evals reaches as well: tests/test_sumcheck_isa.py holds it
            assert "13sumcheck_fold" not in name, "no budget entry for %s" % name
            continue
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
    """fused_points_of decides the points of the fused launch; the remaining ones go in chunks of points_of, then the rest.  The
    instantiation file instantiates the launchers, so the listing and the dispatcher cannot drift."""
    import test_sumcheck_isa as RI

    fused, rest = set(), set()
    for field, per in FUSED.items():
        for d, fp in zip((1, 2, 3, 4), per):
            fused.add(("slot_fold_round_kernel" if field.startswith("Slot") else "fold_round_kernel", field, d, fp))
            left, p = d + 1 - fp, PER_LAUNCH[field][d - 1]
            kernel = "slot_round_kernel" if field.startswith("Slot") else "round_kernel"
            if left >= p:
                rest.add((kernel, field, d, p))
            if left % p:
                rest.add((kernel, field, d, left % p))
    got_fused, got_rest = set(), set()
    for name, _, _ in _kernels(_listing()):
        m = re.search(r"(?:13sumcheck_fold|8sumcheck)\d+(\w*?round_kernel)INS_\d+(\w+?)ELi(\d)ELi(\d)E", name)
        key = (m.group(1), m.group(2), int(m.group(3)), int(m.group(4)))
        (got_fused if "13sumcheck_fold" in name else got_rest).add(key)
    assert got_fused == fused, (got_fused - fused, fused - got_fused)
    assert got_rest == rest, (got_rest - rest, rest - got_rest)
    # every round kernel of the remaining launches has a budget: here, or in the round kernels' own test
    for kernel, field, d, p in rest:
        frag = "%sINS_%d%sELi%dELi%dELb1E" % (kernel, len(field), field, d, p)
        assert frag in BUDGET or frag in RI.BUDGET, frag
    isa = open(SRC).read()
    for line in ("POW2(Goldilocks)", "POW2(BabyBear)", "POW2(Stark)", "SLOT(SlotG24)", "SLOT(SlotB72)", "SLOT(SlotFrog)"):
        assert line in isa, line


def test_one_limb_fused_kernels_stream_the_tables_with_sixteen_byte_non_temporal_accesses():
    n = 0
    for name, body, _ in _kernels(_listing()):
        if "17fold_round_kernelINS_10Goldilocks" not in name and "17fold_round_kernelINS_8BabyBear" not in name:
            continue
        n += 1
        tables = int(re.search(r"ELi(\d)ELi\dE", name).group(1))
        loads = len(re.findall(r"global_load_dwordx4 .* nt\b", body))
        stores = len(re.findall(r"global_store_dwordx4 .* nt\b", body))
        assert loads >= 4 * tables, "%s: %d non-temporal 16-byte table loads" % (name, loads)
        assert stores >= 2 * tables, "%s: %d non-temporal 16-byte stores of folded elements" % (name, stores)
    assert n == 8, n
