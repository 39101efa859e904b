"""Static budget of the fraction-tree kernels (no GPU): hipcc -S of tools/ubench/frac_tree_isa.hip, which instantiates every kernel
the launcher dispatches to (csrc/frac_tree.hpp: kMaxJ / kSlotMaxJ bound the levels per launch), and a count of what the listing
holds.  The tree streams, so a spill, a lost 16-byte or non-temporal access or a register count that costs a wave is a regression the
parity tests cannot see.  Registers, loads and stores are counted, nothing else."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "ubench", "frac_tree_isa.hip")
OUT = os.path.join(ROOT, "build_tmp", "frac_tree_isa_budget.s")
CSRC = os.path.join(ROOT, "stark_rings_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("frac_tree.hpp", "prod_tree.hpp", "mle.hpp", "sparse_mle.hpp", "fields.hpp", "ntt_generic.hpp",
                                                "small_rings.hpp", "small_linalg.hpp", "frog_ring.hpp")]

# every kernel is __launch_bounds__(256): four waves per workgroup.  128 VGPRs keep four waves on each SIMD (512 registers per lane),
# the bound csrc/prod_tree.hpp uses.
MAX_VGPR = 128
# kernel (mangled-name fragment; Lb1: numerators stored, Lb0: not) -> max VALU instructions in the listing: what the compiler produced
# when the kernel was written, plus 2 % (the one-limb kernels hold the 16-byte path and the one-coefficient fallback, both counted)
WRITTEN = {
    "tree_kernelINS_10GoldilocksELi1ELb1E": 258, "tree_kernelINS_10GoldilocksELi1ELb0E": 251,
    "tree_kernelINS_10GoldilocksELi2ELb1E": 694, "tree_kernelINS_10GoldilocksELi2ELb0E": 679,
    "tree_kernelINS_8BabyBearELi1ELb1E": 171, "tree_kernelINS_8BabyBearELi1ELb0E": 164,
    "tree_kernelINS_8BabyBearELi2ELb1E": 440, "tree_kernelINS_8BabyBearELi2ELb0E": 425,
    "tree_kernelINS_8BabyBearELi3ELb1E": 1015, "tree_kernelINS_8BabyBearELi3ELb0E": 985,
    "tree_kernelINS_5StarkELi1ELb1E": 889, "tree_kernelINS_5StarkELi1ELb0E": 898,
    "tree_kernelINS_5StarkELi2ELb1E": 2609, "tree_kernelINS_5StarkELi2ELb0E": 2616,
    "slot_tree_kernelINS_7SlotG24ELi1ELb1E": 832, "slot_tree_kernelINS_7SlotG24ELi1ELb0E": 566,
    "slot_tree_kernelINS_7SlotG24ELi2ELb1E": 2459, "slot_tree_kernelINS_7SlotG24ELi2ELb0E": 2216,
    "slot_tree_kernelINS_7SlotB72ELi1ELb1E": 1411, "slot_tree_kernelINS_7SlotB72ELi1ELb0E": 839,
    "slot_tree_kernelINS_8SlotFrogELi1ELb1E": 3123, "slot_tree_kernelINS_8SlotFrogELi1ELb0E": 1528,
    "slot_tree_kernelINS_8SlotFrogELi2ELb1E": 9366, "slot_tree_kernelINS_8SlotFrogELi2ELb0E": 7748,
}
BUDGET = {k: v + v // 50 for k, v in WRITTEN.items()}
# levels per launch at most, per family (ring id, bound).  One level more needs, with numerators stored: Goldilocks 152 VGPRs,
# Stark 173, goldilocks24 130, babybear72 140 (144 without numerators), frog16 172; BabyBear's three levels take 78.
TOP = {"GoldilocksE": (0, 2), "BabyBearE": (1, 3), "StarkE": (2, 2), "SlotG24E": (3, 2), "SlotB72E": (4, 1), "SlotFrogE": (5, 2)}
ONE_LIMB = ("GoldilocksE", "BabyBearE")


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
    for m in re.finditer(r"^(_ZN2sr5ftree\w+):.*?\n(.*?)\.Lfunc_end", s, flags=re.S | re.M):
        name, body = m.group(1), m.group(2)
        meta = s[s.index(".amdhsa_kernel " + name):]
        yield name, body, meta[:meta.index(".end_amdhsa_kernel")]


def _fragment(name):
    frags = [f for f in BUDGET if "5ftree%d%s" % (len(f.split("INS_")[0]), f) in name]
    assert len(frags) == 1, "no budget entry for %s" % name
    return frags[0]


def test_every_dispatched_tree_kernel_stays_within_its_register_and_instruction_budget():
    seen = set()
    for name, body, meta in _kernels(_listing()):
        frag = _fragment(name)
        seen.add(frag)
        valu = sum(1 for line in body.split("\n") if re.match(r"\s+v_[a-z0-9_]+\s", line))
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", meta).group(1))
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", meta).group(1))
        print("%-46s VALU %5d (budget %5d)  VGPR %3d  scratch %d" % (frag, valu, BUDGET[frag], vgpr, scratch))
        assert scratch == 0, "%s: %d bytes of scratch (spills)" % (name, scratch)
        assert vgpr <= MAX_VGPR, "%s: %d VGPRs (budget %d: four waves per SIMD)" % (name, vgpr, MAX_VGPR)
        assert valu <= BUDGET[frag], "%s: %d VALU instructions (budget %d)" % (name, valu, BUDGET[frag])
    assert seen == set(BUDGET), "kernels not found in the listing: %s" % (set(BUDGET) - seen)


def test_the_launcher_dispatches_only_what_the_listing_holds():
    """csrc/frac_tree.hpp bounds the levels per launch by kMaxJ / kSlotMaxJ, the launchers refuse anything above them and
    sr_frac_tree_plan never exceeds them: the budget table holds J = 1 .. that bound for every family, with and without numerators,
    and nothing else, and the plan's launch count shows the bound in use."""
    import ctypes

    from stark_rings_amd import _lib

    src = open(os.path.join(CSRC, "frac_tree.hpp")).read()
    assert re.search(r"kMaxJ = std::is_same<F, BabyBear>::value \? 3 : 2;", src)
    assert re.search(r"kSlotMaxJ = std::is_same<SL, SlotB72>::value \? 1 : 2;", src)
    assert re.search(r"j > kMaxJ<F>", src) and re.search(r"j > kSlotMaxJ<SL>", src), "the launchers bound j"
    # every launch site names its J as a literal, only 1, 2, 3 appear, and every J above 1 is guarded by the family's bound
    sites = re.findall(r"(if constexpr \(k(?:Slot)?MaxJ<\w+> >= (\d)\) )?hipLaunchKernelGGL\(\((?:slot_)?tree_kernel<\w+, (\d), HP>\)", src)
    assert sorted(j for _, _, j in sites) == ["1", "1", "2", "2", "3", "3"]
    assert all((j == "1" and not guard) or bound == j for guard, bound, j in sites), sites
    lib = _lib.load()
    for fam, (ring, j) in TOP.items():
        for hp in ("Lb1E", "Lb0E"):
            have = sorted(int(f[-6]) for f in BUDGET if fam + "Li" in f and f.endswith(hp))
            assert have == list(range(1, j + 1)), (fam, hp, have)
        elems, launches = ctypes.c_size_t(), ctypes.c_int()
        for order in (0, 1):
            assert lib.sr_frac_tree_plan(ring, 4, 12, order, ctypes.byref(elems), ctypes.byref(launches)) == 0
            assert launches.value == 12 // j, (fam, launches.value)
            assert lib.sr_frac_tree_plan(ring, 4, 13, order, ctypes.byref(elems), ctypes.byref(launches)) == 0
            assert launches.value == 12 // j + 1, (fam, launches.value)


def test_one_limb_accesses_are_sixteen_byte_and_non_temporal():
    """the aligned path of a one-limb kernel reads the 2^J numerators and 2^J denominators of its group (the denominators alone
    where no numerators are stored) and writes the 2^J - 1 nodes of both sides with one non-temporal 16-byte access each, and nothing
    of 16 bytes goes any other way; the one-coefficient fallback does the same in 8-byte accesses"""
    n = 0
    for name, body, _ in _kernels(_listing()):
        if not any(f in name for f in ONE_LIMB) or "slot_" in name:
            continue
        n += 1
        j, hp = re.search(r"tree_kernelINS_\d+\w+?ELi(\d)ELb([01])E", name).groups()
        loads, stores = (2 if hp == "1" else 1) << int(j), 2 * ((1 << int(j)) - 1)
        assert len(re.findall(r"global_load_dwordx4 .* nt\b", body)) == loads, name
        assert len(re.findall(r"global_store_dwordx4 .* nt\b", body)) == stores, name
        assert len(re.findall(r"global_load_dwordx4", body)) == loads, "%s: a 16-byte load that is not non-temporal" % name
        assert len(re.findall(r"global_store_dwordx4", body)) == stores, "%s: a 16-byte store that is not non-temporal" % name
    assert n == 10, n
