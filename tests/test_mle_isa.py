"""Static budget of the multilinear-fold kernels (no GPU): hipcc -S of tools/ubench/mle_isa.hip, which instantiates every fold and
multiply-add kernel the library dispatches to (csrc/mle.hpp: kMaxJ / kSlotMaxJ bound the variables per launch), and a count of what
the listing holds.  The folds stream, so a spill, a lost 16-byte access or a register count that costs a wave is a regression the
parity tests cannot see."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "ubench", "mle_isa.hip")
OUT = os.path.join(ROOT, "build_tmp", "mle_isa_budget.s")
CSRC = os.path.join(ROOT, "stark_rings_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("mle.hpp", "fields.hpp", "ntt_generic.hpp", "small_rings.hpp", "small_linalg.hpp", "frog_ring.hpp")]

# every kernel is __launch_bounds__(256): four waves per workgroup.  128 VGPRs keep four waves on each SIMD (512 registers per lane),
# i.e. four workgroups per CU, which is what the launchers' one-piece-per-lane grids count on to keep the loads of a CU in flight.
MAX_VGPR = 128
# kernel (mangled-name fragment) -> max VALU instructions in the listing: what the compiler produced when the kernel was written,
# plus 2 % (the one-limb fold kernels hold the 16-byte path and the one-coefficient fallback, both counted)
BUDGET = {
    "fold_kernelINS_10GoldilocksELi0E": 44,
    "fold_kernelINS_10GoldilocksELi1E": 141,
    "fold_kernelINS_10GoldilocksELi2E": 328,
    "fold_kernelINS_10GoldilocksELi3E": 697,
    "fold_kernelINS_8BabyBearELi0E": 50,
    "fold_kernelINS_8BabyBearELi1E": 111,
    "fold_kernelINS_8BabyBearELi2E": 230,
    "fold_kernelINS_8BabyBearELi3E": 466,
    "fold_kernelINS_5StarkELi0E": 28,
    "fold_kernelINS_5StarkELi1E": 459,
    "fold_kernelINS_5StarkELi2E": 1291,
    "slot_fold_kernelINS_7SlotG24ELi0E": 32,
    "slot_fold_kernelINS_7SlotG24ELi1E": 306,
    "slot_fold_kernelINS_7SlotG24ELi2E": 845,
    "slot_fold_kernelINS_7SlotG24ELi3E": 1920,
    "slot_fold_kernelINS_7SlotB72ELi0E": 40,
    "slot_fold_kernelINS_7SlotB72ELi1E": 556,
    "slot_fold_kernelINS_7SlotB72ELi2E": 1584,
    "slot_fold_kernelINS_8SlotFrogELi0E": 29,
    "slot_fold_kernelINS_8SlotFrogELi1E": 1038,
    "slot_fold_kernelINS_8SlotFrogELi2E": 3055,
    "slot_fold_kernelINS_8SlotFrogELi3E": 7091,
    "mul_elem_add_kernelINS_10GoldilocksE": 97,
    "mul_elem_add_kernelINS_8BabyBearE": 65,
    "mul_elem_add_kernelINS_5StarkE": 355,
    "slot_mul_elem_add_kernelINS_7SlotG24E": 270,
    "slot_mul_elem_add_kernelINS_7SlotB72E": 495,
    "slot_mul_elem_add_kernelINS_8SlotFrogE": 991,
}
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
    for m in re.finditer(r"^(_ZN2sr3mle\w+):.*?\n(.*?)\.Lfunc_end", s, flags=re.S | re.M):
        name, body = m.group(1), m.group(2)
        meta = s[s.index(".amdhsa_kernel " + name):]
        yield name, body, meta[:meta.index(".end_amdhsa_kernel")]


def _fragment(name):
    frags = [f for f in BUDGET if "3mle%d%s" % (len(f.split("INS_")[0]), f) in name]
    assert len(frags) == 1, "no budget entry for %s" % name
    return frags[0]


def test_every_dispatched_fold_kernel_stays_within_its_register_and_instruction_budget():
    seen = set()
    for name, body, meta in _kernels(_listing()):
        frag = _fragment(name)
        seen.add(frag)
        valu = sum(1 for line in body.split("\n") if re.match(r"\s+v_[a-z0-9_]+\s", line))
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", meta).group(1))
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", meta).group(1))
        print("%-42s VALU %5d (budget %5d)  VGPR %3d  scratch %d" % (frag, valu, BUDGET[frag], vgpr, scratch))
        assert scratch == 0, "%s: %d bytes of scratch (spills)" % (name, scratch)
        assert vgpr <= MAX_VGPR, "%s: %d VGPRs (budget %d: four waves per SIMD)" % (name, vgpr, MAX_VGPR)
        assert valu <= BUDGET[frag], "%s: %d VALU instructions (budget %d)" % (name, valu, BUDGET[frag])
    assert seen == set(BUDGET), "kernels not found in the listing: %s" % (set(BUDGET) - seen)


def test_the_listing_holds_every_fold_width_the_plan_can_choose():
    """csrc/mle.hpp bounds the variables per launch by kMaxJ / kSlotMaxJ, and sr_mle_plan never exceeds them: the budget table holds
    J = 0 .. that bound for every family, and the plan's launch count shows the bound in use."""
    import ctypes

    from stark_rings_amd import _lib

    src = open(os.path.join(CSRC, "mle.hpp")).read()
    assert re.search(r"kMaxJ = std::is_same<F, Stark>::value \? 2 : 3;", src)
    assert re.search(r"kSlotMaxJ = std::is_same<SL, SlotB72>::value \? 2 : 3;", src)
    top = {"GoldilocksE": (0, 3), "BabyBearE": (1, 3), "StarkE": (2, 2), "SlotG24E": (3, 3), "SlotB72E": (4, 2), "SlotFrogE": (5, 3)}
    lib = _lib.load()
    for fam, (ring, j) in top.items():
        have = sorted(int(f[-2]) for f in BUDGET if "fold_kernel" in f and fam + "Li" in f)
        assert have == list(range(j + 1)), (fam, have)
        work, launches = ctypes.c_size_t(), ctypes.c_int()
        assert lib.sr_mle_plan(ring, 4, 12, 12, 0, ctypes.byref(work), ctypes.byref(launches)) == 0
        assert launches.value == 12 // j, (fam, launches.value)


def test_one_limb_table_accesses_are_sixteen_byte_and_non_temporal():
    n = 0
    for name, body, _ in _kernels(_listing()):
        if not any(f in name for f in ONE_LIMB) or "slot_" in name:
            continue
        n += 1
        assert re.search(r"global_load_dwordx4 .* nt\b", body), "%s: no non-temporal 16-byte table load" % name
        assert re.search(r"global_store_dwordx4 .* nt\b", body), "%s: no non-temporal 16-byte store" % name
        m = re.search(r"fold_kernelINS_\d+\w+?ELi(\d)E", name)
        if m:  # 2^J table loads and J point loads of 16 bytes each in the paired path
            j = int(m.group(1))
            assert len(re.findall(r"global_load_dwordx4", body)) >= (1 << j) + j, name
            assert len(re.findall(r"global_load_dwordx4 .* nt\b", body)) >= 1 << j, name
    assert n == 10, n
