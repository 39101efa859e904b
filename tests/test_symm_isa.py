"""Static budget of the symmetric-matrix kernels (no GPU): hipcc -S of tools/ubench/symm_isa.hip, which instantiates every Gram,
partial-sum, weight and recompose kernel the launchers of csrc/symmetric.hpp dispatch to, and a count of what the listing holds.  A
spill or a register count that costs a wave is a regression the parity tests cannot see."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "ubench", "symm_isa.hip")
OUT = os.path.join(ROOT, "build_tmp", "symm_isa_budget.s")
CSRC = os.path.join(ROOT, "stark_rings_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("symmetric.hpp", "mle.hpp", "fields.hpp", "ntt_generic.hpp", "small_rings.hpp", "small_linalg.hpp",
                                                "frog_ring.hpp", "stark_lazy.hpp")]

# every kernel is __launch_bounds__(256): four waves per workgroup.  128 VGPRs keep four waves on each SIMD (512 registers per lane),
# i.e. four workgroups per CU, which is what the plan's fill target (1024 workgroups on 256 CUs) counts on.
MAX_VGPR = 128
# kernel (mangled-name fragment) -> max VALU instructions in the listing: what the compiler produced when the kernel was written,
# plus 2 % (the one-limb recompose kernels hold the 16-byte path and the one-coefficient fallback, both counted)
BUDGET = {
    "gram_kernelINS_10GoldilocksELi4ELi2E": 911,
    "gram_kernelINS_8BabyBearELi8ELi4E": 743,
    "gram_kernelINS_5StarkELi2ELi1E": 797,
    "gram_kernelINS_6StarkLELi2ELi1E": 1172,
    "sum_parts_kernelINS_10GoldilocksE": 19,
    "sum_parts_kernelINS_8BabyBearE": 18,
    "sum_parts_kernelINS_5StarkE": 104,
    "sum_parts_kernelINS_4FrogE": 21,
    "weights_kernelINS_10GoldilocksE": 126,
    "weights_kernelINS_8BabyBearE": 116,
    "weights_kernelINS_5StarkE": 373,
    "recompose_kernelINS_10GoldilocksES2_E": 397,
    "recompose_kernelINS_8BabyBearES2_E": 164,
    "recompose_kernelINS_5StarkES2_E": 417,
    "recompose_kernelINS_5StarkENS_6StarkLEE": 602,
    "slot_gram_kernelINS_7SlotG24E": 574,
    "slot_weights_kernelINS_7SlotG24E": 377,
    "slot_recompose_kernelINS_7SlotG24E": 709,
    "slot_gram_kernelINS_7SlotB72E": 768,
    "slot_weights_kernelINS_7SlotB72E": 568,
    "slot_recompose_kernelINS_7SlotB72E": 867,
    "slot_gram_kernelINS_8SlotFrogE": 1177,
    "slot_weights_kernelINS_8SlotFrogE": 1143,
    "slot_recompose_kernelINS_8SlotFrogE": 1513,
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
    for m in re.finditer(r"^(_ZN2sr4symm\w+):.*?\n(.*?)\.Lfunc_end", s, flags=re.S | re.M):
        name, body = m.group(1), m.group(2)
        meta = s[s.index(".amdhsa_kernel " + name):]
        yield name, body, meta[:meta.index(".end_amdhsa_kernel")]


def _fragment(name):
    frags = [f for f in BUDGET if "4symm%d%s" % (len(f.split("INS_")[0]), f) in name]
    assert len(frags) == 1, "no budget entry for %s" % name
    return frags[0]


def test_every_dispatched_symmetric_kernel_stays_within_its_register_and_instruction_budget():
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


def test_the_listing_holds_the_register_blocks_the_launchers_choose():
    """csrc/symmetric.hpp picks the Gram block per field (GramBlock) and the plan's tile arithmetic uses the same numbers: the
    instantiation file must name exactly those, and every launcher's kernel must be in the budget table."""
    src = open(os.path.join(CSRC, "symmetric.hpp")).read()
    assert re.search(r"RB = std::is_same<F, BabyBear>::value \? 8 : std::is_same<F, Goldilocks>::value \? 4 : 2, CB = RB / 2;", src)
    isa = open(SRC).read()
    for line in ("GRAM(Goldilocks, 4, 2)", "GRAM(BabyBear, 8, 4)", "GRAM(Stark, 2, 1)", "GRAM(StarkL, 2, 1)"):
        assert line in isa, line
    for kernel in re.findall(r"hipLaunchKernelGGL\(\((\w+)<", src):
        assert any(f.startswith(kernel + "INS_") for f in BUDGET), kernel


def test_one_limb_recompose_streams_the_matrix_with_sixteen_byte_non_temporal_loads():
    n = 0
    for name, body, _ in _kernels(_listing()):
        if "recompose_kernel" not in name or "slot_" in name or not any(f in name for f in ("10GoldilocksES2_", "8BabyBearES2_")):
            continue
        n += 1
        assert re.search(r"global_load_dwordx4 .* nt\b", body), "%s: no non-temporal 16-byte matrix load" % name
        assert re.search(r"global_store_dwordx4 .* nt\b", body), "%s: no non-temporal 16-byte store" % name
    assert n == 2, n
