"""Static budget of the sparse multilinear-extension kernels (no GPU): hipcc -S of tools/ubench/smle_isa.hip, which instantiates
every eq-table, fold and combine kernel the library dispatches to (smle_dispatch in csrc/capi.hip: the 16-byte pair and the
one-coefficient unit of the one-limb fields, Stark with and without the lazy sum of products, the three slot rings), and a count of
what the listing holds.  A spill, a lost 16-byte access or a register count that costs a wave is a regression the parity tests
cannot see."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "ubench", "smle_isa.hip")
OUT = os.path.join(ROOT, "build_tmp", "smle_isa_budget.s")
CSRC = os.path.join(ROOT, "stark_rings_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("sparse_mle.hpp", "mle.hpp", "fields.hpp", "stark_lazy.hpp", "ntt_generic.hpp", "small_rings.hpp",
                                                "small_linalg.hpp", "frog_ring.hpp")]

# every kernel is __launch_bounds__(256): 128 VGPRs keep four waves on each SIMD
MAX_VGPR = 128
# kernel (mangled-name fragment) -> max VALU instructions in the listing: what the compiler produced when the kernel was written,
# plus two percent
BUDGET = {
    "eq_kernelINS0_6PowOpsINS_10GoldilocksES3_Li2EEELi3EE": 456,
    "fold_kernelINS0_6PowOpsINS_10GoldilocksES3_Li2EEELb1EE": 457,
    "fold_kernelINS0_6PowOpsINS_10GoldilocksES3_Li2EEELb0EE": 476,
    "combine_kernelINS0_6PowOpsINS_10GoldilocksES3_Li2EEEE": 107,
    "eq_kernelINS0_6PowOpsINS_10GoldilocksES3_Li1EEELi3EE": 254,
    "fold_kernelINS0_6PowOpsINS_10GoldilocksES3_Li1EEELb1EE": 277,
    "fold_kernelINS0_6PowOpsINS_10GoldilocksES3_Li1EEELb0EE": 287,
    "combine_kernelINS0_6PowOpsINS_10GoldilocksES3_Li1EEEE": 96,
    "eq_kernelINS0_6PowOpsINS_8BabyBearES3_Li2EEELi3EE": 312,
    "fold_kernelINS0_6PowOpsINS_8BabyBearES3_Li2EEELb1EE": 158,
    "fold_kernelINS0_6PowOpsINS_8BabyBearES3_Li2EEELb0EE": 174,
    "combine_kernelINS0_6PowOpsINS_8BabyBearES3_Li2EEEE": 164,
    "eq_kernelINS0_6PowOpsINS_8BabyBearES3_Li1EEELi3EE": 175,
    "fold_kernelINS0_6PowOpsINS_8BabyBearES3_Li1EEELb1EE": 127,
    "fold_kernelINS0_6PowOpsINS_8BabyBearES3_Li1EEELb0EE": 133,
    "combine_kernelINS0_6PowOpsINS_8BabyBearES3_Li1EEEE": 129,
    "eq_kernelINS0_6PowOpsINS_5StarkENS_6StarkLELi4EEELi2EE": 1382,
    "fold_kernelINS0_6PowOpsINS_5StarkENS_6StarkLELi4EEELb1EE": 1202,
    "fold_kernelINS0_6PowOpsINS_5StarkENS_6StarkLELi4EEELb0EE": 1339,
    "combine_kernelINS0_6PowOpsINS_5StarkENS_6StarkLELi4EEEE": 261,
    "eq_kernelINS0_6PowOpsINS_5StarkES3_Li4EEELi2EE": 1382,
    "fold_kernelINS0_6PowOpsINS_5StarkES3_Li4EEELb1EE": 717,
    "fold_kernelINS0_6PowOpsINS_5StarkES3_Li4EEELb0EE": 853,
    "combine_kernelINS0_6PowOpsINS_5StarkES3_Li4EEEE": 261,
    "eq_kernelINS0_7SlotOpsINS_7SlotG24EEELi3EE": 2128,
    "fold_kernelINS0_7SlotOpsINS_7SlotG24EEELb1EE": 618,
    "fold_kernelINS0_7SlotOpsINS_7SlotG24EEELb0EE": 644,
    "combine_kernelINS0_7SlotOpsINS_7SlotG24EEEE": 124,
    "eq_kernelINS0_7SlotOpsINS_7SlotB72EEELi2EE": 2020,
    "fold_kernelINS0_7SlotOpsINS_7SlotB72EEELb1EE": 1577,
    "fold_kernelINS0_7SlotOpsINS_7SlotB72EEELb0EE": 1630,
    "combine_kernelINS0_7SlotOpsINS_7SlotB72EEEE": 231,
    "eq_kernelINS0_7SlotOpsINS_8SlotFrogEEELi3EE": 7898,
    "fold_kernelINS0_7SlotOpsINS_8SlotFrogEEELb1EE": 2039,
    "fold_kernelINS0_7SlotOpsINS_8SlotFrogEEELb0EE": 2088,
    "combine_kernelINS0_7SlotOpsINS_8SlotFrogEEEE": 191,
}
PAIRED = ("GoldilocksES3_Li2E", "BabyBearES3_Li2E")  # the 16-byte unit of the one-limb fields


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
    for m in re.finditer(r"^(_ZN2sr4smle\w+):.*?\n(.*?)\.Lfunc_end", s, flags=re.S | re.M):
        name, body = m.group(1), m.group(2)
        meta = s[s.index(".amdhsa_kernel " + name):]
        yield name, body, meta[:meta.index(".end_amdhsa_kernel")]


def _fragment(name):
    m = re.match(r"_ZN2sr4smle\d+(\w+?E)Ev(?:NT_|Pm)", name)
    assert m and m.group(1) in BUDGET, "no budget entry for %s" % name
    return m.group(1)


def test_every_dispatched_kernel_stays_within_its_register_and_instruction_budget():
    seen = set()
    for name, body, meta in _kernels(_listing()):
        frag = _fragment(name)
        seen.add(frag)
        valu = sum(1 for line in body.split("\n") if re.match(r"\s+v_[a-z0-9_]+\s", line))
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", meta).group(1))
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", meta).group(1))
        print("%-64s VALU %5d (budget %5d)  VGPR %3d  scratch %d" % (frag, valu, BUDGET[frag], vgpr, scratch))
        assert scratch == 0, "%s: %d bytes of scratch (spills)" % (name, scratch)
        assert vgpr <= MAX_VGPR, "%s: %d VGPRs (budget %d: four waves per SIMD)" % (name, vgpr, MAX_VGPR)
        assert valu <= BUDGET[frag], "%s: %d VALU instructions (budget %d)" % (name, valu, BUDGET[frag])
    assert seen == set(BUDGET), "kernels not found in the listing: %s" % (set(BUDGET) - seen)


def test_the_listing_holds_every_unit_the_dispatch_can_choose():
    """nine units (smle_dispatch) times four kernels; the eq kernels expand the variables mle.hpp allows per launch"""
    src = open(os.path.join(CSRC, "capi.hip")).read()
    body = src[src.index("int smle_dispatch("):src.index("bool aligned16(")]
    assert len(re.findall(r"fn\(SmleKind<", body)) == 9
    assert len(BUDGET) == 36
    for fam, j in (("GoldilocksES3_Li2E", 3), ("GoldilocksES3_Li1E", 3), ("BabyBearES3_Li2E", 3), ("BabyBearES3_Li1E", 3), ("StarkENS_6StarkLELi4E", 2),
                   ("StarkES3_Li4E", 2), ("SlotG24E", 3), ("SlotB72E", 2), ("SlotFrogE", 3)):
        assert len([f for f in BUDGET if fam in f]) == 4, fam
        assert any(f.startswith("eq_kernel") and fam in f and f.endswith("Li%dEE" % j) for f in BUDGET), fam


def test_one_limb_accesses_are_sixteen_byte_and_the_streams_non_temporal():
    n = 0
    for name, body, _ in _kernels(_listing()):
        if not any(f in name for f in PAIRED):
            continue
        n += 1
        assert re.search(r"global_load_dwordx4", body), "%s: no 16-byte load" % name
        assert re.search(r"global_store_dwordx4", body), "%s: no 16-byte store" % name
        if "combine_kernel" not in name:
            assert re.search(r"global_store_dwordx4 .* nt\b", body), "%s: the output store is not non-temporal" % name
        if "fold_kernel" in name:  # vals is read once: non-temporal; the tables and the point stay cached
            assert re.search(r"global_load_dwordx4 .* nt\b", body), "%s: no non-temporal 16-byte load of the values" % name
            assert len(re.findall(r"global_load_dwordx4", body)) > len(re.findall(r"global_load_dwordx4 .* nt\b", body)), name
    assert n == 8, n
