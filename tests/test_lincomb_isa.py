"""Static budget of the linear-combination kernels (no GPU): hipcc -S of tools/ubench/lincomb_isa.hip, which instantiates every kernel
the launcher dispatches to (csrc/lincomb.hpp: kRegOutputs / kRunOutputs bound the outputs per launch), and a count of what the listing
holds.  The call streams, so a spill, a lost 16-byte or non-temporal access or a register count that costs a wave is a regression the
parity tests cannot see.  Registers, scratch, loads and stores are counted, nothing else."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "ubench", "lincomb_isa.hip")
OUT = os.path.join(ROOT, "build_tmp", "lincomb_isa_budget.s")
CSRC = os.path.join(ROOT, "stark_rings_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("lincomb.hpp", "sumcheck.hpp", "mle.hpp", "fields.hpp", "ntt_generic.hpp", "small_rings.hpp",
                                                "small_linalg.hpp", "frog_ring.hpp")]

# every kernel is __launch_bounds__(256): four waves per workgroup.  128 VGPRs keep four waves on each SIMD (512 registers per lane).
MAX_VGPR = 128
# kernel (mangled-name fragment; Li<M>: outputs of the launch; Lb1: coefficients in registers (K <= 4), Lb0: the run-time-K kernel) ->
# VALU instructions in the listing when the kernel was written (the one-limb kernels hold the 16-byte path and the one-coefficient
# fallback, both counted); the budget adds 2 %
WRITTEN = {
    "lincomb_kernelINS_10GoldilocksELi1ELb1E": 526, "lincomb_kernelINS_10GoldilocksELi2ELb1E": 1041,
    "lincomb_kernelINS_10GoldilocksELi1ELb0E": 545, "lincomb_kernelINS_10GoldilocksELi2ELb0E": 991,
    "lincomb_kernelINS_10GoldilocksELi3ELb0E": 1439,
    "lincomb_kernelINS_8BabyBearELi1ELb1E": 238, "lincomb_kernelINS_8BabyBearELi2ELb1E": 410,
    "lincomb_kernelINS_8BabyBearELi1ELb0E": 239, "lincomb_kernelINS_8BabyBearELi2ELb0E": 388,
    "lincomb_kernelINS_8BabyBearELi3ELb0E": 532, "lincomb_kernelINS_8BabyBearELi4ELb0E": 674,
    "lincomb_kernelINS_5StarkELi1ELb1E": 1452, "lincomb_kernelINS_5StarkELi1ELb0E": 1508,
    "slot_lincomb_kernelINS_7SlotG24ELi1ELb1E": 749, "slot_lincomb_kernelINS_7SlotG24ELi1ELb0E": 476,
    "slot_lincomb_kernelINS_7SlotB72ELi1ELb0E": 669,
    "slot_lincomb_kernelINS_8SlotFrogELi1ELb0E": 1068,
}
BUDGET = {k: v + v // 50 for k, v in WRITTEN.items()}
# family -> (ring id, outputs with the coefficients in registers, outputs per launch of the run-time-K kernel).  One output more
# needs (registers / run-time K): Goldilocks - / 166 VGPRs, Stark 188 / 152, goldilocks24 150 / 130, babybear72 194 (one output in
# registers) / 168, frog16 150 (one output in registers) / 188; BabyBear's four outputs take 72.
TOP = {"GoldilocksE": (0, 2, 3), "BabyBearE": (1, 2, 4), "StarkE": (2, 1, 1), "SlotG24E": (3, 1, 1), "SlotB72E": (4, 0, 1), "SlotFrogE": (5, 0, 1)}
ONE_LIMB = ("GoldilocksE", "BabyBearE")
REG_TABLES = 4


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
    for m in re.finditer(r"^(_ZN2sr7lincomb\w+):.*?\n(.*?)\.Lfunc_end", s, flags=re.S | re.M):
        name, body = m.group(1), m.group(2)
        meta = s[s.index(".amdhsa_kernel " + name):]
        yield name, body, meta[:meta.index(".end_amdhsa_kernel")]


def _fragment(name):
    frags = [f for f in BUDGET if "7lincomb%d%s" % (len(f.split("INS_")[0]), f) in name]
    assert len(frags) == 1, "no budget entry for %s" % name
    return frags[0]


def test_every_dispatched_kernel_stays_within_its_register_and_instruction_budget():
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
    """csrc/lincomb.hpp bounds the outputs of a launch by kRegOutputs / kRunOutputs, the launcher refuses anything above them and
    sr_lincomb_plan never exceeds them: the budget table holds M = 1 .. that bound of each kernel for every family and nothing else,
    and the plan shows the bounds in use."""
    from stark_rings_amd import _lib

    src = open(os.path.join(CSRC, "lincomb.hpp")).read()
    assert re.search(r"constexpr int kRegTables = %d;" % REG_TABLES, src)
    assert re.search(r"kRegOutputs = std::is_same<T, Goldilocks>::value \|\| std::is_same<T, BabyBear>::value \? 2\s*"
                     r": std::is_same<T, Stark>::value \|\| std::is_same<T, SlotG24>::value\s*\? 1\s*: 0;", src)
    assert re.search(r"kRunOutputs = std::is_same<T, BabyBear>::value \? 4 : std::is_same<T, Goldilocks>::value \? 3 : 1;", src)
    assert re.search(r"m > kRunOutputs<T> \|\| \(reg && m > kRegOutputs<T>\)", src), "the launcher bounds m"
    # every launch site of more than one output is guarded by the family's bound, and the register kernel by kRegOutputs
    sites = re.findall(r"(if constexpr \(kRunOutputs<T> >= (\d)\) )?launch_m<T, (\d)>", src)
    assert sorted(m for _, _, m in sites) == ["1", "2", "3", "4"]
    assert all((m == "1" and not guard) or bound == m for guard, bound, m in sites), sites
    assert len(re.findall(r"if constexpr \(M <= kRegOutputs<T>\) \{\s*if \(reg\) \{\s*hipLaunchKernelGGL\(\((?:slot_)?lincomb_kernel<T, M, true>\)", src)) == 2
    lib = _lib.load()
    for fam, (ring, reg_m, run_m) in TOP.items():
        assert sorted(int(f[-6]) for f in BUDGET if fam + "Li" in f and f.endswith("Lb1E")) == list(range(1, reg_m + 1)), fam
        assert sorted(int(f[-6]) for f in BUDGET if fam + "Li" in f and f.endswith("Lb0E")) == list(range(1, run_m + 1)), fam
        launches, per = ctypes.c_int(), ctypes.c_int()
        for K in (1, REG_TABLES, REG_TABLES + 1, 16):
            for M in (1, 2, 3, 4):
                assert lib.sr_lincomb_plan(ring, 4, K, M, ctypes.byref(launches), ctypes.byref(per)) == 0
                reg = K <= REG_TABLES and M <= reg_m
                assert per.value == (M if reg else min(M, run_m)), (fam, K, M, per.value)
                assert launches.value == -(-M // per.value), (fam, K, M)


def test_one_limb_accesses_are_sixteen_byte_and_non_temporal():
    """the aligned path of a one-limb kernel reads the table units of an element -- four: the register kernel's K <= 4, the run-time-K
    kernel's group of four -- with one non-temporal 16-byte load each and writes every output unit with one non-temporal 16-byte
    store; the 16-byte loads that are not non-temporal are the coefficient units (four per output) and the constants (one per
    output), which are re-read and keep the default cache policy; no other 16-byte store exists"""
    n = 0
    for name, body, _ in _kernels(_listing()):
        if not any(f in name for f in ONE_LIMB) or "slot_" in name:
            continue
        n += 1
        m = int(re.search(r"lincomb_kernelINS_\d+\w+?ELi(\d)ELb[01]E", name).group(1))
        assert len(re.findall(r"global_load_dwordx4 .* nt\b", body)) == REG_TABLES, name
        assert len(re.findall(r"global_store_dwordx4 .* nt\b", body)) == m, name
        assert len(re.findall(r"global_load_dwordx4", body)) == REG_TABLES + m * (REG_TABLES + 1), "%s: coefficient and constant units" % name
        assert len(re.findall(r"global_store_dwordx4", body)) == m, "%s: a 16-byte store that is not non-temporal" % name
    assert n == 11, n
