"""Static budget of the integer-column kernels (no GPU): hipcc -S of tools/ubench/lincomb_index_isa.hip, which instantiates every kernel
the launcher can dispatch (csrc/lincomb_index.hpp: kRegOutputs / kRunOutputs bound the outputs per launch), and a count of what the
listing holds: registers within the bound, zero scratch, and the 16-byte and non-temporal accesses of the one-limb pair path.
Nothing else is inspected."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "ubench", "lincomb_index_isa.hip")
OUT = os.path.join(ROOT, "build_tmp", "lincomb_index_isa_budget.s")
CSRC = os.path.join(ROOT, "stark_rings_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("lincomb_index.hpp", "lincomb.hpp", "sumcheck.hpp", "mle.hpp", "fields.hpp", "ntt_generic.hpp",
                                                "small_rings.hpp", "small_linalg.hpp", "frog_ring.hpp")]

# every kernel is __launch_bounds__(256): four waves per workgroup.  128 VGPRs keep four waves on each SIMD (512 registers per lane).
MAX_VGPR = 128
# kernel (mangled-name fragment; Li<M>: outputs of the launch; Lb1: coefficients in registers (K + J <= 4), Lb0: the run-time kernel) ->
# VGPRs of the listing when the kernel was written (the bound is MAX_VGPR; these are the record behind the plan's table)
WRITTEN = {
    "lincomb_index_kernelINS_10GoldilocksELi1ELb1E": 70, "lincomb_index_kernelINS_10GoldilocksELi2ELb1E": 120,
    "lincomb_index_kernelINS_10GoldilocksELi1ELb0E": 72, "lincomb_index_kernelINS_10GoldilocksELi2ELb0E": 106,
    "lincomb_index_kernelINS_10GoldilocksELi3ELb0E": 126,
    "lincomb_index_kernelINS_8BabyBearELi1ELb1E": 64, "lincomb_index_kernelINS_8BabyBearELi2ELb1E": 114,
    "lincomb_index_kernelINS_8BabyBearELi1ELb0E": 44, "lincomb_index_kernelINS_8BabyBearELi2ELb0E": 52,
    "lincomb_index_kernelINS_8BabyBearELi3ELb0E": 62, "lincomb_index_kernelINS_8BabyBearELi4ELb0E": 72,
    "lincomb_index_kernelINS_5StarkELi1ELb0E": 116,
    "slot_lincomb_index_kernelINS_7SlotG24ELi1ELb1E": 116, "slot_lincomb_index_kernelINS_7SlotG24ELi1ELb0E": 82,
    "slot_lincomb_index_kernelINS_7SlotB72ELi1ELb0E": 107,
    "slot_lincomb_index_kernelINS_8SlotFrogELi1ELb0E": 108,
    "index_count_kernelILb1E": 18, "index_count_kernelILb0E": 10,
}
# family -> (ring id, outputs with the coefficients in registers, outputs per launch of the run-time kernel).  One output more needs
# (registers / run-time): Goldilocks - / 166 VGPRs, Stark 156 (one output in registers) / 146, goldilocks24 178 / 134, babybear72 - /
# 170, frog16 149 (one output in registers) / 188
TOP = {"GoldilocksE": (0, 2, 3), "BabyBearE": (1, 2, 4), "StarkE": (2, 0, 1), "SlotG24E": (3, 1, 1), "SlotB72E": (4, 0, 1), "SlotFrogE": (5, 0, 1)}
ONE_LIMB = ("GoldilocksE", "BabyBearE")
REG_TERMS = 4


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
    for m in re.finditer(r"^(_ZN2sr13lincomb_index\w+):.*?\n(.*?)\.Lfunc_end", s, flags=re.S | re.M):
        name, body = m.group(1), m.group(2)
        meta = s[s.index(".amdhsa_kernel " + name):]
        yield name, body, meta[:meta.index(".end_amdhsa_kernel")]


def _fragment(name):
    frags = [f for f in WRITTEN if "13lincomb_index%d%s" % (len(re.match(r"[a-z_]+", f).group(0)), f) in name]
    assert len(frags) == 1, "no entry for %s" % name
    return frags[0]


def test_every_dispatched_kernel_stays_within_the_register_bound_without_scratch():
    seen = set()
    for name, body, meta in _kernels(_listing()):
        frag = _fragment(name)
        seen.add(frag)
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", meta).group(1))
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", meta).group(1))
        print("%-52s VGPR %3d (written %3d)  scratch %d" % (frag, vgpr, WRITTEN[frag], scratch))
        assert scratch == 0, "%s: %d bytes of scratch (spills)" % (name, scratch)
        assert vgpr <= MAX_VGPR, "%s: %d VGPRs (bound %d: four waves per SIMD)" % (name, vgpr, MAX_VGPR)
    assert seen == set(WRITTEN), "kernels not found in the listing: %s" % (set(WRITTEN) - seen)


def test_the_launcher_dispatches_only_what_the_listing_holds():
    """the table holds M = 1 .. the family's bound of each kernel and nothing else, and the plan shows the bounds in use"""
    import ctypes

    from stark_rings_amd import _lib

    lib = _lib.load()
    for fam, (ring, reg_m, run_m) in TOP.items():
        assert sorted(int(f[-6]) for f in WRITTEN if fam + "Li" in f and f.endswith("Lb1E")) == list(range(1, reg_m + 1)), fam
        assert sorted(int(f[-6]) for f in WRITTEN if fam + "Li" in f and f.endswith("Lb0E")) == list(range(1, run_m + 1)), fam
        launches, per = ctypes.c_int(), ctypes.c_int()
        for K, J in ((0, 1), (1, 2), (3, 1), (0, 4), (4, 1), (3, 2), (0, 8), (8, 8)):
            for M in (1, 2, 3, 4):
                assert lib.sr_lincomb_index_plan(ring, 4, K, J, M, ctypes.byref(launches), ctypes.byref(per)) == 0
                reg = K + J <= REG_TERMS and M <= reg_m
                assert per.value == (M if reg else min(M, run_m)), (fam, K, J, M, per.value)
                assert launches.value == -(-M // per.value), (fam, K, J, M)


def test_one_limb_accesses_are_sixteen_byte_and_non_temporal():
    """the aligned path of a one-limb kernel reads the table units of an element -- four: the register kernel's slots, the run-time
    kernel's group of four, which Goldilocks' run-time kernel holds twice (its sum of few canonical products and its lazy sum are
    two loops) -- with one non-temporal 16-byte load each and writes every output unit with one non-temporal 16-byte store; no other
    16-byte store exists, and every other 16-byte load (coefficient and constant units) keeps the default policy"""
    n = 0
    for name, body, _ in _kernels(_listing()):
        if not any(f in name for f in ONE_LIMB) or "slot_" in name or "index_count" in name:
            continue
        n += 1
        m = int(re.search(r"lincomb_index_kernelINS_\d+\w+?ELi(\d)ELb[01]E", name).group(1))
        loops = 2 if "GoldilocksE" in name and name.endswith("Lb0EEEvNS0_4ArgsEiimiim") else 1
        assert len(re.findall(r"global_load_dwordx4 .* nt\b", body)) == loops * REG_TERMS, name
        assert len(re.findall(r"global_store_dwordx4 .* nt\b", body)) == m, name
        assert len(re.findall(r"global_store_dwordx4", body)) == m, "%s: a 16-byte store that is not non-temporal" % name
        assert len(re.findall(r"global_load_dwordx4", body)) > REG_TERMS, "%s: coefficient units" % name
    assert n == 11, n
