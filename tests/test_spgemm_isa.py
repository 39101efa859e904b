"""Static budget of the sparse-matrix kernels (no GPU): hipcc -S of tools/ubench/spgemm_isa.hip, which instantiates every gather /
transpose, numeric-phase and flag-count kernel the launchers of csrc/sparse_matrix.hpp dispatch to, and a count of what the listing
holds.  A spill or a register count that costs a wave is a regression the parity tests cannot see."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "ubench", "spgemm_isa.hip")
OUT = os.path.join(ROOT, "build_tmp", "spgemm_isa_budget.s")
CSRC = os.path.join(ROOT, "stark_rings_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("sparse_matrix.hpp", "mle.hpp", "fields.hpp", "ntt_generic.hpp", "small_rings.hpp", "small_linalg.hpp",
                                                "frog_ring.hpp", "stark_lazy.hpp")]

# every kernel is __launch_bounds__(256): four waves per workgroup.  128 VGPRs keep four waves on each SIMD (512 registers per lane).
# Every family meets it, the multi-limb ones included (Stark 56, Stark on lazy limbs 44, Frog-16 108).
MAX_VGPR = 128
# kernel (mangled-name fragment) -> max VALU instructions in the listing: what the compiler produced when the kernel was written, plus 2 %
BUDGET = {
    "count_dead_kernelE": 54,
    "move_kernelILi1E": 31,
    "move_kernelILi2E": 31,
    "spgemm_kernelINS_10GoldilocksE": 127,
    "spgemm_kernelINS_8BabyBearE": 49,
    "spgemm_kernelINS_5StarkE": 402,
    "spgemm_kernelINS_6StarkLE": 588,
    "slot_spgemm_kernelINS_7SlotG24E": 623,
    "slot_spgemm_kernelINS_7SlotB72E": 785,
    "slot_spgemm_kernelINS_8SlotFrogE": 1436,
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
    for m in re.finditer(r"^(_ZN2sr3spm\w+):.*?\n(.*?)\.Lfunc_end", s, flags=re.S | re.M):
        name, body = m.group(1), m.group(2)
        meta = s[s.index(".amdhsa_kernel " + name):]
        yield name, body, meta[:meta.index(".end_amdhsa_kernel")]


def _fragment(name):
    frags = [f for f in BUDGET if "3spm%d%s" % (len(re.split("INS_|ILi|E$", f)[0]), f) in name]
    assert len(frags) == 1, "no budget entry for %s" % name
    return frags[0]


def test_every_dispatched_sparse_matrix_kernel_stays_within_its_register_and_instruction_budget():
    seen = set()
    for name, body, meta in _kernels(_listing()):
        frag = _fragment(name)
        seen.add(frag)
        valu = sum(1 for line in body.split("\n") if re.match(r"\s+v_[a-z0-9_]+\s", line))
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", meta).group(1))
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", meta).group(1))
        print("%-36s VALU %5d (budget %5d)  VGPR %3d  scratch %d" % (frag, valu, BUDGET[frag], vgpr, scratch))
        assert scratch == 0, "%s: %d bytes of scratch (spills)" % (name, scratch)
        assert vgpr <= MAX_VGPR, "%s: %d VGPRs (budget %d: four waves per SIMD)" % (name, vgpr, MAX_VGPR)
        assert valu <= BUDGET[frag], "%s: %d VALU instructions (budget %d)" % (name, valu, BUDGET[frag])
    assert seen == set(BUDGET), "kernels not found in the listing: %s" % (set(BUDGET) - seen)


def test_every_kernel_the_launchers_name_is_in_the_budget_table():
    src = open(os.path.join(CSRC, "sparse_matrix.hpp")).read()
    kernels = set(re.findall(r"hipLaunchKernelGGL\(\(?(\w+)[<,]", src))
    assert kernels == {"move_kernel", "spgemm_kernel", "slot_spgemm_kernel", "count_dead_kernel"}, kernels
    for kernel in kernels:
        assert any(f.startswith(kernel) for f in BUDGET), kernel
