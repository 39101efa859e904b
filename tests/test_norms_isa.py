"""Static budget of the norm kernels (no GPU): hipcc -S of tools/ubench/norms_isa.hip, which instantiates every kernel the launcher of
csrc/norms.hpp dispatches to (wide, narrow and fold; four fields; three masks), and a count of what the listing holds.  The norms
stream, so a spill, a lost 16-byte access or a register count that costs a wave is a regression the parity tests cannot see."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "ubench", "norms_isa.hip")
OUT = os.path.join(ROOT, "build_tmp", "norms_isa_budget.s")
CSRC = os.path.join(ROOT, "stark_rings_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("norms.hpp", "decompose.hpp", "fields.hpp")]

# wide_kernel and narrow_kernel are __launch_bounds__(256): four waves per workgroup; 128 VGPRs keep four waves on each SIMD (512
# registers per lane), i.e. four workgroups per CU -- with eight (one-limb) or two (Stark) loads in flight per lane that is what keeps the
# memory system of a CU busy.  fold_kernel is __launch_bounds__(1024): sixteen waves per workgroup, four per SIMD, the same 128.
MAX_VGPR = 128
# kernel (mangled-name fragment) -> max VALU instructions in the listing: what the compiler produced when the kernel was written,
# plus 2 %
BUDGET = {
    "wide_kernelINS_10GoldilocksELi1E": 487,
    "narrow_kernelINS_10GoldilocksELi1E": 174,
    "fold_kernelINS_10GoldilocksELi1E": 177,
    "wide_kernelINS_10GoldilocksELi2E": 1029,
    "narrow_kernelINS_10GoldilocksELi2E": 287,
    "fold_kernelINS_10GoldilocksELi2E": 373,
    "wide_kernelINS_10GoldilocksELi3E": 1117,
    "narrow_kernelINS_10GoldilocksELi3E": 302,
    "fold_kernelINS_10GoldilocksELi3E": 411,
    "wide_kernelINS_8BabyBearELi1E": 451,
    "narrow_kernelINS_8BabyBearELi1E": 174,
    "fold_kernelINS_8BabyBearELi1E": 177,
    "wide_kernelINS_8BabyBearELi2E": 693,
    "narrow_kernelINS_8BabyBearELi2E": 226,
    "fold_kernelINS_8BabyBearELi2E": 373,
    "wide_kernelINS_8BabyBearELi3E": 820,
    "narrow_kernelINS_8BabyBearELi3E": 249,
    "fold_kernelINS_8BabyBearELi3E": 411,
    "wide_kernelINS_4FrogELi1E": 674,
    "narrow_kernelINS_4FrogELi1E": 229,
    "fold_kernelINS_4FrogELi1E": 177,
    "wide_kernelINS_4FrogELi2E": 1211,
    "narrow_kernelINS_4FrogELi2E": 349,
    "fold_kernelINS_4FrogELi2E": 373,
    "wide_kernelINS_4FrogELi3E": 1303,
    "narrow_kernelINS_4FrogELi3E": 365,
    "fold_kernelINS_4FrogELi3E": 411,
    "wide_kernelINS_5StarkELi1E": 1036,
    "narrow_kernelINS_5StarkELi1E": 945,
    "fold_kernelINS_5StarkELi1E": 331,
    "wide_kernelINS_5StarkELi2E": 1647,
    "narrow_kernelINS_5StarkELi2E": 1630,
    "fold_kernelINS_5StarkELi2E": 394,
    "wide_kernelINS_5StarkELi3E": 1829,
    "narrow_kernelINS_5StarkELi3E": 1807,
    "fold_kernelINS_5StarkELi3E": 529,
}
ONE_LIMB = ("10GoldilocksE", "8BabyBearE", "4FrogE")
# Every scalar instruction of the listing must be one of these: scalar ALU, control flow, waits, and -- the only scalar access to
# memory -- loads of kernel arguments and constants.  Records and partial records leave through vector stores; anything else a
# scalar unit could do to memory is not on the list and fails the test.
SCALAR_ALLOWED = re.compile(
    r"s_(nop|waitcnt\w*|barrier|endpgm|branch|cbranch_\w+|sleep|setprio|getpc_b64|setpc_b64|swappc_b64|version|code_end|"
    r"load_dword(x2|x4|x8|x16)?|buffer_load_dword(x2|x4|x8|x16)?|"
    r"(mov|movk|cmov|cmovk|cselect|add|addc|addk|sub|subb|mul|mulk|mul_hi|and|andn2|or|orn2|xor|xnor|nand|nor|not|lshl|lshr|ashr|bfe|bfm|"
    r"brev|abs|min|max|sext|ff0|ff1|flbit|bcnt0|bcnt1|bitcmp0|bitcmp1|bitset0|bitset1|lshl1_add|lshl2_add|lshl3_add|lshl4_add|pack_ll|"
    r"pack_lh|pack_hh|cmp_\w+|cmpk_\w+|wqm|quadmask)_[a-z0-9_]+|"
    r"(and|or|xor|andn2|orn2|nand|nor|xnor|andn1|orn1)_saveexec_b64)$")

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
    for m in re.finditer(r"^(_ZN2sr5norms\w+):.*?\n(.*?)\.Lfunc_end", s, flags=re.S | re.M):
        name, body = m.group(1), m.group(2)
        meta = s[s.index(".amdhsa_kernel " + name):]
        yield name, body, meta[:meta.index(".end_amdhsa_kernel")]


def _fragment(name):
    frags = [f for f in BUDGET if "5norms%d%s" % (len(f.split("INS_")[0]), f) in name]
    assert len(frags) == 1, "no budget entry for %s" % name
    return frags[0]


def test_every_dispatched_norm_kernel_stays_within_its_register_and_instruction_budget():
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
    assert len(BUDGET) == 3 * 4 * 3


def test_the_launcher_dispatches_only_what_the_listing_holds():
    """launch() of csrc/norms.hpp switches over the three masks and launch_w over the three kernels; the listing holds all of them for
    the four base fields DISPATCH_BASE_FIELD reaches."""
    src = open(os.path.join(CSRC, "norms.hpp")).read()
    assert sorted(set(re.findall(r"hipLaunchKernelGGL\(\((\w+)<F, W>\)", src))) == ["fold_kernel", "narrow_kernel", "wide_kernel"]
    names = [n for n, _, _ in _kernels(_listing())]
    for kern in ("11wide_kernel", "13narrow_kernel", "11fold_kernel"):
        for fam in ONE_LIMB + ("5StarkE",):
            for w in (1, 2, 3):
                assert any("%sINS_%sLi%dE" % (kern, fam, w) in n for n in names), (kern, fam, w)


def test_one_limb_wide_kernels_read_sixteen_bytes_non_temporal():
    n = 0
    for name, body, _ in _kernels(_listing()):
        if "wide_kernel" not in name or not any(f in name for f in ONE_LIMB):
            continue
        n += 1
        # kUnroll = 8 loads in flight per lane
        assert len(re.findall(r"global_load_dwordx4 .* nt\b", body)) >= 8, "%s: fewer than eight non-temporal 16-byte loads" % name
    assert n == 9, n


def test_records_leave_through_vector_stores_and_scalar_instructions_only_read_memory():
    s = _listing()
    scalar = set(re.findall(r"^\s+(s_[a-z0-9_]+)", s, flags=re.M))
    assert scalar, "no scalar instructions found: the listing is not what this test expects"
    unknown = sorted(m for m in scalar if not SCALAR_ALLOWED.match(m))
    assert not unknown, "scalar instructions outside the allowed set: %s" % unknown
    for name, body, _ in _kernels(s):
        assert re.search(r"global_store_dword", body), "%s: no vector store of its record" % name
        assert not re.search(r"global_atomic|flat_atomic|buffer_atomic", body), "%s: an atomic (the records need none)" % name
        assert not re.search(r"\bv_(add|mul|fma|mac|max|min)_f(16|32|64)\b", body), "%s: floating point in an exact integer reduction" % name
