"""Static check of the lane column kernels' addressing (no GPU): cols256_keep_kernel<0> / <1> form the global addresses of a ring
element's 32 coefficient accesses from wave-uniform scalar bases plus ONE lane offset per run of 16 (and an immediate where the
constant fits), not from one vector add per access.  Before that the listing held 1 292 / 1 324 VALU instructions and 120 / 126
VGPRs for one loop body, about 32 of the former feeding addresses (profiles/r07/isa_cols_keep.txt).  Same listing as
tests/test_isa_budget.py."""
import re

import pytest

from test_isa_budget import _listing

# mangled-name fragment -> (VALU instructions, VGPRs) of the kernel before the addressing moved to the scalar side
PARENT = {
    "cols256_keep_kernelILi0E": (1292, 120),
    "cols256_keep_kernelILi1E": (1324, 126),
}
MIN_VALU_SAVED = 24
MAX_ADDRESS_VALU_PER_ITERATION = 4
# vector instructions that could form an address: the 32-bit adds / ors the old listing used, and their wider or fused relatives
ADDRESS_OPS = re.compile(r"v_(add_u32|or_b32|add_co_u32|addc_co_u32|lshl_add_u32|lshl_or_b32|add3_u32|or3_b32|lshl_add_u64|add_lshl_u32)")
LABEL = re.compile(r"^(?:\.LBB\d+_\d+:|; %bb\.\d+:)(.*)$")
INSTR = re.compile(r"^\s+([a-z][a-z0-9_]+)\s+(.*?)\s*(?:;.*)?$")


def _regs(operand):
    """the 32-bit vector registers an operand names: v7 -> {7}, v[4:5] -> {4, 5}"""
    m = re.fullmatch(r"v(\d+)", operand)
    if m:
        return {int(m.group(1))}
    m = re.fullmatch(r"v\[(\d+):(\d+)\]", operand)
    return set(range(int(m.group(1)), int(m.group(2)) + 1)) if m else set()


def _kernel(s, frag):
    for m in re.finditer(r"^(_Z\w+):.*?\n(.*?)\.Lfunc_end", s, flags=re.S | re.M):
        if frag in m.group(1):
            meta = s[s.index(".amdhsa_kernel " + m.group(1)):]
            return m.group(1), m.group(2), meta[:meta.index(".end_amdhsa_kernel")]
    raise AssertionError("kernel not found in the listing: %s" % frag)


def _loop_lines(body):
    """the instructions of the blocks the assembler's comments place in the kernel's loop, in listing order"""
    out, inside = [], False
    for line in body.split("\n"):
        m = LABEL.match(line)
        if m:
            inside = "Loop" in m.group(1)
            continue
        if inside and INSTR.match(line) and not line.strip().startswith((".", ";")):
            out.append(line)
    return out


def _address_valu(loop):
    """(global accesses, the coefficient accesses among them that have a scalar base, listing lines of the vector adds / ors whose
    result is a global access's address).  Coefficient accesses: every store, and the loads outside the once-per-launch block
    (which holds the W table word and the 16 twist factors and follows the coefficient loads)."""
    last_def, feeding, accesses, loads, scalar_base = {}, set(), 0, 0, 0
    for n, line in enumerate(loop):
        op, rest = INSTR.match(line).groups()
        ops = [o.strip() for o in re.split(r",\s*(?![^\[]*\])", rest)]
        if op.startswith(("global_load", "global_store")):
            accesses += 1
            addr = ops[1] if op.startswith("global_load") else ops[0]
            loads += op.startswith("global_load")
            if op.startswith("global_store") or loads <= 16:
                scalar_base += bool(re.match(r"s\[\d+:\d+\]", ops[2].split()[0]))
            for r in _regs(addr):
                d = last_def.get(r)
                if d is not None and ADDRESS_OPS.fullmatch(re.sub(r"_e(32|64)$", "", d[1])):
                    feeding.add(d[0])
        if op.startswith("v_") or op.startswith(("global_load", "ds_read")):
            for r in _regs(ops[0]):
                last_def[r] = (n, op)
    return accesses, scalar_base, sorted(feeding)


@pytest.mark.parametrize("frag", sorted(PARENT))
def test_keep_kernel_addresses_come_from_scalar_bases(frag):
    name, body, meta = _kernel(_listing(), frag)
    parent_valu, parent_vgpr = PARENT[frag]
    valu = sum(1 for line in body.split("\n") if re.match(r"\s+v_[a-z0-9_]+\s", line))
    vgpr = int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", meta).group(1))
    scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", meta).group(1))
    loop = _loop_lines(body)
    accesses, scalar_base, feeding = _address_valu(loop)
    print("%s: %d VALU, %d VGPRs, %d bytes of scratch; loop: %d global accesses, %d coefficient accesses with a scalar base, %d vector adds / ors feed addresses"
          % (name, valu, vgpr, scratch, accesses, scalar_base, len(feeding)))
    assert scratch == 0, "%s: %d bytes of scratch (spills)" % (name, scratch)
    assert vgpr <= parent_vgpr, "%s: %d VGPRs (was %d)" % (name, vgpr, parent_vgpr)
    assert valu <= parent_valu - MIN_VALU_SAVED, "%s: %d VALU instructions (was %d, at least %d fewer asked)" % (
        name, valu, parent_valu, MIN_VALU_SAVED)
    # 16 loads + 16 stores of coefficients, the W table word and the 16 twist factors of iteration 0
    assert accesses == 49, "%s: %d global accesses in the loop" % (name, accesses)
    assert len(feeding) <= MAX_ADDRESS_VALU_PER_ITERATION, "%s: vector adds / ors feeding global addresses:\n%s" % (
        name, "\n".join(loop[n] for n in feeding))
    assert scalar_base == 32, "%s: %d of the 32 coefficient accesses have a scalar base" % (name, scalar_base)
