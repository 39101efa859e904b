"""Static residency check of the Goldilocks D = 2^16 rows kernels (no GPU): the fused products are built to share a CU five
workgroups at a time.  A CU of gfx950 gives each SIMD lane 512 vector registers, handed out in granules of 8, and the workgroups on it
160 KiB of LDS.  Five 256-lane workgroups (five waves per SIMD) therefore need
    512 / 5 = 102.4 -> rounded down to the granule: <= 96 registers per lane,
    160 KiB / 5                                  : <= 32 768 bytes of LDS per workgroup,
and no scratch (a spill is a regression the parity tests cannot see).  Same listing as tests/test_isa_budget.py."""
import re

from test_isa_budget import _listing

SIMD_VGPRS, VGPR_GRANULE, CU_LDS_BYTES, WORKGROUPS_PER_CU = 512, 8, 160 * 1024, 5
MAX_VGPR = SIMD_VGPRS // WORKGROUPS_PER_CU // VGPR_GRANULE * VGPR_GRANULE
MAX_LDS = CU_LDS_BYTES // WORKGROUPS_PER_CU
KERNELS = ("rows256_kernelILi2E", "rows256_kernelILi3E")


def test_bounds_are_those_of_five_workgroups_per_cu():
    assert (MAX_VGPR, MAX_LDS) == (96, 32768)


def test_fused_rows256_kernels_fit_five_workgroups_per_cu():
    s = _listing()
    seen = set()
    for name in re.findall(r"^\s*\.amdhsa_kernel (_Z\w+)", s, flags=re.M):
        frag = next((k for k in KERNELS if k in name), None)
        if frag is None:
            continue
        seen.add(frag)
        meta = s[s.index(".amdhsa_kernel " + name):]
        meta = meta[:meta.index(".end_amdhsa_kernel")]
        field = lambda key: int(re.search(r"\.amdhsa_%s\s+(\d+)" % key, meta).group(1))  # noqa: E731
        vgpr, lds, scratch = field("next_free_vgpr"), field("group_segment_fixed_size"), field("private_segment_fixed_size")
        print("%s: %d VGPRs, %d bytes of LDS, %d bytes of scratch" % (name, vgpr, lds, scratch))
        assert vgpr <= MAX_VGPR, "%s: %d VGPRs (five waves per SIMD need <= %d)" % (name, vgpr, MAX_VGPR)
        assert lds <= MAX_LDS, "%s: %d bytes of LDS (five workgroups per CU need <= %d)" % (name, lds, MAX_LDS)
        assert scratch == 0, "%s: %d bytes of scratch (spills)" % (name, scratch)
    assert seen == set(KERNELS), "kernels not found in the listing: %s" % (set(KERNELS) - seen)
