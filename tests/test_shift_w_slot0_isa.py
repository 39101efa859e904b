"""Static check (no GPU) of what three changes took out of the D = 2^16 Goldilocks kernels: the shift products 2^32 .. 2^63 without a
borrow chain (Goldilocks::mad_eps_less_eps), the W layer of the column passes on the register side of the exchange (15 products per 16
coefficients, not 16) and the lazy slot-0 chain of the DFT_16 networks.  Counts instruction classes, VGPRs and scratch bytes in the
listing of tools/ubench/gl_isa.hip (the one tests/test_isa_budget.py compiles), against the figures of the listing before the change
(profiles/r08/isa_shift_w_slot0.txt, profiles/r08/isa_shift_q1.txt)."""
import re

import pytest

from test_cols_keep_isa import _kernel
from test_isa_budget import _listing

# mangled-name fragment -> (VALU, SALU-class, VGPRs) of the listing before, and the VALU instructions that had to go at least
PARENT = {
    "rows256_kernelILi2E": (2806, 2069, 94, 70),
    "cols256_keep_kernelILi0E": (1166, 957, 100, 34),
    "cols256_keep_kernelILi1E": (1202, 953, 102, 34),
}
PARENT_PROBE_POW2_48_VALU = 11   # profiles/r08/isa_shift_q1.txt: ten for the product (nine arithmetic, one v_mov of a zero), one address shift


def _counts(body):
    valu = sum(1 for line in body.split("\n") if re.match(r"\s+v_[a-z0-9_]+\s", line))
    salu = sum(1 for line in body.split("\n") if re.match(r"\s+s_[a-z0-9_]+\s", line))   # as tools/isa_count.py counts them
    return valu, salu


@pytest.mark.parametrize("frag", sorted(PARENT))
def test_headline_kernels_lost_the_instructions(frag):
    name, body, meta = _kernel(_listing(), frag)
    p_valu, p_salu, p_vgpr, min_saved = PARENT[frag]
    valu, salu = _counts(body)
    vgpr = int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", meta).group(1))
    scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", meta).group(1))
    print("%s: %d VALU (was %d), %d SALU-class (was %d), %d VGPRs (was %d), %d bytes of scratch" % (name, valu, p_valu, salu, p_salu, vgpr, p_vgpr, scratch))
    assert scratch == 0, "%s: %d bytes of scratch (spills)" % (name, scratch)
    assert vgpr <= p_vgpr, "%s: %d VGPRs (was %d)" % (name, vgpr, p_vgpr)
    assert valu <= p_valu - min_saved, "%s: %d VALU instructions (was %d, at least %d fewer asked)" % (name, valu, p_valu, min_saved)
    assert salu <= p_salu, "%s: %d SALU-class instructions (was %d)" % (name, salu, p_salu)


def test_isolated_middle_class_shift_product_is_shorter():
    name, body, _ = _kernel(_listing(), "probe_pow2ILi48E")
    valu, _ = _counts(body)
    print("%s: %d VALU (was %d)" % (name, valu, PARENT_PROBE_POW2_48_VALU))
    assert valu <= PARENT_PROBE_POW2_48_VALU - 1
