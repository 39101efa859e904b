"""The case table of tests/test_dev_boundaries_gpu.py, checked without a GPU: it names every device-resident method of
CyclotomicRing, and its size rules really yield the coefficient counts they claim."""
import inspect

import pytest

import test_dev_boundaries_gpu as B

# the calls whose own GPU files already place their pointers 8 bytes behind a 16-byte boundary, with guards and poison
SHIFTED_IN_THEIR_OWN_FILES = {
    "mle_fix_variables_dev": "test_mle_gpu.py", "prod_tree_dev": "test_prod_tree_gpu.py", "mle_round_evals_dev": "test_sumcheck_gpu.py",
    "vpoly_round_evals_dev": "test_vpoly_gpu.py", "mle_round_fold_evals_dev": "test_sumcheck_fold_gpu.py",
    "vpoly_round_fold_evals_dev": "test_vpoly_fold_gpu.py", "eq_table_dev": "test_smle_gpu.py", "smle_fix_variables_dev": "test_smle_gpu.py",
    "norm_batch_dev": "test_norms_gpu.py", "linf_norm_dev": "test_norms_gpu.py", "l2_norm_squared_dev": "test_norms_gpu.py",
    "norms_dev": "test_norms_gpu.py", "gram_ntt_dev": "test_symm_gpu.py", "symm_recompose_dev": "test_symm_gpu.py",
    "gather_dev": "test_spgemm_gpu.py", "transpose_dev": "test_spgemm_gpu.py", "spgemm_ntt_dev": "test_spgemm_gpu.py",
}


def dev_methods():
    from stark_rings_amd import CyclotomicRing

    return sorted(n for n, f in inspect.getmembers(CyclotomicRing, inspect.isfunction) if n.endswith("_dev") and not n.startswith("_"))


def test_every_dev_method_is_in_the_table_or_the_named_list():
    tabled = [c for g in B.GROUPS.values() for c in g["calls"]]
    assert len(tabled) == len(set(tabled)), "a call stands in two groups"
    methods = dev_methods()
    assert len(methods) > 40
    missing = [n for n in methods if n not in tabled and n not in SHIFTED_IN_THEIR_OWN_FILES]
    assert not missing, "device calls without a placement test: %s" % ", ".join(missing)
    stale = [n for n in list(tabled) + list(SHIFTED_IN_THEIR_OWN_FILES) if n not in methods]
    assert not stale, "named, but no method of CyclotomicRing: %s" % ", ".join(stale)
    assert not set(tabled) & set(SHIFTED_IN_THEIR_OWN_FILES)


def test_every_group_has_its_test_in_the_gpu_file():
    """a group is a parametrised test over its rings: the table is what the tests iterate, not a copy of it"""
    source = inspect.getsource(B)
    for group, g in B.GROUPS.items():
        for call in g["calls"]:
            assert source.count(call) >= 2, "%s (%s) is named in the table only" % (call, group)


@pytest.mark.parametrize("group", sorted(g for g, v in B.GROUPS.items() if v["sizes"]))
def test_size_rules_yield_the_counts_they_claim(group):
    g = B.GROUPS[group]
    rule, span = B.SIZE_RULES[g["sizes"]]
    seen = set()
    for name, k in g["rings"]:
        d = B.degree(name, k)
        counts = [b * d for b in rule(d)]
        assert counts == sorted(set(counts)) and counts[0] == d, (name, k)
        below = [c for c in counts if c <= span - 2]
        assert below and max(below) + d > span - 2, (name, k, "the largest count not above span - 2")
        assert min(c for c in counts if c > span) - d <= span, (name, k, "the first count above one workgroup")
        assert (span in counts) == (span % d == 0), (name, k, "exactly one workgroup where the degree divides it")
        assert any(c > 2 * span and c % span for c in counts), (name, k, "above two workgroups, no multiple of one")
        assert all(c in counts for c in (1, 2, 3) if c % d == 0), (name, k, "one, two and three coefficients")
        if d == 1:   # k = 0: every odd batch is an odd count
            assert sum(c % 2 for c in counts) >= 3, (name, k)
            if span == 1024:
                assert 4 in counts and 5 in counts, (name, k, "a whole quad and a quad with a tail")
        seen.update(counts)
    assert span in seen and any(c > 2 * span for c in seen), group
    # reduce_dev runs at k >= 1 only: its odd counts are the odd in_len of its input rows
    assert any(c % 2 for c in seen) or group == "reduce", group


def test_the_rings_the_issue_names():
    assert set(B.RINGS) == {("goldilocks", 0), ("goldilocks", 1), ("goldilocks", 6), ("babybear", 0), ("babybear", 1), ("babybear", 5),
                            ("stark", 0), ("stark", 4), ("goldilocks24", 0), ("babybear72", 0), ("frog16", 0)}
    assert (B.degree("goldilocks", 1) // 2) % 2 == 1, "k = 1 makes D / 2 odd for rot"
    assert all(k >= 1 for _, k in B.REDUCE_RINGS) and {n for n, _ in B.REDUCE_RINGS} == {"goldilocks", "babybear", "stark"}
    assert {k for _, k in B.PACKED_NTT_RINGS} == {0, 4, 12}
    assert {("goldilocks", 6), ("goldilocks", 13), ("goldilocks", 16), ("babybear", 5), ("babybear", 12), ("babybear", 16), ("stark", 4),
            ("stark", 12)} <= set(B.NTT_RINGS)
    assert B.FOLD_LENGTHS == (1, 2, 3, 33, 67) and B.BASES == (2, 10, 1 << 16, (1 << 32) + 2) and B.WIDE_BASIS >= 1 << 64
