"""CPU checks of the grand-product entry points (include/stark_rings_hip.h: sr_prod_tree_plan, sr_prod_tree_dev, sr_prod_tree): the
exports, the plan arithmetic for every ring, the refusals that need no device, the layer offsets of the mirrors, and the pair-at-a-time
restatement of both orders (tools/model_prod_tree.py, the oracle of tests/test_prod_tree_gpu.py) against the closed form; the pinned
vectors of tests/golden/prod_tree_kats.json regenerate byte for byte."""
import ctypes
import os
import random
import re
import sys

import numpy as np
import pytest

from stark_rings_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import model_prod_tree as PT  # noqa: E402

NEW = ("sr_prod_tree_plan", "sr_prod_tree_dev", "sr_prod_tree")
LEADING, TRAILING = 0, 1
# levels one launch produces at most, per ring id (csrc/prod_tree.hpp: kMaxJ / kSlotMaxJ; tests/test_prod_tree_isa.py holds the counts)
JMAX = {0: 3, 1: 3, 2: 3, 3: 3, 4: 2, 5: 3}
RINGS = [(0, 10), (1, 16), (2, 12), (3, 0), (4, 0), (5, 0)]


def test_header_library_and_ctypes_table_carry_the_new_names():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "stark_rings_hip.h")).read()
    declared = set(re.findall(r"\b(sr_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared, "%s is not declared in the header" % name
        assert name in _lib.SYMBOLS, "%s is missing from _lib.SYMBOLS" % name
        assert hasattr(lib, name), "the library does not export %s" % name


def _plan(ring, k, nv, order):
    lib = _lib.load()
    elems, launches = ctypes.c_size_t(1 << 60), ctypes.c_int(-1)
    rc = lib.sr_prod_tree_plan(ring, k, nv, order, ctypes.byref(elems), ctypes.byref(launches))
    return rc, elems.value, launches.value


@pytest.mark.parametrize("ring,k", RINGS)
def test_plan_for_every_ring_size_and_order(ring, k):
    for order in (LEADING, TRAILING):
        for nv in range(48):
            rc, elems, launches = _plan(ring, k, nv, order)
            where = "ring %d nv %d order %d: layer_elems %d launches %d" % (ring, nv, order, elems, launches)
            assert rc == 0, where
            assert elems == (1 << nv) - 1, where
            assert launches == -(-nv // JMAX[ring]), where   # full launches first, the remainder last; none for num_vars = 0


def test_plan_refuses_bad_arguments():
    lib = _lib.load()
    elems, launches = ctypes.c_size_t(), ctypes.c_int()
    for args, msg in (((0, 10, 4, 2), "unknown order"), ((0, 10, 4, -1), "unknown order"), ((0, 10, 48, LEADING), "num_vars must be below 48"),
                      ((6, 0, 4, LEADING), "unknown ring"), ((-1, 0, 4, LEADING), "unknown ring"), ((0, 25, 4, LEADING), "log2_degree")):
        assert lib.sr_prod_tree_plan(*args, ctypes.byref(elems), ctypes.byref(launches)) == 1, args
        assert msg in _lib.last_error(), (args, _lib.last_error())
    assert lib.sr_prod_tree_plan(0, 10, 4, LEADING, None, ctypes.byref(launches)) == 1 and "null" in _lib.last_error()
    assert lib.sr_prod_tree_plan(0, 10, 4, LEADING, ctypes.byref(elems), None) == 1 and "null" in _lib.last_error()


def test_entry_points_refuse_a_null_context_before_anything_else():
    lib = _lib.load()
    buf = np.zeros(16, dtype=np.uint64)
    p = buf.ctypes.data_as(_lib.u64p)
    assert lib.sr_prod_tree(None, p, p, 1, 1, TRAILING) == 1 and "null context" in _lib.last_error()
    assert lib.sr_prod_tree_dev(None, buf.ctypes.data, buf.ctypes.data, 1, 1, TRAILING, None) == 1 and "null context" in _lib.last_error()


def test_no_cpu_fallback_for_the_product_tree():
    """Without a HIP device there is no context, hence no tree: the host-pointer call cannot quietly compute on the CPU."""
    try:
        import torch

        if torch.cuda.is_available():
            pytest.skip("a HIP device is present")
    except ImportError:
        pass
    from stark_rings_amd import CyclotomicRing, RingError

    with pytest.raises(RingError, match="no HIP device|no CPU fallback"):
        ring = CyclotomicRing("goldilocks", 6)
        ring.prod_tree(np.zeros(4 << 6, dtype=np.uint64), 2)


def test_layer_offsets_of_the_mirrors():
    """layer k of 2^(n-k) elements at element offset 2^n - 2^(n-k+1): layer 1 first, the layers back to back, the root last -- in the
    model, in the Python class (whose offsets need no device) and in the text of the C++ class"""
    from stark_rings_amd import ProductTree
    from stark_rings_amd.grand_product import ProductTree as PT2

    assert ProductTree is PT2
    for nv in range(1, 12):
        end = 0
        tree = ProductTree.__new__(ProductTree)   # the offsets are arithmetic on num_vars alone
        tree._num_vars = nv
        for k in range(1, nv + 1):
            assert PT.layer_offset(nv, k) == end == tree.layer_offset(k), (nv, k)
            end += 1 << (nv - k)
        assert end == (1 << nv) - 1
        assert PT.layer_offset(nv, nv) == (1 << nv) - 2
    hpp = open(os.path.join(ROOT, "include", "stark_rings.hpp")).read()
    body = hpp[hpp.index("class ProductTree"):]
    assert re.search(r"\(\(size_t\)1 << num_vars_\) - \(\(size_t\)1 << \(num_vars_ - k \+ 1\)\)", body), "ProductTree::layer_offset in stark_rings.hpp"


# ---- the restatement the GPU tests use as their oracle, pinned on a small prime field ---------------------------------------------
P = 2013265921


def _closed_form(leaves, nv, order):
    """[L_0 .. L_nv] from the definition as products over index sets; absent leaves are one"""
    leaf = lambda i: leaves[i] if i < len(leaves) else 1  # noqa: E731
    out = []
    for k in range(nv + 1):
        layer = []
        for i in range(1 << (nv - k)):
            acc = 1
            for t in range(1 << k):
                acc = acc * leaf(i * (1 << k) + t if order == LEADING else i + t * (1 << (nv - k))) % P
            layer.append(acc)
        out.append(layer)
    return out


@pytest.mark.parametrize("nv", [0, 1, 2, 3, 4, 6])
def test_python_restatement_of_both_orders_agrees_with_the_closed_form(nv):
    rng = random.Random(2000 + nv)
    mul = lambda a, b: a * b % P  # noqa: E731
    full = 1 << nv
    for n_leaves in sorted({0, 1, full // 2, max(full - 1, 0), full, min(5, full)}):
        leaves = [rng.choice((0, 1, P - 1, rng.randrange(P), rng.randrange(P))) for _ in range(n_leaves)]
        for order in (LEADING, TRAILING):
            tree = PT.layers(leaves, nv, order, 1, mul)
            assert tree == _closed_form(leaves, nv, order), (nv, n_leaves, order)
            assert [len(layer) for layer in tree] == [1 << (nv - k) for k in range(nv + 1)]
            assert len(PT.flat(tree)) == full - 1
            for k in range(1, nv + 1):
                off = PT.layer_offset(nv, k)
                assert PT.flat(tree)[off:off + (1 << (nv - k))] == tree[k]
    # both orders multiply the same leaves: one root
    leaves = [rng.randrange(1, P) for _ in range(full)]
    assert PT.layers(leaves, nv, LEADING, 1, mul)[-1] == PT.layers(leaves, nv, TRAILING, 1, mul)[-1]


def test_the_pinned_vectors_regenerate_byte_for_byte():
    path = os.path.join(ROOT, "tests", "golden", "prod_tree_kats.json")
    assert open(path).read() == PT.dump_kats()
    import json

    cases = json.load(open(path))["cases"]
    assert sorted(c["ring_id"] for c in cases) == list(range(6))
    lib = _lib.load()
    for c in cases:
        elems, launches = ctypes.c_size_t(), ctypes.c_int()
        for key, order in (("leading", LEADING), ("trailing", TRAILING)):
            assert lib.sr_prod_tree_plan(c["ring_id"], c["log2_degree"], c["num_vars"], order, ctypes.byref(elems), ctypes.byref(launches)) == 0
            assert launches.value == 2, c["ring"]   # every case crosses a launch boundary
            assert len(c[key]) == elems.value
        assert 0 < c["n_leaves"] < 1 << c["num_vars"] and len(c["leaves"]) == c["n_leaves"]
        group = 1 << JMAX[c["ring_id"]]
        assert c["n_leaves"] % group != 0, "n_leaves on a group boundary of the leading order"
