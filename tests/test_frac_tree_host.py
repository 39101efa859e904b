"""CPU checks of the fraction-tree entry points (include/stark_rings_hip.h: sr_frac_tree_plan, sr_frac_tree_dev, sr_frac_tree): the
exports, the plan arithmetic for every ring, the refusals that need no device, the layer offsets of the mirrors, and the
pair-at-a-time restatement of both orders (tools/model_frac_tree.py, the oracle of tests/test_frac_tree_gpu.py) against the closed
forms P = sum_i p_i prod_{j != i} q_j and Q = prod_j q_j, the product tree and the logUp identity; the pinned vectors of
tests/golden/frac_tree_kats.json regenerate byte for byte."""
import ctypes
import json
import os
import random
import re
import sys

import numpy as np
import pytest

from stark_rings_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import model_frac_tree as FT  # noqa: E402
import model_prod_tree as PT  # noqa: E402

NEW = ("sr_frac_tree_plan", "sr_frac_tree_dev", "sr_frac_tree")
LEADING, TRAILING = 0, 1
# levels one launch produces at most, per ring id (csrc/frac_tree.hpp: kMaxJ / kSlotMaxJ; tests/test_frac_tree_isa.py holds the counts)
JMAX = {0: 2, 1: 3, 2: 2, 3: 2, 4: 1, 5: 2}
RINGS = [(0, 10), (1, 16), (2, 12), (3, 0), (4, 0), (5, 0)]
PRIMES = [0xFFFFFFFF00000001, 2013265921, 0x800000000000011000000000000000000000000000000000000000000000001, 15912092521325583641]


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
    rc = lib.sr_frac_tree_plan(ring, k, nv, order, ctypes.byref(elems), ctypes.byref(launches))
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
    ids = dict(PT.POW2_RINGS, **{name: v[0] for name, v in PT.SLOT_RINGS.items()})
    assert JMAX == {ids[name]: j for name, j in FT.LEVELS_PER_LAUNCH.items()}, "the model's table of levels per launch"


def test_plan_refuses_bad_arguments():
    lib = _lib.load()
    elems, launches = ctypes.c_size_t(), ctypes.c_int()
    for args, msg in (((0, 10, 4, 2), "unknown order"), ((0, 10, 4, -1), "unknown order"), ((0, 10, 48, LEADING), "num_vars must be below 48"),
                      ((6, 0, 4, LEADING), "unknown ring"), ((-1, 0, 4, LEADING), "unknown ring"), ((0, 25, 4, LEADING), "log2_degree")):
        assert lib.sr_frac_tree_plan(*args, ctypes.byref(elems), ctypes.byref(launches)) == 1, args
        assert msg in _lib.last_error(), (args, _lib.last_error())
    assert lib.sr_frac_tree_plan(0, 10, 4, LEADING, None, ctypes.byref(launches)) == 1 and "null" in _lib.last_error()
    assert lib.sr_frac_tree_plan(0, 10, 4, LEADING, ctypes.byref(elems), None) == 1 and "null" in _lib.last_error()


def test_entry_points_refuse_a_null_context_before_anything_else():
    lib = _lib.load()
    buf = np.zeros(16, dtype=np.uint64)
    p = buf.ctypes.data_as(_lib.u64p)
    assert lib.sr_frac_tree(None, p, p, p, p, 1, 1, TRAILING) == 1 and "null context" in _lib.last_error()
    d = buf.ctypes.data
    assert lib.sr_frac_tree_dev(None, d, d, d, d, 1, 1, TRAILING, None) == 1 and "null context" in _lib.last_error()


def test_the_device_call_is_no_method_of_the_ring():
    """the device call lives in stark_rings_amd/frac_tree.py; CyclotomicRing gains nothing"""
    import stark_rings_amd as S
    from stark_rings_amd import frac_tree as mod

    assert not [n for n in dir(S.CyclotomicRing) if "frac_tree" in n]
    assert S.frac_tree is mod and callable(mod.frac_tree)   # the host-pointer form keeps the module's name: frac_tree.frac_tree
    for name in ("frac_tree_plan", "frac_tree_dev", "FractionTree"):
        assert getattr(S, name) is getattr(mod, name)


def test_no_cpu_fallback_for_the_fraction_tree():
    """Without a HIP device there is no context, hence no tree: the host-pointer call cannot quietly compute on the CPU."""
    try:
        import torch

        if torch.cuda.is_available():
            pytest.skip("a HIP device is present")
    except ImportError:
        pass
    from stark_rings_amd import CyclotomicRing, RingError
    from stark_rings_amd.frac_tree import frac_tree

    with pytest.raises(RingError, match="no HIP device|no CPU fallback"):
        ring = CyclotomicRing("goldilocks", 6)
        frac_tree(ring, None, np.zeros(4 << 6, dtype=np.uint64), 2)


def test_layer_offsets_of_the_mirrors():
    from stark_rings_amd import FractionTree

    for nv in range(1, 12):
        end = 0
        tree = FractionTree.__new__(FractionTree)   # the offsets are arithmetic on num_vars alone
        tree._num_vars = nv
        for k in range(1, nv + 1):
            assert FT.layer_offset(nv, k) == end == tree.layer_offset(k), (nv, k)
            end += 1 << (nv - k)
        assert end == (1 << nv) - 1
    hpp = open(os.path.join(ROOT, "include", "stark_rings.hpp")).read()
    body = hpp[hpp.index("class FractionTree"):]
    assert re.search(r"\(\(size_t\)1 << num_vars_\) - \(\(size_t\)1 << \(num_vars_ - k \+ 1\)\)", body), "FractionTree::layer_offset in stark_rings.hpp"


# ---- the restatement the GPU tests use as their oracle, pinned on integers modulo each prime --------------------------------------
def _ops(p):
    return 0, 1, (lambda a, b: (a + b) % p), (lambda a, b: a * b % p)


def _sizes(nv):
    full = 1 << nv
    return sorted({n for n in (0, 1, 5, full - 1, full) if 0 <= n <= full})


@pytest.mark.parametrize("p", PRIMES, ids=["goldilocks", "babybear", "stark", "frog"])
def test_the_root_is_the_closed_form_and_the_q_side_is_the_product_tree(p):
    zero, one, add, mul = _ops(p)
    rng = random.Random(p)
    draw = lambda: rng.choice((0, 1, p - 1, rng.randrange(p), rng.randrange(p)))  # noqa: E731
    for nv in range(6):
        for n in _sizes(nv):
            q = [draw() for _ in range(n)]
            stored = [draw() for _ in range(n)]
            for pl in (stored, None):
                num = pl if pl is not None else [1] * n
                want_p = 0
                for i in range(n):
                    term = num[i]
                    for j in range(n):
                        if j != i:
                            term = term * q[j] % p
                    want_p = (want_p + term) % p
                want_q = 1
                for x in q:
                    want_q = want_q * x % p
                for order in (LEADING, TRAILING):
                    ps, qs = FT.layers(pl, q, nv, order, zero, one, add, mul)
                    where = (nv, n, order, pl is None)
                    assert (ps[-1], qs[-1]) == ([want_p], [want_q]), where
                    assert qs == PT.layers(q, nv, order, one, mul), where
                    assert [len(x) for x in ps] == [len(x) for x in qs] == [1 << (nv - k) for k in range(nv + 1)]
                    fp, fq = FT.flat((ps, qs))
                    assert len(fp) == len(fq) == (1 << nv) - 1
                    for k in range(1, nv + 1):
                        off = FT.layer_offset(nv, k)
                        assert fp[off:off + (1 << (nv - k))] == ps[k] and fq[off:off + (1 << (nv - k))] == qs[k]
                    # a stored left child with an absent right child is passed up as it is
                    if nv and order == LEADING and n % 2:
                        assert (ps[1][n // 2], qs[1][n // 2]) == (num[n - 1], q[n - 1]), where
                    if pl is None and nv:   # level 1 of sum 1 / q_i is q_l + q_r where both are stored
                        half = 1 << (nv - 1)
                        for i in range(half):
                            l, r = (2 * i, 2 * i + 1) if order == LEADING else (i, i + half)
                            if r < n:
                                assert ps[1][i] == (q[l] + q[r]) % p, where
                            elif l < n:
                                assert ps[1][i] == 1, where
                            else:
                                assert (ps[1][i], qs[1][i]) == (0, 1), where


@pytest.mark.parametrize("p", PRIMES, ids=["goldilocks", "babybear", "stark", "frog"])
def test_the_logup_identity(p):
    """sum_j m_j / (alpha - t_j) - sum_i 1 / (alpha - a_i) = 0: 8 table values with their multiplicities and 20 lookups make 28 stored
    leaves of 32; the root numerator is exactly zero, and is not after one lookup is moved off the table"""
    zero, one, add, mul = _ops(p)
    rng = random.Random(p + 1)
    table = rng.sample(range(1, 1000), 8)
    lookups = [rng.choice(table) for _ in range(20)]
    alpha = rng.randrange(1 << 20, p)

    def root(lookups):
        p_leaves = [lookups.count(t) % p for t in table] + [p - 1] * len(lookups)
        q_leaves = [(alpha - t) % p for t in table] + [(alpha - a) % p for a in lookups]
        assert len(q_leaves) == 28
        out = []
        for order in (LEADING, TRAILING):
            ps, qs = FT.layers(p_leaves, q_leaves, 5, order, zero, one, add, mul)
            out.append((ps[-1][0], qs[-1][0]))
        assert out[0] == out[1]
        return out[0]

    num, den = root(lookups)
    assert num == 0 and den != 0
    off = list(lookups)
    off[7] = 1001   # not a table value
    num, den = root(off)
    assert num != 0 and den != 0


def test_the_pinned_vectors_regenerate_byte_for_byte():
    path = os.path.join(ROOT, "tests", "golden", "frac_tree_kats.json")
    assert open(path).read() == FT.dump_kats()
    cases = json.load(open(path))["cases"]
    assert sorted(c["ring_id"] for c in cases) == list(range(6))
    lib = _lib.load()
    for c in cases:
        elems, launches = ctypes.c_size_t(), ctypes.c_int()
        for key, order in (("leading", LEADING), ("trailing", TRAILING)):
            assert lib.sr_frac_tree_plan(c["ring_id"], c["log2_degree"], c["num_vars"], order, ctypes.byref(elems), ctypes.byref(launches)) == 0
            assert launches.value >= 2, c["ring"]   # every case crosses a launch boundary
            for tag in ("", "_no_numerators"):
                assert len(c[key + tag]["p"]) == len(c[key + tag]["q"]) == elems.value
            assert c[key]["q"] == c[key + "_no_numerators"]["q"]
        assert c["num_vars"] == max(JMAX[c["ring_id"]] + 1, 3)   # one more than a launch's levels, and room for the five leaves
        assert 0 < c["n_leaves"] < 1 << c["num_vars"] and len(c["p_leaves"]) == len(c["q_leaves"]) == c["n_leaves"] == 5
