"""CPU checks of the sparse multilinear-extension entry points (include/stark_rings_hip.h: sr_eq_table*, sr_smle_fix_pattern,
sr_smle_plan, sr_smle_fix_variables*): the exports, the plan arithmetic and its workspace bound for every ring, the run pattern
against the model, the argument checks, the absence of a CPU fallback, and the pure-Python restatement of sparse.rs
(tools/model_sparse_mle.py, the oracle of tests/test_smle_gpu.py) against the closed form and the reference's own test vectors."""
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
import model_mle as MD  # noqa: E402
import model_sparse_mle as M  # noqa: E402

NEW = ("sr_eq_table_dev", "sr_eq_table", "sr_smle_fix_pattern", "sr_smle_plan", "sr_smle_fix_variables_dev", "sr_smle_fix_variables")
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "sparse_mle_kats.json")))


def _consts():
    from stark_rings_amd import rings

    return rings.SMLE_WINDOW_BITS, rings.SMLE_TABLE_MIN_NNZ, rings.SMLE_MAX_TABLE_ELEMS


def test_header_library_and_ctypes_table_carry_the_new_names():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "stark_rings_hip.h")).read()
    declared = set(re.findall(r"\b(sr_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared, "%s is not declared in the header" % name
        assert name in _lib.SYMBOLS, "%s is missing from _lib.SYMBOLS" % name
        assert hasattr(lib, name), "the library does not export %s" % name
    w, tmin, k = _consts()
    for name, value in (("SR_SMLE_WINDOW_BITS", w), ("SR_SMLE_TABLE_MIN_NNZ", tmin), ("SR_SMLE_MAX_TABLE_ELEMS", k)):
        assert re.search(r"#define %s %d\b" % (name, value), header), name
    assert k == -(-63 // w) << w


def _plan(ring, k, nnz, n_out, nf):
    work, launches = ctypes.c_size_t(1 << 60), ctypes.c_int(-1)
    rc = _lib.load().sr_smle_plan(ring, k, nnz, n_out, nf, ctypes.byref(work), ctypes.byref(launches))
    return rc, work.value, launches.value


@pytest.mark.parametrize("ring,k", [(0, 10), (0, 0), (0, 20), (1, 16), (2, 12), (3, 0), (4, 0), (5, 0)])
def test_plan_sweep_workspace_bound_and_launches(ring, k):
    """work_elems <= nnz + K with K the largest table set; launches >= 1; no workspace exactly where the header promises none: one
    launch, i.e. no tables (n_fixed < 2 or nnz below SR_SMLE_TABLE_MIN_NNZ) and no run that can cross a span (n_out == nnz, or a
    single span: nnz < 4 always is one)."""
    w, tmin, kmax = _consts()
    sizes = sorted({0, 1, 2, 3, 5, 17, 255, 256, 1000, tmin - 1, tmin, tmin + 1, 4097, 1 << 16, (1 << 20) - 1, 1 << 20})
    for nnz in sizes:
        for n_out in sorted({0 if nnz == 0 else 1, min(nnz, 2), nnz // 2, max(nnz - 1, 0), nnz}):
            if n_out > nnz or (nnz and not n_out):
                continue
            for nf in range(64):
                rc, work, launches = _plan(ring, k, nnz, n_out, nf)
                where = "ring %d k %d nnz %d n_out %d n_fixed %d: work %d launches %d" % (ring, k, nnz, n_out, nf, work, launches)
                assert rc == 0, where
                assert work <= nnz + kmax, where
                assert 1 <= launches <= 3, where
                tables = nf >= 2 and nnz >= tmin
                if launches == 1:
                    assert work == 0, where
                    assert not tables, where
                if nnz == 0 or nf == 0:
                    assert (work, launches) == (0, 1), where
                elif tables:
                    n_tab = -(-nf // min(w, nf))
                    assert work >= n_tab << min(w, nf) and launches >= 2, where
                elif n_out == nnz or nnz < 4:
                    assert (work, launches) == (0, 1), where
                else:
                    assert work <= nnz, where


def test_plan_refuses_bad_arguments():
    lib = _lib.load()
    work, launches = ctypes.c_size_t(), ctypes.c_int()
    for args, msg in (((0, 10, 4, 5, 2), "n_out exceeds nnz"), ((0, 10, 4, 0, 2), "n_out is zero"), ((0, 10, 4, 2, 64), "n_fixed must be below 64"),
                      ((6, 0, 4, 2, 2), "unknown ring"), ((0, 25, 4, 2, 2), "log2_degree")):
        assert lib.sr_smle_plan(*args, ctypes.byref(work), ctypes.byref(launches)) == 1, args
        assert msg in _lib.last_error(), (args, _lib.last_error())
    assert lib.sr_smle_plan(0, 10, 4, 2, 2, None, ctypes.byref(launches)) == 1
    assert "null" in _lib.last_error()


def _pattern(idx, nv, nf):
    from stark_rings_amd.rings import smle_fix_pattern

    return smle_fix_pattern(np.array(idx, dtype=np.uint64), nv, nf)


@pytest.mark.parametrize("nv", [0, 1, 5, 12, 33, 40, 63])
def test_fix_pattern_agrees_with_the_model(nv):
    rng = random.Random(400 + nv)
    sets = [[], [0], [(1 << nv) - 1]]
    for count in (2, 7, 300):
        if count <= 1 << nv:
            sets.append(sorted(rng.sample(range(1 << nv), count)) if nv <= 20 else sorted({rng.randrange(1 << nv) for _ in range(count)}))
    if nv >= 33:  # a cluster under one key beside keys above 2^32
        base = (1 << nv) - (1 << 12)
        sets.append(sorted(set(range(base, base + 500)) | {rng.randrange(1 << 32, 1 << nv) for _ in range(50)}))
    for idx in sets:
        for nf in sorted({0, min(1, nv), nv // 2, max(nv - 1, 0), nv}):
            keys, seg = _pattern(idx, nv, nf)
            mkeys, mseg = M.fix_pattern(idx, nf)
            assert keys.tolist() == mkeys and seg.tolist() == mseg, (nv, nf, len(idx))
            assert sorted({i >> nf for i in idx}) == mkeys


def test_fix_pattern_refuses_bad_arguments():
    from stark_rings_amd import RingError

    for idx, nv, nf, msg in (([1, 1], 4, 2, "strictly ascending"), ([3, 2], 4, 2, "strictly ascending"), ([0, 16], 4, 2, "not below 2\\^num_vars"),
                             ([0], 64, 2, "num_vars must be below 64"), ([0], 4, 5, "n_fixed exceeds num_vars")):
        with pytest.raises(RingError, match=msg):
            _pattern(idx, nv, nf)
    lib = _lib.load()
    buf = np.zeros(4, dtype=np.uint64)
    p = buf.ctypes.data_as(_lib.u64p)
    n = ctypes.c_size_t()
    assert lib.sr_smle_fix_pattern(p, 1, 4, 2, p, None, ctypes.byref(n)) == 1 and "null" in _lib.last_error()
    assert lib.sr_smle_fix_pattern(None, 1, 4, 2, p, p, ctypes.byref(n)) == 1 and "null" in _lib.last_error()
    assert lib.sr_smle_fix_pattern(p, 1, 4, 2, p, p, None) == 1 and "null" in _lib.last_error()
    assert lib.sr_smle_fix_pattern(None, 0, 4, 2, None, p, ctypes.byref(n)) == 0 and n.value == 0 and buf[0] == 0


def test_entry_points_refuse_a_null_context_before_anything_else():
    lib = _lib.load()
    buf = np.zeros(16, dtype=np.uint64)
    p, d = buf.ctypes.data_as(_lib.u64p), buf.ctypes.data
    n = ctypes.c_size_t()
    assert lib.sr_eq_table(None, p, p, 1) == 1 and "null context" in _lib.last_error()
    assert lib.sr_eq_table_dev(None, d, d, 1, None) == 1 and "null context" in _lib.last_error()
    assert lib.sr_smle_fix_variables(None, p, p, ctypes.byref(n), p, p, 1, 1, p, 1) == 1 and "null context" in _lib.last_error()
    assert lib.sr_smle_fix_variables_dev(None, d, d, d, 1, d, 1, d, 1, None, 0, None) == 1 and "null context" in _lib.last_error()


def test_no_cpu_fallback_for_the_sparse_mle_calls():
    """Without a HIP device there is no context, hence no fold and no eq table: nothing is quietly computed on the CPU."""
    try:
        import torch

        if torch.cuda.is_available():
            pytest.skip("a HIP device is present")
    except ImportError:
        pass
    from stark_rings_amd import CyclotomicRing, RingError

    with pytest.raises(RingError, match="no HIP device|no CPU fallback"):
        ring = CyclotomicRing("goldilocks", 6)
        ring.smle_fix_variables(np.zeros(2 << 6, dtype=np.uint64), np.array([0, 3], dtype=np.uint64), 2, np.zeros(2 << 6, dtype=np.uint64))


# ---- the restatement the GPU tests use as their oracle, pinned on a small prime field ---------------------------------------------
P = 2013265921
ADD, SUB, MUL = (lambda a, b: (a + b) % P), (lambda a, b: (a - b) % P), (lambda a, b: a * b % P)
OPS = (ADD, SUB, MUL, 0, 1)


@pytest.mark.parametrize("n", [0, 1, 2, 3, 6])
def test_precompute_eq_agrees_with_the_closed_form_product(n):
    rng = random.Random(20 + n)
    for _ in range(4):
        g = [rng.choice((0, 1, P - 1, rng.randrange(P))) for _ in range(n)]
        table = M.precompute_eq(g, SUB, MUL, 1)
        assert table == [M.eq_product(g, b, SUB, MUL, 1) for b in range(1 << n)]
        assert sum(table) % P == 1


@pytest.mark.parametrize("nv", [0, 1, 2, 3, 5])
def test_model_agrees_with_the_dense_closed_form(nv):
    rng = random.Random(3000 + nv)
    for count in sorted({0, 1, (1 << nv) // 2, 1 << nv}):
        idx = sorted(rng.sample(range(1 << nv), count))
        ev = {i: rng.choice((0, rng.randrange(P))) for i in idx}  # stored zeros included
        dense = [ev.get(i, 0) for i in range(1 << nv)]
        for nf in range(nv + 1):
            point = [rng.choice((0, 1, P - 1, rng.randrange(P))) for _ in range(nf)]
            got, rest = M.fix_variables(ev, nv, point, *OPS)
            assert rest == nv - nf and list(got) == M.fix_pattern(idx, nf)[0]  # every key stays, zero sums too
            want = MD.eq_closed_form(dense, nv, point, 0, P)
            assert [got.get(i, 0) for i in range(1 << rest)] == want
            if nf == nv:
                assert M.evaluate(ev, nv, point, *OPS) == want[0]


def test_model_reproduces_the_reference_matrix_vectors():
    for case in KATS["matrix_to_mle"]:
        rows, nrows, ncols = M.matrix_cast(case["matrix"])
        num_vars, ev = M.from_matrix(rows, nrows, ncols)
        assert (len(ev), num_vars) == (case["entries"], case["num_vars"])
        n_cols = M.next_pow2(ncols)
        s = M.ceil_log2(n_cols)
        for r in range(nrows):  # boolean row and column points pick the stored entry or zero
            for c in range(n_cols):
                i = r * n_cols + c
                bits = [(i >> b) & 1 for b in range(num_vars)]
                assert M.evaluate(ev, num_vars, bits, *OPS) == (case["matrix"][r][c] if c < ncols else 0)
        assert s + M.ceil_log2(M.next_pow2(nrows)) == num_vars


def test_model_reproduces_the_reference_vector_on_the_hypercube():
    kat = KATS["vec_to_mle"]
    ev = dict(enumerate(kat["z"]))
    nv = kat["n_vars"]
    for i, want in enumerate(kat["evaluate_on_hypercube"]):
        bits = [(i >> b) & 1 for b in range(nv)]
        assert M.evaluate(ev, nv, bits, *OPS) == want
