"""GPU parity of the sparse multilinear-extension calls (sr_eq_table[_dev], sr_smle_fix_variables[_dev]) for all six ring ids.  Every
comparison is bit-exact.  Expected values come from tools/model_sparse_mle.py, the restatement of crates/poly mle/sparse.rs:170-207
and 381-394 with the reference's own windows (pinned against the closed form by tests/test_smle_host.py): on standard-form Python
integers for the power-of-two rings, on the oracle's Fq3 / Fq9 / Fq4 slot products plus integer add / sub for the reference's own
rings.  The rings and degrees are those of tests/test_mle_gpu.py."""
import json
import os
import random
import sys

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import model_sparse_mle as M  # noqa: E402

pytestmark = pytest.mark.gpu
# (ring, log2 D, num_vars of the family's small sparse case)
CASES = [("goldilocks", 6, 10), ("goldilocks", 16, 4), ("babybear", 5, 9), ("stark", 4, 8), ("stark", 12, 3),
         ("goldilocks24", 0, 11), ("babybear72", 0, 9), ("frog16", 0, 11)]
LARGER = {("goldilocks", 16), ("stark", 12)}
IDS = ["%s-%d-nv%d" % c for c in CASES]
SMALL = [c for c in CASES if (c[0], c[1]) not in LARGER]
SMALL_IDS = ["%s-%d-nv%d" % c for c in SMALL]
BASE = {"goldilocks24": "goldilocks", "babybear72": "babybear", "frog16": "frog"}
SLOT_MUL = {"goldilocks24": ("sro_g24_ntt_mul", 3), "babybear72": ("sro_bb72_ntt_mul", 9), "frog16": ("sro_frog16_ntt_mul", 4)}
POISON = 0xDEADBEEFCAFEF00D  # not canonical in any of the fields: a kernel that read it would show it
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "sparse_mle_kats.json")))
WINDOW = 8  # SR_SMLE_WINDOW_BITS


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


_rings = {}


def ring_for(name, k):
    from stark_rings_amd import CyclotomicRing

    if (name, k) not in _rings:
        _rings[(name, k)] = CyclotomicRing(name, k, device=0)
    return _rings[(name, k)]


class Model:
    """the restatement's element type and operations for one ring"""

    def __init__(self, name, k):
        self.name, self.k = name, k
        self.ring = ring_for(name, k)
        self.F = O.FIELD_ID[BASE.get(name, name)]
        self.p = self.ring.modulus
        self.w = self.ring.words_per_elem
        self.pow2 = name not in SLOT_MUL
        p = self.p
        if self.pow2:  # elements: numpy object arrays of D standard-form integers
            self.add = lambda a, b: (a + b) % p
            self.sub = lambda a, b: (a - b) % p
            self.mul = lambda r, a: (r * a) % p
        else:          # elements: uint64 memory images; the product is the oracle's slot product
            fn = SLOT_MUL[name][0]
            self.add = lambda a, b: ((a.astype(object) + b.astype(object)) % p).astype(np.uint64)
            self.sub = lambda a, b: ((a.astype(object) - b.astype(object)) % p).astype(np.uint64)
            self.mul = lambda r, a: O.small(fn, a, r)

    def elems(self, words):
        words = np.ascontiguousarray(words, dtype=np.uint64)
        if self.pow2:
            ints = np.array(O.from_mont(self.F, words), dtype=object) if words.size else np.zeros(0, dtype=object)
            return [ints[i * self.ring.degree:(i + 1) * self.ring.degree] for i in range(words.size // self.w)]
        return [words[i * self.w:(i + 1) * self.w].copy() for i in range(words.size // self.w)]

    def words(self, elems):
        if not elems:
            return np.zeros(0, dtype=np.uint64)
        if self.pow2:
            return O.to_mont(self.F, [int(x) for e in elems for x in e])
        return np.concatenate(elems)

    def zero(self):
        return np.array([0] * self.ring.degree, dtype=object) if self.pow2 else np.zeros(self.w, dtype=np.uint64)

    def one_words(self):
        m1 = O.to_mont(self.F, [1])
        if self.pow2:
            return np.tile(m1, self.ring.degree)
        out = np.zeros(self.w, dtype=np.uint64)
        out[::SLOT_MUL[self.name][1]] = m1[0]
        return out

    def one(self):
        return self.elems(self.one_words())[0]

    def ops(self):
        return self.add, self.sub, self.mul, self.zero(), self.one()

    def uniform(self, seed, n_elems):
        return O.fill_uniform(self.F, seed, 0, n_elems * self.ring.degree)

    def const(self, value, n_elems=1):
        """the constant ring element `value` (an integer embedded in the base ring) in CRT/NTT form"""
        return np.tile(self.ring.add_scalar(np.zeros(self.w, dtype=np.uint64), O.to_mont(self.F, [value % self.p]), True), n_elems)

    def point(self, seed, n):
        """n point elements drawn from {0, 1, p - 1, random}"""
        rng = random.Random(seed)
        rnd = self.uniform(seed, max(n, 1))
        parts = []
        for i in range(n):
            kind = rng.randrange(4)
            parts.append(rnd[i * self.w:(i + 1) * self.w] if kind == 3 else self.const((0, 1, self.p - 1)[kind]))
        return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint64)

    def expect_fold(self, idx, vals, nv, point):
        """(keys, memory words of the folded values) by the reference's own windowing"""
        ev = dict(zip([int(i) for i in idx], self.elems(vals)))
        got, _ = M.fix_variables(ev, nv, self.elems(point), *self.ops())
        return list(got), self.words(list(got.values()))


_models = {}


def model_for(name, k):
    if (name, k) not in _models:
        _models[(name, k)] = Model(name, k)
    return _models[(name, k)]


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def fold_dev(torch, ring, t_vals, idx, nv, t_point, stream=None, tail=2):
    """the _dev call with a poisoned workspace of exactly the planned size and a poisoned output tail; returns (keys, out words)"""
    from stark_rings_amd.rings import smle_fix_pattern

    w = ring.words_per_elem
    nf = t_point.numel() // w
    keys, seg = smle_fix_pattern(idx, nv, nf)
    work_elems, launches = ring.smle_plan(len(idx), len(keys), nf)
    out = torch.full(((len(keys) + tail) * w,), POISON - (1 << 64), dtype=torch.int64, device="cuda")
    work = torch.full((work_elems * w,), POISON - (1 << 64), dtype=torch.int64, device="cuda") if work_elems else None
    if len(keys):
        ring.smle_fix_variables_dev(out[:len(keys) * w], t_vals, dev(torch, np.asarray(idx, dtype=np.uint64)), dev(torch, seg), t_point, work, stream)
    torch.cuda.synchronize()
    got = host(out)
    assert (got[len(keys) * w:] == POISON).all(), "the output tail was written"
    return keys.tolist(), got[:len(keys) * w]


def check_fold(torch, m, idx, vals, nv, point, what):
    ring = m.ring
    t_vals, t_point = dev(torch, vals), dev(torch, point)
    keys, got = fold_dev(torch, ring, t_vals, idx, nv, t_point)
    want_keys, want = m.expect_fold(idx, vals, nv, point)
    assert keys == want_keys, what
    assert not (got == POISON).any(), "%s: poison (an unwritten workspace or output word) shows" % (what,)
    assert np.array_equal(got, want), what
    if got.size:
        assert ring.count_noncanonical_dev(dev(torch, got)) == 0
    assert np.array_equal(host(t_vals), vals) and np.array_equal(host(t_point), point), "an input was written"
    return keys, got


# ---- the eq table ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k,nv", CASES, ids=IDS)
def test_eq_table_matches_the_doubling_recurrence(torch_cuda, name, k, nv):
    torch = torch_cuda
    m = model_for(name, k)
    ring, w = m.ring, m.w
    top = {("goldilocks", 16): 4, ("stark", 12): 3}.get((name, k), 12)
    point = m.point(0x500 + k, top)
    P = m.elems(point)
    t_point = dev(torch, point)
    for n in range(top + 1):
        want = m.words(M.precompute_eq(P[:n], m.sub, m.mul, m.one()))
        out = torch.full(((1 << n) * w + w,), POISON - (1 << 64), dtype=torch.int64, device="cuda")
        ring.eq_table_dev(out[:w << n], t_point[:n * w])
        torch.cuda.synchronize()
        got = host(out)
        assert np.array_equal(got[:w << n], want), (name, n)
        assert (got[w << n:] == POISON).all()
        assert np.array_equal(ring.eq_table(point[:n * w]), want), "host-pointer form, n %d" % n
        s = torch.zeros(w, dtype=torch.int64, device="cuda")
        ring.sum_dev(s, out[:w << n])
        torch.cuda.synchronize()
        assert np.array_equal(host(s), m.one_words()), "sum_b eq[b] is not one(), n %d" % n
    assert np.array_equal(host(t_point), point)
    # unaligned buffers take the one-coefficient path: an offset of one word
    if m.pow2 and ring.limbs == 1 and k >= 1:
        n = min(top, 5)
        pool = torch.zeros((w << n) + 1 + n * w + 1, dtype=torch.int64, device="cuda")
        pool[(w << n) + 2:(w << n) + 2 + n * w] = t_point[:n * w]
        ring.eq_table_dev(pool[1:1 + (w << n)], pool[(w << n) + 2:(w << n) + 2 + n * w])
        torch.cuda.synchronize()
        assert np.array_equal(host(pool[1:1 + (w << n)]), m.words(M.precompute_eq(P[:n], m.sub, m.mul, m.one())))


@pytest.mark.parametrize("name,k,nv", CASES, ids=IDS)
def test_eq_table_evaluates_a_dense_table(torch_cuda, name, k, nv):
    """sum_b eq[b] f[b], composed from sr_mul_elem_add_batch_dev, equals the dense evaluate of f"""
    torch = torch_cuda
    from stark_rings_amd import DenseMultilinearExtension

    m = model_for(name, k)
    ring, w = m.ring, m.w
    n = min(nv, 6)
    f, point = m.uniform(0x610 + n, 1 << n), m.uniform(0x620 + n, n)
    t_f, t_point = dev(torch, f), dev(torch, point)
    eq = DenseMultilinearExtension.eq(ring, t_point)
    assert eq.num_vars == n and len(eq) == 1 << n
    acc = torch.zeros(w, dtype=torch.int64, device="cuda")
    for b in range(1 << n):
        ring.mul_elem_add_dev(acc, t_f[b * w:(b + 1) * w], eq.evaluations[b * w:(b + 1) * w].clone())
    want = DenseMultilinearExtension(ring, n, t_f).evaluate(t_point)
    torch.cuda.synchronize()
    assert np.array_equal(host(acc), host(want)), name


# ---- the sparse fold ---------------------------------------------------------------------------------------------------------------
def index_sets(rng, nv):
    full = list(range(1 << nv))
    return {"empty": [], "one": [rng.randrange(1 << nv)], "all": full, "rand": sorted(rng.sample(full, 1 << (nv // 2)))}


@pytest.mark.parametrize("name,k,nv", CASES, ids=IDS)
def test_small_index_sets_every_n_fixed(torch_cuda, name, k, nv):
    torch = torch_cuda
    m = model_for(name, k)
    rng = random.Random(0x700 + nv)
    for sname, idx in index_sets(rng, nv).items():
        vals = m.uniform(0x710 + len(idx), len(idx))
        if len(idx) >= 4:  # stored zeros stay stored
            vals[:m.w] = 0
        steps = range(nv + 1) if sname != "all" or (name, k) not in LARGER else (0, 1, nv)
        for nf in steps:
            point = m.point(0x720 + nf, nf)
            keys, got = check_fold(torch, m, idx, vals, nv, point, "%s %s n_fixed %d" % (name, sname, nf))
            assert len(keys) == len({i >> nf for i in idx})  # zero sums and stored zeros stay in the output
            hv, hi = m.ring.smle_fix_variables(vals, np.array(idx, dtype=np.uint64), nv, point)
            assert hi.tolist() == keys and np.array_equal(hv, got), "host-pointer form %s n_fixed %d" % (sname, nf)


@pytest.mark.parametrize("name,k,nv", SMALL, ids=SMALL_IDS)
def test_a_run_that_sums_to_zero_stays(torch_cuda, name, k, nv):
    """indices 4 and 5 share key 2 once variable 0 is fixed; at r = 2 their weights are 1 - r = -1 and r = 2, so the values
    v = 2 v' and v' cancel: -2 v' + 2 v' = 0.  The key stays in the output with a zero element, as in the reference's map."""
    torch = torch_cuda
    m = model_for(name, k)
    vp = m.uniform(0x7A0, 1)
    v = m.ring.add(vp.copy(), vp)
    vals = np.concatenate([v, vp, m.uniform(0x7A1, 1)])
    idx = [4, 5, 9]
    keys, got = check_fold(torch, m, idx, vals, nv, m.const(2), "zero-sum run")
    assert keys == [2, 4] and not got[:m.w].any() and got[m.w:].any()


@pytest.mark.parametrize("name,k,nv", SMALL, ids=SMALL_IDS)
def test_a_long_cluster_beside_singletons(torch_cuda, name, k, nv):
    """thousands of entries under one key beside many keys of one entry: runs cut into spans (partial elements and the combine
    launch) and runs inside a span in one call; tables in use (nnz >= SR_SMLE_TABLE_MIN_NNZ), on both sides of the window"""
    torch = torch_cuda
    m = model_for(name, k)
    nvars = 24
    rng = random.Random(0x800 + k)
    cluster = [(5 << 12) + i for i in sorted(rng.sample(range(1 << 12), 2500))]
    singles = sorted({(rng.randrange(6, 1 << 12) << 12) + rng.randrange(1 << 12) for _ in range(600)} | {(2 << 12) + 7, (2 << 12) + 9})
    idx = sorted(set(cluster) | set(singles))
    vals = m.uniform(0x810, len(idx))
    for nf in (12, WINDOW - 1, WINDOW, WINDOW + 1, 2 * WINDOW, 2 * WINDOW + 1, nvars):
        work, launches = m.ring.smle_plan(len(idx), len({i >> nf for i in idx}), nf)
        assert launches == 3 and work > 0
        check_fold(torch, m, idx, vals, nvars, m.point(0x820 + nf, nf), "%s cluster n_fixed %d" % (name, nf))


@pytest.mark.parametrize("name,k,nv", SMALL, ids=SMALL_IDS)
def test_forty_variables_and_indices_above_two_to_the_32(torch_cuda, name, k, nv):
    torch = torch_cuda
    m = model_for(name, k)
    rng = random.Random(0x900 + k)
    idx = sorted({rng.randrange(1 << 40) for _ in range(1 << 10)} | {(1 << 40) - 1, 1 << 39})[:1 << 10]
    assert max(idx) > 1 << 32
    vals = m.uniform(0x910, len(idx))
    for nf in (1, WINDOW, WINDOW + 1, 4 * WINDOW, 4 * WINDOW + 1, 39, 40):
        check_fold(torch, m, idx, vals, 40, m.point(0x920 + nf, nf), "%s nv 40 n_fixed %d" % (name, nf))
    # below the table threshold the same point is multiplied in on the fly
    few = idx[::8]
    check_fold(torch, m, few, m.uniform(0x930, len(few)), 40, m.point(0x940, 40), "%s nv 40 on the fly" % name)


@pytest.mark.parametrize("name,k,nv", CASES, ids=IDS)
def test_sparse_fold_equals_the_dense_fold_of_the_scattered_table(torch_cuda, name, k, nv):
    """no model: SparseMultilinearExtension against sr_mle_fix_variables_dev(SR_MLE_LEADING) of to_evaluations()"""
    torch = torch_cuda
    from stark_rings_amd import DenseMultilinearExtension, SparseMultilinearExtension

    m = model_for(name, k)
    ring, w = m.ring, m.w
    n = min(nv, 12)
    rng = random.Random(0xA00 + n)
    for idx in (list(range(1 << n)), sorted(rng.sample(range(1 << n), max(1, (1 << n) // 3)))):
        vals = m.uniform(0xA10 + len(idx), len(idx))
        point = m.uniform(0xA20, n)
        t_point = dev(torch, point)
        sp = SparseMultilinearExtension(ring, n, np.array(idx, dtype=np.uint64), dev(torch, vals))
        dense = DenseMultilinearExtension(ring, n, sp.to_evaluations())
        for nf in sorted({0, 1, n // 2, n}):
            a = sp.fixed_variables(t_point[:nf * w])
            b = dense.fixed_variables(t_point[:nf * w])
            torch.cuda.synchronize()
            assert a.num_vars == n - nf and np.array_equal(host(a.to_evaluations()), host(b.to_evaluations())), (name, len(idx), nf)
        assert np.array_equal(host(sp.evaluate(t_point)), host(dense.evaluate(t_point)))
        assert len(sp) == len(idx) and sp.num_vars == n
        j = len(idx) // 2
        assert np.array_equal(host(sp[idx[j]]), vals[j * w:(j + 1) * w])
        neg = sp.neg()
        assert np.array_equal(host(neg.values), ring.neg(vals.copy())) and np.array_equal(host(sp.values), vals)
    empty = SparseMultilinearExtension(ring, n, np.zeros(0, dtype=np.uint64), dev(torch, np.zeros(0, dtype=np.uint64)))
    assert not host(empty.evaluate(t_point)).any() and len(empty.fixed_variables(t_point[:w])) == 0 and not host(empty[3]).any()


@pytest.mark.parametrize("name", ["goldilocks", "goldilocks24"])
def test_reference_vectors_end_to_end(torch_cuda, name):
    """sparse.rs:463-510 on device: integers embedded as constant elements"""
    torch = torch_cuda
    from stark_rings_amd import SparseMultilinearExtension

    k = 6 if name == "goldilocks" else 0
    m = model_for(name, k)
    ring = m.ring
    bits = lambda i, n: dev(torch, np.concatenate([m.const((i >> b) & 1) for b in range(n)]))
    kat = KATS["vec_to_mle"]
    z = SparseMultilinearExtension.from_slice(ring, kat["n_vars"], dev(torch, np.concatenate([m.const(v) for v in kat["z"]])))
    for i, want in enumerate(kat["evaluate_on_hypercube"]):
        assert np.array_equal(host(z.evaluate(bits(i, kat["n_vars"]))), m.const(want)), (name, i)
    for case in KATS["matrix_to_mle"]:
        rows, nrows, ncols = M.matrix_cast(case["matrix"])
        cols = np.array([c for row in rows for _, c in row], dtype=np.int32)
        row_ptr = np.cumsum([0] + [len(row) for row in rows]).astype(np.int64)
        vals = np.concatenate([m.const(v) for row in rows for v, _ in row])
        a = SparseMultilinearExtension.from_matrix(ring, dev(torch, vals), cols, row_ptr, nrows, ncols)
        assert (len(a), a.num_vars) == (case["entries"], case["num_vars"])
        n_cols = M.next_pow2(ncols)
        for r in range(nrows):
            for c in range(n_cols):
                want = case["matrix"][r][c] if c < ncols else 0
                assert np.array_equal(host(a.evaluate(bits(r * n_cols + c, a.num_vars))), m.const(want)), (name, r, c)


@pytest.mark.parametrize("name,k,nv", SMALL, ids=SMALL_IDS)
def test_from_matrix_on_the_csr_triple_of_a_sparse_matvec(torch_cuda, name, k, nv):
    torch = torch_cuda
    from stark_rings_amd import SparseMultilinearExtension

    m = model_for(name, k)
    ring, w = m.ring, m.w
    nrows, ncols = 5, 6
    rng = random.Random(0xB00 + k)
    rows = [sorted(rng.sample(range(ncols), rng.randrange(0, 5))) for _ in range(nrows)]
    rows[2] = rows[2][::-1] if len(rows[2]) > 1 else [4, 1]  # one row with descending columns: the values are permuted
    cols = np.array([c for row in rows for c in row], dtype=np.int32)
    row_ptr = np.cumsum([0] + [len(row) for row in rows]).astype(np.int64)
    vals = m.uniform(0xB10, cols.size)
    t_vals, t_cols, t_ptr = dev(torch, vals), torch.from_numpy(cols).cuda(), torch.from_numpy(row_ptr).cuda()
    v = m.uniform(0xB20, ncols)
    y = torch.zeros(nrows * w, dtype=torch.int64, device="cuda")
    ring.spmv_ntt_dev(y, t_vals, t_cols, t_ptr, dev(torch, v), nrows, ncols)
    a = SparseMultilinearExtension.from_matrix(ring, t_vals, t_cols, t_ptr, nrows, ncols)
    assert a.num_vars == 6 and len(a) == cols.size
    one, zero = m.one_words(), np.zeros(w, dtype=np.uint64)
    entry = {(r, c): vals[j * w:(j + 1) * w] for j, (r, c) in enumerate((r, c) for r, row in enumerate(rows) for c in row)}
    for r in range(8):
        for c in range(8):
            i = r * 8 + c
            pt = dev(torch, np.concatenate([one if (i >> b) & 1 else zero for b in range(6)]))
            assert np.array_equal(host(a.evaluate(pt)), entry.get((r, c), zero)), (name, r, c)
    assert np.array_equal(host(a.values), np.concatenate([entry[key] for key in sorted(entry)]))  # ascending index = (row, column) order
    for r, row in enumerate(rows):  # the same triple drives the mat-vec
        want = np.zeros(w, dtype=np.uint64)
        for c in row:
            want = ring.add(want, ring.ntt_mul(entry[(r, c)].copy(), v[c * w:(c + 1) * w]))
        assert np.array_equal(host(y[r * w:(r + 1) * w]), want), (name, r)


def test_workspace_overlap_and_argument_refusals(torch_cuda):
    torch = torch_cuda
    from stark_rings_amd import RingError, SparseMultilinearExtension, _lib
    from stark_rings_amd.rings import smle_fix_pattern

    ring = ring_for("goldilocks", 6)
    lib, ctx, w = ring._lib, ring._ctx, ring.words_per_elem
    E = w * 8
    nnz, nv, nf = 2048, 16, 12
    idx = np.arange(nnz, dtype=np.uint64) * 3
    keys, seg = smle_fix_pattern(idx, nv, nf)
    n_out = len(keys)
    need, launches = ring.smle_plan(nnz, n_out, nf)
    assert need > 0 and launches == 3
    pool = torch.zeros((2 * nnz + 64 + need + n_out) * w, dtype=torch.int64, device="cuda")
    base = pool.data_ptr()
    vals, point, out, work = base, base + nnz * E, base + (nnz + 32) * E, base + (nnz + 32 + n_out + 8) * E
    d_idx, d_seg = dev(torch, idx), dev(torch, seg)
    pi, ps = d_idx.data_ptr(), d_seg.data_ptr()

    def call(o, v, i, n, s, no, p, f, wk, wn):
        return lib.sr_smle_fix_variables_dev(ctx, o, v, i, n, s, no, p, f, wk, wn, None), _lib.last_error()

    assert call(out, vals, pi, nnz, ps, n_out, point, nf, work, need)[0] == 0
    for args, msg in (
        ((None, vals, pi, nnz, ps, n_out, point, nf, work, need), "null buffer"),
        ((out, None, pi, nnz, ps, n_out, point, nf, work, need), "null buffer"),
        ((out, vals, None, nnz, ps, n_out, point, nf, work, need), "null buffer"),
        ((out, vals, pi, nnz, None, n_out, point, nf, work, need), "null buffer"),
        ((out, vals, pi, nnz, ps, n_out, None, nf, work, need), "null buffer"),
        ((out, vals, pi, nnz, ps, n_out, point, nf, None, need), "null buffer"),
        ((out, vals, pi, nnz, ps, n_out, point, nf, work, need - 1), "workspace too small"),
        ((out, vals, pi, nnz, ps, nnz + 1, point, nf, work, need), "n_out exceeds nnz"),
        ((out, vals, pi, nnz, ps, 0, point, nf, work, need), "n_out is zero"),
        ((out, vals, pi, nnz, ps, n_out, point, 64, work, need), "n_fixed must be below 64"),
        ((vals + E, vals, pi, nnz, ps, n_out, point, nf, work, need), "d_out_vals overlaps d_vals"),
        ((point + E, vals, pi, nnz, ps, n_out, point, nf, work, need), "d_out_vals overlaps d_point"),
        ((work + E, vals, pi, nnz, ps, n_out, point, nf, work, need), "d_out_vals overlaps d_work"),
    ):
        rc, err = call(*args)
        assert rc == 1 and msg in err, (args, rc, err)
    assert lib.sr_eq_table_dev(ctx, point + E, point, 3, None) == 1 and "d_out overlaps d_point" in _lib.last_error()
    assert lib.sr_eq_table_dev(ctx, out, None, 3, None) == 1 and "null buffer" in _lib.last_error()
    assert lib.sr_eq_table_dev(ctx, out, point, 48, None) == 1 and "n_vars must be below 48" in _lib.last_error()
    torch.cuda.synchronize()
    t_vals = pool[:2 * w]
    for bad, nvars, msg in (([3, 3], 4, "strictly ascending"), ([1, 16], 4, "not below"), ([0, 1], 64, "below 64")):
        with pytest.raises(RingError, match=msg):
            SparseMultilinearExtension(ring, nvars, np.array(bad, dtype=np.uint64), t_vals)
        with pytest.raises(RingError, match=msg):
            ring.smle_fix_variables(np.zeros(2 * w, dtype=np.uint64), np.array(bad, dtype=np.uint64), nvars, np.zeros(w, dtype=np.uint64))
    with pytest.raises(RingError, match="n_fixed exceeds num_vars"):
        ring.smle_fix_variables(np.zeros(2 * w, dtype=np.uint64), np.array([0, 1], dtype=np.uint64), 1, np.zeros(2 * w, dtype=np.uint64))
    with pytest.raises(RingError, match="invalid partial point"):
        SparseMultilinearExtension(ring, 1, np.array([0, 1], dtype=np.uint64), t_vals).fix_variables(pool[:2 * w])


@pytest.mark.parametrize("name,k,nv", [CASES[0], CASES[3], CASES[5], CASES[7]], ids=[IDS[0], IDS[3], IDS[5], IDS[7]])
def test_eq_table_and_fold_are_capturable(torch_cuda, name, k, nv):
    """one graph on one non-default stream: eq table, then a fold with tables, partial elements and the combine launch, on a context
    that has run nothing eagerly; replayed after the values and the point change"""
    torch = torch_cuda
    from stark_rings_amd import CyclotomicRing
    from stark_rings_amd.rings import smle_fix_pattern

    m = model_for(name, k)
    fresh = CyclotomicRing(name, k, device=0)
    w = m.w
    nvars, nf, n_eq = 20, 14, 5
    rng = random.Random(0xC00 + k)
    idx = sorted(set(rng.sample(range(1 << nvars), 900)) | {(3 << 14) + i for i in range(0, 1400, 2)})
    keys, seg = smle_fix_pattern(np.array(idx, dtype=np.uint64), nvars, nf)
    need, launches = fresh.smle_plan(len(idx), len(keys), nf)
    assert launches == 3 and need > 0
    t_vals, t_point = dev(torch, m.uniform(0xC10, len(idx))), dev(torch, m.uniform(0xC11, nf))
    d_idx, d_seg = dev(torch, np.array(idx, dtype=np.uint64)), dev(torch, seg)
    out = torch.zeros(len(keys) * w, dtype=torch.int64, device="cuda")
    eq = torch.zeros(w << n_eq, dtype=torch.int64, device="cuda")
    work = torch.full((need * w,), POISON - (1 << 64), dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        cur = torch.cuda.current_stream()
        fresh.eq_table_dev(eq, t_point[:n_eq * w], stream=cur)
        fresh.smle_fix_variables_dev(out, t_vals, d_idx, d_seg, t_point, work, stream=cur)
    torch.cuda.synchronize()
    for seed in (0xC21, 0xC22):
        vals, point = m.uniform(seed, len(idx)), m.point(seed + 16, nf)
        t_vals.copy_(dev(torch, vals))
        t_point.copy_(dev(torch, point))
        out.zero_()
        eq.zero_()
        work.fill_(POISON - (1 << 64))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want_keys, want = m.expect_fold(idx, vals, nvars, point)
        assert want_keys == keys.tolist() and np.array_equal(host(out), want), (name, seed)
        assert np.array_equal(host(eq), m.words(M.precompute_eq(m.elems(point)[:n_eq], m.sub, m.mul, m.one())))
    del g
    fresh.close()
