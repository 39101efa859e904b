"""GPU parity of the sparse-matrix calls (sr_gather_batch_dev, sr_transpose_dev, sr_spgemm_ntt[_dev], sr_sparse_transpose, sr_transpose)
for all six ring ids.  Every comparison is bit-exact.  Expected values come from tools/model_sparse_matrix.py, the line-by-line
restatement of sparse_matrix.rs:129-156, 219-275 and ops.rs:9-62 (pinned against dense products by tests/test_spgemm_host.py): on
standard-form Python integers for the power-of-two rings, on the oracle's Fq3 / Fq9 / Fq4 slot products plus integer addition for the
reference's own rings.  The independent device paths are sr_matmul_ntt_dev on the dense operands and sr_spmv_ntt_dev column by column."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import model_sparse_matrix as M  # noqa: E402

pytestmark = pytest.mark.gpu
RINGS = [("goldilocks", 6), ("goldilocks", 16), ("babybear", 5), ("stark", 4), ("goldilocks24", 0), ("babybear72", 0), ("frog16", 0)]
IDS = ["%s-%d" % r for r in RINGS]
BASE = {"goldilocks24": "goldilocks", "babybear72": "babybear", "frog16": "frog"}
SLOT_MUL = {"goldilocks24": "sro_g24_ntt_mul", "babybear72": "sro_bb72_ntt_mul", "frog16": "sro_frog16_ntt_mul"}
SLOT_W = {"goldilocks24": 3, "babybear72": 9, "frog16": 4}
POISON = 0xDEADBEEFCAFEF00D  # not canonical in any of the fields: a kernel that read it would show it
# Stark sums on lazy limbs are weakly reduced every four terms (SumOfProducts, csrc/ntt_generic.hpp): one entry of five pairs is one past it
FOLD = 4


def shapes(k):
    """(n, m, p, density of A, density of B): sizes from {1, 2, 5, 9}; density 0 gives empty results, 0.3 empty rows and one-pair
    entries; 1 x (FOLD + 1) x 1 is one past the fold interval; 1 x 300 x 1 one entry of 300 pairs.  D = 2^16: one small shape."""
    if k == 16:
        return [(2, 2, 2, 1.0, 1.0)]
    return [(1, 1, 1, 1.0, 1.0), (2, 5, 9, 0.3, 0.3), (9, 2, 5, 0.5, 0.5), (5, 9, 2, 0.3, 0.6), (5, 5, 5, 0.0, 0.5), (9, 9, 9, 0.15, 0.15),
            (1, FOLD + 1, 1, 1.0, 1.0), (1, 300, 1, 1.0, 1.0)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


_rings, _models = {}, {}


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
        self.w = self.ring.words_per_elem
        self.pow2 = name not in SLOT_MUL
        self.slot_words = self.ring.limbs if self.pow2 else SLOT_W[name]   # memory words of one slot
        p = self.p = self.ring.modulus
        if self.pow2:  # elements: numpy object arrays of D standard-form integers
            self.add = lambda a, b: (a + b) % p
            self.mul = lambda a, b: (a * b) % p
            self.zero = np.array([0] * self.ring.degree, dtype=object)
        else:          # elements: uint64 memory images; the product is the oracle's slot product
            fn = SLOT_MUL[name]
            self.add = lambda a, b: ((a.astype(object) + b.astype(object)) % p).astype(np.uint64)
            self.mul = lambda a, b: O.small(fn, a, b).reshape(-1)
            self.zero = np.zeros(self.w, dtype=np.uint64)
        self.is_zero = lambda a: not a.any()

    def elem(self, words):
        words = np.ascontiguousarray(words, dtype=np.uint64)
        return np.array(O.from_mont(self.F, words), dtype=object) if self.pow2 else words.copy()

    def words(self, e):
        return O.to_mont(self.F, [int(x) for x in e]) if self.pow2 else np.asarray(e, dtype=np.uint64)

    def uniform(self, seed, n_elems):
        return O.fill_uniform(self.F, seed, 0, n_elems * self.ring.degree).reshape(n_elems, self.w)

    def neg(self, words):
        e = self.elem(words)
        return self.words((self.p - e) % self.p) if self.pow2 else ((self.p - e.astype(object)) % self.p).astype(np.uint64)

    def halves(self, words):
        """(lo, hi): the element with the upper half of its slots zeroed, and with the lower half zeroed -- both non-zero, product zero"""
        lo, hi = words.copy(), words.copy()
        lo[self.w // 2:] = 0
        hi[:self.w // 2] = 0
        assert self.w // 2 % self.slot_words == 0 and lo.any() and hi.any()
        return lo, hi

    def model_matrix(self, rows, ncols):
        return M.SparseMatrix(len(rows), ncols, [[(self.elem(v), c) for v, c in row] for row in rows])

    def product(self, rows_a, rows_b, m, p):
        c = self.model_matrix(rows_a, m).checked_mul_mat(self.model_matrix(rows_b, p), self.add, self.mul, self.is_zero)
        return [[(self.words(v), j) for v, j in row] for row in c.coeffs]


def model_for(name, k):
    if (name, k) not in _models:
        _models[(name, k)] = Model(name, k)
    return _models[(name, k)]


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def dev32(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def poison(torch, n_words):
    return dev(torch, np.full(n_words, POISON, dtype=np.uint64))


def random_rows(m_, rng, seed, nrows, ncols, density, zeros=0.0, sort=True):
    """rows of (element words, column); a fraction `zeros` of the stored values is the zero element"""
    pool = m_.uniform(seed, nrows * ncols + 1)
    rows = []
    for i in range(nrows):
        cols = [c for c in range(ncols) if rng.random() < density]
        if not sort:
            rng.shuffle(cols)
        rows.append([(np.zeros(m_.w, dtype=np.uint64) if rng.random() < zeros else pool[i * ncols + c].copy(), c) for c in cols])
    return rows


def same_rows(got, want):
    return len(got) == len(want) and all(len(g) == len(w) and all(gc == wc and np.array_equal(gv, wv) for (gv, gc), (wv, wc) in zip(g, w))
                                         for g, w in zip(got, want))


def dense_words(m_, rows, ncols):
    out = np.zeros((len(rows), ncols, m_.w), dtype=np.uint64)
    for i, row in enumerate(rows):
        for v, c in row:
            out[i, c] = v
    return out


def numeric_dev(torch, m_, a, b):
    """sr_spgemm_ntt_dev on the structural pattern of two SparseMatrixNTT, poisoned output with a guard element and poisoned flags
    with a guard word; returns (pattern, values as rows of words, live flags)"""
    from stark_rings_amd import rings

    ring, w = m_.ring, m_.w
    pat = rings.spgemm_pattern(a.cols, a.row_ptr, a.nrows, a.ncols, b.cols, b.row_ptr, b.ncols)
    n_out = pat[1].size
    assert ring.spgemm_plan(n_out, pat[3].size) == (0, 2 if n_out else 0)
    out, live = poison(torch, (n_out + 1) * w), dev32(torch, np.full(n_out + 1, 0xDEADBEEF, dtype=np.uint32))
    ring.spgemm_ntt_dev(out[:n_out * w], live[:n_out], a.vals, b.vals, torch.from_numpy(pat[2].view(np.int64)).cuda(), dev32(torch, pat[3]),
                        dev32(torch, pat[4]))
    torch.cuda.synchronize()
    got, flags = host(out), live.cpu().numpy().view(np.uint32)
    assert (got[n_out * w:] == POISON).all() and flags[n_out] == 0xDEADBEEF, "the element or the flag behind the output was written"
    return pat, got[:n_out * w].reshape(n_out, w), flags[:n_out]


def check_product(torch, m_, rows_a, rows_b, m, p, where):
    """every path to A B against the restatement; returns the number of dead structural entries"""
    from stark_rings_amd import SparseMatrixNTT

    ring, w, n = m_.ring, m_.w, len(rows_a)
    want = m_.product(rows_a, rows_b, m, p)
    a, b = SparseMatrixNTT.from_rows(ring, rows_a, m), SparseMatrixNTT.from_rows(ring, rows_b, p)
    ring.spgemm_dead_count()
    # the numeric phase: values, flags and the counter against the restatement on the structural pattern
    pat, vals, flags = numeric_dev(torch, m_, a, b)
    lists = tuple([int(x) for x in arr] for arr in pat)
    a_elems, b_elems = [m_.elem(v) for row in rows_a for v, _ in row], [m_.elem(v) for row in rows_b for v, _ in row]
    want_vals, want_live = M.product_by_pairs(lists, a_elems, b_elems, m_.add, m_.mul, m_.is_zero, m_.zero)
    bad = sum(0 if np.array_equal(vals[e], m_.words(want_vals[e])) else 1 for e in range(len(want_vals)))
    print("%s: %d structural entries, %d pairs, %d dead, %d values differ" % (where, len(want_vals), len(lists[3]), want_live.count(0), bad))
    assert bad == 0, where
    assert [int(f) for f in flags] == want_live, where
    dead = want_live.count(0)
    assert ring.spgemm_dead_count() == dead, where
    assert ring.spgemm_dead_count() == 0, where + ": the counter is cleared by the read"
    # the compacting mirrors return the reference's matrix
    c = a.matmul(b)
    assert same_rows(c.rows(), want), where + " SparseMatrixNTT.matmul"
    assert ring.spgemm_dead_count() == dead, where + ": matmul compacts by the flags and leaves the counter to the caller"
    assert same_rows(ring.spgemm_ntt(rows_a, rows_b, m, p), want), where + " spgemm_ntt (host-pointer form)"
    assert ring.spgemm_dead_count() == 0, where + ": the host-pointer form leaves no count behind"
    # independent device paths: the dense product, and the sparse matrix-vector product column by column
    da, db = dense_words(m_, rows_a, m), dense_words(m_, rows_b, p)
    if n and p:
        y = torch.zeros(n * p * w, dtype=torch.int64, device="cuda")
        if m:
            ring.matmul_ntt_dev(y, dev(torch, da), dev(torch, db), n, m, p)
        assert np.array_equal(host(c.to_dense()), host(y)), where + " against sr_matmul_ntt_dev"
        if m:
            for j in range(p):
                col = a.mul_vec(dev(torch, db[:, j]))
                assert np.array_equal(host(col).reshape(n, w), host(y).reshape(n, p, w)[:, j]), where + " column %d against sr_spmv_ntt_dev" % j
    return dead


@pytest.mark.parametrize("name,k", RINGS, ids=IDS)
def test_product_matches_the_restatement_and_the_dense_and_spmv_paths(torch_cuda, name, k):
    m_ = model_for(name, k)
    rng = random.Random(17 * k + len(name))
    for n, m, p, da, db in shapes(k):
        rows_a = random_rows(m_, rng, 0x3000 + 7 * n + m, n, m, da, zeros=0.2 if n * m > 4 and m < 300 else 0.0)
        rows_b = random_rows(m_, rng, 0x4000 + 7 * m + p, m, p, db)
        check_product(torch_cuda, m_, rows_a, rows_b, m, p, "%s %dx%dx%d" % (name, n, m, p))


@pytest.mark.parametrize("name,k", RINGS, ids=IDS)
def test_stored_pattern_depends_on_the_values(torch_cuda, name, k):
    """stored zeros in A; non-zero elements with complementary zero slots (product zero); a b + (-a) b (live, value zero); entries all
    of whose products are zero (dead).  At D = 2^16 an entry is shared by 256 workgroups and the lower and upper halves of the slots
    fall in different ones: lo * b is live through the first 128 alone, lo * hi is dead although every workgroup sees a non-zero
    factor -- the flag is decided across all of them."""
    m_ = model_for(name, k)
    u = m_.uniform(0x5000 + k, 3)
    a, b = u[0], u[1]
    lo, hi = m_.halves(u[2])
    zero = np.zeros(m_.w, dtype=np.uint64)
    rows_a = [[(a, 0), (m_.neg(a), 1)], [(lo, 0)], [(zero, 0), (lo, 1)]]
    rows_b = [[(b, 0), (hi, 1)], [(b, 0), (hi, 1)]]
    want = m_.product(rows_a, rows_b, 2, 2)
    assert [[j for _, j in row] for row in want] == [[0, 1], [0], [0]]              # (1, 1) and (2, 1) are dead
    assert not want[0][0][0].any() and not want[0][1][0].any()                       # live with a zero value
    assert check_product(torch_cuda, m_, rows_a, rows_b, 2, 2, name + " value-dependent pattern") == 2


@pytest.mark.parametrize("name,k", RINGS, ids=IDS)
def test_gather_and_transposes(torch_cuda, name, k):
    from stark_rings_amd import SparseMatrixNTT

    torch = torch_cuda
    m_ = model_for(name, k)
    ring, w = m_.ring, m_.w
    rng = random.Random(k + 99)
    # sparse: unsorted rows too (the counting sort is stable whatever the order inside a row)
    for nrows, ncols, density, sort in ([(2, 3, 0.7, False)] if k == 16 else [(5, 9, 0.4, True), (9, 5, 0.5, False), (1, 1, 1.0, True), (3, 4, 0.0, True)]):
        rows = random_rows(m_, rng, 0x6000 + nrows, nrows, ncols, density, sort=sort)
        want = [[(m_.words(v), r) for v, r in row] for row in m_.model_matrix(rows, ncols).transpose().coeffs]
        s = SparseMatrixNTT.from_rows(ring, rows, ncols)
        st = s.transpose()
        assert (st.nrows, st.ncols) == (ncols, nrows) and same_rows(st.rows(), want)
        assert same_rows(ring.sparse_transpose(rows, ncols), want), "sr_sparse_transpose (host-pointer form)"
        # spmv(S^T, v) == matmul(dense(S)^T, v), the dense transpose made on the device
        v = m_.uniform(0x6100 + nrows, nrows)
        dt = poison(torch, (nrows * ncols + 1) * w)
        ring.transpose_dev(dt[:nrows * ncols * w], s.to_dense(), nrows, ncols)
        y = torch.zeros(ncols * w, dtype=torch.int64, device="cuda")
        ring.matmul_ntt_dev(y, dt[:nrows * ncols * w], dev(torch, v), ncols, nrows, 1)
        assert np.array_equal(host(st.mul_vec(dev(torch, v))), host(y))
        assert (host(dt)[nrows * ncols * w:] == POISON).all()
    # dense
    for nrows, ncols in ((1, 1), (3, 5), (5, 3)) if k != 16 else ((2, 3),):
        a = m_.uniform(0x6200 + nrows, nrows * ncols)
        want = np.ascontiguousarray(a.reshape(nrows, ncols, w).transpose(1, 0, 2)).reshape(-1)
        out = poison(torch, (nrows * ncols + 1) * w)
        ring.transpose_dev(out[:nrows * ncols * w], dev(torch, a), nrows, ncols)
        torch.cuda.synchronize()
        got = host(out)
        assert np.array_equal(got[:want.size], want) and (got[want.size:] == POISON).all()
        assert np.array_equal(ring.transpose(a.reshape(-1), nrows, ncols), want), "sr_transpose (host-pointer form)"
    # gather: an unaligned output takes the 8-byte path; a position outside the input is skipped and counted
    src = m_.uniform(0x6300, 4)
    perm = np.array([3, 0, 7, 2, 2, 4], dtype=np.uint32)
    ring.spmv_bad_index_count()
    for shift in (0, 1):
        buf = poison(torch, (perm.size + 1) * w + shift)
        ring.gather_dev(buf[shift:shift + perm.size * w], dev(torch, src), dev32(torch, perm))
        torch.cuda.synchronize()
        got = host(buf)[shift:].reshape(perm.size + 1, w)
        for t, q in enumerate(perm):
            assert np.array_equal(got[t], src[q]) if q < 4 else (got[t] == POISON).all(), (t, q)
        assert (got[perm.size] == POISON).all()
        assert ring.spmv_bad_index_count() == 2 and ring.spmv_bad_index_count() == 0


@pytest.mark.parametrize("name,k", [("goldilocks", 6), ("stark", 4), ("frog16", 0)])
def test_refusals(torch_cuda, name, k):
    """every SR_E_INVALID of the _dev calls; overlapping buffers are carved from one allocation"""
    torch = torch_cuda
    m_ = model_for(name, k)
    ring, w, lib = m_.ring, m_.w, m_.ring._lib
    arena = torch.zeros(16 * w, dtype=torch.int64, device="cuda")
    base, eb = arena.data_ptr(), w * 8
    idx = torch.zeros(64, dtype=torch.int64, device="cuda")      # pair_ptr = 0 .. : every list empty, every position 0
    ip = idx.data_ptr()
    st = ring._stream(None)

    def spgemm(out=base, live=ip + 256, a=base + 4 * eb, nnz_a=2, b=base + 6 * eb, nnz_b=2, pp=ip, pa=ip + 64, pb=ip + 128, n_out=2, n_pairs=2,
               work=None, work_elems=0):
        return lib.sr_spgemm_ntt_dev(ring._ctx, out, live, a, nnz_a, b, nnz_b, pp, pa, pb, n_out, n_pairs, work, work_elems, st)

    assert spgemm() == 0
    assert lib.sr_spgemm_ntt_dev(None, base, ip + 256, base + 4 * eb, 2, base + 6 * eb, 2, ip, ip + 64, ip + 128, 2, 2, None, 0, st) == 1
    for null in ("out", "live", "a", "b", "pp", "pa", "pb"):
        assert spgemm(**{null: None}) == 1, null
    assert spgemm(n_out=0, out=None, live=None) == 0                                   # n_out == 0 writes nothing, needs nothing
    assert spgemm(out=base + 3 * eb) == 1 and "overlaps d_a_vals" in ring._lib.sr_last_error_string().decode()
    assert spgemm(out=base + 5 * eb) == 1                                              # ... d_a_vals and d_b_vals
    assert spgemm(a=base + eb) == 1
    assert spgemm(live=base + 4 * eb) == 1 and "d_live overlaps" in ring._lib.sr_last_error_string().decode()
    assert spgemm(live=base + 8) == 1                                                  # the flags inside the output
    assert spgemm(out=ip) == 1                                                         # the output over the pair arrays
    assert spgemm(live=ip + 4) == 1
    assert spgemm(work=base + eb, work_elems=1) == 1 and "d_work" in ring._lib.sr_last_error_string().decode()
    assert spgemm(work=base + 10 * eb, work_elems=1) == 0                              # a workspace beyond the plan's (none) is accepted
    assert spgemm(nnz_a=1 << 32) == 1 and spgemm(nnz_b=1 << 32) == 1                   # positions are 32-bit
    assert spgemm(n_out=1 << 62) == 1 and spgemm(n_pairs=1 << 62) == 1                 # size overflow
    assert spgemm(n_out=(0xFFFFFF // max(1, ring.degree // 256 if m_.pow2 else 1)) + 1) == 1   # a grid past one launch's limit
    # gather and transpose
    g = lambda out=base, src=base + 4 * eb, perm=ip, n=2, n_in=2: lib.sr_gather_batch_dev(ring._ctx, out, src, perm, n, n_in, st)  # noqa: E731
    t = lambda out=base, src=base + 6 * eb, r=2, c=3: lib.sr_transpose_dev(ring._ctx, out, src, r, c, st)                          # noqa: E731
    assert g() == 0 and t() == 0
    assert g(out=None) == 1 and g(src=None) == 1 and g(perm=None) == 1 and g(n=0, out=None, perm=None) == 0
    assert g(out=base + 3 * eb) == 1 and g(out=ip) == 1 and g(n=1 << 62) == 1 and g(n_in=1 << 62) == 1
    assert t(out=None) == 1 and t(src=None) == 1 and t(r=0, out=None, src=None) == 0
    assert t(out=base + eb) == 1 and t(r=1 << 40, c=1 << 40) == 1
    assert lib.sr_gather_batch_dev(None, base, base, ip, 1, 1, st) == 1 and lib.sr_transpose_dev(None, base, base, 1, 1, st) == 1
    n = ctypes.c_ulonglong()
    assert lib.sr_spgemm_dead_count(ring._ctx, None, st) == 1 and lib.sr_spgemm_dead_count(None, ctypes.byref(n), st) == 1
    torch.cuda.synchronize()
    ring.spgemm_dead_count()
    with pytest.raises(Exception):
        ring.spgemm_ntt([[(np.zeros(w, dtype=np.uint64), 0)]], [], 1, 1)              # the reference returns None: ncols != m.nrows


@pytest.mark.parametrize("name,k", [("goldilocks", 6), ("stark", 4), ("babybear72", 0)])
def test_graph_capture_of_a_fixed_pattern(torch_cuda, name, k):
    """sr_spgemm_ntt_dev captured once on a single non-default stream, on a context that has never run anything eagerly (no warm-up);
    replayed twice on changed values in the same buffers.  One stream, a linear chain."""
    torch = torch_cuda
    from stark_rings_amd import CyclotomicRing, SparseMatrixNTT, rings

    m_ = model_for(name, k)
    w = m_.w
    fresh = CyclotomicRing(name, k, device=0)
    rng = random.Random(5)
    rows_a, rows_b = random_rows(m_, rng, 0x7000, 5, 9, 0.4), random_rows(m_, rng, 0x7001, 9, 5, 0.4)
    a, b = SparseMatrixNTT.from_rows(fresh, rows_a, 9), SparseMatrixNTT.from_rows(fresh, rows_b, 5)
    pat = rings.spgemm_pattern(a.cols, a.row_ptr, 5, 9, b.cols, b.row_ptr, 5)
    n_out = pat[1].size
    assert n_out
    out, live = poison(torch, n_out * w), dev32(torch, np.full(n_out, 7, dtype=np.uint32))
    d_pat = (torch.from_numpy(pat[2].view(np.int64)).cuda(), dev32(torch, pat[3]), dev32(torch, pat[4]))
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=s):
        fresh.spgemm_ntt_dev(out, live, a.vals, b.vals, *d_pat, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    lists = tuple([int(x) for x in arr] for arr in pat)
    for seed in (0x7100, 0x7200):
        va, vb = m_.uniform(seed, a.nnz()), m_.uniform(seed + 1, b.nnz())
        va[0] = 0                                                 # a stored zero: flags and counter follow the values of the replay
        a.vals.copy_(dev(torch, va.reshape(-1)))
        b.vals.copy_(dev(torch, vb.reshape(-1)))
        graph.replay()
        torch.cuda.synchronize()
        want_vals, want_live = M.product_by_pairs(lists, [m_.elem(v) for v in va], [m_.elem(v) for v in vb], m_.add, m_.mul, m_.is_zero, m_.zero)
        assert np.array_equal(host(out).reshape(n_out, w), np.stack([m_.words(v) for v in want_vals])), (name, seed)
        assert [int(f) for f in live.cpu().numpy()] == want_live, (name, seed)
        assert fresh.spgemm_dead_count() == want_live.count(0)
    del graph
    fresh.close()
