"""Runs the operands of tests/crafted_poly_operands.py, and the family tests' edge tables, through the device calls of the dense, round
and sparse multilinear-extension families (`poly`) and of the symmetric and sparse matrices (`linalg`), and compares every output bit
for bit with the integer models.  tests/test_crafted_poly_gpu.py drives it on the product library; tests/rep_invariants_worker.py on
the invariant-checking build, where `check(group)` reads the counters after every group of calls."""
import numpy as np

import crafted_poly_operands as C
from test_mle_gpu import dev, fold_dev, host, ring_for  # noqa: F401
from test_smle_gpu import fold_dev as smle_fold_dev
from test_spgemm_gpu import dev32, numeric_dev
from test_sumcheck_fold_gpu import fold_round_dev
from test_sumcheck_gpu import round_dev
from test_symm_gpu import gram_dev, packed, recompose_dev
from test_vpoly_gpu import vp_dev

LEADING, TRAILING, ROUND_SUM = C.LEADING, C.TRAILING, C.ROUND_SUM
ORDERS = (LEADING, TRAILING)
FAMILY = {"goldilocks": "one-limb", "babybear": "one-limb"}  # every other ring is a family of its own
SMALL_NV = 4       # the short table of every ring: a single launch in every family


def shifted(torch, words):
    """the words at a pointer with data_ptr() % 16 == 8: the one-coefficient lane path"""
    buf = torch.empty(words.size + 1, dtype=torch.int64, device="cuda")
    buf[1:] = dev(torch, words)
    assert buf[1:].data_ptr() % 16 == 8
    return buf[1:]


class Run:
    def __init__(self, torch, name, k, check=None):
        self.torch, self.name, self.k = torch, name, k
        self.o = C.Ops(name, k)
        self.ring = ring_for(name, k)
        assert self.ring.words_per_elem == self.o.w and self.ring.modulus == self.o.p
        self.cols = C.columns(self.o)
        self.check = check or (lambda group: None)
        self.paths = {}           # call family -> set of "launches == 1" seen
        self.tag = "%s D=2^%d" % (name, k) if self.o.pow2 else name

    def same(self, got_t, want, what, cols="default"):
        got = host(got_t) if not isinstance(got_t, np.ndarray) else got_t
        assert C.agree(self.o, got, want, self.cols if cols == "default" else cols), "%s: %s differs from the model" % (self.tag, what)
        if got.size:
            assert self.ring.count_noncanonical_dev(dev(self.torch, got)) == 0, "%s: %s holds a word >= p" % (self.tag, what)

    def saw(self, family, launches):
        self.paths.setdefault(family, set()).add(launches == 1)

    # ---- dense fold -----------------------------------------------------------------------------------------------------------------
    def fold(self, table, nv, point, order, what, put=dev):
        o, torch = self.o, self.torch
        t = put(torch, o.words(table))
        got, _ = fold_dev(torch, self.ring, t, nv, dev(torch, o.words(point)), order)
        torch.cuda.synchronize()
        self.saw("fold", self.ring.mle_plan(nv, len(point), order)[1])
        self.same(got, C.model_fold(o, table, nv, point, order, self.cols), what)

    def dense(self, nv):
        o, torch = self.o, self.torch
        for order in ORDERS:
            for nf in (1, 2, 3, nv):
                table, point = C.craft_fold(o, nv, nf, order)
                self.fold(table, nv, point, order, "crafted fold n_fixed %d order %d" % (nf, order))
            table, point = C.craft_fold(o, nv, 3, order, seed=1)
            self.fold(table[:(1 << nv) - 3], nv, point, order, "truncated crafted fold order %d" % order)
            table, point = C.craft_fold(o, SMALL_NV, 2, order, seed=2)
            self.fold(table, SMALL_NV, point, order, "short crafted fold order %d" % order)
        table, point = C.craft_fold(o, nv, 2, LEADING, seed=3)
        self.fold(table, nv, point, LEADING, "crafted fold at an odd 8-byte pointer", put=shifted)
        pt = C.edge_point(o, nv)
        for tn, table in C.edge_tables(o, 1 << nv).items():
            for order in ORDERS:
                self.fold(table, nv, pt[:2] if order == LEADING else pt[nv - 2:], order, "edge table %s order %d" % (tn, order))
        acc, xs, r = C.craft_mul_elem_add(o, 5)
        t_acc = dev(torch, o.words(acc))
        self.ring.mul_elem_add_dev(t_acc, dev(torch, o.words(xs)), dev(torch, o.words([r])))
        torch.cuda.synchronize()
        self.same(t_acc, [o.add(o.elem(a), o.mul(o.elem(r), o.elem(x))) for a, x in zip(acc, xs)], "crafted mul_elem_add", cols=None)
        self.check("dense fold")

    # ---- round messages ---------------------------------------------------------------------------------------------------------------
    def message(self, tables, nv, mode, what, put=dev):
        o, torch = self.o, self.torch
        got = round_dev(torch, self.ring, [put(torch, o.words(t)) for t in tables], nv, mode)
        if mode != ROUND_SUM:
            self.saw("round", self.ring.mle_round_plan(nv, len(tables), mode)[1])
        self.same(got, C.model_round(o, tables, nv, mode, self.cols), what)

    def rounds(self, nv):
        o = self.o
        for d in (2, 3, 4):
            for order in ORDERS:
                tables, _ = C.craft_round(o, nv, d, order)
                self.message(tables, nv, order, "crafted round d %d order %d" % (d, order))
                if order == LEADING:
                    self.message(tables, nv, ROUND_SUM, "crafted plain sum d %d" % d)
        for order in ORDERS:
            tables, _ = C.craft_round(o, nv, 3, order, seed=1)
            cutt = [t[:(1 << nv) - 3] for t in tables]
            for mode in (order, ROUND_SUM):
                self.message(cutt, nv, mode, "truncated crafted round mode %d" % mode)
            tables, _ = C.craft_round(o, SMALL_NV, 2, order, seed=2)
            self.message(tables, SMALL_NV, order, "short crafted round order %d" % order)
        tables, _ = C.craft_round(o, nv, 2, LEADING, seed=3)
        self.message(tables, nv, LEADING, "crafted round at odd 8-byte pointers", put=shifted)
        edge = C.edge_tables(o, 1 << nv)
        for trio in (("zero", "uniform", "1"), ("p-1", "p-1", "p-1"), ("1", "uniform", "p-1")):
            for mode in (LEADING, TRAILING, ROUND_SUM):
                self.message([edge[n] for n in trio], nv, mode, "edge tables %r mode %d" % (trio, mode))
        self.message([edge["uniform"][:8]], 3, LEADING, "one short uniform table")   # d = 1, eight entries: a single launch in every ring
        self.check("round messages")

    # ---- the fused fold and round -----------------------------------------------------------------------------------------------------
    def fused_call(self, tables, nv, r, order, what, put=dev):
        o, torch = self.o, self.torch
        msg, got, _ = fold_round_dev(torch, self.ring, [put(torch, o.words(t)) for t in tables], nv, dev(torch, o.words([r])), order)
        torch.cuda.synchronize()
        self.saw("fused", self.ring.mle_round_fold_plan(nv, len(tables), order)[1])
        folded, message = C.model_fold_round(o, tables, nv, r, order, self.cols)
        self.same(msg, message, what + " (message)")
        for g, f in zip(got, folded):
            self.same(g, f, what + " (folded table)")

    def fused(self, nv):
        o = self.o
        for d in (2, 3):
            for order in ORDERS:
                tables, r, _ = C.craft_fold_round(o, nv, d, order)
                self.fused_call(tables, nv, r, order, "crafted fused round d %d order %d" % (d, order))
        for order in ORDERS:
            tables, r, _ = C.craft_fold_round(o, nv, 2, order, seed=1)
            self.fused_call([t[:(1 << nv) - 3] for t in tables], nv, r, order, "truncated crafted fused round order %d" % order)
            tables, r, _ = C.craft_fold_round(o, SMALL_NV + 1, 2, order, seed=2)
            self.fused_call(tables, SMALL_NV + 1, r, order, "short crafted fused round order %d" % order)
        tables, r, _ = C.craft_fold_round(o, nv, 2, LEADING, seed=3)
        self.fused_call(tables, nv, r, LEADING, "crafted fused round at odd 8-byte pointers", put=shifted)
        edge = C.edge_tables(o, 1 << nv)
        for order in ORDERS:
            self.fused_call([edge["p-1"], edge["uniform"]], nv, o.lanes_of(o.p - 1), order, "edge tables, challenge p - 1, order %d" % order)
            self.fused_call([edge["1"], edge["zero"]], nv, o.lanes_of(1), order, "edge tables, challenge 1, order %d" % order)
        self.fused_call([edge["uniform"][:8]], 3, o.lanes_of(o.p - 1), LEADING, "one short uniform table")   # a single launch in every ring
        self.check("fused fold and round")

    # ---- sums of products ---------------------------------------------------------------------------------------------------------------
    def vpoly_call(self, tables, terms, coeffs, nv, mode, what, put=dev):
        o, torch = self.o, self.torch
        got = vp_dev(torch, self.ring, [put(torch, o.words(t)) for t in tables], terms, put(torch, o.words(coeffs)), nv, mode)
        self.saw("vpoly", self.ring.vpoly_round_plan(nv, len(tables), len(terms), max(len(t) for t in terms), mode)[1])
        self.same(got, C.model_vpoly(o, tables, terms, coeffs, nv, mode, self.cols), what)

    def vpoly(self, nv):
        o = self.o
        for structure in ("R1CS", "THREE"):
            for order in ORDERS:
                tables, terms, coeffs, _ = C.craft_vpoly(o, nv, structure, order)
                self.vpoly_call(tables, terms, coeffs, nv, order, "crafted %s order %d" % (structure, order))
                if order == LEADING:
                    self.vpoly_call(tables, terms, coeffs, nv, ROUND_SUM, "crafted %s plain sum" % structure)
        tables, terms, coeffs, _ = C.craft_vpoly(o, nv, "R1CS", TRAILING, seed=1)
        self.vpoly_call([t[:(1 << nv) - 3] for t in tables], terms, coeffs, nv, TRAILING, "truncated crafted R1CS")
        tables, terms, coeffs, _ = C.craft_vpoly(o, SMALL_NV, "R1CS", LEADING, seed=2)
        for mode in (LEADING, ROUND_SUM):
            self.vpoly_call(tables, terms, coeffs, SMALL_NV, mode, "short crafted R1CS mode %d" % mode)
        tables, terms, coeffs, _ = C.craft_vpoly(o, nv, "R1CS", LEADING, seed=3)
        self.vpoly_call(tables, terms, coeffs, nv, LEADING, "crafted R1CS at odd 8-byte pointers", put=shifted)
        edge = C.edge_tables(o, 1 << nv)
        minus_one = o.scalar(o.lanes_of(o.p - o.ONE))
        for names, c0 in ((("p-1", "uniform", "1", "p-1"), o.lanes_of(o.p - 1)), (("uniform", "p-1", "p-1", "zero"), o.lanes_of(1))):
            for mode in (LEADING, TRAILING, ROUND_SUM):
                self.vpoly_call([edge[n] for n in names], C.VP.R1CS, [c0, minus_one], nv, mode, "R1CS on edge tables %r mode %d" % (names, mode))
        self.check("sums of products")

    # ---- sparse MLE ---------------------------------------------------------------------------------------------------------------------
    def sparse_call(self, idx, vals, nv, point, what):
        o, torch = self.o, self.torch
        keys, got = smle_fold_dev(torch, self.ring, dev(torch, o.words(vals)), idx, nv, dev(torch, o.words(point)))
        want_keys, want = C.model_smle(o, idx, vals, nv, point)
        assert keys == want_keys, what
        self.same(got, want, what, cols=None)
        n_out = len(keys)
        self.saw("sparse", self.ring.smle_plan(len(idx), n_out, len(point))[1])

    def sparse(self, nv):
        o, torch = self.o, self.torch
        w = o.w
        for n, seed in ((min(nv, 12), 0), (3, 1)):
            point = C.craft_eq_point(o, n, seed)
            out = torch.empty(w << n, dtype=torch.int64, device="cuda")
            self.ring.eq_table_dev(out, dev(torch, o.words(point)))
            torch.cuda.synchronize()
            self.same(out, C.model_eq(o, point), "eq table of %d crafted point elements" % n, cols=None)
        nf, nnz = C.SMLE_SHAPE(o)
        idx, vals, point = C.craft_smle(o, C.SMLE_NV, nf, nnz)
        self.sparse_call(idx, vals, C.SMLE_NV, point, "crafted sparse fold")
        pt = C.craft_eq_point(o, nf, 2)                       # words of S and one - s; the eq table is zero in many places
        for tn in ("p-1", "1", "uniform"):
            self.sparse_call(idx, C.edge_tables(o, len(idx), 5)[tn], C.SMLE_NV, pt, "sparse fold of edge values %s at a point of S" % tn)
        few = [3, 9, 1 << 12, (1 << 19) + 5, (1 << 20) - 1]      # five runs of one entry: a single launch
        self.sparse_call(few, C.edge_tables(o, 5, 6)["uniform"], C.SMLE_NV, pt[:2], "sparse fold of five single entries")
        self.check("sparse MLE")

    def poly(self, nv):
        self.dense(nv)
        self.rounds(nv)
        self.fused(nv)
        self.vpoly(nv)
        self.sparse(nv)

    # ---- symmetric and sparse matrices ---------------------------------------------------------------------------------------------------
    def gram(self, a, n, m, what):
        o, torch = self.o, self.torch
        got, launches = gram_dev(torch, self.ring, dev(torch, o.words(a)), n, m)
        self.saw("gram", launches)
        self.same(got, C.model_gram(o, a, n, m), what, cols=None)
        return got

    def recompose(self, mat, n, d, powers, what):
        o, torch = self.o, self.torch
        got = recompose_dev(torch, self.ring, dev(torch, o.words(mat)), n, d, dev(torch, o.words(powers)))
        self.same(got, C.model_recompose(o, mat, n, d, powers), what, cols=None)

    def spgemm(self, rows_a, rows_b, m, p_cols, what):
        from stark_rings_amd import SparseMatrixNTT

        o, torch, ring = self.o, self.torch, self.ring
        wa = [[(o.words([v]), c) for v, c in row] for row in rows_a]
        wb = [[(o.words([v]), c) for v, c in row] for row in rows_b]
        a, b = SparseMatrixNTT.from_rows(ring, wa, m), SparseMatrixNTT.from_rows(ring, wb, p_cols)
        ring.spgemm_dead_count()

        class Words:          # what numeric_dev reads of the family's Model
            pass

        mm = Words()
        mm.ring, mm.w = ring, o.w
        pat, vals, flags = numeric_dev(torch, mm, a, b)
        lists = tuple([int(x) for x in arr] for arr in pat)
        want, live = C.model_spgemm_pairs(o, lists, [v for row in rows_a for v, _ in row], [v for row in rows_b for v, _ in row])
        self.same(vals.reshape(-1), want, what, cols=None)
        assert [int(f) for f in flags] == live, what
        assert ring.spgemm_dead_count() == live.count(0), what
        return max((lists[2][e + 1] - lists[2][e] for e in range(len(lists[2]) - 1)), default=0)

    def movers(self, src_rows, ncols):
        """gather_dev and transpose_dev move words and compute nothing: crafted words come out as they went in"""
        o, torch, ring, w = self.o, self.torch, self.ring, self.o.w
        words = o.words(src_rows)
        nrows = len(src_rows) // ncols
        out = torch.empty(words.size, dtype=torch.int64, device="cuda")
        ring.transpose_dev(out, dev(torch, words), nrows, ncols)
        torch.cuda.synchronize()
        assert np.array_equal(host(out), np.ascontiguousarray(words.reshape(nrows, ncols, w).transpose(1, 0, 2)).reshape(-1)), "transpose_dev"
        perm = np.array([(7 * i + 3) % len(src_rows) for i in range(len(src_rows))], dtype=np.uint32)
        ring.gather_dev(out, dev(torch, words), dev32(torch, perm))
        torch.cuda.synchronize()
        assert np.array_equal(host(out), words.reshape(-1, w)[perm].reshape(-1)), "gather_dev"
        assert ring.count_noncanonical_dev(out) == 0

    def linalg(self):
        o = self.o
        for n, m in ((9, 41), (5, 41)) + (((5, 4096),) if (self.name, self.k) == ("goldilocks", 6) else ()):
            a = C.craft_gram(o, n, m)
            self.gram(a, n, m, "crafted Gram matrix %d x %d" % (n, m))
        edge = C.edge_tables(o, 5 * 41)
        self.gram(edge["p-1"], 5, 41, "Gram matrix of p - 1 words")
        self.gram(edge["uniform"], 5, 41, "Gram matrix of uniform words")
        self.check("Gram")
        mat, powers = C.craft_recompose(o, 5, 3)
        self.recompose(mat, 5, 3, powers, "crafted recompose")
        self.recompose(C.edge_tables(o, 120)["p-1"], 5, 3, [o.lanes_of(o.p - 1)] * 3, "recompose of p - 1 words")
        self.recompose(C.edge_tables(o, 120)["uniform"], 5, 3, C.edge_point(o, 3), "recompose of uniform words, edge weights")
        self.check("recompose")
        longest = 0
        for n, m, p_cols in ((5, 41, 2), (1, 9, 5), (9, 2, 1), (2, 5, 9)):
            rows_a, rows_b = C.craft_spgemm(o, n, m, p_cols)
            longest = max(longest, self.spgemm(rows_a, rows_b, m, p_cols, "crafted sparse product %d x %d x %d" % (n, m, p_cols)))
        assert longest >= 41
        rows_a, rows_b = C.craft_spgemm(o, 5, 41, 2)
        self.movers([v for row in rows_a for v, _ in row], 41)
        self.check("sparse x sparse, gather, transpose")

    # ---- Stark: every operand a max-limb image ------------------------------------------------------------------------------------------
    def stark_max(self, nv, n, m):
        """every table, point, challenge, weight, coefficient and matrix entry is a max_limb_images flavour, different flavours meeting
        each other; returns {family: the largest |limb| any add / sub produced} as check() reports it"""
        o, torch = self.o, self.torch
        T = lambda count, shift: C.stark_flavour_table(o, count, shift)  # noqa: E731
        high = {}
        for order in ORDERS:
            for nf in (1, 2, 3):
                self.fold(T(1 << nv, nf), nv, T(nf, order + 1), order, "max-limb fold n_fixed %d order %d" % (nf, order))
        acc, xs, r = T(5, 0), T(5, 1), T(1, 2)[0]
        t_acc = dev(torch, o.words(acc))
        self.ring.mul_elem_add_dev(t_acc, dev(torch, o.words(xs)), dev(torch, o.words([r])))
        torch.cuda.synchronize()
        self.same(t_acc, [o.add(a, o.mul(r, x)) for a, x in zip(acc, xs)], "max-limb mul_elem_add", cols=None)
        high["dense fold"] = self.check("max-limb dense fold")
        for d in (2, 3, 4):
            for mode in (LEADING, TRAILING, ROUND_SUM):
                self.message([T(1 << nv, j) for j in range(d)], nv, mode, "max-limb round d %d mode %d" % (d, mode))
        high["round messages"] = self.check("max-limb round messages")
        for order in ORDERS:
            self.fused_call([T(1 << nv, j) for j in range(3)], nv, T(1, order)[0], order, "max-limb fused round order %d" % order)
        high["fused fold and round"] = self.check("max-limb fused fold and round")
        for mode in (LEADING, TRAILING, ROUND_SUM):
            self.vpoly_call([T(1 << nv, j) for j in range(4)], C.VP.R1CS, T(2, mode), nv, mode, "max-limb R1CS mode %d" % mode)
            self.vpoly_call([T(1 << nv, j + 1) for j in range(5)], C.THREE, T(3, mode + 1), nv, mode, "max-limb three terms mode %d" % mode)
        high["sums of products"] = self.check("max-limb sums of products")
        point = T(nv, 1)
        out = torch.empty(o.w << nv, dtype=torch.int64, device="cuda")
        self.ring.eq_table_dev(out, dev(torch, o.words(point)))
        torch.cuda.synchronize()
        self.same(out, C.model_eq(o, point), "max-limb eq table", cols=None)
        idx = sorted(set(range(40, 40 + 45)) | {3, 9, 200, 201, 1000, (1 << 20) - 1})
        self.sparse_call(idx, T(len(idx), 2), 20, T(3, 0), "max-limb sparse fold")
        high["sparse MLE"] = self.check("max-limb sparse MLE")
        g = self.gram(T(n * m, 0), n, m, "max-limb Gram matrix")
        high["Gram"] = self.check("max-limb Gram")
        self.recompose(T(packed(6), 1), 2, 3, T(3, 2), "max-limb recompose")
        del g
        high["recompose"] = self.check("max-limb recompose")
        rows_a = [[(v, c) for c, v in enumerate(T(m, i))] for i in range(n)]
        rows_b = [[(v, c) for c, v in enumerate(T(2, i + 1))] for i in range(m)]
        assert self.spgemm(rows_a, rows_b, m, 2, "max-limb sparse product") >= 41
        self.movers(T(n * m, 2), m)
        high["sparse x sparse, gather, transpose"] = self.check("max-limb sparse x sparse")
        return high
