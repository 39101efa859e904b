"""The test of the test: tests/crafted_poly_operands.py promises operands whose INTERMEDIATE memory words (differences, running points,
products, partial sums, stored results) sit on the borders of the number formats.  Here the integer models of tools/ alone -- no GPU,
no library of the product -- recompute every stage and count: each class occurs at each stage at least 8 times per ring and shape of
the invariant-checking runs, the summands of the sums are the words 0, 1 and p - 1 only, and 64 seeded random subsets of the pairs sum
to within +- (their size) of 0 mod p."""
import os
import sys

import numpy as np
import pytest

import oracle_lib as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crafted_poly_operands as C  # noqa: E402

CASES = C.POLY_CASES
IDS = ["%s-%d-nv%d" % c for c in CASES]
ORDERS = (C.LEADING, C.TRAILING)
AT_LEAST = 8

_ops = {}


def ops(name, k):
    if (name, k) not in _ops:
        _ops[(name, k)] = C.Ops(name, k)
    return _ops[(name, k)]


def count_in(o, elems, values=None):
    """how often each value occurs among the lane words of the model elements"""
    flat = np.concatenate([o.lanes(e) for e in elems])
    return {v: int((flat == v).sum()) for v in (o.S if values is None else values)}


def every_class(o, elems, what, values=None):
    c = count_in(o, elems, values)
    assert min(c.values()) >= AT_LEAST, "%s %s: %r" % (o.name, what, c)


@pytest.mark.parametrize("name", sorted(C.RINGS))
def test_the_word_domain_product_is_the_oracles(name):
    """a b / R on memory words is to_mont(from_mont(a) from_mont(b)), the image of 1 is R mod p, and in the rings of slots a per-slot
    scalar multiplies every word of its slot by that rule"""
    o = ops(name, 3)
    F = O.FIELD_ID[o.base]
    rng = C.rng_for("pin", name)
    a, b = o.rnd(rng), o.rnd(rng)
    assert O.limbs_to_ints(O.to_mont(F, [1]), o.limbs) == [o.ONE]
    if o.pow2:
        sa, sb = O.from_mont(F, o.words([a])), O.from_mont(F, o.words([b]))
        want = O.limbs_to_ints(O.to_mont(F, [x * y % o.p for x, y in zip(sa, sb)]), o.limbs)
        assert [int(v) for v in o.mul(a, b)] == want
        assert o.from_words(o.words([a, b]))[1].tolist() == b.tolist()
        big = ops(name, 12)
        if big.tile > 1:      # repeated lanes: every repetition is written, and one that differs is seen
            x = big.rnd(rng)
            words = big.words([x])
            assert words.size == 1 << 12 and big.from_words(words)[0].tolist() == x.tolist()
            words[3 * 1024 + 5] ^= np.uint64(1)
            assert big.from_words(words)[0][5] == -1
    else:
        r = o.scalar(b)
        assert o.mul(o.elem(r), o.elem(a)).astype(object).tolist() == o.lmul(o.eff(r), a).tolist()
        assert np.array_equal(o.mul(o.one, o.elem(a)), o.elem(a))
    assert o.sqrtR * o.sqrtR * o.Rinv % o.p == 1
    if name == "stark":
        assert np.array_equal(o.words(o.from_words(C.max_limb_images(8, "topbits"))), C.max_limb_images(8, "topbits"))


def first_stage(o, table, r, nv, order):
    T, re = o.elems(table), o.elem(r)
    diffs, prods, outs = [], [], []
    for lo_i, hi_i in C.first_pairs(nv, order):
        diffs.append(o.sub(T[hi_i], T[lo_i]))
        prods.append(o.mul(re, diffs[-1]))
        outs.append(o.add(T[lo_i], prods[-1]))
    return diffs, prods, outs


@pytest.mark.parametrize("name,k,nv", CASES, ids=IDS)
def test_dense_fold_operands_reach_every_class_at_every_stage(name, k, nv):
    o = ops(name, k)
    for order in ORDERS:
        for nf in (1, 2, 3):
            table, point = C.craft_fold(o, nv, nf, order)
            r = point[0] if order == C.LEADING else point[-1]
            diffs, prods, outs = first_stage(o, table, r, nv, order)
            where = "fold nv %d n_fixed %d order %d" % (nv, nf, order)
            every_class(o, diffs, where + " hi - lo")
            every_class(o, prods, where + " r (hi - lo)")
            every_class(o, outs, where + " first-stage result")
            if nf >= 2:
                every_class(o, C.model_fold(o, table, nv, point, order), where + " stored word")
            if o.L >= 4 * len(o.S) * o.slotw:
                assert set(o.S) <= set(int(v) for v in o.eff(r)), "the challenge carries S"
    acc, xs, r = C.craft_mul_elem_add(o, 5)
    every_class(o, [o.add(o.elem(a), o.mul(o.elem(r), o.elem(x))) for a, x in zip(acc, xs)], "mul_elem_add")


def signed(o, elems):
    """(len, L) array of the summands as -1, 0, +1; asserts that they are the words p - 1, 0, 1"""
    rows = np.stack([o.lanes(e) for e in elems])
    ok = (rows == 0) | (rows == 1) | (rows == o.p - 1)
    assert ok.all(), "%s: a summand is not one of the words 0, 1, p - 1" % o.name
    return np.where(rows == 1, 1, np.where(rows == 0, 0, -1)).astype(np.int64), rows


def subsets_stay_near_zero(o, elems, what, seed):
    """64 seeded random subsets: the sum mod p, by the model's add, is within +- (size) of 0"""
    sg, rows = signed(o, elems)
    rng = np.random.default_rng(seed)
    for _ in range(64):
        pick = rng.integers(0, 2, size=len(elems)) == 1
        n = int(pick.sum())
        total = rows[pick].sum(axis=0) % o.p if n else o.lanes_of(0)
        dist = np.minimum(total, (o.p - total) % o.p)
        assert (dist <= n).all() and (np.abs(sg[pick].sum(axis=0)) == dist).all(), what
    return sg


def round_stages(o, tables, nv, d, order, kinds):
    """per table the differences and the running points t = 2 .. d; per t the summand of every unsolved pair"""
    T = [o.elems(t) for t in tables]
    diffs, running, summands = [], [], [[] for _ in range(d + 1)]
    for q, (lo_i, hi_i) in enumerate(C.first_pairs(nv, order)):
        pts = []
        for f in T:
            dl = o.sub(f[hi_i], f[lo_i])
            v = [f[lo_i], o.add(f[lo_i], dl)]
            for _ in range(2, d + 1):
                v.append(o.add(v[-1], dl))
            assert np.array_equal(o.lanes(v[1]), o.lanes(f[hi_i]))
            diffs.append(dl)
            running.extend(v[2:])
            pts.append(v)
        if kinds[q] in ("a", "b"):
            for t in range(d + 1):
                term = pts[0][t]
                for v in pts[1:]:
                    term = o.mul(v[t], term)
                summands[t].append(term)
    return diffs, running, summands


@pytest.mark.parametrize("d", [2, 3, 4])
@pytest.mark.parametrize("name,k,nv", CASES, ids=IDS)
def test_round_operands_reach_every_class_and_their_partial_sums_stay_near_zero(name, k, nv, d):
    o = ops(name, k)
    cols = C.columns(o)
    for order in ORDERS:
        tables, info = C.craft_round(o, nv, d, order)
        where = "round nv %d d %d order %d" % (nv, d, order)
        diffs, running, summands = round_stages(o, tables, nv, d, order, info["kinds"])
        every_class(o, diffs, where + " (a) hi - lo")
        every_class(o, running, where + " (a) running points")
        for t in range(d + 1):
            sg = subsets_stay_near_zero(o, summands[t], where + " (b) t = %d" % t, 1000 * d + t)
            if info["kinds"].count("b") >= 2 * AT_LEAST:
                assert (sg == 1).sum() >= AT_LEAST and (sg == -1).sum() >= AT_LEAST, where
        msg = C.model_round(o, tables, nv, order, cols)
        want = [x if cols is None else x[cols] for x in info["targets"]]
        assert all(np.array_equal(o.lanes(m), x) for m, x in zip(msg, want)), where + " (c): the message is not the target"
        every_class(o, info["targets"], where + " (c) message words")
        # the plain sum runs over the same entries: its summands are those of t = 0 and t = 1
        # (d) the fused call: the tables fold, at the challenge, onto crafted round tables of one variable less
        if nv - 1 >= d + 2:
            big, r, inner = C.craft_fold_round(o, nv, d, order)
            folded, msg = C.model_fold_round(o, big, nv, r, order, cols)
            again, _ = C.craft_round(o, nv - 1, d, order)
            for f, g in zip(folded, again):
                assert all(np.array_equal(o.lanes(a), b if cols is None else b[cols]) for a, b in zip(f, g)), where + " (d)"
            assert all(np.array_equal(o.lanes(m), x if cols is None else x[cols]) for m, x in zip(msg, inner["targets"])), where + " (d) message"


@pytest.mark.parametrize("structure", ["R1CS", "THREE"])
@pytest.mark.parametrize("name,k,nv", CASES, ids=IDS)
def test_vpoly_operands(name, k, nv, structure):
    o = ops(name, k)
    cols = C.columns(o)
    order = C.LEADING if structure == "R1CS" else C.TRAILING
    tables, terms, coeffs, info = C.craft_vpoly(o, nv, structure, order)
    where = "vpoly %s nv %d" % (structure, nv)
    # (e) the coefficient words: values of S and the image of -1
    lanes0 = np.arange(o.L) % o.slotw == 0
    assert set(o.S) <= set(int(v) for v in coeffs[0][lanes0]), where
    assert (coeffs[1][lanes0] == o.p - o.ONE).all()
    # every term's summands at the unsolved pairs are the words 0, 1, p - 1
    for term in terms:
        _, _, summands = round_stages(o, [tables[j] for j in term], nv, 3, order, info["kinds"])
        for t in range(4):
            subsets_stay_near_zero(o, summands[t], where + " term %r t = %d" % (term, t), 77 + t)
    diffs, running, _ = round_stages(o, [tables[3]], nv, 3, order, info["kinds"])
    every_class(o, diffs, where + " c: hi - lo")
    every_class(o, running, where + " c: running points")
    msg = C.model_vpoly(o, tables, terms, coeffs, nv, order, cols)
    solved = o.eff(coeffs[0]) != 0
    solved = solved if cols is None else solved[cols]
    for m, x in zip(msg, info["targets"]):
        x = x if cols is None else x[cols]
        assert np.array_equal(o.lanes(m)[solved], x[solved]), where + ": the message is not the target"
    every_class(o, [np.where(o.eff(coeffs[0]) != 0, x, -1) for x in info["targets"]], where + " message words")


@pytest.mark.parametrize("name,k,nv", CASES, ids=IDS)
def test_sparse_mle_operands(name, k, nv):
    o = ops(name, k)
    n = min(nv, 12)
    point = C.craft_eq_point(o, n)
    every_class(o, point, "eq point", list(o.S) + [(o.ONE - s) % o.p for s in o.S if (o.ONE - s) % o.p not in o.S])
    nf, nnz = C.SMLE_SHAPE(o)
    idx, vals, pt = C.craft_smle(o, C.SMLE_NV, nf, nnz)
    pre = C.model_eq(o, pt)
    prods = [o.mul(pre[i & ((1 << nf) - 1)], o.elem(v)) for i, v in zip(idx, vals)]
    sg = subsets_stay_near_zero(o, prods, "sparse fold products", 5)
    assert (sg != 0).all()
    runs = {}
    for i in idx:
        runs[i >> nf] = runs.get(i >> nf, 0) + 1
    assert max(runs.values()) == 1 << nf and min(runs.values()) == 1


@pytest.mark.parametrize("name,k,nv", CASES, ids=IDS)
def test_matrix_operands(name, k, nv):
    o = ops(name, k)
    if o.tile > 1:
        o = ops(name, 6)      # the matrix runs of the checking build use D = 2^6 for goldilocks
    for n, m in ((9, 41), (5, 41)):
        a = C.craft_gram(o, n, m)
        A = o.elems(a)
        for i, j in ((0, 0), (1, 0), (2, 0), (2, 1)) + (((3, 0), (6, 4)) if n == 9 else ()):
            prods = [o.mul(A[i * m + t], A[j * m + t]) for t in range(m)]
            sg = subsets_stay_near_zero(o, prods, "gram products", 9)
            assert (sg[:, 0] != 0).all()
        g = C.model_gram(o, a, n, m)
        at = lambda i, j: o.lanes(g[i * (i + 1) // 2 + j])  # noqa: E731
        assert np.array_equal(at(1, 0), at(0, 0)) and np.array_equal(at(2, 0), (o.p - at(0, 0)) % o.p)
        assert np.array_equal(at(n - 1, n - 2), (o.p - at(n - 1, n - 1)) % o.p)
        zero_sum = (at(n - 1, n - 2) + at(n - 1, n - 1)) % o.p
        assert not zero_sum.any()
    mat, powers = C.craft_recompose(o, 5, 3)
    every_class(o, powers, "recompose weights")
    rows_a, rows_b = C.craft_spgemm(o, 5, 41, 2)
    prods = [o.mul(o.elem(rows_b[t][0][0]), o.elem(rows_a[0][t][0])) for t in range(41)]
    subsets_stay_near_zero(o, prods, "spgemm products", 11)
    assert all(np.array_equal(row[1][0], o.neg(row[0][0])) for row in rows_b)


def test_the_three_max_limb_flavours_are_canonical_and_differ():
    o = ops("stark", 4)
    imgs = [o.from_words(C.max_limb_images(16, f))[0] for f in C.FLAVOURS]
    assert all((x < o.p).all() and (x >> 250).all() or f == "alternating" for x, f in zip(imgs, C.FLAVOURS))
    assert all(not np.array_equal(a, b) for a in imgs for b in imgs if a is not b)
    t = C.stark_flavour_table(o, 7, 1)
    assert np.array_equal(t[0], imgs[1]) and np.array_equal(t[2], imgs[0])
