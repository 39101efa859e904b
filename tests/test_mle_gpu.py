"""GPU parity of the dense multilinear-extension calls (sr_mle_fix_variables[_dev], sr_mul_elem_add_batch[_dev]) for all six ring
ids.  Every comparison is bit-exact.  Expected values come from tools/model_mle.py, the one-variable-at-a-time restatement of
crates/poly mle/dense.rs:171-199 and polynomials/multilinear_polynomial.rs:251-286 (pinned against the closed form by
tests/test_mle_host.py): on standard-form Python integers for the power-of-two rings, on the oracle's Fq3 / Fq9 / Fq4 slot products
plus integer add / sub for the reference's own rings."""
import os
import sys

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import model_mle as M  # noqa: E402

pytestmark = pytest.mark.gpu
LEADING, TRAILING = 0, 1
ORDERS = (LEADING, TRAILING)
# (ring, log2 D, num_vars); SMALLEST: the smallest table of each family, where every n_fixed is run
CASES = [("goldilocks", 6, 10), ("goldilocks", 16, 4), ("babybear", 5, 9), ("stark", 4, 8), ("stark", 12, 3),
         ("goldilocks24", 0, 11), ("babybear72", 0, 9), ("frog16", 0, 11)]
LARGER = {("goldilocks", 16), ("stark", 12)}
IDS = ["%s-%d-nv%d" % c for c in CASES]
BASE = {"goldilocks24": "goldilocks", "babybear72": "babybear", "frog16": "frog"}
SLOT_MUL = {"goldilocks24": ("sro_g24_ntt_mul", 3), "babybear72": ("sro_bb72_ntt_mul", 9), "frog16": ("sro_frog16_ntt_mul", 4)}
POISON = 0xDEADBEEFCAFEF00D  # not canonical in any of the fields: a kernel that read it would show it


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
        """flat memory words -> list of model elements"""
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

    def expect(self, table, nv, point, order):
        """the folded table as memory words; table (memory words, or a list of model elements from elems()) may hold fewer than
        2^nv elements"""
        table = self.elems(table) if isinstance(table, np.ndarray) else table
        point = self.elems(point) if isinstance(point, np.ndarray) else point
        return self.words(M.fold(M.pad(table, nv, self.zero()), nv, point, order, self.add, self.sub, self.mul))

    def uniform(self, seed, n_elems):
        return O.fill_uniform(self.F, seed, 0, n_elems * self.ring.degree)

    def const(self, word, n_elems):
        """every coefficient the memory word `word` (all limbs of a Stark coefficient together)"""
        return np.tile(O.ints_to_limbs([word], self.ring.limbs), n_elems * self.ring.degree)

    def one(self):
        """the ring's one in CRT/NTT form: 1 in every slot"""
        m1 = O.to_mont(self.F, [1])
        if self.pow2:
            return np.tile(m1, self.ring.degree)
        out = np.zeros(self.w, dtype=np.uint64)
        out[::SLOT_MUL[self.name][1]] = m1[0]
        return out


_models = {}


def model_for(name, k):
    if (name, k) not in _models:
        _models[(name, k)] = Model(name, k)
    return _models[(name, k)]


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def fold_dev(torch, ring, evals_t, nv, point_t, order, out_t=None, stream=None):
    """the _dev call with a workspace of exactly the planned size; returns (out tensor, workspace or None)"""
    w = ring.words_per_elem
    nf = point_t.numel() // w
    if out_t is None:
        out_t = torch.full((w << (nv - nf),), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    work_elems, launches = ring.mle_plan(nv, nf, order)
    work = torch.full((max(work_elems, 1) * w,), 0x3C3C3C3C3C3C3C3C, dtype=torch.int64, device="cuda") if work_elems else None
    ring.mle_fix_variables_dev(out_t, evals_t, nv, point_t, order, work, stream=stream)
    return out_t, work


def n_fixed_list(name, k, nv):
    return [j for j in (1, 2, 3, 4, nv) if j <= nv] if (name, k) in LARGER else list(range(nv + 1))


@pytest.mark.parametrize("name,k,nv", CASES, ids=IDS)
@pytest.mark.parametrize("order", ORDERS, ids=["leading", "trailing"])
def test_full_tables_match_the_restatement(torch_cuda, name, k, nv, order):
    torch = torch_cuda
    m = model_for(name, k)
    ring = m.ring
    table = m.uniform(0xE0 + k + nv, 1 << nv)
    point = m.uniform(0xF0 + k + nv, nv)
    t_table, t_point = dev(torch, table), dev(torch, point)
    T, Pt = m.elems(table), m.elems(point)
    for nf in sorted(set(n_fixed_list(name, k, nv))):
        pt = point[:nf * m.w] if order == LEADING else point[(nv - nf) * m.w:]
        want = m.expect(T, nv, Pt[:nf] if order == LEADING else Pt[nv - nf:], order)
        got, _ = fold_dev(torch, ring, t_table, nv, dev(torch, pt), order)
        torch.cuda.synchronize()
        assert np.array_equal(host(got), want), "%s nv %d n_fixed %d order %d" % (name, nv, nf, order)
        assert ring.count_noncanonical_dev(got) == 0
        assert np.array_equal(ring.mle_fix_variables(table, nv, pt, order), want), "host-pointer form, n_fixed %d" % nf
    assert np.array_equal(host(t_table), table) and np.array_equal(host(t_point), point), "an input was written"


@pytest.mark.parametrize("name,k,nv", CASES, ids=IDS)
def test_truncated_tables_and_poison_behind_them(torch_cuda, name, k, nv):
    torch = torch_cuda
    m = model_for(name, k)
    ring = m.ring
    full = m.uniform(0xA0 + k + nv, 1 << nv)
    point = m.uniform(0xB0 + k + nv, nv)
    T, Pt = m.elems(full), m.elems(point)
    odd = (1 << (nv - 2)) - 1   # the largest odd number below 2^(nv-2) (every case has nv >= 3)
    assert odd % 2 == 1
    for n_evals in sorted({0, 1, (1 << nv) - 1, (1 << (nv - 1)) + 1, odd}):
        buf = full.copy()
        buf[n_evals * m.w:] = POISON
        t_buf = dev(torch, buf)
        for order in ORDERS:
            for nf in sorted({1, min(3, nv), min(4, nv), nv}):
                pt = point[:nf * m.w] if order == LEADING else point[(nv - nf) * m.w:]
                want = m.expect(T[:n_evals], nv, Pt[:nf] if order == LEADING else Pt[nv - nf:], order)
                got, _ = fold_dev(torch, ring, t_buf[:n_evals * m.w], nv, dev(torch, pt), order)
                torch.cuda.synchronize()
                assert np.array_equal(host(got), want), "%s n_evals %d n_fixed %d order %d" % (name, n_evals, nf, order)
                assert ring.count_noncanonical_dev(got) == 0
        assert np.array_equal(host(t_buf), buf)
        got0, _ = fold_dev(torch, ring, t_buf[:n_evals * m.w], nv, t_buf[:0], LEADING)   # n_fixed = 0: copy and zero-pad
        torch.cuda.synchronize()
        assert np.array_equal(host(got0), np.concatenate([full[:n_evals * m.w], np.zeros(((1 << nv) - n_evals) * m.w, dtype=np.uint64)]))


@pytest.mark.parametrize("name,k,nv", CASES, ids=IDS)
def test_edge_tables_and_edge_points(torch_cuda, name, k, nv):
    torch = torch_cuda
    m = model_for(name, k)
    ring = m.ring
    p = m.p
    tables = {"zero": m.const(0, 1 << nv), "p-1": m.const(p - 1, 1 << nv), "1": m.const(1, 1 << nv), "uniform": m.uniform(0x33 + nv, 1 << nv)}
    words = [0, 1, p - 1]
    points = {"edge": np.concatenate([m.const(words[i % 3], 1) for i in range(nv)]), "uniform": m.uniform(0x44 + nv, nv)}
    P = {pn: m.elems(point) for pn, point in points.items()}
    for tn, table in tables.items():
        T = m.elems(table)
        for pn, point in points.items():
            if tn == "uniform" and pn == "uniform":
                continue
            for order in ORDERS:
                for nf in sorted({min(2, nv), nv}):
                    pt = point[:nf * m.w] if order == LEADING else point[(nv - nf) * m.w:]
                    got, _ = fold_dev(torch, ring, dev(torch, table), nv, dev(torch, pt), order)
                    torch.cuda.synchronize()
                    want = m.expect(T, nv, P[pn][:nf] if order == LEADING else P[pn][nv - nf:], order)
                    assert np.array_equal(host(got), want), (name, tn, pn, order, nf)
                    assert ring.count_noncanonical_dev(got) == 0


@pytest.mark.parametrize("name,k,nv", CASES, ids=IDS)
def test_a_boolean_point_selects_one_evaluation(torch_cuda, name, k, nv):
    torch = torch_cuda
    from stark_rings_amd import DenseMultilinearExtension

    m = model_for(name, k)
    ring = m.ring
    table = m.uniform(0x55 + nv, 1 << nv)
    t_table = dev(torch, table)
    one, zero = m.one(), np.zeros(m.w, dtype=np.uint64)
    for index in sorted({0, 1, (1 << nv) // 3, (1 << nv) - 2, (1 << nv) - 1}):
        point = np.concatenate([one if (index >> i) & 1 else zero for i in range(nv)])
        want = table[index * m.w:(index + 1) * m.w]
        for order in ORDERS:
            got, _ = fold_dev(torch, ring, t_table, nv, dev(torch, point), order)
            torch.cuda.synchronize()
            assert np.array_equal(host(got), want), (name, index, order)
        mle = DenseMultilinearExtension(ring, nv, t_table)
        assert np.array_equal(host(mle.evaluate(dev(torch, point))), want)
        assert mle.evaluate(dev(torch, point[m.w:])) is None if nv else True


@pytest.mark.parametrize("name,k,nv", CASES, ids=IDS)
def test_splits_in_place_and_the_class(torch_cuda, name, k, nv):
    """Fixing point[:j] and then point[j:] equals fixing point at once for every j (one-variable launches against fused ones, for both
    orders); a trailing fold in place equals the one out of place; the DenseMultilinearExtension methods agree with the calls."""
    torch = torch_cuda
    from stark_rings_amd import DenseMultilinearExtension

    m = model_for(name, k)
    ring = m.ring
    w = m.w
    n_evals = (1 << nv) - 3 if nv >= 2 else 1 << nv
    table = m.uniform(0x66 + nv, n_evals)
    point = m.uniform(0x77 + nv, nv)
    t_table, t_point = dev(torch, table), dev(torch, point)
    whole = {order: host(fold_dev(torch, ring, t_table, nv, t_point, order)[0]) for order in ORDERS}
    torch.cuda.synchronize()
    T, Pt = m.elems(table), m.elems(point)
    want = m.expect(T, nv, Pt, LEADING)
    assert np.array_equal(whole[LEADING], want) and np.array_equal(whole[TRAILING], want)
    for j in range(nv + 1):
        first, _ = fold_dev(torch, ring, t_table, nv, t_point[:j * w], LEADING)
        second, _ = fold_dev(torch, ring, first, nv - j, t_point[j * w:], LEADING)
        last, _ = fold_dev(torch, ring, t_table, nv, t_point[j * w:], TRAILING)
        rest, _ = fold_dev(torch, ring, last, j, t_point[:j * w], TRAILING)
        # one variable per call, j calls: the one-variable kernel against the fused plan
        step = t_table
        for i in range(j):
            step, _ = fold_dev(torch, ring, step, nv - i, t_point[i * w:(i + 1) * w], LEADING)
        torch.cuda.synchronize()
        assert np.array_equal(host(second), want) and np.array_equal(host(rest), want), (name, j)
        if j:   # j = 0: `first` is the zero-padded copy, `step` still the truncated table
            assert np.array_equal(host(step), host(first)), (name, j)
        # in place: the table in a buffer of 2^nv elements, folded onto itself
        buf = torch.full((w << nv,), POISON - (1 << 64), dtype=torch.int64, device="cuda")
        buf[:n_evals * w] = t_table
        ring.mle_fix_variables_dev(buf[:w << j], buf[:n_evals * w], nv, t_point[j * w:], TRAILING, None)
        torch.cuda.synchronize()
        assert np.array_equal(host(buf[:w << j]), host(last)), (name, j)
    assert np.array_equal(host(t_table), table) and np.array_equal(host(t_point), point)
    mle = DenseMultilinearExtension.from_evaluations_vec_padded(ring, nv, t_table)
    assert mle.num_vars == nv and np.array_equal(host(mle.to_evaluations())[:table.size], table) and not host(mle.to_evaluations())[table.size:].any()
    j = nv // 2
    fixed = mle.fixed_variables(t_point[:j * w])
    lastv = mle.fix_last_variables(t_point[j * w:])
    assert fixed.num_vars == nv - j and lastv.num_vars == j and mle.num_vars == nv
    assert np.array_equal(host(fixed.evaluations), m.expect(T, nv, Pt[:j], LEADING))
    assert np.array_equal(host(lastv.evaluations), m.expect(T, nv, Pt[j:], TRAILING))
    mle.fix_variables(t_point[:j * w]).fix_variables(t_point[j * w:])
    assert mle.num_vars == 0 and np.array_equal(host(mle.evaluations), want)


@pytest.mark.parametrize("name,k,nv", [CASES[0], CASES[3], CASES[5], CASES[7]], ids=[IDS[0], IDS[3], IDS[5], IDS[7]])
@pytest.mark.parametrize("order", ORDERS, ids=["leading", "trailing"])
def test_a_fold_is_capturable_on_a_fresh_context(torch_cuda, name, k, nv, order):
    """Captured into a graph on a non-default stream with a caller-supplied workspace, on a context that has never run the call (or
    anything else) eagerly; replayed twice on new values in the same buffers.  One branch, nothing forked."""
    torch = torch_cuda
    from stark_rings_amd import CyclotomicRing

    m = model_for(name, k)
    fresh = CyclotomicRing(name, k, device=0)
    w = m.w
    t_table = dev(torch, m.uniform(0x88, 1 << nv))
    t_point = dev(torch, m.uniform(0x89, nv))
    out = torch.zeros(w, dtype=torch.int64, device="cuda")
    work_elems, launches = fresh.mle_plan(nv, nv, order)
    assert launches >= 2 and work_elems > 0
    work = torch.zeros(work_elems * w, dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        fresh.mle_fix_variables_dev(out, t_table, nv, t_point, order, work, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    for seed in (0x91, 0x92):
        table = m.uniform(seed, 1 << nv)
        t_table.copy_(dev(torch, table))
        want, _ = fold_dev(torch, m.ring, t_table, nv, t_point, order)     # eager, on the long-lived context
        torch.cuda.synchronize()
        out.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(host(out), host(want)), (name, order, seed)
    assert np.array_equal(host(out), m.expect(table, nv, host(t_point), order))
    del g
    fresh.close()


def test_every_refusal_names_its_reason(torch_cuda):
    torch = torch_cuda
    from stark_rings_amd import RingError, _lib

    ring = ring_for("goldilocks", 6)
    lib, ctx, w = ring._lib, ring._ctx, ring.words_per_elem
    nv = 6
    pool = torch.zeros(256 * w, dtype=torch.int64, device="cuda")
    base = pool.data_ptr()
    E = w * 8                                     # bytes per element
    evals, point, out, work = base, base + 64 * E, base + 80 * E, base + 100 * E   # 64, 6, up to 16 and 16 elements: all disjoint
    need = ring.mle_plan(nv, nv, LEADING)[0]
    assert need > 0

    def call(o, e, n_evals, num_vars, p, nf, order, wk, wn):
        rc = lib.sr_mle_fix_variables_dev(ctx, o, e, n_evals, num_vars, p, nf, order, wk, wn, None)
        return rc, _lib.last_error()

    assert call(out, evals, 64, nv, point, nv, LEADING, work, need)[0] == 0
    for args, msg in (
        ((out, evals, 64, nv, point, nv, 7, work, need), "unknown order"),
        ((out, evals, 64, 48, point, nv, LEADING, work, need), "num_vars must be below 48"),
        ((out, evals, 64, nv, point, nv + 1, LEADING, work, need), "n_fixed exceeds num_vars"),
        ((out, evals, 65, nv, point, nv, LEADING, work, need), "n_evals exceeds 2^num_vars"),
        ((None, evals, 64, nv, point, nv, LEADING, work, need), "null buffer"),
        ((out, None, 64, nv, point, nv, LEADING, work, need), "null buffer"),
        ((out, evals, 64, nv, None, nv, LEADING, work, need), "null buffer"),
        ((out, evals, 64, nv, point, nv, LEADING, None, need), "null buffer"),
        ((out, evals, 64, nv, point, nv, LEADING, work, need - 1), "workspace too small"),
        ((evals, evals, 64, nv, point, nv, LEADING, work, need), "d_out overlaps d_evals"),
        ((evals + E, evals, 64, nv, point, 1, TRAILING, work, need), "d_out overlaps d_evals"),
        ((point, evals, 64, nv, point, nv, LEADING, work, need), "d_out overlaps d_point"),
        ((work, evals, 64, nv, point, nv, LEADING, work, need), "d_out overlaps d_work"),
        ((out, evals, 64, nv, point, nv, LEADING, evals + 8 * E, need), "d_evals overlaps d_work"),
        ((out, evals, 64, nv, point, nv, LEADING, point + 2 * E, need), "d_point overlaps d_work"),
        ((out, evals, 64, nv, evals + 3 * E, nv, LEADING, work, need), "d_evals overlaps d_point"),
    ):
        rc, err = call(*args)
        assert rc == 1 and msg in err, (args, rc, err)
    # in place is the trailing order's privilege, and needs no workspace
    assert call(evals, evals, 64, nv, point, nv, TRAILING, None, 0)[0] == 0
    torch.cuda.synchronize()
    acc, x, r = base, base + 32 * E, base + 200 * E
    assert lib.sr_mul_elem_add_batch_dev(ctx, acc, x, r, 16, None) == 0
    assert lib.sr_mul_elem_add_batch_dev(ctx, acc, x, acc + 3 * E, 16, None) == 1 and "r must not lie inside" in _lib.last_error()
    assert lib.sr_mul_elem_add_batch_dev(ctx, acc, x, x + 15 * E, 16, None) == 1 and "r must not lie inside" in _lib.last_error()
    assert lib.sr_mul_elem_add_batch_dev(ctx, acc, acc + E, r, 16, None) == 1 and "same buffer or disjoint" in _lib.last_error()
    torch.cuda.synchronize()
    t = pool[:4 * w]
    with pytest.raises(RingError, match="2\\^\\(num_vars - n_fixed\\)"):
        ring.mle_fix_variables_dev(pool[:3 * w], t, 2, pool[64 * w:65 * w], LEADING)
    with pytest.raises(RingError, match="more entries"):
        ring.mle_fix_variables_dev(pool[:w], t, 2, pool[64 * w:67 * w], LEADING)
    with pytest.raises(RingError, match="one ring element"):
        ring.mul_elem_add_dev(t, t, pool[64 * w:66 * w])


@pytest.mark.parametrize("name,k,batch", [("goldilocks", 6, 37), ("goldilocks", 0, 5), ("babybear", 5, 13), ("stark", 4, 11), ("stark", 0, 3),
                                          ("goldilocks24", 0, 101), ("babybear72", 0, 67), ("frog16", 0, 259), ("goldilocks", 12, 3)])
def test_mul_elem_add_matches_add_of_the_slot_product(torch_cuda, name, k, batch):
    """acc + ntt_mul(x, tile(r)) with the existing (oracle-pinned) entry points, ragged batches, r = 0, acc aliasing x, both forms"""
    torch = torch_cuda
    m = model_for(name, k)
    ring = m.ring
    acc, x, r = m.uniform(0x21, batch), m.uniform(0x22, batch), m.uniform(0x23, 1)
    for rr in (r, np.zeros(m.w, dtype=np.uint64)):
        want = ring.add(acc.copy(), ring.ntt_mul(x.copy(), np.tile(rr, batch)))
        t_acc = dev(torch, acc)
        ring.mul_elem_add_dev(t_acc, dev(torch, x), dev(torch, rr))
        torch.cuda.synchronize()
        assert np.array_equal(host(t_acc), want), (name, "dev")
        assert ring.count_noncanonical_dev(t_acc) == 0
        assert np.array_equal(ring.mul_elem_add(acc.copy(), x, rr), want), (name, "host")
        alias = ring.add(x.copy(), ring.ntt_mul(x.copy(), np.tile(rr, batch)))
        t_x = dev(torch, x)
        ring.mul_elem_add_dev(t_x, t_x, dev(torch, rr))
        torch.cuda.synchronize()
        assert np.array_equal(host(t_x), alias), (name, "alias")
        h = x.copy()
        assert np.array_equal(ring.mul_elem_add(h, h, rr), alias), (name, "host alias")


def test_add_assign_scaled_of_the_class(torch_cuda):
    torch = torch_cuda
    from stark_rings_amd import DenseMultilinearExtension, RingError

    m = model_for("goldilocks24", 0)
    ring = m.ring
    nv = 5
    a, b, r = m.uniform(0x31, 1 << nv), m.uniform(0x32, 1 << nv), m.uniform(0x33, 1)
    A = DenseMultilinearExtension(ring, nv, dev(torch, a))
    B = DenseMultilinearExtension(ring, nv, dev(torch, b))
    A.add_assign_scaled(dev(torch, r), B)
    torch.cuda.synchronize()
    assert np.array_equal(host(A.evaluations), ring.add(a.copy(), ring.ntt_mul(b.copy(), np.tile(r, 1 << nv))))
    with pytest.raises(RingError):
        A.add_assign_scaled(dev(torch, r), DenseMultilinearExtension(ring, nv, dev(torch, b[:m.w])))
