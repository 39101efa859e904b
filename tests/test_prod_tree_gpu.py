"""GPU parity of the grand-product calls (sr_prod_tree[_dev], ProductTree) for all six ring ids.  Every comparison is bit-exact.
Expected values come from tools/model_prod_tree.py, the pair-at-a-time restatement of both orders (pinned against the closed form by
tests/test_prod_tree_host.py): on standard-form Python integers for the power-of-two rings, on the oracle's Fq3 / Fq9 / Fq4 slot
products for the reference's own rings.  The cases are the smallest tables at which a launch split, a group boundary or an access
width can go wrong."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

import oracle_lib as O
from test_mle_gpu import POISON, dev, host, model_for, ring_for
from test_sumcheck_gpu import _interp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import model_prod_tree as PT  # noqa: E402

pytestmark = pytest.mark.gpu
LEADING, TRAILING = 0, 1
ORDERS = (LEADING, TRAILING)
ORDER_IDS = ["leading", "trailing"]
# (ring, log2 D, num_vars)
CASES = [("goldilocks", 6, 7), ("goldilocks", 16, 4), ("babybear", 5, 7), ("stark", 4, 5), ("stark", 12, 3),
         ("goldilocks24", 0, 8), ("babybear72", 0, 7), ("frog16", 0, 8)]
IDS = ["%s-%d-nv%d" % c for c in CASES]
SMALL = [c for c in CASES if c[:2] not in {("goldilocks", 16), ("stark", 12)}]
SMALL_IDS = ["%s-%d-nv%d" % c for c in SMALL]
# the smallest ring of each family, where every num_vars = 0 .. jmax + 1 is run
SMALLEST = [("babybear", 5), ("stark", 4), ("babybear72", 0), ("frog16", 0)]
JMAX = {"babybear72": 2}   # levels per launch: three everywhere else
GUARD = 0x6B6B6B6B6B6B6B6B
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "prod_tree_kats.json")))["cases"]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def jmax(name):
    return JMAX.get(name, 3)


def one_elem(m):
    return m.elems(m.one())[0]


def mul(m):
    return lambda a, b: m.mul(b, a)


_trees = {}


def want_tree(m, key, leaf_elems, nv, order):
    """the layers 1 .. nv as memory words, computed once per key"""
    k = (m.name, m.k, nv, order, key)
    if k not in _trees:
        _trees[k] = m.words(PT.flat(PT.layers(leaf_elems, nv, order, one_elem(m), mul(m))))
    return _trees[k]


_leaves = {}


def leaves_for(m, nv):
    """the shared leaves of a case: (memory words, model elements)"""
    k = (m.name, m.k, nv)
    if k not in _leaves:
        words = m.uniform(0x9A00 + m.k + nv, 1 << nv)
        _leaves[k] = (words, m.elems(words))
    return _leaves[k]


def tree_dev(torch, ring, t_leaves, nv, order, stream=None, layers=None):
    """the _dev call into a buffer with one guard element behind the 2^nv - 1 outputs; returns (layers view, whole buffer)"""
    w = ring.words_per_elem
    n = ((1 << nv) - 1) * w
    if layers is None:
        layers = torch.full((n + w,), GUARD, dtype=torch.int64, device="cuda")
    ring.prod_tree_dev(layers[:n], t_leaves, nv, order, stream=stream)
    return layers[:n], layers


def guard_intact(whole, w):
    return bool((host(whole[-w:]) == np.uint64(GUARD)).all())


@pytest.mark.parametrize("name,k,nv", CASES, ids=IDS)
@pytest.mark.parametrize("order", ORDERS, ids=ORDER_IDS)
def test_full_tables_match_the_restatement(torch_cuda, name, k, nv, order):
    torch = torch_cuda
    m = model_for(name, k)
    ring = m.ring
    words, els = leaves_for(m, nv)
    t_leaves = dev(torch, words)
    want = want_tree(m, "full", els, nv, order)
    got, whole = tree_dev(torch, ring, t_leaves, nv, order)
    torch.cuda.synchronize()
    assert np.array_equal(host(got), want), "%s nv %d order %d" % (name, nv, order)
    assert guard_intact(whole, m.w)
    assert ring.count_noncanonical_dev(got) == 0
    assert np.array_equal(host(t_leaves), words), "the leaves were written"
    elems, launches = ring.prod_tree_plan(nv, order)
    assert elems == (1 << nv) - 1 and launches == -(-nv // jmax(name))


@pytest.mark.parametrize("name,k", SMALLEST, ids=["%s-%d" % c for c in SMALLEST])
def test_every_num_vars_up_to_one_past_a_launch(torch_cuda, name, k):
    torch = torch_cuda
    m = model_for(name, k)
    ring = m.ring
    for nv in range(jmax(name) + 2):
        full = 1 << nv
        words = m.uniform(0x9B00 + nv, full)
        els = m.elems(words)
        for order in ORDERS:
            for n_leaves in sorted({full, full - 1, 0}):
                want = m.words(PT.flat(PT.layers(els[:n_leaves], nv, order, one_elem(m), mul(m))))
                got, whole = tree_dev(torch, ring, dev(torch, words)[:n_leaves * m.w], nv, order)
                torch.cuda.synchronize()
                assert np.array_equal(host(got), want), "%s nv %d n_leaves %d order %d" % (name, nv, n_leaves, order)
                assert guard_intact(whole, m.w)   # num_vars = 0 writes nothing at all
                assert ring.prod_tree_plan(nv, order) == (full - 1, -(-nv // jmax(name)))


def truncations(name, nv):
    """0, 1, a value inside a group of the first launch, one below a group boundary, 2^nv - 1"""
    g, full = 1 << jmax(name), 1 << nv
    inside = g + 3 if g + 3 < full else 3
    below = 2 * g - 1 if 2 * g <= full else g - 1
    return sorted({0, 1, inside, below, full - 1})


@pytest.mark.parametrize("name,k,nv", CASES, ids=IDS)
def test_truncated_tables_poison_behind_the_leaves_and_a_guard_behind_the_layers(torch_cuda, name, k, nv):
    torch = torch_cuda
    m = model_for(name, k)
    ring = m.ring
    words, els = leaves_for(m, nv)
    for n_leaves in truncations(name, nv):
        buf = words.copy()
        buf[n_leaves * m.w:] = POISON   # not canonical in any of the fields: a kernel that read it would show it
        t_buf = dev(torch, buf)
        for order in ORDERS:
            want = want_tree(m, n_leaves, els[:n_leaves], nv, order)
            got, whole = tree_dev(torch, ring, t_buf[:n_leaves * m.w], nv, order)
            torch.cuda.synchronize()
            assert np.array_equal(host(got), want), "%s n_leaves %d order %d" % (name, n_leaves, order)
            assert guard_intact(whole, m.w)
            assert ring.count_noncanonical_dev(got) == 0
        assert np.array_equal(host(t_buf), buf), "the leaves (or the poison behind them) were written"


@pytest.mark.parametrize("name,k,nv", SMALL, ids=SMALL_IDS)
def test_edge_leaves_and_a_single_zero(torch_cuda, name, k, nv):
    torch = torch_cuda
    m = model_for(name, k)
    ring = m.ring
    full = 1 << nv
    top = m.const(m.p - 1, 1)   # every coefficient the memory word p - 1
    one = m.one()
    for what, leaf in (("p - 1", top), ("zero", np.zeros(m.w, dtype=np.uint64)), ("one", one)):
        words = np.tile(leaf, full)
        for order in ORDERS:
            want = want_tree(m, what, m.elems(words), nv, order)
            got, _ = tree_dev(torch, ring, dev(torch, words), nv, order)
            torch.cuda.synchronize()
            assert np.array_equal(host(got), want), "%s all %s order %d" % (name, what, order)
            if what != "p - 1":
                assert np.array_equal(host(got), np.tile(leaf, full - 1))
    # a single zero among leaves that are all one(): exactly the nodes above it are zero, every other node is one()
    for z in sorted({0, 5, full // 2, full - 1}):
        words = np.tile(one, full)
        words[z * m.w:(z + 1) * m.w] = 0
        for order in ORDERS:
            got, _ = tree_dev(torch, ring, dev(torch, words), nv, order)
            torch.cuda.synchronize()
            got = host(got)
            for lvl in range(1, nv + 1):
                above = z >> lvl if order == LEADING else z & ((1 << (nv - lvl)) - 1)
                off = PT.layer_offset(nv, lvl)
                for i in range(1 << (nv - lvl)):
                    e = got[(off + i) * m.w:(off + i + 1) * m.w]
                    assert np.array_equal(e, np.zeros_like(e) if i == above else one), (name, order, z, lvl, i)
    # and among uniform leaves: the model, whose zero stays where the products carry it
    words, _ = leaves_for(m, nv)
    words = words.copy()
    words[5 * m.w:6 * m.w] = 0
    for order in ORDERS:
        want = want_tree(m, "zero at 5", m.elems(words), nv, order)
        got, _ = tree_dev(torch, ring, dev(torch, words), nv, order)
        torch.cuda.synchronize()
        assert np.array_equal(host(got), want)


@pytest.mark.parametrize("name,k,nv", [("goldilocks", 6, 7), ("babybear", 5, 7), ("stark", 4, 5), ("goldilocks", 0, 5), ("babybear", 0, 4),
                                       ("goldilocks24", 0, 4)],
                         ids=["goldilocks-6", "babybear-5", "stark-4", "goldilocks-0", "babybear-0", "goldilocks24"])
def test_the_one_coefficient_path_at_odd_eight_byte_pointers_and_at_degree_one(torch_cuda, name, k, nv):
    """d_layers or d_leaves 8 bytes past a 16-byte boundary takes the one-coefficient path of the one-limb kernels, as does D = 1"""
    torch = torch_cuda
    m = model_for(name, k)
    ring = m.ring
    w, full = m.w, 1 << nv
    words, els = leaves_for(m, nv)
    n_out = (full - 1) * w
    for n_leaves in (full, full - 3):
        for order in ORDERS:
            want = want_tree(m, n_leaves if n_leaves != full else "full", els[:n_leaves], nv, order)
            for shift_leaves, shift_layers in ((1, 0), (0, 1), (1, 1), (0, 0)):
                src = torch.zeros(full * w + 2, dtype=torch.int64, device="cuda")
                assert src.data_ptr() % 16 == 0
                src[shift_leaves:shift_leaves + full * w] = dev(torch, words)
                dst = torch.full((n_out + w + 2,), GUARD, dtype=torch.int64, device="cuda")
                ring.prod_tree_dev(dst[shift_layers:shift_layers + n_out], src[shift_leaves:shift_leaves + n_leaves * w], nv, order)
                torch.cuda.synchronize()
                got = host(dst)
                assert np.array_equal(got[shift_layers:shift_layers + n_out], want), (name, n_leaves, order, shift_leaves, shift_layers)
                assert (got[:shift_layers] == np.uint64(GUARD)).all() and (got[shift_layers + n_out:] == np.uint64(GUARD)).all()


@pytest.mark.parametrize("name,k,nv", CASES, ids=IDS)
def test_existing_calls_are_a_second_witness(torch_cuda, name, k, nv):
    """the root is sr_product_batch_dev of the leaves; in trailing order every layer is sr_pointwise_mul_batch_dev of the halves of
    the layer below"""
    torch = torch_cuda
    m = model_for(name, k)
    ring = m.ring
    w, full = m.w, 1 << nv
    words, _ = leaves_for(m, nv)
    for n_leaves in (full, full - 3):
        t_leaves = dev(torch, words)[:n_leaves * w]
        root = torch.zeros(w, dtype=torch.int64, device="cuda")
        ring.product_dev(root, t_leaves)
        for order in ORDERS:
            got, _ = tree_dev(torch, ring, t_leaves, nv, order)
            torch.cuda.synchronize()
            assert torch.equal(got[-w:], root), (name, n_leaves, order)
        # trailing: got still holds the trailing tree
        below = torch.cat([t_leaves, dev(torch, np.tile(m.one(), full - n_leaves))]) if n_leaves < full else t_leaves
        for lvl in range(1, nv + 1):
            half = (1 << (nv - lvl)) * w
            prod = below[:half].clone()
            ring.ntt_mul_dev(prod, below[half:2 * half])   # sr_pointwise_mul_batch_dev
            off = PT.layer_offset(nv, lvl) * w
            assert torch.equal(got[off:off + half], prod), (name, n_leaves, lvl)
            below = got[off:off + half]


@pytest.mark.parametrize("name,k,nv", [("goldilocks", 6, 7), ("babybear", 5, 7), ("stark", 4, 5), ("goldilocks24", 0, 5), ("babybear72", 0, 4),
                                       ("frog16", 0, 5)], ids=["goldilocks", "babybear", "stark", "goldilocks24", "babybear72", "frog16"])
def test_the_layer_claim_of_the_grand_product_argument(torch_cuda, name, k, nv):
    """The GKR layer the feature exists for: with a trailing tree and a point z, L_k(z) = sum_b eq(z, b) lo_k(b) hi_k(b) for every k,
    lo_k and hi_k the halves of layer k - 1 as they lie; and one run of all rounds of that sum-check ends at eq, lo and hi at the
    point of the challenges."""
    torch = torch_cuda
    from stark_rings_amd import DenseMultilinearExtension as MLE, ProductTree, RingError, VirtualPolynomial

    m = model_for(name, k)
    ring = m.ring
    w = m.w
    words, _ = leaves_for(m, nv)
    tree = ProductTree(ring, dev(torch, words), nv, order=TRAILING)
    z = dev(torch, m.uniform(0x2A2A, nv))
    for lvl in range(1, nv + 1):
        n = nv - lvl
        zk = z[:n * w]
        value = tree.layer(lvl).evaluate(zk)
        lo, hi = tree.halves(lvl)
        assert lo.num_vars == hi.num_vars == n
        g = VirtualPolynomial(ring, n)
        g.add_mle_list([MLE.eq(ring, zk), lo, hi])
        torch.cuda.synchronize()
        assert torch.equal(g.sum(), value), (name, lvl)
    assert torch.equal(tree.root(), tree.layer(nv).evaluations)
    # all rounds at layer 1: n = nv - 1 variables, trailing order (round i fixes variable n - 1 - i at challenge i)
    n = nv - 1
    zk = z[:n * w]
    eq = MLE.eq(ring, zk)
    lo, hi = tree.halves(1)
    g = VirtualPolynomial(ring, n)
    g.add_mle_list([eq, lo, hi])
    claim_t = tree.layer(1).evaluate(zk)
    challenges = [dev(torch, m.uniform(0x7100 + i, 1)) for i in range(n)]
    msgs = [g.round_evals(TRAILING)]
    for rnd in range(1, n):
        msg, g = g.fold_round_evals(challenges[rnd - 1], TRAILING)
        msgs.append(msg)
    last = g.fixed_variables(challenges[n - 1], TRAILING)
    torch.cuda.synchronize()
    point = torch.cat(list(reversed(challenges)))   # variable j of the point is the challenge of round n - 1 - j
    finals = [t.evaluations for t in last.tables]
    assert last.num_vars == 0 and len(finals) == 3
    for f, table in zip(finals, (eq, lo, hi)):
        assert torch.equal(f, table.evaluate(point)), name
    if m.pow2:  # prime-field slots: p(0) + p(1) is the running claim, and the last claim is eq * lo * hi at the point
        claim = m.elems(host(claim_t))[0]
        for rnd, msg in enumerate(msgs):
            p = m.elems(host(msg))
            assert np.array_equal(m.add(p[0], p[1]), claim), (name, rnd)
            claim = _interp(m, host(msg), host(challenges[rnd]), 3)
        e, a, b = [m.elems(host(f))[0] for f in finals]
        assert np.array_equal(m.mul(e, m.mul(a, b)), claim)
    with pytest.raises(RingError, match="trailing"):
        ProductTree(ring, dev(torch, words), nv, order=LEADING).halves(1)


@pytest.mark.parametrize("name,k,nv", SMALL, ids=SMALL_IDS)
def test_permuted_leaves_have_one_root_and_a_changed_leaf_another(torch_cuda, name, k, nv):
    torch = torch_cuda
    from stark_rings_amd import ProductTree

    m = model_for(name, k)
    ring = m.ring
    w, full = m.w, 1 << nv
    words, _ = leaves_for(m, nv)
    perm = np.random.RandomState(nv).permutation(full)
    assert not np.array_equal(perm, np.arange(full))
    shuffled = words.reshape(full, w)[perm].reshape(-1).copy()
    for order in ORDERS:
        a = ProductTree(ring, dev(torch, words), nv, order=order)
        b = ProductTree(ring, dev(torch, shuffled), nv, order=order)
        torch.cuda.synchronize()
        assert torch.equal(a.root(), b.root()), (name, order)
        assert not torch.equal(a.layers, b.layers)
        changed = shuffled.copy()
        changed[3 * w:4 * w] = m.uniform(0x5151, 1)
        c = ProductTree(ring, dev(torch, changed), nv, order=order)
        torch.cuda.synchronize()
        assert not torch.equal(a.root(), c.root()), (name, order)
    lead = ProductTree(ring, dev(torch, words), nv, order=LEADING)
    trail = ProductTree(ring, dev(torch, words), nv, order=TRAILING)
    torch.cuda.synchronize()
    assert torch.equal(lead.root(), trail.root())


@pytest.mark.parametrize("name,k,nv", [("goldilocks", 6, 7), ("stark", 4, 5), ("babybear72", 0, 7)], ids=["goldilocks", "stark", "babybear72"])
@pytest.mark.parametrize("order", ORDERS, ids=ORDER_IDS)
def test_a_tree_is_capturable_on_a_fresh_context(torch_cuda, name, k, nv, order):
    """Captured into a graph on a non-default stream on a context that has never run the call (or anything else) eagerly; replayed
    twice on new leaves in the same buffers.  One branch, nothing forked: later launches read what earlier ones wrote."""
    torch = torch_cuda
    from stark_rings_amd import CyclotomicRing

    m = model_for(name, k)
    fresh = CyclotomicRing(name, k, device=0)
    w, full = m.w, 1 << nv
    assert fresh.prod_tree_plan(nv, order)[1] >= 2
    t_leaves = dev(torch, m.uniform(0x88, full))
    out = torch.zeros((full - 1) * w, dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        fresh.prod_tree_dev(out, t_leaves[:(full - 3) * w], nv, order, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    for seed in (0x91, 0x92):
        leaves = m.uniform(seed, full)
        t_leaves.copy_(dev(torch, leaves))
        want, _ = tree_dev(torch, m.ring, t_leaves[:(full - 3) * w], nv, order)     # eager, on the long-lived context
        torch.cuda.synchronize()
        out.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(host(out), host(want)), (name, order, seed)
    assert np.array_equal(host(out), m.words(PT.flat(PT.layers(m.elems(leaves)[:full - 3], nv, order, one_elem(m), mul(m)))))
    del g
    fresh.close()


@pytest.mark.parametrize("name,k,nv", CASES, ids=IDS)
def test_the_host_pointer_form_and_the_class_agree_with_the_device_call(torch_cuda, name, k, nv):
    torch = torch_cuda
    from stark_rings_amd import ProductTree, RingError

    m = model_for(name, k)
    ring = m.ring
    w, full = m.w, 1 << nv
    words, _ = leaves_for(m, nv)
    t_leaves = dev(torch, words)
    for n_leaves in (full, full - 3, 0):
        for order in ORDERS:
            want, _ = tree_dev(torch, ring, t_leaves[:n_leaves * w], nv, order)
            torch.cuda.synchronize()
            assert np.array_equal(ring.prod_tree(words[:n_leaves * w], nv, order), host(want)), (name, n_leaves, order)
            tree = ProductTree(ring, t_leaves, nv, n_leaves=n_leaves, order=order)
            torch.cuda.synchronize()
            assert tree.num_vars == nv and tree.n_leaves == n_leaves
            assert torch.equal(tree.layers, want)
            end = 0
            for lvl in range(1, nv + 1):
                layer = tree.layer(lvl)
                assert tree.layer_offset(lvl) == end and layer.num_vars == nv - lvl and len(layer) == 1 << (nv - lvl)
                assert torch.equal(layer.evaluations, want[end * w:(end + len(layer)) * w])
                assert layer.evaluations.data_ptr() == tree.layers.data_ptr() + end * w * 8, "a view, not a copy"
                end += len(layer)
            assert torch.equal(tree.root(), want[-w:])
            if n_leaves == full:
                assert tree.layer(0).evaluations.data_ptr() == t_leaves.data_ptr()
            else:
                with pytest.raises(RingError, match="truncated"):
                    tree.layer(0)
            with pytest.raises(RingError, match="out of range"):
                tree.layer(nv + 1)
    single = ProductTree(ring, t_leaves[:w], 0)
    assert single.layers.numel() == 0 and torch.equal(single.root(), t_leaves[:w])


def test_the_pinned_vectors(torch_cuda):
    torch = torch_cuda
    for c in KATS:
        name, k, nv, n = c["ring"], c["log2_degree"], c["num_vars"], c["n_leaves"]
        m = model_for(name, k)
        to_words = (lambda els: O.to_mont(m.F, [int(x) for e in els for x in e])) if c["form"] == "standard" else \
            (lambda els: np.array([x for e in els for x in e], dtype=np.uint64))
        t_leaves = dev(torch, to_words(c["leaves"]))
        assert t_leaves.numel() == n * m.w
        for key, order in (("leading", LEADING), ("trailing", TRAILING)):
            got, whole = tree_dev(torch, m.ring, t_leaves, nv, order)
            torch.cuda.synchronize()
            assert np.array_equal(host(got), to_words(c[key])), (name, key)
            assert guard_intact(whole, m.w)


def test_every_refusal_names_its_reason(torch_cuda):
    torch = torch_cuda
    from stark_rings_amd import ProductTree, RingError, _lib

    ring = ring_for("goldilocks", 6)
    w = ring.words_per_elem
    nv = 4
    lib, ctx = ring._lib, ring._ctx
    leaves = torch.zeros(16 * w, dtype=torch.int64, device="cuda")
    layers = torch.zeros(15 * w, dtype=torch.int64, device="cuda")
    pl, pe = ctypes.c_void_p(layers.data_ptr()), ctypes.c_void_p(leaves.data_ptr())
    null = ctypes.c_void_p(0)

    def refused(args, reason):
        assert lib.sr_prod_tree_dev(ctx, *args, None) == 1, args
        assert reason in _lib.last_error(), (reason, _lib.last_error())

    refused((pl, pe, 16, nv, 2), "unknown order")
    refused((pl, pe, 17, nv, TRAILING), "n_leaves exceeds 2^num_vars")
    refused((pl, pe, 16, 48, TRAILING), "num_vars must be below 48")
    refused((pl, pe, 16, 47, TRAILING), "element count too large")
    refused((null, pe, 16, nv, TRAILING), "null buffer")
    refused((pl, null, 16, nv, TRAILING), "null buffer")
    # any overlap of the layers and the stored leaves: the first and the last word of either range
    both = torch.zeros(31 * w, dtype=torch.int64, device="cuda")
    base = both.data_ptr()
    refused((ctypes.c_void_p(base), ctypes.c_void_p(base + (15 * w - 1) * 8), 16, nv, TRAILING), "d_layers overlaps d_leaves")
    refused((ctypes.c_void_p(base + (16 * w - 1) * 8), ctypes.c_void_p(base), 16, nv, TRAILING), "d_layers overlaps d_leaves")
    refused((ctypes.c_void_p(base), ctypes.c_void_p(base), 16, nv, LEADING), "d_layers overlaps d_leaves")
    # back to back is no overlap; neither are leaves that are not stored
    assert lib.sr_prod_tree_dev(ctx, ctypes.c_void_p(base + 16 * w * 8), ctypes.c_void_p(base), 16, nv, TRAILING, None) == 0
    assert lib.sr_prod_tree_dev(ctx, ctypes.c_void_p(base), ctypes.c_void_p(base), 0, nv, TRAILING, None) == 0
    assert lib.sr_prod_tree_dev(ctx, null, null, 0, 0, TRAILING, None) == 0   # num_vars = 0: nothing written
    torch.cuda.synchronize()
    host_buf = np.zeros(16 * w, dtype=np.uint64)
    hp = host_buf.ctypes.data_as(_lib.u64p)
    assert lib.sr_prod_tree(ctx, hp, hp, 16, nv, TRAILING) == 1 and "overlaps" in _lib.last_error()
    assert lib.sr_prod_tree(ctx, hp, hp, 1, nv, 7) == 1 and "unknown order" in _lib.last_error()
    # the mirror
    with pytest.raises(RingError, match="layers must hold"):
        ring.prod_tree_dev(layers[:14 * w], leaves, nv)
    with pytest.raises(RingError, match="more leaves"):
        ring.prod_tree_dev(layers, leaves, 3)
    with pytest.raises(RingError, match="unknown order"):
        ProductTree(ring, leaves, nv, order=2)
    with pytest.raises(RingError, match="n_leaves"):
        ProductTree(ring, leaves, nv, n_leaves=17)
    with pytest.raises(RingError, match="num_vars"):
        ProductTree(ring, leaves, 48)
