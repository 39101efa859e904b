"""GPU parity of the linear-combination calls (sr_lincomb_dev, sr_lincomb) and of what is built on them
(DenseMultilinearExtension.linear_combination, lookup.py) for all six ring ids.  Every comparison is bit-exact.  Expected values come
from tools/model_lincomb.py, the term-at-a-time restatement (pinned against its second formulation and closed forms by
tests/test_lincomb_host.py): on standard-form Python integers for the power-of-two rings, on the oracle's Fq3 / Fq9 / Fq4 slot products
plus integer adds for the reference's own rings.  Every output has a guard behind (and, where shifted, before) it and every stored
part of a table has poison behind it.

Sizes are the smallest at which a path changes: D = 1 (no 16-byte pair), several lane-groups in a workgroup with n no power of two,
one element across many workgroups, and on every family both sides of the bound of the kernel that keeps its coefficients in registers
(K = 4 / 5, and its outputs) and of the outputs of one launch (tests/test_lincomb_isa.py holds the table)."""
import json
import os
import sys

import numpy as np
import pytest

import oracle_lib as O
from test_mle_gpu import POISON, dev, host, model_for, ring_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import model_lincomb as LC  # noqa: E402

pytestmark = pytest.mark.gpu
# (ring, log2 D, n)
CASES = [("goldilocks", 0, 300), ("goldilocks", 6, 37), ("goldilocks", 16, 3), ("babybear", 5, 37), ("stark", 4, 21), ("stark", 12, 2),
         ("goldilocks24", 0, 70), ("babybear72", 0, 70), ("frog16", 0, 70)]
IDS = ["%s-%d-n%d" % c for c in CASES]
LARGER = {("goldilocks", 16), ("stark", 12)}
SMALL = [c for c in CASES if c[:2] not in LARGER]
SMALL_IDS = ["%s-%d-n%d" % c for c in SMALL]
CHECKS = [("goldilocks", 6), ("stark", 4), ("babybear72", 0)]
CHECK_IDS = [c[0] for c in CHECKS]
GUARD = 0x6B6B6B6B6B6B6B6B
ONES = 0xFFFFFFFFFFFFFFFF
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "lincomb_kats.json")))["cases"]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def i64(x):
    return x - (1 << 64) if x >= 1 << 63 else x


def expected(md, tw, cw, uses, n):
    """the model's outputs as memory words; tw: the stored words of each table, cw: the M (K + 1) coefficient elements"""
    K, M = len(tw), len(uses)
    ce = md.elems(cw)
    rows = [[ce[m * (K + 1) + k] if uses[m] >> k & 1 else None for k in range(K + 1)] for m in range(M)]
    outs = LC.lincomb([md.elems(t) for t in tw], rows, uses, n, md.zero(), md.add, md.mul)
    return [md.words(o) for o in outs]


def draw(md, K, M, n, n_evals=None, seed=0x11C0):
    ne = list(n_evals) if n_evals is not None else [n] * K
    return [md.uniform(seed + k, ne[k]) for k in range(K)], md.uniform(seed + 0x80, M * (K + 1))


def run(torch, md, tw, cw, uses, n, shift=0, stream=None, want=None, pass_n_evals=True):
    """one device call on fresh buffers: poison behind every stored part, ONES in every coefficient whose bit is clear, guards around
    the outputs; compares with the model and checks the guards.  shift: every buffer starts `shift` words past a 16-byte boundary."""
    from stark_rings_amd import lincomb_dev

    ring, w = md.ring, md.w
    K, M = len(tw), len(uses)
    want = expected(md, tw, cw, uses, n) if want is None else want
    tabs = []
    for t in tw:
        buf = torch.full((t.size + w + 2,), i64(POISON), dtype=torch.int64, device="cuda")
        assert buf.data_ptr() % 16 == 0
        buf[shift:shift + t.size] = dev(torch, t)
        tabs.append(buf[shift:shift + t.size])
    cp = cw.copy()
    for m in range(M):
        for k in range(K + 1):
            if not uses[m] >> k & 1:
                cp[(m * (K + 1) + k) * w:(m * (K + 1) + k + 1) * w] = np.uint64(ONES)
    cbuf = torch.zeros(cp.size + 2, dtype=torch.int64, device="cuda")
    cbuf[shift:shift + cp.size] = dev(torch, cp)
    whole = [torch.full((n * w + w + 2,), i64(GUARD), dtype=torch.int64, device="cuda") for _ in range(M)]
    outs = [b[shift:shift + n * w] for b in whole]
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    lincomb_dev(ring, outs, tabs, cbuf[shift:shift + cp.size], uses, n, [t.size // w for t in tw] if pass_n_evals else None, stream)
    torch.cuda.synchronize()
    for m in range(M):
        got = host(whole[m])
        assert np.array_equal(got[shift:shift + n * w], want[m]), (md.name, md.k, K, M, n, m, shift)
        assert (got[:shift] == np.uint64(GUARD)).all() and (got[shift + n * w:] == np.uint64(GUARD)).all(), "guard overwritten"
    return want


def shapes(name, k):
    if (name, k) in LARGER:
        return [(3, 2), (4, 1), (4, 3), (5, 1), (9, 1)]   # three groups of four tables; sixteen are run at the smaller degrees
    return [(K, M) for K in (1, 2, 3, 4, 5, 16) for M in (1, 2, 3, 4)]


@pytest.mark.parametrize("name,k,n", CASES, ids=IDS)
def test_every_shape_matches_the_model_with_and_without_the_constant(torch_cuda, name, k, n):
    """K in {1, 2, 3, 4, 5, 16} x M in {1, 2, 3, 4}: both kernels and every split of the outputs over launches; the even outputs add
    their constant, the odd ones do not (their constants hold 0xFF.. words)"""
    from stark_rings_amd import lincomb_plan

    md = model_for(name, k)
    seen = set()
    for K, M in shapes(name, k):
        tw, cw = draw(md, K, M, n, seed=0x1000 + 16 * K + M)
        uses = [(1 << K) - 1 | ((1 << K) if m % 2 == 0 else 0) for m in range(M)]
        run(torch_cuda, md, tw, cw, uses, n, pass_n_evals=(K + M) % 2 == 0)
        seen.add(lincomb_plan(md.ring, K, M) + (LC.plan(md.ring.ring, K, M)[2],))
    assert {s[2] for s in seen} == ({True, False} if LC.OUTPUTS[md.ring.ring][0] else {False})
    if (name, k) not in LARGER:
        assert max(s[0] for s in seen) == -(-4 // LC.OUTPUTS[md.ring.ring][1])


@pytest.mark.parametrize("name,k,n", SMALL, ids=SMALL_IDS)
def test_masks_drop_tables_and_never_read_the_dropped_coefficients(torch_cuda, name, k, n):
    md = model_for(name, k)
    for K, uses in ((3, [0b1011, 0b1101]), (3, [0b0001, 0b0110, 0b1000]), (5, [0b110101, 0b001010]), (5, [0b000001, 0b111110, 0b100000, 0b010101]),
                    (16, [0x15555, 0x0AAAA])):
        tw, cw = draw(md, K, len(uses), n, seed=0x2000 + K)
        run(torch_cuda, md, tw, cw, uses, n)


@pytest.mark.parametrize("name,k,n", CASES, ids=IDS)
def test_truncated_tables_and_a_table_used_twice(torch_cuda, name, k, n):
    """n_evals of 0, 1, n - 1 and n, mixed across tables, on both kernels; poison lies behind every stored part"""
    torch = torch_cuda
    from stark_rings_amd import lincomb_dev

    md = model_for(name, k)
    w = md.w
    for K, M, ne in ((4, 1, [0, 1, n - 1, n]), (3, 2, [n - 1, 0, 1]), (5, 2, [n, 0, 1, n - 1, 1]), (2, 1, [0, 0])):
        tw, cw = draw(md, K, M, n, ne, seed=0x3000 + K)
        run(torch, md, tw, cw, [LC.full_mask(K)] * M, n)
    # the same tensor as tables 0 and 2, with different stored lengths
    tw, cw = draw(md, 3, 1, n, seed=0x3100)
    tw[2] = tw[0][:(n - 1) * w]
    want = expected(md, tw, cw, [0b1111], n)
    t0, t1 = dev(torch, tw[0]), dev(torch, tw[1])
    out = torch.full((n * w + w,), i64(GUARD), dtype=torch.int64, device="cuda")
    lincomb_dev(md.ring, [out[:n * w]], [t0, t1, t0], dev(torch, cw), [0b1111], n, [n, n, n - 1])
    torch.cuda.synchronize()
    assert np.array_equal(host(out)[:n * w], want[0]) and (host(out)[n * w:] == np.uint64(GUARD)).all()


@pytest.mark.parametrize("name,k,n", SMALL, ids=SMALL_IDS)
def test_the_worst_case_of_the_lazy_sums_and_all_zero_coefficients(torch_cuda, name, k, n):
    """every word p - 1 in sixteen tables, seventeen coefficients: the largest sum a lazy accumulator of this call can hold"""
    md = model_for(name, k)
    n = min(n, 5)
    top = md.const(md.p - 1, 1)
    for K, M in ((16, 1), (16, LC.OUTPUTS[md.ring.ring][1]), (4, max(LC.OUTPUTS[md.ring.ring][0], 1))):
        tw = [np.tile(top, n) for _ in range(K)]
        run(torch_cuda, md, tw, np.tile(top, M * (K + 1)), [LC.full_mask(K)] * M, n)
        want = run(torch_cuda, md, tw, np.zeros(M * (K + 1) * md.w, dtype=np.uint64), [LC.full_mask(K)] * M, n)
        assert not any(x.any() for x in want)


@pytest.mark.parametrize("name,k,n", SMALL, ids=SMALL_IDS)
def test_every_buffer_off_by_eight_bytes_takes_the_one_coefficient_path(torch_cuda, name, k, n):
    md = model_for(name, k)
    for K, M in ((3, 2), (5, 1), (5, 3)):
        tw, cw = draw(md, K, M, n, [n] * (K - 1) + [n - 1], seed=0x4000 + K)
        want = run(torch_cuda, md, tw, cw, [LC.full_mask(K)] * M, n, shift=0)
        run(torch_cuda, md, tw, cw, [LC.full_mask(K)] * M, n, shift=1, want=want)


@pytest.mark.parametrize("name,k,n", CASES, ids=IDS)
def test_in_place_on_the_first_and_on_the_last_table(torch_cuda, name, k, n):
    torch = torch_cuda
    from stark_rings_amd import lincomb_dev

    md = model_for(name, k)
    w = md.w
    for K in (3, 5):
        tw, cw = draw(md, K, 1, n, seed=0x5000 + K)
        want = expected(md, tw, cw, [LC.full_mask(K)], n)
        for which in (0, K - 1):
            tabs = [torch.cat([dev(torch, t), torch.full((w,), i64(GUARD), dtype=torch.int64, device="cuda")]) for t in tw]
            views = [t[:n * w] for t in tabs]
            lincomb_dev(md.ring, [views[which]], views, dev(torch, cw), None, n)
            torch.cuda.synchronize()
            for j in range(K):
                got = host(tabs[j])
                assert np.array_equal(got[:n * w], want[0] if j == which else tw[j]), (name, K, which, j)
                assert (got[n * w:] == np.uint64(GUARD)).all()


def test_refused_overlaps_leave_the_outputs_unchanged(torch_cuda):
    torch = torch_cuda
    from stark_rings_amd import RingError, lincomb_dev

    md = model_for("goldilocks", 6)
    ring, w, n = md.ring, md.w, 8
    tw, cw = draw(md, 2, 2, n, seed=0x6000)
    t0, t1 = dev(torch, tw[0]), dev(torch, tw[1])
    coef = torch.cat([dev(torch, cw), torch.full((n * w,), i64(GUARD), dtype=torch.int64, device="cuda")])
    c = coef[:cw.size]
    big = torch.full((3 * n * w,), i64(GUARD), dtype=torch.int64, device="cuda")
    a, b = big[:n * w], big[2 * n * w:]
    keep = [t.clone() for t in (t0, t1, coef, big)]
    for outs, tables, msg in (([t0, a], [t0, t1], "in place needs n_outputs == 1"),
                              ([a, big[w:w + n * w]], [t0, t1], "two outputs overlap"),
                              ([a, a], [t0, t1], "two outputs overlap"),
                              ([a, coef[w:w + n * w]], [t0, t1], "an output overlaps the coefficients"),
                              ([a, b], [t0, big[w:w + n * w]], "an output overlaps a table")):
        with pytest.raises(RingError, match=msg):
            lincomb_dev(ring, outs, tables, c, None, n)
    with pytest.raises(RingError, match="an output overlaps a table"):   # one output, but not the same base pointer
        lincomb_dev(ring, [big[w:w + n * w]], [a, t1], c[:3 * w], None, n)
    torch.cuda.synchronize()
    for t, was in zip((t0, t1, coef, big), keep):
        assert torch.equal(t, was)
    # n = 0 succeeds and writes nothing
    lincomb_dev(ring, [a], [t0, t1], c[:3 * w], None, 0)
    torch.cuda.synchronize()
    assert torch.equal(big, keep[3])


def scalar_elem(md, c):
    """the ring element c * one() as memory words"""
    if md.pow2:
        return md.words([np.array([c % md.p] * md.ring.degree, dtype=object)])
    return ((md.one().astype(object) * c) % md.p).astype(np.uint64)


@pytest.mark.parametrize("name,k,n", CASES, ids=IDS)
def test_the_composition_from_the_existing_calls_is_the_same_bit_for_bit(torch_cuda, name, k, n):
    """copy, sr_mul_elem_batch_dev, sr_mul_elem_add_batch_dev per further table, sr_add_scalar_batch_dev: the constant is a base-field
    scalar times one(), which is what that call adds"""
    torch = torch_cuda
    from stark_rings_amd import lincomb_dev

    md = model_for(name, k)
    ring, w, K = md.ring, md.w, 4
    tw, cw = draw(md, K, 1, n, seed=0x7000)
    scalar = O.fill_uniform(md.F, 0x7001, 0, 1)
    const = torch.zeros(w, dtype=torch.int64, device="cuda")
    ring.add_scalar_dev(const, scalar, True)
    tabs = [dev(torch, t) for t in tw]
    coef = torch.cat([dev(torch, cw)[:K * w], const])
    comp = tabs[0].clone()
    ring.mul_elem_dev(comp, coef[:w])
    for j in range(1, K):
        ring.mul_elem_add_dev(comp, tabs[j], coef[j * w:(j + 1) * w])
    ring.add_scalar_dev(comp, scalar, True)
    out = torch.empty_like(comp)
    lincomb_dev(ring, [out], tabs, coef, None, n)
    torch.cuda.synchronize()
    assert torch.equal(out, comp), name


@pytest.mark.parametrize("name,k,n", [("goldilocks", 6, 37), ("frog16", 0, 70)], ids=["goldilocks", "frog16"])
def test_a_non_default_stream(torch_cuda, name, k, n):
    md = model_for(name, k)
    tw, cw = draw(md, 3, 2, n, seed=0x8000)
    run(torch_cuda, md, tw, cw, [0b1011, 0b1101], n, stream=torch_cuda.cuda.Stream())


@pytest.mark.parametrize("name,k,n", [("babybear", 5, 37), ("goldilocks24", 0, 70)], ids=["babybear", "goldilocks24"])
def test_the_host_pointer_form(torch_cuda, name, k, n):
    from stark_rings_amd import RingError
    from stark_rings_amd.lincomb import lincomb

    md = model_for(name, k)
    for K, M, ne in ((3, 2, None), (5, 3, [n, 0, 1, n - 1, n]), (16, 1, None)):
        tw, cw = draw(md, K, M, n, ne, seed=0x9000 + K)
        uses = [LC.full_mask(K)] * M
        got = lincomb(md.ring, tw, cw, uses, n, n_evals=ne)
        for g, want in zip(got, expected(md, tw, cw, uses, n)):
            assert np.array_equal(g, want), (name, K, M)
    tw, cw = draw(md, 2, 1, n, seed=0x9100)
    for bad, msg in ((dict(uses=[0]), "empty mask"), (dict(uses=[0b1000]), "mask bit above"), (dict(uses=[0b101]), "no output uses"),
                     (dict(uses=[0b111], n_evals=[n + 1, n]), "exceeds n")):
        with pytest.raises(RingError, match=msg):
            lincomb(md.ring, tw, cw, n=n, **bad)
    assert lincomb(md.ring, tw, cw, [0b111], 0)[0].size == 0


def test_the_pinned_vectors_on_the_device(torch_cuda):
    for c in KATS:
        name = c["ring"]
        md = model_for(name, c["log2_degree"])
        to_words = (lambda e: md.words([np.array(e, dtype=object)])) if c["form"] == "standard" else (lambda e: np.array(e, dtype=np.uint64))
        cat = lambda els: np.concatenate([to_words(e) for e in els]) if els else np.zeros(0, dtype=np.uint64)  # noqa: E731
        for key, s in c.items():
            if not isinstance(s, dict):
                continue
            tw = [cat(t) for t in s["tables"]]
            cw = cat([e for row in s["coef"] for e in row])
            run(torch_cuda, md, tw, cw, s["uses"], s["n"], want=[cat(o) for o in s["outs"]])


@pytest.mark.parametrize("name,k", CHECKS, ids=CHECK_IDS)
def test_linear_combination_of_the_class(torch_cuda, name, k):
    """against add_assign_scaled chained on a zero table; truncated inputs and a constant against the model; out one of the inputs"""
    torch = torch_cuda
    from stark_rings_amd import DenseMultilinearExtension as MLE

    md = model_for(name, k)
    ring, w, nv = md.ring, md.w, 3
    full = 1 << nv
    tw, cw = draw(md, 3, 1, full, seed=0xA000)
    coeffs = [dev(torch, cw[j * w:(j + 1) * w]) for j in range(3)]
    mles = [MLE(ring, nv, dev(torch, t)) for t in tw]
    acc = MLE(ring, nv, torch.zeros(full * w, dtype=torch.int64, device="cuda"))
    for c, m in zip(coeffs, mles):
        acc.add_assign_scaled(c, m)
    got = MLE.linear_combination(mles, coeffs)
    torch.cuda.synchronize()
    assert torch.equal(got.evaluations, acc.evaluations) and got.num_vars == nv
    got = MLE.linear_combination(mles, dev(torch, cw[:3 * w]))   # one tensor of K coefficients
    assert torch.equal(got.evaluations, acc.evaluations)
    # truncated inputs: the result stores the longest; with a constant, all 2^num_vars
    ne = [5, 0, 3]
    short = [MLE(ring, nv, dev(torch, t[:e * w])) for t, e in zip(tw, ne)]
    got = MLE.linear_combination(short, coeffs)
    want = expected(md, [t[:e * w] for t, e in zip(tw, ne)], cw, [0b0111], 5)
    assert len(got) == 5 and np.array_equal(host(got.evaluations), want[0])
    const = dev(torch, cw[3 * w:4 * w])
    got = MLE.linear_combination(short, coeffs, const)
    want = expected(md, [t[:e * w] for t, e in zip(tw, ne)], cw, [0b1111], full)
    assert len(got) == full and np.array_equal(host(got.evaluations), want[0])
    # in place: out is the last input
    back = MLE.linear_combination(mles, coeffs, const, out=mles[2])
    want = expected(md, tw, cw, [0b1111], full)
    assert back is mles[2] and np.array_equal(host(mles[2].evaluations), want[0])
    assert np.array_equal(host(mles[0].evaluations), tw[0])


def _explicit_messages_agree(torch, md, tree, layer, claim_of):
    """the layer claim (an EqSumCheck) sends, round for round, the messages of the explicit prover: the same VirtualPolynomial with
    the table eq(z, .) multiplied in, round_evals and fold_round_evals"""
    from stark_rings_amd import DenseMultilinearExtension as MLE, VirtualPolynomial
    from test_sumcheck_fold_gpu import challenge

    ring = md.ring
    nv = tree.num_vars - layer
    z = dev(torch, md.uniform(0xB2E0, nv))
    prover = claim_of(z)
    e = VirtualPolynomial(ring, nv).add_mle_list(list(tree.halves(layer))).mul_by_mle(MLE.eq(ring, z))
    msg = e.round_evals(1)
    for j in range(nv):
        assert torch.equal(prover.message(), msg), (md.name, j)
        r = challenge(torch, md, 0xB100 + j)
        prover.next(r)
        if j + 1 < nv:
            msg, e = e.fold_round_evals(r, 1)


@pytest.mark.parametrize("name,k", CHECKS, ids=CHECK_IDS)
def test_permutation_check(torch_cuda, name, k):
    """three wire columns of 2^5 rows; sigma permutes the 96 positions inside classes of equal wire value; the leaves of every column
    come from one call into slices of the two leaf tensors, whose tail is one()"""
    torch = torch_cuda
    from stark_rings_amd import PermutationCheck, permutation_leaves

    md = model_for(name, k)
    ring, w = md.ring, md.w
    rows, cols, nv = 32, 3, 7
    total = rows * cols
    rng = np.random.RandomState(0xBEEF)
    classes = rng.randint(0, 12, total)
    perm = np.arange(total)
    for c in range(12):
        members = np.flatnonzero(classes == c)
        perm[members] = np.roll(members, -1)
    assert (np.sort(perm) == np.arange(total)).all() and (perm != np.arange(total)).any()
    values = md.uniform(0xC000, 12).reshape(12, w)
    ident = md.uniform(0xC001, total).reshape(total, w)
    f = values[classes]
    beta, gamma = dev(torch, md.uniform(0xC002, 1)), dev(torch, md.uniform(0xC003, 1))

    def check(sigma):
        num = dev(torch, np.tile(md.one(), 1 << nv))
        den = num.clone()
        for c in range(cols):
            s = slice(c * rows * w, (c + 1) * rows * w)
            part = slice(c * rows, (c + 1) * rows)
            permutation_leaves(ring, dev(torch, f[part].reshape(-1)), dev(torch, ident[part].reshape(-1)), dev(torch, sigma[part].reshape(-1)),
                               beta, gamma, num=num[s], den=den[s])
        return PermutationCheck(ring, num, den, nv), num, den

    pc, num, den = check(ident[perm])
    assert pc.holds()
    # the leaves against the model, column 1
    b, g = md.elems(host(beta))[0], md.elems(host(gamma))[0]
    part = slice(rows, 2 * rows)
    one = md.elems(md.one())[0]
    want = LC.permutation_leaves(md.elems(f[part].reshape(-1)), md.elems(ident[part].reshape(-1)), md.elems(ident[perm][part].reshape(-1)), b, g,
                                 one, md.zero(), md.add, md.mul)
    assert np.array_equal(host(num)[rows * w:2 * rows * w], md.words(want[0])) and np.array_equal(host(den)[rows * w:2 * rows * w], md.words(want[1]))
    assert np.array_equal(host(num)[total * w:], np.tile(md.one(), (1 << nv) - total))
    a, bb = pc.roots()
    assert torch.equal(a, bb) and torch.equal(a, pc.num.root())
    for side in (0, 1):
        tree = pc.num if side == 0 else pc.den
        _explicit_messages_agree(torch, md, tree, 1, lambda z: pc.layer_claim(side, 1, z))
    bad = ident[perm].copy()
    bad[17] = ident[(perm[17] + 1) % total]
    assert not check(bad)[0].holds()


@pytest.mark.parametrize("name,k", CHECKS, ids=CHECK_IDS)
def test_lookup_check(torch_cuda, name, k):
    """2^6 witness rows drawn from a 2^4-row table of two columns; denominators beta - (c_0 + gamma c_1) from fingerprint(); true
    multiplicities as ring elements.  Also with beta equal to a table fingerprint, where a denominator is zero and no inverse exists."""
    torch = torch_cuda
    from stark_rings_amd import LookupCheck, fingerprint

    md = model_for(name, k)
    ring, w = md.ring, md.w
    rng = np.random.RandomState(0xF00D)
    cols = [md.uniform(0xD000 + j, 16).reshape(16, w) for j in range(2)]
    picks = rng.randint(0, 16, 64)
    mults = np.bincount(picks, minlength=16)
    zero, one = md.zero(), md.elems(md.one())[0]
    gamma = md.elems(md.uniform(0xD010, 1))[0]
    coeffs = dev(torch, md.words([md.sub(zero, one), md.sub(zero, gamma)]))
    used = int(np.flatnonzero(mults)[0])
    t_els = [md.elems(c.reshape(-1)) for c in cols]
    at_row = md.words([md.add(t_els[0][used], md.mul(gamma, t_els[1][used]))])

    def check(beta_words, mults):
        beta = dev(torch, beta_words)
        q_t = fingerprint(ring, [dev(torch, c.reshape(-1)) for c in cols], coeffs, beta)
        q_w = fingerprint(ring, [dev(torch, c[picks].reshape(-1)) for c in cols], coeffs, beta)
        m = dev(torch, np.concatenate([scalar_elem(md, int(c)) for c in mults]))
        return LookupCheck(ring, q_w, q_t, m, 6, 4), q_t

    lc, q_t = check(md.uniform(0xD020, 1), mults)
    assert lc.holds()
    want = expected(md, [c.reshape(-1) for c in cols], np.concatenate([host(coeffs), md.uniform(0xD020, 1)]), [0b111], 16)
    assert np.array_equal(host(q_t), want[0])
    claim = lc.layer_claim(1, 1, dev(torch, md.uniform(0xD030, 3)), dev(torch, md.uniform(0xD031, 1)))
    assert claim.message().numel() > 0
    lc, q_t = check(at_row, mults)   # a zero denominator
    assert not host(q_t)[used * w:(used + 1) * w].any()
    assert lc.holds()
    off = mults.copy()
    off[used] += 1
    assert not check(md.uniform(0xD020, 1), off)[0].holds()
