"""GPU parity of the fused fold-and-round call (sr_mle_round_fold_evals[_dev]) for all six ring ids.  Every comparison is bit-exact.
Expected values come from tools/model_sumcheck_fold.py (model_mle.fold of every table, then model_sumcheck.round_evals of the folded
tables; pinned by tests/test_sumcheck_fold_host.py) and from the two device calls that the fused call merges: sr_mle_fix_variables_dev
per table, then sr_mle_round_evals_dev."""
import ctypes
import json
import os
import random
import sys

import numpy as np
import pytest

import oracle_lib as O
from test_mle_gpu import POISON, dev, fold_dev, host, model_for, ring_for
from test_sumcheck_gpu import _interp, columns, elems_for, round_dev, tables_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import model_sumcheck_fold as SF  # noqa: E402

pytestmark = pytest.mark.gpu
LEADING, TRAILING = 0, 1
ORDERS = (LEADING, TRAILING)
# (ring, log2 D, num_vars) of test_sumcheck_gpu.CASES; the fused plan of num_vars is the round plan of num_vars - 1, so num_vars of
# babybear-5 grows by two and that of stark-4, goldilocks24, babybear72 and frog16 by one: the minimum at which their records split
# (a workgroup of 256 lanes is one record and a lane takes at least 16 pairs).  goldilocks-6 still splits at 10; the short tables are
# the single launches.  The largest table (babybear72, 2^12 elements) is 2.25 MiB.
CASES = [("goldilocks", 6, 10), ("goldilocks", 16, 4), ("babybear", 5, 11), ("stark", 4, 11), ("stark", 12, 3),
         ("goldilocks24", 0, 12), ("babybear72", 0, 12), ("frog16", 0, 13), ("goldilocks24", 0, 3), ("babybear72", 0, 3), ("frog16", 0, 3)]
IDS = ["%s-%d-nv%d" % c for c in CASES]
FAMILY = {"goldilocks": "one-limb", "babybear": "one-limb"}  # every other ring is a family of its own
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "sumcheck_fold_kats.json")))
POISON_I64 = POISON - (1 << 64)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def fold_round_dev(torch, ring, tables, nv, r, order, outs=None, stream=None, work_fill=0x3C3C3C3C3C3C3C3C):
    """the _dev call with a workspace of exactly the planned size.  Without `outs` every folded table goes to the head of a poisoned
    buffer with two elements of poison behind it.  Returns (message, folded tables cut to what was written, whole output buffers)."""
    w, d = ring.words_per_elem, len(tables)
    out = torch.full(((d + 1) * w,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    want = [SF.folded_len(t.numel() // w, nv, order) for t in tables]
    if outs is None:
        bufs = [torch.full(((n + 2) * w,), POISON_I64, dtype=torch.int64, device="cuda") for n in want]
        outs = [b[:n * w] for b, n in zip(bufs, want)]
    else:
        bufs = outs
    work_elems, _ = ring.mle_round_fold_plan(nv, d, order)
    work = torch.full((work_elems * w,), work_fill, dtype=torch.int64, device="cuda") if work_elems else None
    n_out = ring.mle_round_fold_evals_dev(out, outs, tables, nv, r, order, work, stream=stream)
    assert n_out == want, (n_out, want)
    return out, [b[:n * w] for b, n in zip(bufs, n_out)], bufs


def two_calls(torch, ring, tables, nv, r, order):
    """the same round from the two calls that were there before: (message, whole folded tables of 2^(nv-1) elements)"""
    folded = [fold_dev(torch, ring, t, nv, r, order)[0] for t in tables]
    return round_dev(torch, ring, folded, nv - 1, order), folded


def same_as_two_calls(torch, ring, tables, nv, r, order, **kw):
    """every word of every folded table and of the message; the poison behind the folded tables is still there"""
    w = ring.words_per_elem
    msg, got, bufs = fold_round_dev(torch, ring, tables, nv, r, order, **kw)
    want_msg, want = two_calls(torch, ring, tables, nv, r, order)
    ok = torch.equal(msg, want_msg)
    for g, b, f in zip(got, bufs, want):
        ok = ok and torch.equal(g, f[:g.numel()]) and not bool(f[g.numel():].any())
        ok = ok and (b is g or bool((b[g.numel():] == POISON_I64).all()))
    return ok


def challenge(torch, m, seed):
    return dev(torch, m.uniform(seed, 1))


_model = {}


def model_fold_round(m, name, k, nv, d, order, r_words):
    """(folded tables, message) of the first d shared tables as model elements, computed once; on the columns() subset where that
    rule applies"""
    key = (name, k, nv, d, order)
    if key not in _model:
        cols = columns(m, max(d, 2), order)  # the subset for every d, the folded tables of d = 1 included
        els, r = elems_for(name, k, nv)[:d], m.elems(r_words)[0]
        if cols is None:
            zero, one = m.zero(), m.elems(m.one())[0]
        else:
            els, r = [[e[cols] for e in f] for f in els], r[cols]
            zero, one = np.array([0] * cols.size, dtype=object), np.array([1] * cols.size, dtype=object)
        _model[key] = (cols, SF.fold_round(els, nv, r, order, zero, one, m.add, m.sub, m.mul))
    return _model[key]


def elems_agree(m, got_words, want, cols):
    got = m.elems(got_words)
    if cols is None:
        return len(got) == len(want) and all(np.array_equal(g, x) for g, x in zip(got, want))
    return len(got) == len(want) and all(np.array_equal(g[cols], x) for g, x in zip(got, want))


def test_the_cases_reach_the_single_launch_and_the_split_path():
    seen = {}
    for name, k, nv in CASES:
        ring = ring_for(name, k)
        for d in (1, 2, 3, 4):
            for order in ORDERS:
                work, launches = ring.mle_round_fold_plan(nv, d, order)
                assert (work == 0) == (launches == 1)
                # the smallest table is one record: more than one launch there means that the points alone force the workspace
                # (two records by convention), so only a plan whose smallest form is a single launch shows a split of the pairs
                forced = ring.mle_round_fold_plan(2, d, order)[1] > 1
                fam = seen.setdefault(FAMILY.get(name, name), set())
                fam.add("single" if launches == 1 else "split" if forced else "records")
                if not forced and launches > 1:
                    assert launches == 2 and work >= 2 * (d + 1)
    for f in ("one-limb", "stark", "goldilocks24", "babybear72", "frog16"):
        assert {"single", "records"} <= seen[f], seen


@pytest.mark.parametrize("d", [1, 2, 3, 4])
@pytest.mark.parametrize("name,k,nv", CASES, ids=IDS)
def test_full_tables_match_the_model_in_both_orders(torch_cuda, name, k, nv, d):
    torch = torch_cuda
    m, ring = model_for(name, k), ring_for(name, k)
    dt = [dev(torch, t) for t in tables_for(name, k, nv)[:d]]
    r_words = m.uniform(0xF01D, 1)
    for order in ORDERS:
        msg, got, _ = fold_round_dev(torch, ring, dt, nv, dev(torch, r_words), order)
        cols, (folded, message) = model_fold_round(m, name, k, nv, d, order, r_words)
        assert elems_agree(m, host(msg), message, cols), (name, k, nv, d, order)
        for g, f in zip(got, folded):
            assert elems_agree(m, host(g), f, cols), (name, k, nv, d, order)


def test_the_pinned_vectors_on_the_device(torch_cuda):
    torch = torch_cuda
    for case in KATS["cases"]:
        ring = ring_for(case["ring"], case["log2_degree"])
        F = O.FIELD_ID[case["ring"]]
        nv = case["num_vars"]
        dt = [dev(torch, O.to_mont(F, [x for e in f for x in e])) for f in case["tables"]]
        r = dev(torch, O.to_mont(F, case["r"]))
        for key, order in (("leading", LEADING), ("trailing", TRAILING)):
            msg, got, _ = fold_round_dev(torch, ring, dt, nv, r, order)
            assert [int(x) for x in O.from_mont(F, host(msg))] == [x for e in case[key]["message"] for x in e], (case["ring"], len(dt), key)
            for g, f in zip(got, case[key]["folded"]):
                assert [int(x) for x in O.from_mont(F, host(g))] == [x for e in f for x in e], (case["ring"], len(dt), key)


@pytest.mark.parametrize("name,k,nv", CASES[:8], ids=IDS[:8])
def test_full_and_truncated_tables_agree_with_the_two_device_calls(torch_cuda, name, k, nv):
    """residues 1, 2, 3 mod 4; just below and above the quarter, the half and the three-quarter marks; one element; an empty table
    among stored ones; every table empty; tables of different lengths in one call (a fold loop that stopped at the shortest table would
    leave the longer ones unfolded)"""
    torch = torch_cuda
    m, ring = model_for(name, k), ring_for(name, k)
    w, full = ring.words_per_elem, 1 << nv
    half, q = full // 2, full // 4
    tabs = [dev(torch, t) for t in tables_for(name, k, nv)]
    r = challenge(torch, m, 0xC4A1)
    all_sizes = [(full,), (full, full), (full, full, full), (full, full, full, full), (full - 1, 5), (q - 1, q + 1, full),
                 (half - 1, half + 1, 3 * q + 1, 3 * q - 1), (1, full, full - 2, half + 2), (full - 3, 1), (1,), (full, 0, full - 3), (0, full),
                 (0,), (0, 0, 0)]
    for sizes in all_sizes:
        cut = [tabs[j][:n * w] for j, n in enumerate(sizes)]
        for order in ORDERS:
            assert same_as_two_calls(torch, ring, cut, nv, r, order), (name, sizes, order)


@pytest.mark.parametrize("name,k", [("goldilocks", 6), ("goldilocks", 0), ("babybear", 5), ("stark", 4), ("goldilocks24", 0), ("babybear72", 0),
                                    ("frog16", 0)])
def test_two_variables_are_the_minimum(torch_cuda, name, k):
    torch = torch_cuda
    m, ring = model_for(name, k), ring_for(name, k)
    w = ring.words_per_elem
    tabs = [dev(torch, m.uniform(0x2200 + j, 4)) for j in range(4)]
    r = challenge(torch, m, 0x2222)
    for sizes in ((4,), (4, 4), (3, 1), (2, 4, 1), (4, 4, 4, 3), (0, 4), (0,)):
        cut = [tabs[j][:n * w] for j, n in enumerate(sizes)]
        for order in ORDERS:
            assert same_as_two_calls(torch, ring, cut, 2, r, order), (name, sizes, order)
    r_words = host(r)
    els = [m.elems(host(t)) for t in tabs[:2]]
    for order in ORDERS:
        msg, got, _ = fold_round_dev(torch, ring, tabs[:2], 2, r, order)
        folded, message = SF.fold_round(els, 2, m.elems(r_words)[0], order, m.zero(), m.elems(m.one())[0], m.add, m.sub, m.mul)
        assert elems_agree(m, host(msg), message, None) and all(elems_agree(m, host(g), f, None) for g, f in zip(got, folded))


@pytest.mark.parametrize("name,k,nv", CASES[:8], ids=IDS[:8])
def test_trailing_order_folds_in_place_and_a_table_may_appear_twice(torch_cuda, name, k, nv):
    torch = torch_cuda
    m, ring = model_for(name, k), ring_for(name, k)
    w, full = ring.words_per_elem, 1 << nv
    r = challenge(torch, m, 0x1A1A)
    sizes = (full, full - 3, full // 2 + 1)
    src = [dev(torch, t[:n * w]) for t, n in zip(tables_for(name, k, nv), sizes)]
    want_msg, want, _ = fold_round_dev(torch, ring, src, nv, r, TRAILING)
    work = [t.clone() for t in src]
    msg, got, _ = fold_round_dev(torch, ring, work, nv, r, TRAILING, outs=work)
    assert torch.equal(msg, want_msg)
    for g, x, t, s in zip(got, want, work, src):
        assert torch.equal(g, x)
        assert torch.equal(t[g.numel():], s[g.numel():])  # nothing beyond the folded table is touched
    # f * f out of place: both outputs are the folded f, the message is that of the two calls
    for order in ORDERS:
        assert same_as_two_calls(torch, ring, [src[0], src[0]], nv, r, order), (name, order)
        assert same_as_two_calls(torch, ring, [src[1], src[0], src[1]], nv, r, order), (name, order)


# The last two sit on the boundaries of the launch geometry (test_sumcheck_gpu.py: OFF_BY_EIGHT), one variable up because the plan is
# that of the round that follows the fold.
@pytest.mark.parametrize("name,k,nv", [("goldilocks", 6, 10), ("babybear", 5, 11), ("goldilocks", 8, 8), ("babybear", 9, 7)])
def test_tables_off_by_eight_bytes_take_the_one_coefficient_path_to_the_same_result(torch_cuda, name, k, nv):
    torch = torch_cuda
    m, ring = model_for(name, k), ring_for(name, k)
    w, full = ring.words_per_elem, 1 << nv
    assert all(ring.mle_round_fold_plan(nv, 3, order)[0] > 0 for order in ORDERS)  # several records: the geometry decides where they go
    sizes = (full, full - 3, full // 2 + 1)
    tabs = [t[:n * w] for t, n in zip(tables_for(name, k, nv), sizes)]
    aligned = [dev(torch, t) for t in tabs]
    r = challenge(torch, m, 0x0FF8)

    def shift(t):
        buf = torch.full((t.numel() + 1,), POISON_I64, dtype=torch.int64, device="cuda")
        buf[1:] = t
        assert buf[1:].data_ptr() % 16 == 8
        return buf[1:]

    shifted = [shift(t) for t in aligned]
    for order in ORDERS:
        want_msg, want, _ = fold_round_dev(torch, ring, aligned, nv, r, order)
        for tables, outs_shifted, rr in ((shifted, False, r), ([aligned[0], shifted[1], aligned[2]], False, r), (aligned, True, r),
                                         (aligned, False, shift(r))):
            outs = None
            if outs_shifted:
                outs = [shift(torch.full((x.numel() + 2 * w,), POISON_I64, dtype=torch.int64, device="cuda")) for x in want]
            msg, got, bufs = fold_round_dev(torch, ring, tables, nv, rr, order, outs=outs)
            assert torch.equal(msg, want_msg), (name, order)
            for g, x, b in zip(got, want, bufs):
                assert torch.equal(g, x), (name, order)
                assert bool((b[g.numel():] == POISON_I64).all())


@pytest.mark.parametrize("name,k,nv", [("goldilocks", 6, 10), ("stark", 4, 11), ("babybear72", 0, 12)])
def test_capture_on_a_fresh_context_and_replay_after_the_tables_and_r_change(torch_cuda, name, k, nv):
    torch = torch_cuda
    from stark_rings_amd import CyclotomicRing

    m = model_for(name, k)
    ring = CyclotomicRing(name, k, device=0)  # fresh: nothing has run on it, so nothing is warm
    try:
        w, d, order = ring.words_per_elem, 3, LEADING
        first = tables_for(name, k, nv)[:d]
        second = [m.uniform(0x9900 + j, 1 << nv) for j in range(d)]
        tabs = [dev(torch, t) for t in first]
        r = challenge(torch, m, 0x6001)
        out = torch.empty((d + 1) * w, dtype=torch.int64, device="cuda")
        outs = [torch.empty(w << (nv - 1), dtype=torch.int64, device="cuda") for _ in range(d)]
        work_elems, launches = ring.mle_round_fold_plan(nv, d, order)
        assert work_elems and launches >= 2
        work = torch.full((work_elems * w,), POISON_I64, dtype=torch.int64, device="cuda")
        side = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            ring.mle_round_fold_evals_dev(out, outs, tabs, nv, r, order, work, stream=side)
        graph.replay()
        torch.cuda.synchronize()
        want_msg, want = two_calls(torch, ring_for(name, k), tabs, nv, r, order)
        assert torch.equal(out, want_msg) and all(torch.equal(a, b) for a, b in zip(outs, want))
        for t, new in zip(tabs, second):
            t.copy_(dev(torch, new))
        r.copy_(challenge(torch, m, 0x6002))
        work.fill_(0x1111111111111111)
        graph.replay()
        torch.cuda.synchronize()
        want_msg, want = two_calls(torch, ring_for(name, k), tabs, nv, r, order)
        assert torch.equal(out, want_msg) and all(torch.equal(a, b) for a, b in zip(outs, want))
    finally:
        ring.close()


def test_workspace_contents_do_not_matter(torch_cuda):
    torch = torch_cuda
    for name, k, nv in (("goldilocks", 6, 10), ("frog16", 0, 13)):
        m, ring = model_for(name, k), ring_for(name, k)
        tabs = [dev(torch, t) for t in tables_for(name, k, nv)[:2]]
        r = challenge(torch, m, 0x3003)
        a = fold_round_dev(torch, ring, tabs, nv, r, LEADING, work_fill=0)
        b = fold_round_dev(torch, ring, tabs, nv, r, LEADING, work_fill=POISON_I64)
        assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))


WHOLE = [("goldilocks", 4, 6), ("babybear", 3, 6), ("stark", 2, 5), ("goldilocks24", 0, 5), ("babybear72", 0, 4), ("frog16", 0, 5)]


@pytest.mark.parametrize("name,k,nv", WHOLE, ids=[c[0] for c in WHOLE])
@pytest.mark.parametrize("order", [LEADING, TRAILING])
def test_a_whole_prover_through_the_fused_call_equals_the_two_call_loop(torch_cuda, name, k, nv, order):
    torch = torch_cuda
    m, ring = model_for(name, k), ring_for(name, k)
    w, d = ring.words_per_elem, 3
    sizes = (1 << nv, (1 << nv) - 3, 1 << nv)
    start = [dev(torch, m.uniform(0xABC0 + j, n)) for j, n in enumerate(sizes)]
    challenges = [challenge(torch, m, 0x7000 + i) for i in range(nv)]

    def finals(tabs, r):
        return [fold_dev(torch, ring, t, 1, r, order)[0] for t in tabs]

    # the two-call loop: message, then a fold per table
    tabs, msgs_a = start, []
    for rnd in range(nv):
        left = nv - rnd
        msgs_a.append(round_dev(torch, ring, tabs, left, order))
        tabs = [fold_dev(torch, ring, t, left, challenges[rnd], order)[0] for t in tabs]
    finals_a = tabs
    # round 0 from sr_mle_round_evals_dev, rounds 1 .. nv - 1 from the fused call, the final evaluations from sr_mle_fix_variables_dev
    tabs, msgs_b = start, [round_dev(torch, ring, start, nv, order)]
    for rnd in range(1, nv):
        msg, tabs, _ = fold_round_dev(torch, ring, tabs, nv - rnd + 1, challenges[rnd - 1], order)
        msgs_b.append(msg)
    finals_b = finals(tabs, challenges[nv - 1])
    assert len(msgs_a) == len(msgs_b) == nv
    for rnd, (a, b) in enumerate(zip(msgs_a, msgs_b)):
        assert torch.equal(a, b), (name, order, rnd)
    for a, b in zip(finals_a, finals_b):
        assert torch.equal(a, b), (name, order)
    if m.pow2:  # prime-field slots: p(0) + p(1) is the previous claim, and the last claim is the product of the evaluations
        claim = m.elems(host(round_dev(torch, ring, start, nv, 2)))[0]
        for rnd, msg in enumerate(msgs_b):
            p = m.elems(host(msg))
            assert np.array_equal(m.add(p[0], p[1]), claim), (name, order, rnd)
            claim = _interp(m, host(msg), host(challenges[rnd]), d)
        final = m.elems(host(finals_b[0]))[0]
        for f in finals_b[1:]:
            final = m.mul(m.elems(host(f))[0], final)
        assert np.array_equal(final, claim)


def test_the_host_pointer_form_and_the_class_method(torch_cuda):
    torch = torch_cuda
    from stark_rings_amd import DenseMultilinearExtension as MLE, MLE_TRAILING, RingError

    for name, k, nv in (("goldilocks", 6, 10), ("stark", 4, 11), ("goldilocks24", 0, 12)):
        m, ring = model_for(name, k), ring_for(name, k)
        w, full = ring.words_per_elem, 1 << nv
        words = [t[:n * w] for t, n in zip(tables_for(name, k, nv), (full, full - 5, full // 2 + 1))]
        tabs = [dev(torch, t) for t in words]
        r_words = m.uniform(0x4004, 1)
        r = dev(torch, r_words)
        for order in ORDERS:
            want_msg, want, _ = fold_round_dev(torch, ring, tabs, nv, r, order)
            msg, folded = ring.mle_round_fold_evals(words, nv, r_words, order)
            assert np.array_equal(msg, host(want_msg))
            assert len(folded) == 3 and all(np.array_equal(f, host(x)) for f, x in zip(folded, want))
            msg, mles = MLE.fold_round_evals([MLE(ring, nv, t) for t in tabs], r, order)
            assert torch.equal(msg, want_msg)
            assert all(g.num_vars == nv - 1 and torch.equal(g.evaluations, x) for g, x in zip(mles, want))
        with pytest.raises(RingError):
            MLE.fold_round_evals([MLE(ring, 1, tabs[0][:2 * w])], r)
        with pytest.raises(RingError):
            MLE.fold_round_evals([], r)
        with pytest.raises(RingError):
            MLE.fold_round_evals([MLE(ring, nv, tabs[0])], r, MLE_TRAILING + 1)


def test_every_refusal_names_its_reason_and_launches_nothing(torch_cuda):
    torch = torch_cuda
    from stark_rings_amd import _lib

    ring = ring_for("goldilocks", 6)
    lib, ctx = ring._lib, ring._ctx
    nv, w = 10, ring.words_per_elem
    canary = 0x0123456789ABCDEF
    full, half = 1 << nv, 1 << (nv - 1)
    f = torch.full((w << nv,), 7, dtype=torch.int64, device="cuda")
    f2 = torch.full((w << nv,), 7, dtype=torch.int64, device="cuda")
    g = torch.full((w * half,), canary, dtype=torch.int64, device="cuda")
    g2 = torch.full((w * half,), canary, dtype=torch.int64, device="cuda")
    out = torch.full((3 * w,), canary, dtype=torch.int64, device="cuda")
    r = torch.full((8 * w,), 5, dtype=torch.int64, device="cuda")[:w]  # padded: a d_out or d_work placed on it reaches no other buffer
    need, _ = ring.mle_round_fold_plan(nv, 2, LEADING)
    assert 0 < need <= 8
    work = torch.full((need * w,), canary, dtype=torch.int64, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    n_out = (ctypes.c_size_t * 4)()

    def call(out_p, optrs, ptrs, sizes, nt, num_vars, r_p, order, work_p, work_n, no=n_out):
        oa = (ctypes.c_void_p * 4)(*optrs) if optrs is not None else None
        pa = (ctypes.c_void_p * 4)(*ptrs) if ptrs is not None else None
        sa = (ctypes.c_size_t * 4)(*sizes) if sizes is not None else None
        rc = lib.sr_mle_round_fold_evals_dev(ctx, out_p, oa, no, pa, sa, nt, num_vars, r_p, order, work_p, work_n, st)
        return rc, _lib.last_error()

    fp, f2p, gp, g2p, op, rp, wp = (t.data_ptr() for t in (f, f2, g, g2, out, r, work))
    eb = 8 * w  # bytes of an element
    ok = (op, [gp, g2p], [fp, f2p], [full, full], 2, nv, rp, LEADING, wp, need)

    def but(**kw):
        names = ("out_p", "optrs", "ptrs", "sizes", "nt", "num_vars", "r_p", "order", "work_p", "work_n")
        a = dict(zip(names, ok))
        a.update(kw)
        return a

    bad = [
        (but(out_p=None), "null pointer"), (but(optrs=None), "null pointer"), (but(ptrs=None), "null pointer"), (but(sizes=None), "null pointer"),
        (but(r_p=None), "null pointer"), (but(no=None), "null pointer"), (but(ptrs=[fp, None]), "null pointer"), (but(optrs=[gp, None]), "null pointer"),
        (but(work_p=None), "null pointer"),
        (but(nt=0), "n_tables must be 1 .. 4"), (but(nt=5), "n_tables must be 1 .. 4"),
        (but(order=2), "unknown order"), (but(order=-1), "unknown order"),
        (but(num_vars=48), "num_vars must be below 48"), (but(num_vars=1, sizes=[2, 2]), "num_vars >= 2"), (but(num_vars=0, sizes=[1, 1]), "num_vars >= 2"),
        (but(sizes=[full, full + 1]), "n_evals exceeds 2^num_vars"), (but(num_vars=47, sizes=[1 << 45, 1 << 45]), "element count too large"),
        (but(work_n=need - 1), "workspace too small"),
        (but(out_p=wp + eb), "d_out overlaps d_work"), (but(out_p=rp), "d_out overlaps d_r"), (but(work_p=rp), "d_work overlaps d_r"),
        (but(out_p=fp + eb), "d_out overlaps a table"), (but(work_p=f2p), "d_work overlaps a table"), (but(r_p=fp + 3 * eb), "d_r overlaps a table"),
        (but(out_p=gp + eb), "d_out overlaps a folded table"), (but(work_p=g2p), "d_work overlaps a folded table"),
        (but(r_p=g2p + eb), "d_r overlaps a folded table"),
        (but(optrs=[gp, gp + eb]), "two folded tables overlap"), (but(optrs=[gp, gp]), "two folded tables overlap"),
        (but(optrs=[fp, g2p]), "only a trailing-order fold may run in place"),                      # leading order in place
        (but(optrs=[fp + eb, g2p], order=TRAILING), "only a trailing-order fold may run in place"),  # in place but shifted
        (but(optrs=[f2p, g2p], order=TRAILING), "only a trailing-order fold may run in place"),     # into the other input table
        (but(optrs=[fp, g2p], ptrs=[fp, fp], order=TRAILING), "appears twice cannot be folded in place"),
    ]
    for kw, msg in bad:
        rc, err = call(**kw)
        assert rc == 1 and msg in err, (kw, rc, err)
    torch.cuda.synchronize()
    for t in (out, work, g, g2):
        assert bool((t == canary).all())
    assert bool((f == 7).all()) and bool((f2 == 7).all()) and bool((r == 5).all())
    assert list(n_out) == [0, 0, 0, 0]
    rc, err = call(*ok)
    assert rc == 0, err
    assert list(n_out)[:2] == [half, half]
    rc, err = call(**but(optrs=[fp, f2p], order=TRAILING))  # both tables in place
    assert rc == 0, err
    torch.cuda.synchronize()
