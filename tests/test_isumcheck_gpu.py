"""GPU parity of the weighted sum-check rounds with integer columns as factors (sr_vpoly_iwround_evals[_dev],
sr_vpoly_iwround_fold_evals[_dev], IndexMultilinearExtension in a VirtualPolynomial, EqSumCheck over it) for all six ring ids.  Every
comparison is bit-exact.  The oracle is the composition the header states: from_u64_dev (sr_lincomb_index_dev) expands every column
to the table R::from(col[e]), and the existing weighted calls (wround_dev / wfold_dev of tests/test_wsumcheck_gpu.py) run over the
tables and the expanded columns; the pinned vectors of tools/model_isumcheck.py stand beside it.  The shapes are CASES of
tests/test_sumcheck_fold_gpu.py: single records, split plans, elements below and above one wave (the non-uniform and the uniform column
load) and the 8-slot kernels.
"""
import ctypes
import json
import os
import random
import sys

import numpy as np
import pytest

import oracle_lib as O
from stark_rings_amd import (IndexColumn, IndexMultilinearExtension, from_u64_dev, vpoly_iwround_evals_dev, vpoly_iwround_fold_evals_dev,
                             vpoly_iwround_plan, wsumcheck)
from test_mle_gpu import POISON, dev, host, model_for, ring_for
from test_sumcheck_fold_gpu import CASES, IDS, challenge
from test_vpoly_gpu import one_of, tables_for
from test_wsumcheck_gpu import weights_for, wfold_dev, wround_dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import model_isumcheck as IS  # noqa: E402
import model_vpoly as VP  # noqa: E402
import model_vpoly_fold as VF  # noqa: E402

pytestmark = pytest.mark.gpu
LEADING, TRAILING = 0, 1
ORDERS = (LEADING, TRAILING)
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "isumcheck_kats.json")))
POISON_I64 = POISON - (1 << 64)
U64 = 1 << 64
SIX = [("goldilocks", 6), ("babybear", 5), ("stark", 4), ("goldilocks24", 0), ("babybear72", 0), ("frog16", 0)]
SPLIT = CASES[:8]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def ints_dev(torch, values):
    return torch.from_numpy(np.array([int(x) for x in values], dtype=np.uint64).view(np.int64)).cuda()


def stored(col, nv):
    return 1 << nv if col.is_progression else col.n_evals


def edge_values(p, n):
    """p - 1, p, p + 1 and 2^64 - 1 in turn (modulo 2^64 where p has more than 64 bits)"""
    return ([x % U64 for x in (p - 1, p, p + 1)] + [U64 - 1]) * (n // 4 + 1)


def columns_for(torch, name, k, nv, sname):
    """the columns of a structure: every kind of the issue in at least one structure"""
    p, full = ring_for(name, k).modulus, 1 << nv
    half = full // 2
    rng = random.Random("isumcheck gpu %s %d %d %s" % (name, k, nv, sname))
    uniform = lambda n: ints_dev(torch, [rng.randrange(U64) for _ in range(n)])  # noqa: E731
    if sname == "PLONK":
        return [IndexColumn(ints_dev(torch, [rng.randrange(2) for _ in range(full)])),
                IndexColumn(ints_dev(torch, edge_values(p, full)[:full]), n_evals=full - 1), IndexColumn(start=0),
                IndexColumn(uniform(full), n_evals=half + 1), IndexColumn(start=U64 - full)]
    if sname == "ALLCOL":
        return [IndexColumn(ints_dev(torch, edge_values(p, full)[:full])), IndexColumn(start=U64 - full)]
    if sname == "SQUARE":
        return [IndexColumn(uniform(full), n_evals=half)]
    if sname == "SHARED":
        c = IndexColumn(uniform(full))
        return [c, c]
    return [IndexColumn(ints_dev(torch, [rng.randrange(2) for _ in range(full)])), IndexColumn(uniform(full), n_evals=full - 1)]


def coeffs_for(torch, name, k, sname):
    m = model_for(name, k)
    terms = IS.STRUCTURES[sname][2]
    if sname == "MIXED":
        return None
    c = [m.uniform(0xC01F0 + j, 1) for j in range(len(terms))]
    if sname == "PLONK":
        c[3] = m.words([m.sub(m.zero(), one_of(m))])
    return dev(torch, np.concatenate(c))


def expanded(torch, ring, cols, nv):
    """the tables the columns stand for: from_u64_dev over the stored part (a column that stores nothing: the empty table)"""
    like = torch.empty(0, dtype=torch.int64, device="cuda")
    return [from_u64_dev(ring, c, stored(c, nv), like=like) if stored(c, nv) else like.clone() for c in cols]


def iwround(torch, ring, weights, tables, cols, terms, coeffs, nv, order, stream=None, work_fill=0x3C3C3C3C3C3C3C3C):
    """the _dev call with a workspace of exactly the planned size, pre-filled with a pattern; two elements of poison behind the message"""
    w, d = ring.words_per_elem, VP.degree(terms)
    buf = torch.full(((d + 3) * w,), POISON_I64, dtype=torch.int64, device="cuda")
    work_elems, _ = vpoly_iwround_plan(ring, nv, len(tables), len(cols), len(terms), d, order)
    work = torch.full((work_elems * w,), work_fill, dtype=torch.int64, device="cuda") if work_elems else None
    vpoly_iwround_evals_dev(ring, buf[:(d + 1) * w], weights, tables, cols, terms, coeffs, nv, order, work, stream=stream)
    assert bool((buf[(d + 1) * w:] == POISON_I64).all())
    return buf[:(d + 1) * w]


def iwfold(torch, ring, weights, tables, cols, terms, coeffs, nv, r, order, outs=None, stream=None, work_fill=0x3C3C3C3C3C3C3C3C):
    """(message, folded slots cut to what was written, whole output buffers): two elements of poison behind every output"""
    w, d = ring.words_per_elem, VP.degree(terms)
    buf = torch.full(((d + 3) * w,), POISON_I64, dtype=torch.int64, device="cuda")
    want = [VF.folded_len(t.numel() // w, nv, order) for t in tables] + [VF.folded_len(stored(c, nv), nv, order) for c in cols]
    if outs is None:
        bufs = [torch.full(((n + 2) * w,), POISON_I64, dtype=torch.int64, device="cuda") for n in want]
        outs = [b[:n * w] for b, n in zip(bufs, want)]
    else:
        bufs = outs
    work_elems, _ = vpoly_iwround_plan(ring, nv, len(tables), len(cols), len(terms), d, order, fold=True)
    work = torch.full((work_elems * w,), work_fill, dtype=torch.int64, device="cuda") if work_elems else None
    n_out = vpoly_iwround_fold_evals_dev(ring, buf[:(d + 1) * w], outs, weights, tables, cols, terms, coeffs, nv, r, order, work, stream=stream)
    assert n_out == want, (n_out, want)
    assert bool((buf[(d + 1) * w:] == POISON_I64).all())
    return buf[:(d + 1) * w], [b[:n * w] for b, n in zip(bufs, n_out)], bufs


def both_agree(torch, ring, dw, dwf, tables, cols, terms, dc, nv, r, where, orders=ORDERS):
    """both calls against the composition: d_out, every folded slot, n_evals_out, and the poison behind every output"""
    dense = list(tables) + expanded(torch, ring, cols, nv)
    for order in orders:
        assert torch.equal(iwround(torch, ring, dw, tables, cols, terms, dc, nv, order), wround_dev(torch, ring, dw, dense, terms, dc, nv, order)), \
            (where, order)
        msg, got, bufs = iwfold(torch, ring, dwf, tables, cols, terms, dc, nv, r, order)
        want_msg, want, _ = wfold_dev(torch, ring, dwf, dense, terms, dc, nv, r, order)
        assert torch.equal(msg, want_msg), (where, order)
        assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want)), (where, order)
        assert all(bool((b[g.numel():] == POISON_I64).all()) for g, b in zip(got, bufs)), (where, order)


# ---- both calls against the composition -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sname", sorted(IS.STRUCTURES))
@pytest.mark.parametrize("name,k,nv", CASES, ids=IDS)
def test_both_calls_equal_the_composition_in_both_orders(torch_cuda, name, k, nv, sname):
    torch = torch_cuda
    m, ring = model_for(name, k), ring_for(name, k)
    K, J, terms = IS.STRUCTURES[sname]
    w, full = ring.words_per_elem, 1 << nv
    sizes = (full, full - 3, full // 2 + 1)
    tables = [dev(torch, t[:n * w]) for t, n in zip(tables_for(name, k, nv)[:K], sizes)]
    cols = columns_for(torch, name, k, nv, sname)
    assert len(cols) == J
    dw, dwf = dev(torch, weights_for(name, k, full // 2)), dev(torch, weights_for(name, k, full // 4))
    both_agree(torch, ring, dw, dwf, tables, cols, terms, coeffs_for(torch, name, k, sname), nv, challenge(torch, m, 0x15C0), (name, sname))


@pytest.mark.parametrize("name,k,nv", SPLIT, ids=IDS[:8])
def test_truncated_columns_of_every_length_agree_with_the_composition(torch_cuda, name, k, nv):
    """stored lengths 2^nv - 1, half + 1, half, 1 and 0, in one term only and in every term, beside a truncated table; the integers
    behind n_evals are 2^64 - 1 everywhere and would show if they were read"""
    torch = torch_cuda
    m, ring = model_for(name, k), ring_for(name, k)
    w, full = ring.words_per_elem, 1 << nv
    half = full // 2
    rng = random.Random("isumcheck truncated %s %d" % (name, nv))
    tables = [dev(torch, tables_for(name, k, nv)[0][:(full - 5) * w]), dev(torch, tables_for(name, k, nv)[1])]
    dw, dwf = dev(torch, weights_for(name, k, half)), dev(torch, weights_for(name, k, half // 2))
    r = challenge(torch, m, 0x7C01)
    terms = [[0, 2], [1, 3], [0, 1, 2]]

    def column(n):
        values = ints_dev(torch, [rng.randrange(U64) for _ in range(n)] + [U64 - 1] * (full - n))
        return IndexColumn(values, n_evals=n)

    for na, nb in ((full - 1, half + 1), (half, 1), (0, full), (1, 0), (half + 1, half)):
        both_agree(torch, ring, dw, dwf, tables, [column(na), column(nb)], terms, None, nv, r, (name, na, nb))
    both_agree(torch, ring, dw, dwf, [], [column(0), column(0)], [[0, 1]], None, nv, r, (name, "empty"))


def test_the_pinned_vectors_on_the_device(torch_cuda):
    torch = torch_cuda
    import model_wsumcheck as W

    for case in KATS["cases"]:
        ring = ring_for(case["ring"], case["log2_degree"])
        nv, terms = case["num_vars"], case["terms"]
        if case["form"] == "standard":
            F = O.FIELD_ID[case["ring"]]
            put = lambda elems: dev(torch, O.to_mont(F, [x for e in elems for x in e]))  # noqa: E731
            get = lambda t: [int(x) for x in O.from_mont(F, host(t))]  # noqa: E731
            inputs = (case["tables"], case["coeffs"], case["weights_round"], case["weights_fold"], case["r"])
        else:
            put = lambda elems: dev(torch, np.array([x for e in elems for x in e], dtype=np.uint64))  # noqa: E731
            get = lambda t: [int(x) for x in host(t)]  # noqa: E731
            m = model_for(case["ring"], 0)
            inputs = W.kat_inputs(case["ring"], case["n_evals"], len(terms), nv)
            if case["structure"] == "PLONK":
                inputs[1][3] = m.sub(m.zero(), one_of(m))
        dt = [put(f) for f in inputs[0]]
        dc, dw, dwf, r = put(inputs[1]), put(inputs[2]), put(inputs[3]), put([inputs[4]])
        cols = [IndexColumn(start=c.start) if isinstance(c, IS.Progression) else IndexColumn(ints_dev(torch, c) if c else ints_dev(torch, [0]), n_evals=len(c))
                for c in IS.kat_column_values(case)]
        for key, order in (("leading", LEADING), ("trailing", TRAILING)):
            where = (case["ring"], case["structure"], key)
            assert get(iwround(torch, ring, dw, dt, cols, terms, dc, nv, order)) == [x for e in case[key]["round"] for x in e], where
            fmsg, got, _ = iwfold(torch, ring, dwf, dt, cols, terms, dc, nv, r, order)
            assert get(fmsg) == [x for e in case[key]["fold_message"] for x in e], where
            for g, f in zip(got, case[key].get("folded", [])):
                assert get(g) == [x for e in f for x in e], where


# ---- no columns: the weighted calls -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k,nv", [CASES[0], CASES[3], CASES[5], CASES[9]], ids=[IDS[0], IDS[3], IDS[5], IDS[9]])
def test_without_columns_the_calls_are_the_weighted_calls_bit_for_bit(torch_cuda, name, k, nv):
    torch = torch_cuda
    m, ring = model_for(name, k), ring_for(name, k)
    w, full = ring.words_per_elem, 1 << nv
    tables = [dev(torch, t[:n * w]) for t, n in zip(tables_for(name, k, nv), (full, full - 3, full // 2 + 1, full))]
    dw, dwf = dev(torch, weights_for(name, k, full // 2)), dev(torch, weights_for(name, k, full // 4))
    r, dc = challenge(torch, m, 0x0C01), dev(torch, np.concatenate([m.uniform(0xC0DE + j, 1) for j in range(2)]))
    for order in ORDERS:
        assert vpoly_iwround_plan(ring, nv, 4, 0, 2, 3, order) == ring.vpoly_wround_plan(nv, 4, 2, 3, order)
        assert vpoly_iwround_plan(ring, nv, 4, 0, 2, 3, order, fold=True) == ring.vpoly_wround_fold_plan(nv, 4, 2, 3, order)
        assert torch.equal(iwround(torch, ring, dw, tables, [], VP.R1CS, dc, nv, order), wround_dev(torch, ring, dw, tables, VP.R1CS, dc, nv, order))
        a, b = iwfold(torch, ring, dwf, tables, [], VP.R1CS, dc, nv, r, order), wfold_dev(torch, ring, dwf, tables, VP.R1CS, dc, nv, r, order)
        assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))


# ---- eight bytes off ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k,nv", [("goldilocks", 6, 10), ("babybear", 5, 11)])
def test_every_ring_buffer_off_by_eight_bytes_takes_the_one_coefficient_path_to_the_same_result(torch_cuda, name, k, nv):
    torch = torch_cuda
    m, ring = model_for(name, k), ring_for(name, k)
    w, full = ring.words_per_elem, 1 << nv
    K, J, terms = IS.STRUCTURES["PLONK"]
    aligned = [dev(torch, t[:n * w]) for t, n in zip(tables_for(name, k, nv)[:K], (full, full - 3, full // 2 + 1))]
    cols = columns_for(torch, name, k, nv, "PLONK")
    r, dc = challenge(torch, m, 0x0FF8), coeffs_for(torch, name, k, "PLONK")
    dw, dwf = dev(torch, weights_for(name, k, full // 2)), dev(torch, weights_for(name, k, full // 4))

    def shift(t):
        buf = torch.full((t.numel() + 1,), POISON_I64, dtype=torch.int64, device="cuda")
        buf[1:] = t
        assert buf[1:].data_ptr() % 16 == 8
        return buf[1:]

    shifted = [shift(t) for t in aligned]
    for order in ORDERS:
        want = iwround(torch, ring, dw, aligned, cols, terms, dc, nv, order)
        want_msg, want_folded, _ = iwfold(torch, ring, dwf, aligned, cols, terms, dc, nv, r, order)
        assert torch.equal(iwround(torch, ring, shift(dw), shifted, cols, terms, shift(dc), nv, order), want), (name, order)
        outs = [shift(torch.full((x.numel() + 2 * w,), POISON_I64, dtype=torch.int64, device="cuda")) for x in want_folded]
        msg, got, bufs = iwfold(torch, ring, shift(dwf), shifted, cols, terms, shift(dc), nv, shift(r), order, outs=outs)
        assert torch.equal(msg, want_msg), (name, order)
        for g, x, b in zip(got, want_folded, bufs):
            assert torch.equal(g, x) and bool((b[g.numel():] == POISON_I64).all()), (name, order)


# ---- the workspace, the host-pointer forms, in place ------------------------------------------------------------------------------------
def test_workspace_contents_do_not_matter_and_the_host_pointer_forms_agree(torch_cuda):
    torch = torch_cuda
    for name, k, nv in (("goldilocks", 6, 10), ("stark", 4, 11), ("babybear72", 0, 3), ("frog16", 0, 13)):
        m, ring = model_for(name, k), ring_for(name, k)
        w, full = ring.words_per_elem, 1 << nv
        for sname in ("PLONK", "ALLCOL"):
            K, J, terms = IS.STRUCTURES[sname]
            words = [t[:n * w] for t, n in zip(tables_for(name, k, nv)[:K], (full, full - 5, full // 2 + 1))]
            tabs = [dev(torch, t) for t in words]
            cols = columns_for(torch, name, k, nv, sname)
            hcols = [c if c.is_progression else IndexColumn(host(c.values), n_evals=c.n_evals) for c in cols]
            dc = coeffs_for(torch, name, k, sname)
            cw = host(dc)
            ww, wf, r_words = weights_for(name, k, full // 2), weights_for(name, k, full // 4), m.uniform(0x4004, 1)
            dw, dwf, r = dev(torch, ww), dev(torch, wf), dev(torch, r_words)
            for order in ORDERS:
                a = iwround(torch, ring, dw, tabs, cols, terms, dc, nv, order, work_fill=0)
                assert torch.equal(a, iwround(torch, ring, dw, tabs, cols, terms, dc, nv, order, work_fill=POISON_I64))
                fa = iwfold(torch, ring, dwf, tabs, cols, terms, dc, nv, r, order, work_fill=0)
                fb = iwfold(torch, ring, dwf, tabs, cols, terms, dc, nv, r, order, work_fill=POISON_I64)
                assert torch.equal(fa[0], fb[0]) and all(torch.equal(x, y) for x, y in zip(fa[1], fb[1]))
                assert np.array_equal(wsumcheck.vpoly_iwround_evals(ring, ww, words, hcols, terms, cw, nv, order), host(a)), (name, sname, order)
                msg, folded = wsumcheck.vpoly_iwround_fold_evals(ring, wf, words, hcols, terms, cw, nv, r_words, order)
                assert np.array_equal(msg, host(fa[0])), (name, sname, order)
                assert len(folded) == K + J and all(np.array_equal(f, host(x)) for f, x in zip(folded, fa[1])), (name, sname, order)


def test_table_slots_fold_in_place_in_trailing_order(torch_cuda):
    torch = torch_cuda
    name, k, nv = "goldilocks", 6, 10
    m, ring = model_for(name, k), ring_for(name, k)
    w, full = ring.words_per_elem, 1 << nv
    K, J, terms = IS.STRUCTURES["MIXED"]
    src = [dev(torch, t[:n * w]) for t, n in zip(tables_for(name, k, nv)[:K], (full, full - 3))]
    cols = columns_for(torch, name, k, nv, "MIXED")
    r, dwf = challenge(torch, m, 0x1A1A), dev(torch, weights_for(name, k, full // 4))
    want_msg, want, _ = iwfold(torch, ring, dwf, src, cols, terms, None, nv, r, TRAILING)
    work = [t.clone() for t in src]
    outs = work + [torch.full((x.numel(),), POISON_I64, dtype=torch.int64, device="cuda") for x in want[K:]]
    msg, got, _ = iwfold(torch, ring, dwf, work, cols, terms, None, nv, r, TRAILING, outs=outs)
    assert torch.equal(msg, want_msg) and all(torch.equal(g, x) for g, x in zip(got, want))
    for t, s, g in zip(work, src, got):
        assert torch.equal(t[g.numel():], s[g.numel():])  # nothing beyond the folded length is touched


# ---- capture ------------------------------------------------------------------------------------------------------------------------------
def test_capture_of_the_fused_call_on_a_fresh_context_and_replay_after_columns_weights_and_challenge_change(torch_cuda):
    torch = torch_cuda
    from stark_rings_amd import CyclotomicRing

    name, k, nv = "goldilocks", 6, 10
    m = model_for(name, k)
    ring = CyclotomicRing(name, k, device=0)  # fresh: nothing has run on it, so nothing is warm
    try:
        K, J, terms = IS.STRUCTURES["PLONK"]
        w, order, full = ring.words_per_elem, LEADING, 1 << nv
        tabs = [dev(torch, t) for t in tables_for(name, k, nv)[:K]]
        cols = columns_for(torch, name, k, nv, "PLONK")
        r = challenge(torch, m, 0x6001)
        dc = coeffs_for(torch, name, k, "PLONK")
        dwf = dev(torch, weights_for(name, k, 1 << (nv - 2))).clone()
        out = torch.empty(4 * w, dtype=torch.int64, device="cuda")
        sizes = [VF.folded_len(stored(c, nv), nv, order) for c in cols]
        outs = [torch.empty(w << (nv - 1), dtype=torch.int64, device="cuda") for _ in range(K)] + \
               [torch.empty(n * w, dtype=torch.int64, device="cuda") for n in sizes]
        work_elems, launches = vpoly_iwround_plan(ring, nv, K, J, len(terms), 3, order, fold=True)
        assert work_elems and launches >= 2
        work = torch.full((work_elems * w,), POISON_I64, dtype=torch.int64, device="cuda")
        side = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            vpoly_iwround_fold_evals_dev(ring, out, outs, dwf, tabs, cols, terms, dc, nv, r, order, work, stream=side)
        graph.replay()
        torch.cuda.synchronize()
        want = iwfold(torch, ring_for(name, k), dwf, tabs, cols, terms, dc, nv, r, order)
        assert torch.equal(out, want[0]) and all(torch.equal(a, b) for a, b in zip(outs, want[1]))
        rng = random.Random("isumcheck replay")
        cols[0].values.copy_(ints_dev(torch, [rng.randrange(U64) for _ in range(full)]))
        cols[3].values.copy_(ints_dev(torch, [rng.randrange(2) for _ in range(full)]))
        dwf.copy_(dev(torch, weights_for(name, k, 1 << (nv - 2), seed=0x77)))
        r.copy_(challenge(torch, m, 0x6002))
        work.fill_(0x1111111111111111)
        graph.replay()
        torch.cuda.synchronize()
        again = iwfold(torch, ring_for(name, k), dwf, tabs, cols, terms, dc, nv, r, order)
        assert not torch.equal(again[0], want[0])
        assert torch.equal(out, again[0]) and all(torch.equal(a, b) for a, b in zip(outs, again[1]))
    finally:
        ring.close()


# ---- the classes ----------------------------------------------------------------------------------------------------------------------------
def plonk_claim(torch, ring, m, nv, seed):
    """(the table MLEs a, b, c; the selector columns; build(g, selectors) adds q_L a + q_R b + q_M a b - q_O c + q_C)"""
    from stark_rings_amd import DenseMultilinearExtension as MLE

    full = 1 << nv
    rng = random.Random("isumcheck plonk %d" % seed)
    tabs = [MLE(ring, nv, dev(torch, m.uniform(0xE900 + seed + j, full))) for j in range(3)]
    p = ring.modulus
    cols = [IndexColumn(ints_dev(torch, [rng.randrange(2) for _ in range(full)])), IndexColumn(ints_dev(torch, edge_values(p, full)[:full])),
            IndexColumn(start=U64 - full), IndexColumn(ints_dev(torch, [rng.randrange(U64) for _ in range(full)]), n_evals=full - 3),
            IndexColumn(start=0)]
    minus_one = dev(torch, m.words([m.sub(m.zero(), one_of(m))]))

    def build(g, q):
        a, b, c = tabs
        g.add_mle_list([q[0], a])
        g.add_mle_list([q[1], b])
        g.add_mle_list([q[2], a, b])
        g.add_mle_list([q[3], c], minus_one)
        g.add_mle_list([q[4]])
        return g

    return tabs, cols, build


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name,k", SIX, ids=[c[0] for c in SIX])
def test_eq_sumcheck_over_plonk_with_selector_columns_sends_the_messages_of_expanded_tables_and_verifies(torch_cuda, name, k, order):
    torch = torch_cuda
    from stark_rings_amd import EqSumCheck, VirtualPolynomial
    from protocol_verifier import same
    from test_protocols_gpu import claimed_sum, env_for

    env = env_for(torch, name, k)
    m, ring, V = env.m, env.ring, env.V
    nv, w = 4, ring.words_per_elem
    tabs, cols, build = plonk_claim(torch, ring, m, nv, 7)
    selectors = [IndexMultilinearExtension(ring, nv, c) for c in cols]
    dense = [q.to_dense() for q in selectors]
    for q, d, c in zip(selectors, dense, cols):
        assert torch.equal(d.evaluations, from_u64_dev(ring, c, stored(c, nv), like=tabs[0].evaluations)) and d.num_vars == nv
    g = build(VirtualPolynomial(ring, nv), selectors)
    e = build(VirtualPolynomial(ring, nv), dense)
    assert len(g.tables) == 8 and g.degree == 3 and g.terms == e.terms
    z = dev(torch, m.uniform(0x2E0, nv))
    challenges = env.uniform(0x7100, nv)
    rs = [env.put([r]) for r in challenges]
    # the slow path expands: the unweighted message and the sum are those of the expanded claim
    assert torch.equal(g.round_evals(order), e.round_evals(order)) and torch.equal(g.sum(), e.sum())
    prover, explicit = EqSumCheck(g, z, order), EqSumCheck(e, z, order)
    msgs = []
    for j in range(nv):
        msgs.append(prover.message())
        assert torch.equal(msgs[-1], explicit.message()), (name, order, j)
        prover.next(rs[j])
        explicit.next(rs[j])
        assert all(hasattr(t, "evaluations") for t in prover.g.tables)  # dense tables only after a fold
    (finals, eq_r), (want_finals, want_eq) = prover.final(), explicit.final()
    assert torch.equal(eq_r, want_eq) and all(torch.equal(a, b) for a, b in zip(finals, want_finals))
    # the verifier reads the raw tables: a, b, c and the expanded selectors, in the slots of g
    raw = [env.get(t.evaluations) for t in e.tables]
    minus = V.sub(V.zero, V.one)
    slot = {id(t): j for j, t in enumerate(e.tables)}
    a, b, c = (slot[id(t)] for t in tabs)
    q = [slot[id(t)] for t in dense]

    def g_of(v):
        return V.sum([V.mul(v[q[0]], v[a]), V.mul(v[q[1]], v[b]), V.mul(V.mul(v[q[2]], v[a]), v[b]), V.mul(minus, V.mul(v[q[3]], v[c])), v[q[4]]])

    zs = env.get(z)
    claim0 = claimed_sum(V, zs, nv, lambda i: g_of([t[i] if i < len(t) else V.zero for t in raw]))
    V.verify_eq_sumcheck(claim0, zs, [env.get(s) for s in msgs], challenges, [env.get(f)[0] for f in finals], env.get(eq_r)[0], order, g_of, raw,
                         points=5)
    assert same(env.get(prover.final()[1])[0], V.eq_eval(zs, V.point_of(challenges, order)))


def test_a_column_only_polynomial_and_a_single_variable(torch_cuda):
    """K = 0 through the classes, and num_vars == 1, where EqSumCheck's only fold goes through fixed_variables (the expanding path)"""
    torch = torch_cuda
    from stark_rings_amd import EqSumCheck, VirtualPolynomial

    for name, k in SIX:
        m, ring = model_for(name, k), ring_for(name, k)
        for nv in (1, 3):
            full = 1 << nv
            cols = [IndexColumn(ints_dev(torch, list(range(5, 5 + full)))), IndexColumn(start=U64 - full)]
            f = [IndexMultilinearExtension(ring, nv, c) for c in cols]
            g = VirtualPolynomial(ring, nv).add_mle_list([f[0], f[1]]).add_mle_list([f[0], f[0]])
            e = VirtualPolynomial(ring, nv).add_mle_list([f[0].to_dense(), f[1].to_dense()])
            e.add_mle_list([e.tables[0], e.tables[0]])
            assert len(g.tables) == 2
            z = dev(torch, m.uniform(0x2E7, nv))
            a, b = EqSumCheck(g, z), EqSumCheck(e, z)
            for j in range(nv):
                assert torch.equal(a.message(), b.message()), (name, nv, j)
                r = challenge(torch, m, 0x7200 + j)
                a.next(r)
                b.next(r)
            assert all(torch.equal(x, y) for x, y in zip(a.final()[0], b.final()[0]))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_every_device_refusal_names_its_reason_and_launches_nothing(torch_cuda):
    torch = torch_cuda
    from stark_rings_amd import _lib
    from stark_rings_amd._lib import VPolyTerm
    from stark_rings_amd.index_columns import sr_index_column

    ring = ring_for("goldilocks", 6)
    lib, ctx = ring._lib, ring._ctx
    nv, w = 10, ring.words_per_elem
    canary = 0x0123456789ABCDEF
    full, half = 1 << nv, 1 << (nv - 1)
    f = torch.full((w << nv,), 7, dtype=torch.int64, device="cuda")
    col = torch.full((w * half,), 3, dtype=torch.int64, device="cuda")  # long enough to stand in for a folded table as well
    g = torch.full((w * half,), canary, dtype=torch.int64, device="cuda")
    g2 = torch.full((w * half,), canary, dtype=torch.int64, device="cuda")
    wt = torch.full((w * half,), 9, dtype=torch.int64, device="cuda")
    out = torch.full((3 * w,), canary, dtype=torch.int64, device="cuda")
    r = torch.full((8 * w,), 5, dtype=torch.int64, device="cuda")[:w]
    co = torch.full((8 * w,), 3, dtype=torch.int64, device="cuda")[:2 * w]
    need, _ = vpoly_iwround_plan(ring, nv, 1, 1, 2, 2, LEADING, fold=True)
    need_r, _ = vpoly_iwround_plan(ring, nv, 1, 1, 2, 2, LEADING)
    assert 0 < need <= 16 and 0 < need_r <= 16
    work = torch.full((16 * w,), canary, dtype=torch.int64, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    n_out = (ctypes.c_size_t * 8)()
    arr = (VPolyTerm * 8)()
    arr[0].n_factors, arr[0].table[0], arr[0].table[1] = 2, 0, 1
    arr[1].n_factors, arr[1].table[0] = 1, 1
    fp, colp, gp, g2p, wtp, op, rp, cp, wp = (t.data_ptr() for t in (f, col, g, g2, wt, out, r, co, work))
    eb = 8 * w
    pa, sa, oa = (ctypes.c_void_p * 8)(fp), (ctypes.c_size_t * 8)(full), (ctypes.c_void_p * 8)(gp, g2p)
    stored_col = lambda p=colp, n=full, start=0: (sr_index_column * 8)(sr_index_column(p, n, start))  # noqa: E731

    def rnd(out_p=op, wts=wtp, num_vars=nv, order=LEADING, work_p=wp, work_n=16, co_p=cp, tabs=pa, sizes=sa, terms=arr, cols=stored_col(), K=1, J=1):
        rc = lib.sr_vpoly_iwround_evals_dev(ctx, out_p, wts, tabs, sizes, K, cols, J, terms, 2, co_p, num_vars, order, work_p, work_n, st)
        return rc, _lib.last_error()

    def fold(out_p=op, wts=wtp, num_vars=nv, order=LEADING, work_p=wp, work_n=16, outs=oa, r_p=rp, co_p=cp, tabs=pa, sizes=sa, terms=arr,
             cols=stored_col(), K=1, J=1):
        rc = lib.sr_vpoly_iwround_fold_evals_dev(ctx, out_p, outs, n_out, wts, tabs, sizes, K, cols, J, terms, 2, co_p, num_vars, r_p, order, work_p,
                                                 work_n, st)
        return rc, _lib.last_error()

    def terms_of(*lists):
        t = (VPolyTerm * 8)()
        for i, idx in enumerate(lists):
            t[i].n_factors = len(idx)
            for s, j in enumerate(idx[:4]):
                t[i].table[s] = j
        return t

    assert rnd()[0] == 0 and fold()[0] == 0  # the arguments every refusal below departs from are accepted
    torch.cuda.synchronize()
    out.fill_(canary), g.fill_(canary), g2.fill_(canary), work.fill_(canary)
    torch.cuda.synchronize()
    shared = [(dict(wts=None), "null pointer (d_weights)"), (dict(num_vars=48), "num_vars must be below 48"), (dict(out_p=None), "null pointer"),
              (dict(work_p=None), "null pointer (d_work)"), (dict(terms=terms_of([0, 1], [])), "n_factors must be 1 .. 4 (term 1)"),
              (dict(terms=terms_of([0, 2], [1])), "table index outside 0 .. n_tables - 1 (term 0)"),
              (dict(terms=terms_of([1, 1], [1])), "a table that no term uses"), (dict(terms=terms_of([0, 0], [0])), "a column that no term uses"),
              (dict(sizes=(ctypes.c_size_t * 8)(full + 1)), "n_evals exceeds 2^num_vars"), (dict(tabs=(ctypes.c_void_p * 8)(None)), "null pointer (a table)"),
              (dict(J=9), "n_index must be 0 .. 8"), (dict(J=-1), "n_index must be 0 .. 8"), (dict(K=8), "n_tables + n_index must be 1 .. 8"),
              (dict(cols=None), "null pointer (columns)"), (dict(cols=stored_col(n=full + 1)), "a column's n_evals exceeds 2^num_vars"),
              (dict(cols=stored_col(start=1)), "a stored column with a non-zero start"),
              (dict(cols=stored_col(p=None, n=0, start=U64 - full + 1)), "a progression wraps past 2^64 - 1"),
              (dict(cols=stored_col(p=op - 8 * (full - 1))), "d_out overlaps a column"), (dict(cols=stored_col(p=wp)), "d_work overlaps a column"),
              (dict(out_p=wtp + eb), "d_out overlaps d_weights"), (dict(out_p=fp + eb), "d_out overlaps a table"),
              (dict(co_p=fp + eb), "d_coeffs overlaps a table")]
    rnd_cases = [(dict(order=2), "SR_MLE_ROUND_SUM"), (dict(order=3), "unknown order"),
                 (dict(num_vars=0, cols=stored_col(n=1), sizes=(ctypes.c_size_t * 8)(1)), "num_vars >= 1"),
                 (dict(work_n=need_r - 1), "workspace too small")] + shared
    fold_cases = [(dict(order=2), "unknown order"), (dict(num_vars=1, cols=stored_col(n=2), sizes=(ctypes.c_size_t * 8)(2)), "num_vars >= 2"),
                  (dict(r_p=None), "null pointer"), (dict(work_n=need - 1), "workspace too small"),
                  (dict(outs=(ctypes.c_void_p * 8)(gp, None)), "null pointer (the folded table of a column)"),
                  (dict(outs=(ctypes.c_void_p * 8)(None, g2p)), "null pointer (a table)"),
                  (dict(outs=(ctypes.c_void_p * 8)(gp, gp)), "two folded tables overlap"),
                  (dict(outs=(ctypes.c_void_p * 8)(gp, colp)), "a folded table overlaps a column"),
                  (dict(outs=(ctypes.c_void_p * 8)(fp, g2p)), "only a trailing-order fold may run in place")] + shared
    for call, prefix, cases in ((rnd, "vpoly_iwround: ", rnd_cases), (fold, "vpoly_iwround_fold: ", fold_cases)):
        for kwargs, text in cases:
            rc, err = call(**kwargs)
            assert rc == 1 and err.startswith(prefix) and text in err, (prefix, kwargs, err)
    # allowed: a column over the weights, the coefficients or a table (read only), the same array in two slots, a table in place (trailing)
    two = (sr_index_column * 8)(sr_index_column(colp, full, 0), sr_index_column(colp, half, 0))
    assert rnd(cols=two, K=0, J=2, tabs=None, sizes=None)[0] == 0
    assert rnd(cols=stored_col(p=fp))[0] == 0 and rnd(cols=stored_col(p=wtp, n=8))[0] == 0
    assert fold(outs=(ctypes.c_void_p * 8)(fp, g2p), order=TRAILING)[0] == 0
    torch.cuda.synchronize()
    # the refusals launched nothing: the accepted calls above wrote, so the canaries are checked on fresh fills
    # (every refusal of either family, the family's own included; f and col are inputs here and keep their constant fills)
    out.fill_(canary), g.fill_(canary), g2.fill_(canary), work.fill_(canary), f.fill_(7), col.fill_(3)
    torch.cuda.synchronize()
    for call, cases in ((rnd, rnd_cases), (fold, fold_cases)):
        for kwargs, _ in cases:
            assert call(**kwargs)[0] == 1
    torch.cuda.synchronize()
    for t in (out, g, g2, work):
        assert bool((t == canary).all())
    assert bool((f == 7).all()) and bool((col == 3).all())  # nor was a would-be output among the inputs written
