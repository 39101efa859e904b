"""GPU parity of the sum-check round calls (sr_mle_round_evals[_dev]) for all six ring ids.  Every comparison is bit-exact.  Expected
values come from tools/model_sumcheck.py (every table folded with the point [R::from(t)] by tools/model_mle.py, multiplied and
summed; pinned by tests/test_sumcheck_host.py): on standard-form Python integers for the power-of-two rings, on the oracle's Fq3 /
Fq9 / Fq4 slot products for the reference's own rings -- the element types of tests/test_mle_gpu.py, whose Model class is used."""
import ctypes
import json
import os
import random
import sys

import numpy as np
import pytest

import oracle_lib as O
from test_mle_gpu import POISON, dev, host, model_for, ring_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import model_mle as M  # noqa: E402
import model_sumcheck as SC  # noqa: E402

pytestmark = pytest.mark.gpu
LEADING, TRAILING, ROUND_SUM = 0, 1, 2
MODES = (LEADING, TRAILING, ROUND_SUM)
# (ring, log2 D, num_vars): the issue's list, with num_vars of stark-4, babybear72 and frog16 grown by the minimum at which their round
# modes split (a workgroup of 256 lanes is one record and a lane takes at least 16 pairs), plus one short table per reference ring: the
# only shapes at which those run in a single launch (test_the_cases_reach_the_single_launch_and_the_split_path)
CASES = [("goldilocks", 6, 10), ("goldilocks", 16, 4), ("babybear", 5, 9), ("stark", 4, 10), ("stark", 12, 3),
         ("goldilocks24", 0, 11), ("babybear72", 0, 11), ("frog16", 0, 12), ("goldilocks24", 0, 3), ("babybear72", 0, 3), ("frog16", 0, 3)]
IDS = ["%s-%d-nv%d" % c for c in CASES]
FAMILY = {"goldilocks": "one-limb", "babybear": "one-limb"}  # every other ring is a family of its own
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "sumcheck_kats.json")))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def n_out(mode, d):
    return 1 if mode == ROUND_SUM else d + 1


def round_dev(torch, ring, tables, nv, mode, stream=None, work_fill=0x3C3C3C3C3C3C3C3C):
    """the _dev call with a workspace of exactly the planned size"""
    w = ring.words_per_elem
    out = torch.full((n_out(mode, len(tables)) * w,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    work_elems, _ = ring.mle_round_plan(nv, len(tables), mode)
    work = torch.full((work_elems * w,), work_fill, dtype=torch.int64, device="cuda") if work_elems else None
    ring.mle_round_evals_dev(out, tables, nv, mode, work, stream=stream)
    return out


def message(m, els, nv, mode, zero, one):
    if mode == ROUND_SUM:
        return [SC.product_sum([M.pad(f, nv, zero) for f in els], zero, m.add, m.mul)]
    return SC.round_evals(els, nv, mode, zero, one, m.add, m.sub, m.mul)


def expect(m, tables, nv, mode):
    """tables: memory words (numpy) of at most 2^nv elements each; the message as memory words"""
    return m.words(message(m, [m.elems(t) for t in tables], nv, mode, m.zero(), m.elems(m.one())[0]))


def columns(m, n_tables, mode):
    """The model holds a power-of-two ring element as D Python integers and works slot by slot, so at D > 2^10 and d >= 2 the round
    modes run on 96 columns -- the first and the last 32 and 32 seeded ones in between -- to keep a case within seconds; the other
    columns of those are covered by the composition test's full comparison at the same kernels.  d = 1 and SR_MLE_ROUND_SUM compare
    every column.  None: every column."""
    d = m.ring.degree
    if not m.pow2 or d <= 1024 or n_tables == 1 or mode == ROUND_SUM:
        return None
    rng = random.Random(d)
    return np.array(sorted(set(range(32)) | set(range(d - 32, d)) | {rng.randrange(32, d - 32) for _ in range(32)}))


def agrees(m, got_words, els, nv, mode):
    """els: lists of model elements (from elems_for / m.elems)"""
    cols = columns(m, len(els), mode)
    if cols is None:
        return np.array_equal(got_words, m.words(message(m, els, nv, mode, m.zero(), m.elems(m.one())[0])))
    want = message(m, [[e[cols] for e in f] for f in els], nv, mode, np.array([0] * cols.size, dtype=object), np.array([1] * cols.size, dtype=object))
    got = m.elems(got_words)
    return len(got) == len(want) and all(np.array_equal(g[cols], x) for g, x in zip(got, want))


_tables, _elems = {}, {}


def tables_for(name, k, nv):
    """four full tables per case, made once and never changed"""
    if (name, k, nv) not in _tables:
        m = model_for(name, k)
        _tables[(name, k, nv)] = [m.uniform(0x5C000 + j, 1 << nv) for j in range(4)]
    return _tables[(name, k, nv)]


def elems_for(name, k, nv):
    if (name, k, nv) not in _elems:
        m = model_for(name, k)
        _elems[(name, k, nv)] = [m.elems(t) for t in tables_for(name, k, nv)]
    return _elems[(name, k, nv)]


def test_the_cases_reach_the_single_launch_and_the_split_path():
    seen = {}
    for name, k, nv in CASES:
        ring = ring_for(name, k)
        for d in (1, 2, 3, 4):
            for mode in MODES:
                work, launches = ring.mle_round_plan(nv, d, mode)
                assert (work == 0) == (launches == 1)
                if mode != ROUND_SUM:  # the round modes themselves reach both paths
                    seen.setdefault(FAMILY.get(name, name), set()).add(launches == 1)
    assert seen == {f: {True, False} for f in ("one-limb", "stark", "goldilocks24", "babybear72", "frog16")}, seen


@pytest.mark.parametrize("d", [1, 2, 3, 4])
@pytest.mark.parametrize("name,k,nv", CASES, ids=IDS)
def test_full_tables_match_the_model_in_all_three_modes(torch_cuda, name, k, nv, d):
    torch = torch_cuda
    m, ring = model_for(name, k), ring_for(name, k)
    dt = [dev(torch, t) for t in tables_for(name, k, nv)[:d]]
    els = elems_for(name, k, nv)[:d]
    for mode in MODES:
        assert agrees(m, host(round_dev(torch, ring, dt, nv, mode)), els, nv, mode), (name, k, nv, d, mode)


def test_the_pinned_vectors_on_the_device(torch_cuda):
    torch = torch_cuda
    for case in KATS["cases"]:
        ring = ring_for(case["ring"], case["log2_degree"])
        F = O.FIELD_ID[case["ring"]]
        nv = case["num_vars"]
        dt = [dev(torch, O.to_mont(F, [x for e in f for x in e])) for f in case["tables"]]
        for key, mode in (("leading", LEADING), ("trailing", TRAILING), ("sum", ROUND_SUM)):
            want = case[key] if mode != ROUND_SUM else [case[key]]
            got = O.from_mont(F, host(round_dev(torch, ring, dt, nv, mode)))
            assert [int(x) for x in got] == [x for e in want for x in e], (case["ring"], len(dt), key)


def poisoned(torch, words, total_words):
    """a buffer of total_words poison words whose head holds `words`; returns the head as a view (the poison lies right behind)"""
    buf = torch.full((total_words,), POISON - (1 << 64), dtype=torch.int64, device="cuda")
    buf[:words.size] = dev(torch, words)
    return buf[:words.size], buf


@pytest.mark.parametrize("name,k,nv", CASES[:8], ids=IDS[:8])
def test_truncated_tables_are_never_read_past_their_stored_part(torch_cuda, name, k, nv):
    torch = torch_cuda
    m, ring = model_for(name, k), ring_for(name, k)
    w, full, half = ring.words_per_elem, 1 << nv, 1 << (nv - 1)
    tabs, els = tables_for(name, k, nv), elems_for(name, k, nv)
    for sizes in ((full - 1, 5), (half, half + 1, full), (1, full, full - 1, half + 1)):
        keep = [poisoned(torch, tabs[j][:n * w], full * w) for j, n in enumerate(sizes)]
        cut = [els[j][:n] for j, n in enumerate(sizes)]
        for mode in MODES:
            got = host(round_dev(torch, ring, [v for v, _ in keep], nv, mode))
            assert agrees(m, got, cut, nv, mode), (name, sizes, mode)


@pytest.mark.parametrize("name,k,nv", CASES[:8], ids=IDS[:8])
def test_an_empty_table_gives_zeros_and_loads_nothing(torch_cuda, name, k, nv):
    torch = torch_cuda
    ring = ring_for(name, k)
    w = ring.words_per_elem
    poison = torch.full((w << nv,), POISON - (1 << 64), dtype=torch.int64, device="cuda")
    empty = torch.empty(0, dtype=torch.int64, device="cuda")
    for d in (1, 3):
        for mode in MODES:
            tabs = [poison] * (d - 1) + [empty]
            assert not host(round_dev(torch, ring, tabs, nv, mode)).any(), (name, d, mode)


@pytest.mark.parametrize("name,k,nv", CASES[:8], ids=IDS[:8])
def test_zero_one_and_squared_tables(torch_cuda, name, k, nv):
    torch = torch_cuda
    m, ring = model_for(name, k), ring_for(name, k)
    n, w = 1 << nv, ring.words_per_elem
    f, fe = tables_for(name, k, nv)[0], elems_for(name, k, nv)[0]
    df = dev(torch, f)
    ones = dev(torch, np.tile(m.one(), n))
    zeros = torch.zeros(n * w, dtype=torch.int64, device="cuda")
    one_e, zero_e = [m.elems(m.one())[0]] * n, [m.zero()] * n
    for mode in MODES:
        assert not host(round_dev(torch, ring, [df, zeros], nv, mode)).any(), (name, mode)
        assert agrees(m, host(round_dev(torch, ring, [zeros], nv, mode)), [zero_e], nv, mode), (name, mode)
        assert agrees(m, host(round_dev(torch, ring, [ones, ones], nv, mode)), [one_e, one_e], nv, mode), (name, mode)
        assert agrees(m, host(round_dev(torch, ring, [df, df], nv, mode)), [fe, fe], nv, mode), (name, mode)  # the same pointer twice


LAZY = [("goldilocks", 1), ("babybear", 1), ("goldilocks24", 0), ("babybear72", 0), ("frog16", 0)]


@pytest.mark.parametrize("name,k", LAZY, ids=[c[0] for c in LAZY])
def test_all_p_minus_one_tables_pass_two_lazy_reduction_intervals(torch_cuda, name, k):
    """csrc/sumcheck.hpp reduces its lazy sums every kFlush = 64 terms.  A plan has at most 1024 records of 256 lanes, i.e. 2^18 / units
    lane-groups, so 129 * 2^18 / units pairs give every lane 129 of them: two intervals and one term.  One table, passed d times (up
    to 4.5 GiB for babybear72: a plan that fills the device leaves a lane no more terms on less).  Every word is p - 1, the largest
    canonical image; lo == hi, so p(t) = pairs * e^d at every t, which the model computes from one pair."""
    torch = torch_cuda
    m, ring = model_for(name, k), ring_for(name, k)
    w = ring.words_per_elem
    units = {"goldilocks": 1, "babybear": 1, "goldilocks24": 8, "babybear72": 8, "frog16": 4}[name]
    pairs = 129 * (1 << 18) // units
    nv = (2 * pairs - 1).bit_length()
    assert ring.mle_round_plan(nv, 2, LEADING)[0] == 1024 * 3
    top = m.p - 1 if m.p - 1 < 1 << 63 else m.p - 1 - (1 << 64)  # the word p - 1 as torch's signed 64-bit integer
    table = torch.full((2 * pairs * w,), top, dtype=torch.int64, device="cuda")
    e = m.elems(np.full(w, m.p - 1, dtype=np.uint64))[0]
    for d in (2, 3):
        prod = e
        for _ in range(d - 1):
            prod = m.mul(e, prod)
        for mode, terms, copies in ((LEADING, pairs, d + 1), (ROUND_SUM, 2 * pairs, 1)):
            if m.pow2:
                want = m.words([(prod * terms) % m.p])
            else:
                want = ((prod.astype(object) * terms) % m.p).astype(np.uint64)
            got = host(round_dev(torch, ring, [table] * d, nv, mode))
            assert np.array_equal(got, np.tile(want, copies)), (name, d, mode)
    del table
    torch.cuda.empty_cache()


# The last two plan two records and sit on the boundaries of the launch geometry: aligned, an element of 2^8 Goldilocks coefficients
# is 128 units and two lane-groups of a workgroup meet in LDS, shifted it is 256 units and a lane-group is a record of its own;
# aligned, an element of 2^9 BabyBear coefficients is 256 units, shifted 512, the same two records with twice the lanes.
OFF_BY_EIGHT = [("goldilocks", 6, 10), ("babybear", 5, 9), ("goldilocks", 8, 7), ("babybear", 9, 6)]


@pytest.mark.parametrize("name,k,nv", OFF_BY_EIGHT)
def test_tables_off_by_eight_bytes_take_the_one_coefficient_path_to_the_same_result(torch_cuda, name, k, nv):
    torch = torch_cuda
    m, ring = model_for(name, k), ring_for(name, k)
    tabs = tables_for(name, k, nv)[:3]
    aligned = [dev(torch, t) for t in tabs]
    shifted = []
    for t in tabs:
        buf = torch.empty(t.size + 1, dtype=torch.int64, device="cuda")
        buf[1:] = dev(torch, t)
        assert buf[1:].data_ptr() % 16 == 8
        shifted.append(buf[1:])
    for mode in MODES:
        a = host(round_dev(torch, ring, aligned, nv, mode))
        assert agrees(m, a, elems_for(name, k, nv)[:3], nv, mode), (name, mode)  # equal to each other could hide a common error
        assert np.array_equal(host(round_dev(torch, ring, shifted, nv, mode)), a), (name, mode)
        assert np.array_equal(host(round_dev(torch, ring, [aligned[0], shifted[1], aligned[2]], nv, mode)), a), (name, mode)


def composed(torch, m, tables, nv, mode):
    """the message from the entry points that were there before: one-variable folds at t * one, element-wise products, a sum"""
    ring = m.ring
    w = ring.words_per_elem
    outs = []
    for t in ([None] if mode == ROUND_SUM else range(len(tables) + 1)):
        cols = []
        for f in tables:
            if t is None:
                full = torch.zeros(w << nv, dtype=torch.int64, device="cuda")
                full[:f.numel()] = f
                cols.append(full)
            else:
                pt = dev(torch, m.words([SC.constant(t, m.zero(), m.elems(m.one())[0], m.add)]))
                o = torch.empty(w << (nv - 1), dtype=torch.int64, device="cuda")
                ring.mle_fix_variables_dev(o, f, nv, pt, mode, None)
                cols.append(o)
        acc = cols[0].clone()
        for c in cols[1:]:
            ring.ntt_mul_dev(acc, c)
        o = torch.empty(w, dtype=torch.int64, device="cuda")
        ring.sum_dev(o, acc)
        outs.append(o)
    return torch.cat(outs)


# one slightly larger shape per family, and the two large degrees (every column: test_full_tables compares 96 of them to the model)
LARGER = [("goldilocks", 6, 13), ("babybear", 5, 13), ("stark", 4, 11), ("goldilocks24", 0, 14), ("babybear72", 0, 12), ("frog16", 0, 14),
          ("goldilocks", 16, 4), ("stark", 12, 3)]


@pytest.mark.parametrize("name,k,nv", LARGER, ids=["%s-%d-nv%d" % c for c in LARGER])
def test_the_fused_call_agrees_with_the_composition_of_the_older_entry_points(torch_cuda, name, k, nv):
    torch = torch_cuda
    m, ring = model_for(name, k), ring_for(name, k)
    w = ring.words_per_elem
    sizes = (1 << nv, (1 << nv) - 3, 1 << nv)
    tabs = [dev(torch, m.uniform(0xC0DE + j, n)) for j, n in enumerate(sizes)]
    for d in (2, 3, 4) if k >= 12 else (2, 3):
        for mode in MODES:
            got = round_dev(torch, ring, (tabs + tabs[:1])[:d], nv, mode)
            assert torch.equal(got, composed(torch, m, (tabs + tabs[:1])[:d], nv, mode)), (name, d, mode)


def _interp(m, msg_words, r_words, d):
    """p(r) from the d + 1 message elements, slot by slot on standard-form integers (power-of-two rings)"""
    vals = m.elems(msg_words)
    r = m.elems(r_words)[0]
    deg = m.ring.degree
    return np.array([SC.lagrange_at([int(vals[t][c]) for t in range(d + 1)], int(r[c]), m.p) for c in range(deg)], dtype=object)


@pytest.mark.parametrize("name,k,nv", [("goldilocks", 4, 6), ("stark", 2, 5)])
@pytest.mark.parametrize("order", [LEADING, TRAILING])
def test_a_whole_sum_check_of_three_tables(torch_cuda, name, k, nv, order):
    torch = torch_cuda
    m, ring = model_for(name, k), ring_for(name, k)
    w = ring.words_per_elem
    tabs = [dev(torch, m.uniform(0xABC0 + j, 1 << nv)) for j in range(3)]
    claim = m.elems(host(round_dev(torch, ring, tabs, nv, ROUND_SUM)))[0]
    rng = random.Random("%s %d" % (name, order))
    point = []
    for rnd in range(nv):
        left = nv - rnd
        msg = host(round_dev(torch, ring, tabs, left, order))
        p = m.elems(msg)
        assert np.array_equal(m.add(p[0], p[1]), claim), (name, rnd)
        r_words = m.words([np.array([rng.randrange(m.p) for _ in range(ring.degree)], dtype=object)])
        point.append(r_words)
        claim = _interp(m, msg, r_words, 3)
        r_t = dev(torch, r_words)
        folded = []
        for f in tabs:
            o = torch.empty(w << (left - 1), dtype=torch.int64, device="cuda")
            work_elems, _ = ring.mle_plan(left, 1, order)
            ring.mle_fix_variables_dev(o, f, left, r_t, order, torch.empty(work_elems * w, dtype=torch.int64, device="cuda") if work_elems else None)
            folded.append(o)
        tabs = folded
    final = m.elems(host(tabs[0]))[0]
    for f in tabs[1:]:
        final = m.mul(m.elems(host(f))[0], final)
    assert np.array_equal(final, claim)
    # the folded tables are the evaluations at the challenge point (trailing order fixes the last variable first)
    full_point = dev(torch, np.concatenate(point if order == LEADING else point[::-1]))
    orig = [dev(torch, m.uniform(0xABC0 + j, 1 << nv)) for j in range(3)]
    for f, o in zip(tabs, orig):
        e = torch.empty(w, dtype=torch.int64, device="cuda")
        work_elems, _ = ring.mle_plan(nv, nv, LEADING)
        ring.mle_fix_variables_dev(e, o, nv, full_point, LEADING, torch.empty(max(work_elems, 1) * w, dtype=torch.int64, device="cuda"))
        assert torch.equal(e, f)


@pytest.mark.parametrize("name,nv", [("goldilocks24", 5), ("babybear72", 4), ("frog16", 5)])
def test_the_round_loop_on_the_reference_rings(torch_cuda, name, nv):
    """no interpolation on extension-field slots here: p(0) + p(1) is the plain sum of the tables as they stand in every round"""
    torch = torch_cuda
    m, ring = model_for(name, 0), ring_for(name, 0)
    w = ring.words_per_elem
    tabs = [dev(torch, m.uniform(0xDEF0 + j, 1 << nv)) for j in range(3)]
    for rnd in range(nv):
        left = nv - rnd
        msg = m.elems(host(round_dev(torch, ring, tabs, left, LEADING)))
        total = m.elems(host(round_dev(torch, ring, tabs, left, ROUND_SUM)))[0]
        assert np.array_equal(m.add(msg[0], msg[1]), total), (name, rnd)
        r_t = dev(torch, m.uniform(0x7000 + rnd, 1))
        folded = []
        for f in tabs:
            o = torch.empty(w << (left - 1), dtype=torch.int64, device="cuda")
            ring.mle_fix_variables_dev(o, f, left, r_t, LEADING, None)
            folded.append(o)
        tabs = folded


@pytest.mark.parametrize("name,k,nv", [("goldilocks", 6, 10), ("stark", 4, 10), ("babybear72", 0, 11)])
def test_capture_on_a_fresh_context_and_replay_after_the_tables_change(torch_cuda, name, k, nv):
    torch = torch_cuda
    from stark_rings_amd import CyclotomicRing

    m = model_for(name, k)
    ring = CyclotomicRing(name, k, device=0)  # fresh: nothing has run on it, so nothing is warm
    try:
        w = ring.words_per_elem
        d, mode = 3, TRAILING
        first = tables_for(name, k, nv)[:d]
        second = [m.uniform(0x9900 + j, 1 << nv) for j in range(d)]
        tabs = [dev(torch, t) for t in first]
        out = torch.empty((d + 1) * w, dtype=torch.int64, device="cuda")
        work_elems, launches = ring.mle_round_plan(nv, d, mode)
        assert work_elems and launches >= 2
        work = torch.full((work_elems * w,), POISON - (1 << 64), dtype=torch.int64, device="cuda")
        side = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            ring.mle_round_evals_dev(out, tabs, nv, mode, work, stream=side)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(host(out), expect(m, first, nv, mode))
        for t, new in zip(tabs, second):
            t.copy_(dev(torch, new))
        work.fill_(0x1111111111111111)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(host(out), expect(m, second, nv, mode))
    finally:
        ring.close()


def test_workspace_contents_do_not_matter(torch_cuda):
    torch = torch_cuda
    for name, k, nv in (("goldilocks", 6, 10), ("frog16", 0, 12)):
        ring = ring_for(name, k)
        tabs = [dev(torch, t) for t in tables_for(name, k, nv)[:2]]
        a = round_dev(torch, ring, tabs, nv, LEADING, work_fill=0)
        b = round_dev(torch, ring, tabs, nv, LEADING, work_fill=POISON - (1 << 64))
        assert torch.equal(a, b)


def test_the_class_methods(torch_cuda):
    torch = torch_cuda
    from stark_rings_amd import DenseMultilinearExtension as MLE, MLE_TRAILING, RingError

    for name, k, nv in (("goldilocks", 6, 10), ("stark", 4, 10), ("goldilocks24", 0, 11)):
        m, ring = model_for(name, k), ring_for(name, k)
        w = ring.words_per_elem
        full = 1 << nv
        words = [t[:n * w] for t, n in zip(tables_for(name, k, nv), (full, full - 5, full // 2 + 1))]
        mles = [MLE(ring, nv, dev(torch, t)) for t in words]
        assert np.array_equal(host(MLE.round_evals(mles)), expect(m, words, nv, LEADING))
        assert np.array_equal(host(MLE.round_evals(mles, order=MLE_TRAILING)), expect(m, words, nv, TRAILING))
        assert np.array_equal(host(MLE.product_sum(mles)), expect(m, words, nv, ROUND_SUM))
        assert np.array_equal(host(MLE.round_evals([mles[0], mles[0]])), expect(m, [words[0]] * 2, nv, LEADING))
        # the host-pointer form stages the same tables
        assert np.array_equal(ring.mle_round_evals(words, nv, TRAILING), expect(m, words, nv, TRAILING))
        with pytest.raises(RingError):
            MLE.round_evals([mles[0], MLE(ring, nv - 1, dev(torch, words[0][:w << (nv - 1)]))])
        with pytest.raises(RingError):
            MLE.round_evals([])


def test_every_refusal_names_its_reason_and_launches_nothing(torch_cuda):
    torch = torch_cuda
    from stark_rings_amd import _lib

    ring = ring_for("goldilocks", 6)
    lib, ctx = ring._lib, ring._ctx
    nv, w = 10, ring.words_per_elem
    canary = 0x0123456789ABCDEF
    f = torch.full((w << nv,), 7, dtype=torch.int64, device="cuda")
    out = torch.full((3 * w,), canary, dtype=torch.int64, device="cuda")
    need, _ = ring.mle_round_plan(nv, 2, LEADING)
    work = torch.full((need * w,), canary, dtype=torch.int64, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(out_p, ptrs, sizes, nt, num_vars, mode, work_p, work_n):
        pa = (ctypes.c_void_p * 4)(*ptrs) if ptrs is not None else None
        sa = (ctypes.c_size_t * 4)(*sizes) if sizes is not None else None
        rc = lib.sr_mle_round_evals_dev(ctx, out_p, pa, sa, nt, num_vars, mode, work_p, work_n, st)
        return rc, _lib.last_error()

    fp, op, wp, full = f.data_ptr(), out.data_ptr(), work.data_ptr(), 1 << nv
    bad = [
        ((None, [fp, fp], [full, full], 2, nv, LEADING, wp, need), "null pointer"),
        ((op, None, [full, full], 2, nv, LEADING, wp, need), "null pointer"),
        ((op, [fp, fp], None, 2, nv, LEADING, wp, need), "null pointer"),
        ((op, [fp, None], [full, full], 2, nv, LEADING, wp, need), "null pointer"),
        ((op, [fp, fp], [full, full], 2, nv, LEADING, None, need), "null pointer"),
        ((op, [fp, fp], [full, full], 0, nv, LEADING, wp, need), "n_tables must be 1 .. 4"),
        ((op, [fp, fp], [full, full], 5, nv, LEADING, wp, need), "n_tables must be 1 .. 4"),
        ((op, [fp, fp], [full, full], 2, nv, 3, wp, need), "unknown mode"),
        ((op, [fp, fp], [full, full], 2, 48, LEADING, wp, need), "num_vars must be below 48"),
        ((op, [fp, fp], [1, 1], 2, 0, TRAILING, wp, need), "num_vars >= 1"),
        ((op, [fp, fp], [full, full + 1], 2, nv, LEADING, wp, need), "n_evals exceeds 2^num_vars"),
        ((op, [fp, fp], [1 << 45, 1 << 45], 2, 47, LEADING, wp, need), "element count too large"),
        ((op, [fp, fp], [full, full], 2, nv, LEADING, wp, need - 1), "workspace too small"),
        ((fp + 8 * w, [fp, fp], [full, full], 2, nv, LEADING, wp, need), "d_out overlaps a table"),
        ((op, [fp, fp], [full, full], 2, nv, LEADING, fp, need), "d_work overlaps a table"),
        ((wp + 8 * w, [fp, fp], [full, full], 2, nv, LEADING, wp, need), "d_out overlaps d_work"),
    ]
    for args, msg in bad:
        rc, err = call(*args)
        assert rc == 1 and msg in err, (args, rc, err)
    torch.cuda.synchronize()
    assert bool((out == canary).all()) and bool((work == canary).all()) and bool((f == 7).all())
    rc, err = call(op, [fp, fp], [full, full], 2, nv, LEADING, wp, need)
    assert rc == 0, err
