"""GPU parity of the fused fold-and-round call of a sum of products (sr_vpoly_round_fold_evals[_dev],
VirtualPolynomial.fold_round_evals / fixed_variables) for all six ring ids.  Every comparison is bit-exact.  Expected values come from
tools/model_vpoly_fold.py (model_mle.fold of every table, then model_vpoly.round_evals of the folded tables; pinned by
tests/test_vpoly_fold_host.py) and from the composition of the device calls the fused call merges: sr_mle_fix_variables_dev per table
slot, then sr_vpoly_round_evals_dev in num_vars - 1 variables.  The shapes are those of tests/test_sumcheck_fold_gpu.py, the structures
and coefficients those of tests/test_vpoly_gpu.py.
"""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

import oracle_lib as O
from test_mle_gpu import POISON, dev, fold_dev, host, model_for, ring_for
from test_sumcheck_gpu import _interp, columns
from test_sumcheck_fold_gpu import CASES, FAMILY, IDS, WHOLE, challenge, elems_agree
from test_vpoly_gpu import STRUCTURES, coeffs_for, elems_for, one_of, tables_for, vp_dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import model_vpoly as VP  # noqa: E402
import model_vpoly_fold as VF  # noqa: E402

pytestmark = pytest.mark.gpu
LEADING, TRAILING = 0, 1
ORDERS = (LEADING, TRAILING)
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "vpoly_fold_kats.json")))
POISON_I64 = POISON - (1 << 64)
SPLIT, SIX = CASES[:8], [("goldilocks", 6), ("babybear", 5), ("stark", 4), ("goldilocks24", 0), ("babybear72", 0), ("frog16", 0)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def vfold_dev(torch, ring, tables, terms, coeffs, nv, r, order, outs=None, stream=None, work_fill=0x3C3C3C3C3C3C3C3C):
    """the _dev call with a workspace of exactly the planned size.  Without `outs` every folded table goes to the head of a poisoned
    buffer with two elements of poison behind it.  Returns (message, folded tables cut to what was written, whole output buffers)."""
    w, d = ring.words_per_elem, VP.degree(terms)
    out = torch.full(((d + 1) * w,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    want = [VF.folded_len(t.numel() // w, nv, order) for t in tables]
    if outs is None:
        bufs = [torch.full(((n + 2) * w,), POISON_I64, dtype=torch.int64, device="cuda") for n in want]
        outs = [b[:n * w] for b, n in zip(bufs, want)]
    else:
        bufs = outs
    work_elems, _ = ring.vpoly_round_fold_plan(nv, len(tables), len(terms), d, order)
    work = torch.full((work_elems * w,), work_fill, dtype=torch.int64, device="cuda") if work_elems else None
    n_out = ring.vpoly_round_fold_evals_dev(out, outs, tables, terms, coeffs, nv, r, order, work, stream=stream)
    assert n_out == want, (n_out, want)
    return out, [b[:n * w] for b, n in zip(bufs, n_out)], bufs


def composition(torch, ring, tables, terms, coeffs, nv, r, order):
    """the same round from the calls that were there before: (message, whole folded tables of 2^(nv-1) elements)"""
    folded = [fold_dev(torch, ring, t, nv, r, order)[0] for t in tables]
    return vp_dev(torch, ring, folded, terms, coeffs, nv - 1, order), folded


def same_as_composition(torch, ring, tables, terms, coeffs, nv, r, order, **kw):
    """every word of every folded table and of the message; the poison behind the folded tables is still there"""
    msg, got, bufs = vfold_dev(torch, ring, tables, terms, coeffs, nv, r, order, **kw)
    want_msg, want = composition(torch, ring, tables, terms, coeffs, nv, r, order)
    ok = torch.equal(msg, want_msg)
    for g, b, f in zip(got, bufs, want):
        ok = ok and torch.equal(g, f[:g.numel()]) and not bool(f[g.numel():].any())
        ok = ok and (b is g or bool((b[g.numel():] == POISON_I64).all()))
    return ok


def setup(torch, name, k, nv, structure):
    m = model_for(name, k)
    terms = STRUCTURES[structure]
    nt = VP.n_tables(terms)
    cw = coeffs_for(name, k, structure)
    return ([dev(torch, t) for t in tables_for(name, k, nv)[:nt]], terms, None if cw is None else dev(torch, cw),
            elems_for(name, k, nv)[:nt], None if cw is None else m.elems(cw))


# ---- 12. the plans the cases reach ----------------------------------------------------------------------------------------------------
def test_the_cases_reach_single_records_and_split_plans():
    """single: one launch; records: the pairs of the shape go in several records (the records are those of sr_mle_round_plan at
    num_vars - 1, whose one-table plan never splits its points); split: some points come from the round kernels over the folded tables,
    which forces the workspace by itself.  babybear72 and frog16 fuse at most one point, so no plan of theirs is a single launch."""
    seen = {}
    for name, k, nv in CASES:
        ring = ring_for(name, k)
        for nt in (3, 4, 8):
            for d in (1, 2, 3, 4):
                for order in ORDERS:
                    work, launches = ring.vpoly_round_fold_plan(nv, nt, 2, d, order)
                    assert (work == 0) == (launches == 1)
                    assert (work, launches) == ring.vpoly_round_fold_plan(nv, nt, 8, d, order)
                    records = ring.mle_round_plan(nv - 1, 1, order)[0] // 2  # 0: one record
                    forced = ring.vpoly_round_fold_plan(2, nt, 2, d, order)[1] > 1
                    fam = seen.setdefault(FAMILY.get(name, name), set())
                    fam |= {"single"} if launches == 1 else ({"records"} if records else set()) | ({"split"} if forced else set())
                    assert launches > 1 or not (records or forced)
                    assert work == max(records, 2 if forced else 0) * (d + 1)
                    assert work == ring.vpoly_round_plan(nv - 1, nt, 2, d, order)[0] or (forced and work == 2 * (d + 1))
    for f in ("one-limb", "stark", "goldilocks24"):
        assert seen[f] == {"single", "records", "split"}, seen
    for f in ("babybear72", "frog16"):
        assert seen[f] == {"records", "split"}, seen


# ---- 1. the five structures against the model and the composition ---------------------------------------------------------------------
@pytest.mark.parametrize("structure", ["SINGLE", "R1CS", "REPEAT", "MIXED", "CANCEL"])
@pytest.mark.parametrize("name,k,nv", CASES, ids=IDS)
def test_full_tables_match_the_model_and_the_composition_in_both_orders(torch_cuda, name, k, nv, structure):
    torch = torch_cuda
    m, ring = model_for(name, k), ring_for(name, k)
    dt, terms, dc, els, ce = setup(torch, name, k, nv, structure)
    r_words = m.uniform(0xF01D, 1)
    r = dev(torch, r_words)
    for order in ORDERS:
        msg, got, bufs = vfold_dev(torch, ring, dt, terms, dc, nv, r, order)
        want_msg, want = composition(torch, ring, dt, terms, dc, nv, r, order)
        assert torch.equal(msg, want_msg), (name, structure, order)  # every column
        for g, b, f in zip(got, bufs, want):
            assert torch.equal(g, f) and bool((b[g.numel():] == POISON_I64).all()), (name, structure, order)
        if structure == "CANCEL":
            assert not host(msg).any()
        cols = columns(m, 2, order)
        rr = m.elems(r_words)[0]
        if cols is None:
            e, c, zero, one = els, ce, m.zero(), one_of(m)
        else:
            e, c, rr = [[x[cols] for x in f] for f in els], None if ce is None else [x[cols] for x in ce], rr[cols]
            zero, one = np.array([0] * cols.size, dtype=object), np.array([1] * cols.size, dtype=object)
        folded, message = VF.fold_round(e, terms, c, nv, rr, order, zero, one, m.add, m.sub, m.mul)
        assert elems_agree(m, host(msg), message, cols), (name, structure, order)
        for g, f in zip(got, folded):
            assert elems_agree(m, host(g), f, cols), (name, structure, order)


def test_the_pinned_vectors_on_the_device(torch_cuda):
    torch = torch_cuda
    for case in KATS["cases"]:
        ring = ring_for(case["ring"], case["log2_degree"])
        F = O.FIELD_ID[case["ring"]]
        nv = case["num_vars"]
        dt = [dev(torch, O.to_mont(F, [x for e in f for x in e])) for f in case["tables"]]
        dc = dev(torch, O.to_mont(F, [x for c in case["coeffs"] for x in c]))
        r = dev(torch, O.to_mont(F, case["r"]))
        for key, order in (("leading", LEADING), ("trailing", TRAILING)):
            msg, got, _ = vfold_dev(torch, ring, dt, case["terms"], dc, nv, r, order)
            assert [int(x) for x in O.from_mont(F, host(msg))] == [x for e in case[key]["message"] for x in e], (case["ring"], case["structure"], key)
            for g, f in zip(got, case[key]["folded"]):
                assert [int(x) for x in O.from_mont(F, host(g))] == [x for e in f for x in e], (case["ring"], case["structure"], key)


# ---- 2. truncated and empty tables ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k,nv", SPLIT, ids=IDS[:8])
def test_truncated_and_empty_tables_agree_with_the_composition(torch_cuda, name, k, nv):
    """residues 1, 2, 3 mod 4; just below and above the quarter, the half and the three-quarter marks; one element; tables of different
    lengths in one call (a fold loop that stopped at the longest TERM would leave the longer tables unfolded); an empty table in one term
    only (R1CS: c), in every term (R1CS: e; REPEAT: f1 and f3), every table empty"""
    torch = torch_cuda
    m, ring = model_for(name, k), ring_for(name, k)
    w, full = ring.words_per_elem, 1 << nv
    half, q = full // 2, full // 4
    tabs = [dev(torch, t) for t in tables_for(name, k, nv)]
    r = challenge(torch, m, 0xC4A1)
    four = [(full, full - 1, full - 2, full - 3), (q - 1, q + 1, full, half - 1), (half + 1, 3 * q + 1, 3 * q - 1, 5), (1, full, full - 2, half + 2),
            (full, full, 1, 1), (full, full - 1, full, 0), (0, full, full - 3, full), (full, 0, half + 1, 0), (0, 0, 0, 0)]
    eight = [(full, full - 1, half + 1, 5, full, 1, half, full - 3), (q + 1, full, 0, full, 3, full, full, half - 1)]
    for structure, all_sizes in (("R1CS", four), ("REPEAT", four), ("MIXED", eight)):
        terms = STRUCTURES[structure]
        dc = dev(torch, coeffs_for(name, k, structure))
        for sizes in all_sizes:
            cut = [tabs[j][:n * w] for j, n in enumerate(sizes)]
            for order in ORDERS:
                assert same_as_composition(torch, ring, cut, terms, dc, nv, r, order), (name, structure, sizes, order)
                if structure == "R1CS" and sizes[0] == 0 or structure == "REPEAT" and sizes[1] == 0 and sizes[3] == 0:
                    assert not host(vfold_dev(torch, ring, cut, terms, dc, nv, r, order)[0]).any()  # every term has an empty table


# ---- 3. two variables -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", SIX + [("goldilocks", 0)], ids=[c[0] for c in SIX] + ["goldilocks-0"])
def test_two_variables_are_the_minimum(torch_cuda, name, k):
    torch = torch_cuda
    m, ring = model_for(name, k), ring_for(name, k)
    w = ring.words_per_elem
    tabs = [dev(torch, m.uniform(0x2200 + j, 4)) for j in range(8)]
    r = challenge(torch, m, 0x2222)
    for structure, all_sizes in (("R1CS", [(4, 4, 4, 4), (3, 1, 4, 2), (4, 4, 4, 0), (0, 0, 0, 0)]), ("MIXED", [(4, 3, 2, 1, 4, 4, 0, 3)])):
        terms = STRUCTURES[structure]
        dc = dev(torch, coeffs_for(name, k, structure))
        for sizes in all_sizes:
            cut = [tabs[j][:n * w] for j, n in enumerate(sizes)]
            for order in ORDERS:
                assert same_as_composition(torch, ring, cut, terms, dc, 2, r, order), (name, structure, sizes, order)
    els, ce = [m.elems(host(t)) for t in tabs[:4]], m.elems(coeffs_for(name, k, "R1CS"))
    for order in ORDERS:
        msg, got, _ = vfold_dev(torch, ring, tabs[:4], VP.R1CS, dev(torch, coeffs_for(name, k, "R1CS")), 2, r, order)
        folded, message = VF.fold_round(els, VP.R1CS, ce, 2, m.elems(host(r))[0], order, m.zero(), one_of(m), m.add, m.sub, m.mul)
        assert elems_agree(m, host(msg), message, None) and all(elems_agree(m, host(g), f, None) for g, f in zip(got, folded))


# ---- 4. one term without coefficients is the fused round of a product -------------------------------------------------------------------
@pytest.mark.parametrize("name,k,nv", CASES, ids=IDS)
def test_a_single_product_without_coefficients_is_the_fused_round_call_bit_for_bit(torch_cuda, name, k, nv):
    torch = torch_cuda
    m, ring = model_for(name, k), ring_for(name, k)
    w, full = ring.words_per_elem, 1 << nv
    r = challenge(torch, m, 0x51E6)
    for sizes in ((full, full, full), (full - 3, full, full // 2 + 1)):
        dt = [dev(torch, t[:n * w]) for t, n in zip(tables_for(name, k, nv), sizes)]
        for d in (1, 2, 3):
            for order in ORDERS:
                msg, got, _ = vfold_dev(torch, ring, dt[:d], [list(range(d))], None, nv, r, order)
                want_msg = torch.empty((d + 1) * w, dtype=torch.int64, device="cuda")
                want = [torch.empty_like(g) for g in got]
                need = ring.mle_round_fold_plan(nv, d, order)[0]
                work = torch.empty(need * w, dtype=torch.int64, device="cuda") if need else None
                ring.mle_round_fold_evals_dev(want_msg, want, dt[:d], nv, r, order, work)
                assert torch.equal(msg, want_msg) and all(torch.equal(a, b) for a, b in zip(got, want)), (name, sizes, d, order)


# ---- 5. in place, a pointer in two slots ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k,nv", SPLIT, ids=IDS[:8])
def test_trailing_order_folds_in_place_and_a_pointer_may_sit_in_two_slots(torch_cuda, name, k, nv):
    torch = torch_cuda
    m, ring = model_for(name, k), ring_for(name, k)
    w, full = ring.words_per_elem, 1 << nv
    r = challenge(torch, m, 0x1A1A)
    sizes = (full, full - 3, full // 2 + 1, full - 1)
    src = [dev(torch, t[:n * w]) for t, n in zip(tables_for(name, k, nv), sizes)]
    dc = dev(torch, coeffs_for(name, k, "R1CS"))
    want_msg, want = composition(torch, ring, src, VP.R1CS, dc, nv, r, TRAILING)
    work = [t.clone() for t in src]
    msg, got, _ = vfold_dev(torch, ring, work, VP.R1CS, dc, nv, r, TRAILING, outs=work)  # every slot in place
    assert torch.equal(msg, want_msg)
    for g, x, t, s in zip(got, want, work, src):
        assert torch.equal(g, x[:g.numel()])
        assert torch.equal(t[g.numel():], s[g.numel():])  # nothing beyond the folded length is touched
    # the same pointer in two slots, out of place: each slot gets its own output
    for order in ORDERS:
        assert same_as_composition(torch, ring, [src[0], src[0]], [[0, 1]], None, nv, r, order), (name, order)
        assert same_as_composition(torch, ring, [src[1], src[0], src[1], src[3]], VP.R1CS, dc, nv, r, order), (name, order)


# ---- 6. eight bytes off -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k,nv", [("goldilocks", 6, 10), ("babybear", 5, 11), ("goldilocks", 8, 8), ("babybear", 9, 7)])
def test_buffers_off_by_eight_bytes_take_the_one_coefficient_path_to_the_same_result(torch_cuda, name, k, nv):
    torch = torch_cuda
    m, ring = model_for(name, k), ring_for(name, k)
    w, full = ring.words_per_elem, 1 << nv
    terms = VP.R1CS
    assert all(ring.vpoly_round_fold_plan(nv, 4, 2, 3, order)[0] > 0 for order in ORDERS)  # several records
    sizes = (full, full - 3, full // 2 + 1, full)
    aligned = [dev(torch, t[:n * w]) for t, n in zip(tables_for(name, k, nv), sizes)]
    r = challenge(torch, m, 0x0FF8)
    dc = dev(torch, coeffs_for(name, k, "R1CS"))

    def shift(t):
        buf = torch.full((t.numel() + 1,), POISON_I64, dtype=torch.int64, device="cuda")
        buf[1:] = t
        assert buf[1:].data_ptr() % 16 == 8
        return buf[1:]

    shifted = [shift(t) for t in aligned]
    for order in ORDERS:
        want_msg, want, _ = vfold_dev(torch, ring, aligned, terms, dc, nv, r, order)
        for tables, outs_shifted, rr, cc in ((shifted, False, r, dc), ([aligned[0], shifted[1], aligned[2], aligned[3]], False, r, dc),
                                             (aligned, True, r, dc), (aligned, False, shift(r), dc), (aligned, False, r, shift(dc))):
            outs = None
            if outs_shifted:
                outs = [shift(torch.full((x.numel() + 2 * w,), POISON_I64, dtype=torch.int64, device="cuda")) for x in want]
            msg, got, bufs = vfold_dev(torch, ring, tables, terms, cc, nv, rr, order, outs=outs)
            assert torch.equal(msg, want_msg), (name, order)
            for g, x, b in zip(got, want, bufs):
                assert torch.equal(g, x), (name, order)
                assert bool((b[g.numel():] == POISON_I64).all())


# ---- 7. capture ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k,nv", [("goldilocks", 6, 10), ("stark", 4, 11), ("babybear72", 0, 12)])
def test_capture_on_a_fresh_context_and_replay_after_everything_changes(torch_cuda, name, k, nv):
    torch = torch_cuda
    from stark_rings_amd import CyclotomicRing

    m = model_for(name, k)
    ring = CyclotomicRing(name, k, device=0)  # fresh: nothing has run on it, so nothing is warm
    try:
        w, terms, order = ring.words_per_elem, VP.R1CS, LEADING
        tabs = [dev(torch, t) for t in tables_for(name, k, nv)[:4]]
        second = [m.uniform(0x9900 + j, 1 << nv) for j in range(4)]
        r = challenge(torch, m, 0x6001)
        dc = dev(torch, coeffs_for(name, k, "R1CS")).clone()
        out = torch.empty(4 * w, dtype=torch.int64, device="cuda")
        outs = [torch.empty(w << (nv - 1), dtype=torch.int64, device="cuda") for _ in range(4)]
        work_elems, launches = ring.vpoly_round_fold_plan(nv, 4, 2, 3, order)
        assert work_elems and launches >= 2
        work = torch.full((work_elems * w,), POISON_I64, dtype=torch.int64, device="cuda")
        side = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            ring.vpoly_round_fold_evals_dev(out, outs, tabs, terms, dc, nv, r, order, work, stream=side)
        graph.replay()
        torch.cuda.synchronize()
        want_msg, want = composition(torch, ring_for(name, k), tabs, terms, dc, nv, r, order)
        assert torch.equal(out, want_msg) and all(torch.equal(a, b) for a, b in zip(outs, want))
        for t, new in zip(tabs, second):
            t.copy_(dev(torch, new))
        r.copy_(challenge(torch, m, 0x6002))
        dc[:w].copy_(challenge(torch, m, 0x6003))
        work.fill_(0x1111111111111111)
        graph.replay()
        torch.cuda.synchronize()
        want_msg, want = composition(torch, ring_for(name, k), tabs, terms, dc, nv, r, order)
        assert torch.equal(out, want_msg) and all(torch.equal(a, b) for a, b in zip(outs, want))
    finally:
        ring.close()


# ---- 8. the workspace ---------------------------------------------------------------------------------------------------------------------
def test_workspace_contents_do_not_matter(torch_cuda):
    torch = torch_cuda
    for name, k, nv in (("goldilocks", 6, 10), ("frog16", 0, 13), ("babybear72", 0, 3)):
        m, ring = model_for(name, k), ring_for(name, k)
        dt, terms, dc, _, _ = setup(torch, name, k, nv, "MIXED")
        r = challenge(torch, m, 0x3003)
        a = vfold_dev(torch, ring, dt, terms, dc, nv, r, LEADING, work_fill=0)
        b = vfold_dev(torch, ring, dt, terms, dc, nv, r, LEADING, work_fill=POISON_I64)
        assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))


# ---- 9. a whole R1CS prover -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k,nv", WHOLE, ids=[c[0] for c in WHOLE])
@pytest.mark.parametrize("order", [LEADING, TRAILING])
def test_a_whole_r1cs_prover_through_the_fused_call_equals_the_unfused_loop(torch_cuda, name, k, nv, order):
    torch = torch_cuda
    from stark_rings_amd import DenseMultilinearExtension as MLE, VirtualPolynomial

    m, ring = model_for(name, k), ring_for(name, k)
    w, terms, d = ring.words_per_elem, VP.R1CS, 3
    sizes = (1 << nv, (1 << nv) - 3, 1 << nv, (1 << nv) - 1)
    start = [dev(torch, m.uniform(0xABC0 + j, n)) for j, n in enumerate(sizes)]
    cw = coeffs_for(name, k, "R1CS")
    dc = dev(torch, cw)
    challenges = [challenge(torch, m, 0x7000 + i) for i in range(nv)]
    # the unfused loop: message, then a fold per table
    tabs, msgs_a = start, []
    for rnd in range(nv):
        left = nv - rnd
        msgs_a.append(vp_dev(torch, ring, tabs, terms, dc, left, order))
        tabs = [fold_dev(torch, ring, t, left, challenges[rnd], order)[0] for t in tabs]
    finals_a = tabs
    # round 0 from sr_vpoly_round_evals_dev, rounds 1 .. nv - 1 from the fused call, the final evaluations from fixed_variables
    tabs, msgs_b = start, [vp_dev(torch, ring, start, terms, dc, nv, order)]
    for rnd in range(1, nv):
        msg, tabs, _ = vfold_dev(torch, ring, tabs, terms, dc, nv - rnd + 1, challenges[rnd - 1], order)
        msgs_b.append(msg)
    g = VirtualPolynomial(ring, 1)
    mles = [MLE(ring, 1, t) for t in tabs]
    g.add_mle_list([mles[j] for j in terms[0]], dc[:w])
    g.add_mle_list([mles[j] for j in terms[1]], dc[w:])
    last = g.fixed_variables(challenges[nv - 1], order)
    assert last.num_vars == 0 and last.terms == [list(t) for t in terms] and len(last.tables) == 4
    finals_b = [t.evaluations for t in last.tables]
    assert len(msgs_a) == len(msgs_b) == nv
    for rnd, (a, b) in enumerate(zip(msgs_a, msgs_b)):
        assert torch.equal(a, b), (name, order, rnd)
    for a, b in zip(finals_a, finals_b):
        assert torch.equal(a, b), (name, order)
    if m.pow2:  # prime-field slots: p(0) + p(1) is the running claim, and the last claim is g of the final evaluations
        claim = m.elems(host(vp_dev(torch, ring, start, terms, dc, nv, 2)))[0]
        for rnd, msg in enumerate(msgs_b):
            p = m.elems(host(msg))
            assert np.array_equal(m.add(p[0], p[1]), claim), (name, order, rnd)
            claim = _interp(m, host(msg), host(challenges[rnd]), d)
        vals = [m.elems(host(f))[0] for f in finals_b]
        assert np.array_equal(VP.evaluate(vals, terms, m.elems(cw), m.zero(), m.add, m.mul), claim)


# ---- 10. the host-pointer form and the class ----------------------------------------------------------------------------------------------
def test_the_host_pointer_form_and_the_class_methods(torch_cuda):
    torch = torch_cuda
    from stark_rings_amd import DenseMultilinearExtension as MLE, MLE_TRAILING, RingError, VirtualPolynomial

    for name, k, nv in (("goldilocks", 6, 10), ("goldilocks", 0, 5), ("stark", 4, 11), ("goldilocks24", 0, 12)):
        m, ring = model_for(name, k), ring_for(name, k)
        w, full = ring.words_per_elem, 1 << nv
        terms = VP.R1CS
        words = [t[:n * w] for t, n in zip(tables_for(name, k, nv), (full, full - 5, full // 2 + 1, full))]
        tabs = [dev(torch, t) for t in words]
        cw = coeffs_for(name, k, "R1CS")
        dc = dev(torch, cw)
        r_words = m.uniform(0x4004, 1)
        r = dev(torch, r_words)
        for order in ORDERS:
            want_msg, want, _ = vfold_dev(torch, ring, tabs, terms, dc, nv, r, order)
            msg, folded = ring.vpoly_round_fold_evals(words, terms, cw, nv, r_words, order)
            assert np.array_equal(msg, host(want_msg))
            assert len(folded) == 4 and all(np.array_equal(f, host(x)) for f, x in zip(folded, want))
            msg1, folded1 = ring.vpoly_round_fold_evals(words[:3], [[0, 1, 2]], None, nv, r_words, order)
            want1 = vfold_dev(torch, ring, tabs[:3], [[0, 1, 2]], None, nv, r, order)
            assert np.array_equal(msg1, host(want1[0])) and all(np.array_equal(f, host(x)) for f, x in zip(folded1, want1[1]))
            mles = [MLE(ring, nv, t) for t in tabs]
            g = VirtualPolynomial(ring, nv)
            g.add_mle_list([mles[0], mles[1], mles[2]], dc[:w])
            g.add_mle_list([mles[0], mles[3]], dc[w:])
            msg, h = g.fold_round_evals(r, order)
            assert torch.equal(msg, want_msg)
            assert h.num_vars == nv - 1 and h.terms == g.terms and len(h.tables) == 4 and h.degree == 3  # the slots stay deduplicated
            assert all(t.num_vars == nv - 1 and torch.equal(t.evaluations, x) for t, x in zip(h.tables, want))
            assert torch.equal(h.round_evals(order), want_msg)
            f1 = g.fixed_variables(r, order)  # no message: fix_variables per distinct table
            assert f1.num_vars == nv - 1 and f1.terms == g.terms and len(f1.tables) == 4
            for t, x in zip(f1.tables, want):
                assert torch.equal(t.evaluations[:x.numel()], x) and not bool(t.evaluations[x.numel():].any())
            assert torch.equal(f1.round_evals(order), want_msg)
            two = torch.cat([r, challenge(torch, m, 0x4005)])
            f2 = g.fixed_variables(two, order)
            step = f1.fixed_variables(two[w:], order) if order == LEADING else g.fixed_variables(two[w:], order).fixed_variables(two[:w], order)
            assert f2.num_vars == nv - 2 and all(torch.equal(a.evaluations, b.evaluations) for a, b in zip(f2.tables, step.tables))
        with pytest.raises(RingError):
            g.fold_round_evals(r, MLE_TRAILING + 1)
        with pytest.raises(RingError):
            g.fixed_variables(r, MLE_TRAILING + 1)
        with pytest.raises(RingError):
            VirtualPolynomial(ring, nv).fold_round_evals(r)
        one = VirtualPolynomial(ring, 1)
        one.add_mle_list([MLE(ring, 1, tabs[0][:2 * w])])
        with pytest.raises(RingError):
            one.fold_round_evals(r)


# ---- 11. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_names_its_reason_and_launches_nothing(torch_cuda):
    torch = torch_cuda
    from stark_rings_amd import _lib
    from stark_rings_amd._lib import VPolyTerm

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
    co = torch.full((8 * w,), 3, dtype=torch.int64, device="cuda")[:2 * w]
    need, _ = ring.vpoly_round_fold_plan(nv, 2, 2, 2, LEADING)
    assert 0 < need <= 8
    work = torch.full((need * w,), canary, dtype=torch.int64, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    n_out = (ctypes.c_size_t * 8)()

    def terms_of(lists):
        arr = (VPolyTerm * 8)()
        for i, t in enumerate(lists):
            arr[i].n_factors = t[0]
            for s, j in enumerate(t[1:]):
                arr[i].table[s] = j
        return arr

    def call(out_p, optrs, ptrs, sizes, nt, terms, n_terms, co_p, num_vars, r_p, order, work_p, work_n, no=n_out):
        oa = (ctypes.c_void_p * 8)(*optrs) if optrs is not None else None
        pa = (ctypes.c_void_p * 8)(*ptrs) if ptrs is not None else None
        sa = (ctypes.c_size_t * 8)(*sizes) if sizes is not None else None
        ta = terms_of(terms) if terms is not None else None
        rc = lib.sr_vpoly_round_fold_evals_dev(ctx, out_p, oa, no, pa, sa, nt, ta, n_terms, co_p, num_vars, r_p, order, work_p, work_n, st)
        return rc, _lib.last_error()

    fp, f2p, gp, g2p, op, rp, cp, wp = (t.data_ptr() for t in (f, f2, g, g2, out, r, co, work))
    eb = 8 * w  # bytes of an element
    T = [(2, 0, 1), (1, 1)]  # c0 f0 f1 + c1 f1
    ok = (op, [gp, g2p], [fp, f2p], [full, full], 2, T, 2, cp, nv, rp, LEADING, wp, need)
    names = ("out_p", "optrs", "ptrs", "sizes", "nt", "terms", "n_terms", "co_p", "num_vars", "r_p", "order", "work_p", "work_n")

    def but(**kw):
        a = dict(zip(names, ok))
        a.update(kw)
        return a

    bad = [
        (but(out_p=None), "null pointer"), (but(optrs=None), "null pointer"), (but(ptrs=None), "null pointer"), (but(sizes=None), "null pointer"),
        (but(r_p=None), "null pointer"), (but(no=None), "null pointer"), (but(terms=None), "null pointer"), (but(ptrs=[fp, None]), "null pointer"),
        (but(optrs=[gp, None]), "null pointer"), (but(work_p=None), "null pointer"),
        (but(nt=0), "n_tables must be 1 .. 8"), (but(nt=9), "n_tables must be 1 .. 8"),
        (but(n_terms=0), "n_terms must be 1 .. 8"), (but(n_terms=9), "n_terms must be 1 .. 8"),
        (but(terms=[(0,), (1, 1)]), "n_factors must be 1 .. 4"), (but(terms=[(5, 0, 1, 0, 1), (1, 1)]), "n_factors must be 1 .. 4"),
        (but(terms=[(2, 0, 2), (1, 1)]), "table index outside"), (but(terms=[(2, 0, -1), (1, 1)]), "table index outside"),
        (but(terms=[(2, 0, 0), (1, 0)]), "a table that no term uses"),
        (but(order=2), "unknown order"), (but(order=-1), "unknown order"),
        (but(num_vars=48), "num_vars must be below 48"), (but(num_vars=1, sizes=[2, 2]), "num_vars >= 2"), (but(num_vars=0, sizes=[1, 1]), "num_vars >= 2"),
        (but(sizes=[full, full + 1]), "n_evals exceeds 2^num_vars"),
        (but(work_n=need - 1), "workspace too small"),
        (but(out_p=wp + eb), "d_out overlaps d_work"), (but(out_p=rp), "d_out overlaps d_r"), (but(work_p=rp), "d_work overlaps d_r"),
        (but(out_p=cp + eb), "d_out overlaps d_coeffs"), (but(work_p=cp), "d_work overlaps d_coeffs"), (but(r_p=cp + eb), "d_r overlaps d_coeffs"),
        (but(co_p=f2p + eb), "d_coeffs overlaps a table"), (but(co_p=g2p + eb), "d_coeffs overlaps a folded table"),
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
        assert rc == 1 and msg in err and err.startswith("vpoly_round_fold: "), (kw, rc, err)
    rc, err = call(**but(num_vars=47, sizes=[1 << 45, 1 << 45]))  # within 2^num_vars, beyond what a context addresses
    assert rc == 1 and err == "element count too large", (rc, err)
    torch.cuda.synchronize()
    for t in (out, work, g, g2):
        assert bool((t == canary).all())
    assert bool((f == 7).all()) and bool((f2 == 7).all()) and bool((r == 5).all()) and bool((co == 3).all())
    assert list(n_out) == [0] * 8
    rc, err = call(*ok)
    assert rc == 0, err
    assert list(n_out)[:2] == [half, half]
    rc, err = call(**but(co_p=None))  # no coefficients
    assert rc == 0, err
    rc, err = call(**but(optrs=[fp, f2p], order=TRAILING))  # both tables in place
    assert rc == 0, err
    torch.cuda.synchronize()
