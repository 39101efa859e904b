"""GPU parity of the weighted sum-check rounds (sr_vpoly_wround_evals[_dev], sr_vpoly_wround_fold_evals[_dev],
VirtualPolynomial.round_evals_weighted / fold_round_evals_weighted, EqSumCheck, ProductTree / FractionTree.layer_claim) for all six ring
ids.  Every comparison is bit-exact.  Expected values come from tools/model_wsumcheck.py (pinned by tests/test_wsumcheck_host.py) and
from a composition of the unweighted device calls: the weights expanded to a full table (W[2b] = W[2b+1] = w[b] in leading order,
W[b] = W[b + half] = w[b] in trailing order) as one more factor of every term -- a table that is constant in the round's variable
interpolates to itself at every t, so the first degree + 1 points agree word for word.  The shapes are those of
tests/test_sumcheck_fold_gpu.py, the structures and coefficients those of tests/test_vpoly_gpu.py.
"""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

import oracle_lib as O
from stark_rings_amd import vpoly_wround_evals_dev, vpoly_wround_fold_evals_dev
from test_mle_gpu import POISON, dev, fold_dev, host, model_for, ring_for
from test_sumcheck_gpu import columns
from test_sumcheck_fold_gpu import CASES, FAMILY, IDS, challenge, elems_agree
from test_vpoly_fold_gpu import vfold_dev
from test_vpoly_gpu import STRUCTURES, coeffs_for, elems_for, one_of, tables_for, vp_dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import model_vpoly as VP  # noqa: E402
import model_vpoly_fold as VF  # noqa: E402
import model_wsumcheck as W  # noqa: E402

pytestmark = pytest.mark.gpu
LEADING, TRAILING = 0, 1
ORDERS = (LEADING, TRAILING)
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "wsumcheck_kats.json")))
POISON_I64 = POISON - (1 << 64)
SPLIT, SIX = CASES[:8], [("goldilocks", 6), ("babybear", 5), ("stark", 4), ("goldilocks24", 0), ("babybear72", 0), ("frog16", 0)]
# six tables, degree 3: the 8-slot kernels, with room for the expanded weights as a seventh table and a fourth factor
WIDE = [[0, 1, 2], [3, 4], [5]]
FRACTION = W.FRACTION


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


_weights = {}


def weights_for(name, k, n_elems, seed=0x3E1600):
    if (name, k, n_elems, seed) not in _weights:
        _weights[(name, k, n_elems, seed)] = model_for(name, k).uniform(seed + n_elems, n_elems)
    return _weights[(name, k, n_elems, seed)]


def wround_dev(torch, ring, weights, tables, terms, coeffs, nv, order, stream=None, work_fill=0x3C3C3C3C3C3C3C3C):
    """the _dev call with a workspace of exactly the planned size, pre-filled with a pattern; two elements of poison behind the message"""
    w, d = ring.words_per_elem, VP.degree(terms)
    buf = torch.full(((d + 3) * w,), POISON_I64, dtype=torch.int64, device="cuda")
    work_elems, _ = ring.vpoly_wround_plan(nv, len(tables), len(terms), d, order)
    work = torch.full((work_elems * w,), work_fill, dtype=torch.int64, device="cuda") if work_elems else None
    vpoly_wround_evals_dev(ring, buf[:(d + 1) * w], weights, tables, terms, coeffs, nv, order, work, stream=stream)
    assert bool((buf[(d + 1) * w:] == POISON_I64).all())
    return buf[:(d + 1) * w]


def wfold_dev(torch, ring, weights, tables, terms, coeffs, nv, r, order, outs=None, stream=None, work_fill=0x3C3C3C3C3C3C3C3C):
    """as vfold_dev of tests/test_vpoly_fold_gpu.py: (message, folded tables cut to what was written, whole output buffers)"""
    w, d = ring.words_per_elem, VP.degree(terms)
    buf = torch.full(((d + 3) * w,), POISON_I64, dtype=torch.int64, device="cuda")
    want = [VF.folded_len(t.numel() // w, nv, order) for t in tables]
    if outs is None:
        bufs = [torch.full(((n + 2) * w,), POISON_I64, dtype=torch.int64, device="cuda") for n in want]
        outs = [b[:n * w] for b, n in zip(bufs, want)]
    else:
        bufs = outs
    work_elems, _ = ring.vpoly_wround_fold_plan(nv, len(tables), len(terms), d, order)
    work = torch.full((work_elems * w,), work_fill, dtype=torch.int64, device="cuda") if work_elems else None
    n_out = vpoly_wround_fold_evals_dev(ring, buf[:(d + 1) * w], outs, weights, tables, terms, coeffs, nv, r, order, work, stream=stream)
    assert n_out == want, (n_out, want)
    assert bool((buf[(d + 1) * w:] == POISON_I64).all())
    return buf[:(d + 1) * w], [b[:n * w] for b, n in zip(bufs, n_out)], bufs


def expand(torch, ring, weights, order):
    """one weight per pair -> a full table that is constant in the round's variable"""
    w = ring.words_per_elem
    return weights.view(-1, w).repeat_interleave(2, dim=0).reshape(-1).contiguous() if order == LEADING else torch.cat([weights, weights])


def composed_round(torch, ring, weights, tables, terms, coeffs, nv, order):
    """the first degree + 1 points of the unweighted call with the expanded weights as one more factor of every term"""
    d, w = VP.degree(terms), ring.words_per_elem
    eterms = [list(t) + [len(tables)] for t in terms]
    return vp_dev(torch, ring, list(tables) + [expand(torch, ring, weights, order)], eterms, coeffs, nv, order)[:(d + 1) * w]


def composed_fold(torch, ring, weights, tables, terms, coeffs, nv, r, order):
    """(message, folded tables) from the unweighted fused call, then composed_round on its folded tables"""
    _, folded, _ = vfold_dev(torch, ring, tables, terms, coeffs, nv, r, order)
    whole = [fold_dev(torch, ring, t, nv, r, order)[0] for t in tables]  # 2^(nv-1) elements each: the factor table is full
    return composed_round(torch, ring, weights, whole, terms, coeffs, nv - 1, order), folded


def composed_products(torch, m, ring, weights, tables, terms, coeffs, nv, order):
    """any structure, from the older entry points, point by point: every (full) table folded at R::from(t) (sr_mle_fix_variables_dev),
    per term the element-wise products with the weights (ntt_mul_dev), their sum (sum_dev), times the coefficient (mul_elem_dev), added"""
    w, out = ring.words_per_elem, []
    t_elem = m.zero()
    for t in range(VP.degree(terms) + 1):
        point = dev(torch, m.words([t_elem]))
        folded = [fold_dev(torch, ring, f, nv, point, order)[0] for f in tables]
        total = torch.zeros(w, dtype=torch.int64, device="cuda")
        for k, term in enumerate(terms):
            acc = weights.clone()
            for j in term:
                ring.ntt_mul_dev(acc, folded[j])
            o = torch.empty(w, dtype=torch.int64, device="cuda")
            ring.sum_dev(o, acc)
            if coeffs is not None:
                ring.mul_elem_dev(o, coeffs[k * w:(k + 1) * w].clone())
            ring.add_dev(total, o)
        out.append(total)
        t_elem = m.add(t_elem, one_of(m))
    return torch.cat(out)


def structure(name):
    return {"WIDE": WIDE, "FRACTION": FRACTION}.get(name) or STRUCTURES[name]


def coeff_words(name, k, sname):
    if sname in STRUCTURES:
        return coeffs_for(name, k, sname)
    return np.concatenate([model_for(name, k).uniform(0xC0FF0 + j, 1) for j in range(len(structure(sname)))])


def setup(torch, name, k, nv, sname):
    m = model_for(name, k)
    terms = structure(sname)
    nt = VP.n_tables(terms)
    cw = coeff_words(name, k, sname)
    return ([dev(torch, t) for t in tables_for(name, k, nv)[:nt]], terms, None if cw is None else dev(torch, cw),
            elems_for(name, k, nv)[:nt], None if cw is None else m.elems(cw))


# ---- the plans the cases reach ----------------------------------------------------------------------------------------------------------
def test_the_cases_reach_single_records_split_plans_and_eight_slots():
    seen = {}
    for name, k, nv in CASES:
        ring = ring_for(name, k)
        for nt in (3, 4, 6, 8):
            for d in (1, 2, 3, 4):
                for order in ORDERS:
                    for plan, v in ((ring.vpoly_wround_plan, nv), (ring.vpoly_wround_fold_plan, nv)):
                        work, launches = plan(v, nt, 2, d, order)
                        assert (work == 0) == (launches == 1)
                        assert (work, launches) == plan(v, nt, 8, d, order)
                        rv = v if plan == ring.vpoly_wround_plan else v - 1
                        records = ring.mle_round_plan(rv, 1, order)[0] // 2  # 0: one record
                        forced = plan(2, nt, 2, d, order)[1] > 1             # the points alone need several launches
                        fam = seen.setdefault((FAMILY.get(name, name), plan == ring.vpoly_wround_plan), set())
                        fam |= {"single"} if launches == 1 else ({"records"} if records else set()) | ({"split"} if forced else set())
                        if nt > 4:
                            fam.add("eight")
                        assert work == max(records, 2 if forced else 0) * (d + 1)
    # the round call: the one-limb fields take all five points in one launch (no split); babybear72 and frog16 take one point per
    # launch, so no plan of theirs is a single launch, in either call
    assert seen[("one-limb", True)] == {"single", "records", "eight"}, seen
    for f in ("stark", "goldilocks24"):
        assert seen[(f, True)] == {"single", "records", "split", "eight"}, seen
    for f in ("one-limb", "stark", "goldilocks24"):
        assert seen[(f, False)] == {"single", "records", "split", "eight"}, seen
    for f in ("babybear72", "frog16"):
        assert seen[(f, True)] == seen[(f, False)] == {"records", "split", "eight"}, seen


# ---- both calls against the model and the composition -----------------------------------------------------------------------------------
def model_args(m, els, ce, wel, order, extra=()):
    cols = columns(m, 2, order)
    if cols is None:
        return cols, els, ce, wel, list(extra), m.zero(), one_of(m)
    cut = lambda e: e[cols]  # noqa: E731
    return (cols, [[cut(x) for x in f] for f in els], None if ce is None else [cut(x) for x in ce], [cut(x) for x in wel],
            [cut(x) for x in extra], np.array([0] * cols.size, dtype=object), np.array([1] * cols.size, dtype=object))


@pytest.mark.parametrize("sname", ["SINGLE", "R1CS", "REPEAT", "MIXED", "CANCEL", "WIDE"])
@pytest.mark.parametrize("name,k,nv", CASES, ids=IDS)
def test_both_calls_match_the_model_and_the_composition_in_both_orders(torch_cuda, name, k, nv, sname):
    torch = torch_cuda
    m, ring = model_for(name, k), ring_for(name, k)
    dt, terms, dc, els, ce = setup(torch, name, k, nv, sname)
    ww, wf = weights_for(name, k, 1 << (nv - 1)), weights_for(name, k, 1 << (nv - 2))
    dw, dwf = dev(torch, ww), dev(torch, wf)
    r_words = m.uniform(0xF01D, 1)
    r = dev(torch, r_words)
    composable = VP.degree(terms) < 4 and len(dt) < 8
    small = nv <= 4 or name in ("goldilocks", "babybear", "stark") and (1 << nv) * ring.degree <= 1 << 16
    for order in ORDERS:
        msg = wround_dev(torch, ring, dw, dt, terms, dc, nv, order)
        fmsg, got, _ = wfold_dev(torch, ring, dwf, dt, terms, dc, nv, r, order)
        _, want_folded, _ = vfold_dev(torch, ring, dt, terms, dc, nv, r, order)
        assert all(torch.equal(a, b) for a, b in zip(got, want_folded)), (name, sname, order)
        # the fused message is the round call on the folded tables with the same weights
        assert torch.equal(fmsg, wround_dev(torch, ring, dwf, got, terms, dc, nv - 1, order)), (name, sname, order)
        if composable:
            assert torch.equal(msg, composed_round(torch, ring, dw, dt, terms, dc, nv, order)), (name, sname, order)
            assert torch.equal(fmsg, composed_fold(torch, ring, dwf, dt, terms, dc, nv, r, order)[0]), (name, sname, order)
        if sname == "CANCEL":
            assert not host(msg).any() and not host(fmsg).any()
        else:  # a fourth factor or an eighth table leaves no room for the weights: the composition point by point
            assert torch.equal(msg, composed_products(torch, m, ring, dw, dt, terms, dc, nv, order)), (name, sname, order)
            assert torch.equal(fmsg, composed_products(torch, m, ring, dwf, got, terms, dc, nv - 1, order)), (name, sname, order)
        if small:  # the model where it is cheap
            cols, e, c, wel, (rr,), zero, one = model_args(m, els, ce, m.elems(ww), order, [m.elems(r_words)[0]])
            assert elems_agree(m, host(msg), W.wround_evals(e, terms, c, wel, nv, order, zero, one, m.add, m.sub, m.mul), cols), (name, sname, order)
            wel = model_args(m, els, ce, m.elems(wf), order)[3]
            folded, message = W.wfold_round(e, terms, c, wel, nv, rr, order, zero, one, m.add, m.sub, m.mul)
            assert elems_agree(m, host(fmsg), message, cols), (name, sname, order)
            assert all(elems_agree(m, host(g), f, cols) for g, f in zip(got, folded)), (name, sname, order)


@pytest.mark.parametrize("name,k,nv", CASES, ids=IDS)
def test_all_one_weights_are_the_unweighted_calls_bit_for_bit(torch_cuda, name, k, nv):
    torch = torch_cuda
    m, ring = model_for(name, k), ring_for(name, k)
    ones = dev(torch, np.tile(m.one(), 1 << (nv - 1)))
    r = challenge(torch, m, 0x0E5)
    for sname in ("R1CS", "REPEAT", "MIXED"):
        dt, terms, dc, _, _ = setup(torch, name, k, nv, sname)
        for coeffs in (dc, None):
            for order in ORDERS:
                assert torch.equal(wround_dev(torch, ring, ones, dt, terms, coeffs, nv, order), vp_dev(torch, ring, dt, terms, coeffs, nv, order))
                fmsg, got, _ = wfold_dev(torch, ring, ones[:ones.numel() // 2], dt, terms, coeffs, nv, r, order)
                want_msg, want, _ = vfold_dev(torch, ring, dt, terms, coeffs, nv, r, order)
                assert torch.equal(fmsg, want_msg) and all(torch.equal(a, b) for a, b in zip(got, want)), (name, sname, order)


def test_the_pinned_vectors_on_the_device(torch_cuda):
    torch = torch_cuda
    for case in KATS["cases"]:
        ring = ring_for(case["ring"], case["log2_degree"])
        nv, terms = case["num_vars"], case["terms"]
        if case["form"] == "standard":
            F = O.FIELD_ID[case["ring"]]
            put = lambda elems: dev(torch, O.to_mont(F, [x for e in elems for x in e]))  # noqa: E731
            get = lambda t: [int(x) for x in O.from_mont(F, host(t))]  # noqa: E731
        else:
            put = lambda elems: dev(torch, np.array([x for e in elems for x in e], dtype=np.uint64))  # noqa: E731
            get = lambda t: [int(x) for x in host(t)]  # noqa: E731
        if case["form"] == "standard":
            inputs = (case["tables"], case["coeffs"], case["weights_round"], case["weights_fold"], case["r"])
        else:
            m = model_for(case["ring"], 0)
            inputs = W.kat_inputs(case["ring"], case["n_evals"], len(terms), nv)
            inputs[1][1] = m.sub(m.zero(), one_of(m))  # R1CS: c1 = -one()
        dt = [put(f) for f in inputs[0]]
        dc, dw, dwf, r = put(inputs[1]), put(inputs[2]), put(inputs[3]), put([inputs[4]])
        for key, order in (("leading", LEADING), ("trailing", TRAILING)):
            where = (case["ring"], case["structure"], key)
            assert get(wround_dev(torch, ring, dw, dt, terms, dc, nv, order)) == [x for e in case[key]["round"] for x in e], where
            fmsg, got, _ = wfold_dev(torch, ring, dwf, dt, terms, dc, nv, r, order)
            assert get(fmsg) == [x for e in case[key]["fold_message"] for x in e], where
            for g, f in zip(got, case[key].get("folded", [])):
                assert get(g) == [x for e in f for x in e], where


# ---- truncated tables -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k,nv", SPLIT, ids=IDS[:8])
def test_truncated_tables_of_every_kind_agree_with_the_composition_and_read_no_weight_beyond_the_pass(torch_cuda, name, k, nv):
    """lengths 0, 1, odd, half and half + 1 (and full), in one term only and in every term; the weights beyond the last visited pair are
    poison, which is not canonical in any field and would show"""
    torch = torch_cuda
    m, ring = model_for(name, k), ring_for(name, k)
    w, full = ring.words_per_elem, 1 << nv
    half = full // 2
    tabs = [dev(torch, t) for t in tables_for(name, k, nv)]
    r = challenge(torch, m, 0xC4A1)
    dw, dwf = dev(torch, weights_for(name, k, half)), dev(torch, weights_for(name, k, half // 2))
    terms = STRUCTURES["R1CS"]
    dc = dev(torch, coeffs_for(name, k, "R1CS"))
    for sizes in ((full, full - 1, half + 1, half), (half, 1, full, full), (full, full, full, 0), (0, full, full, full), (1, 1, 1, 1),
                  (half + 1, half + 1, full - 3, 5), (0, 0, 0, 0)):
        cut = [tabs[j][:n * w] for j, n in enumerate(sizes)]
        for order in ORDERS:
            where = (name, sizes, order)
            assert torch.equal(wround_dev(torch, ring, dw, cut, terms, dc, nv, order), composed_round(torch, ring, dw, cut, terms, dc, nv, order)), where
            fmsg, got, bufs = wfold_dev(torch, ring, dwf, cut, terms, dc, nv, r, order)
            want_msg, want = composed_fold(torch, ring, dwf, cut, terms, dc, nv, r, order)
            assert torch.equal(fmsg, want_msg) and all(torch.equal(a, b) for a, b in zip(got, want)), where
            assert all(bool((b[g.numel():] == POISON_I64).all()) for g, b in zip(got, bufs)), where
            # pairs visited: the longest term of (e a b, e c)
            pairs = lambda n: (n + 1) // 2 if order == LEADING else min(n, half)  # noqa: E731
            visited = max(pairs(min(sizes[:3])), pairs(min(sizes[0], sizes[3])))
            poisoned = dw.clone()
            poisoned[visited * w:] = POISON_I64
            assert torch.equal(wround_dev(torch, ring, poisoned, cut, terms, dc, nv, order), wround_dev(torch, ring, dw, cut, terms, dc, nv, order)), where


# ---- in place ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k,nv", SPLIT, ids=IDS[:8])
def test_trailing_order_folds_in_place(torch_cuda, name, k, nv):
    torch = torch_cuda
    m, ring = model_for(name, k), ring_for(name, k)
    w, full = ring.words_per_elem, 1 << nv
    r = challenge(torch, m, 0x1A1A)
    sizes = (full, full - 3, full // 2 + 1, full - 1)
    src = [dev(torch, t[:n * w]) for t, n in zip(tables_for(name, k, nv), sizes)]
    dc, dwf = dev(torch, coeffs_for(name, k, "R1CS")), dev(torch, weights_for(name, k, full // 4))
    want_msg, want, _ = wfold_dev(torch, ring, dwf, src, VP.R1CS, dc, nv, r, TRAILING)
    work = [t.clone() for t in src]
    msg, got, _ = wfold_dev(torch, ring, dwf, work, VP.R1CS, dc, nv, r, TRAILING, outs=work)
    assert torch.equal(msg, want_msg)
    for g, x, t, s in zip(got, want, work, src):
        assert torch.equal(g, x) and torch.equal(t[g.numel():], s[g.numel():])  # nothing beyond the folded length is touched


# ---- eight bytes off --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k,nv", [("goldilocks", 6, 10), ("babybear", 5, 11), ("goldilocks", 8, 8), ("babybear", 9, 7)])
def test_every_buffer_off_by_eight_bytes_takes_the_one_coefficient_path_to_the_same_result(torch_cuda, name, k, nv):
    torch = torch_cuda
    m, ring = model_for(name, k), ring_for(name, k)
    w, full = ring.words_per_elem, 1 << nv
    terms = VP.R1CS
    sizes = (full, full - 3, full // 2 + 1, full)
    aligned = [dev(torch, t[:n * w]) for t, n in zip(tables_for(name, k, nv), sizes)]
    r, dc = challenge(torch, m, 0x0FF8), dev(torch, coeffs_for(name, k, "R1CS"))
    dw, dwf = dev(torch, weights_for(name, k, full // 2)), dev(torch, weights_for(name, k, full // 4))

    def shift(t):
        buf = torch.full((t.numel() + 1,), POISON_I64, dtype=torch.int64, device="cuda")
        buf[1:] = t
        assert buf[1:].data_ptr() % 16 == 8
        return buf[1:]

    shifted = [shift(t) for t in aligned]
    for order in ORDERS:
        want = wround_dev(torch, ring, dw, aligned, terms, dc, nv, order)
        want_msg, want_folded, _ = wfold_dev(torch, ring, dwf, aligned, terms, dc, nv, r, order)
        # every buffer shifted by one word, then the weights alone
        for tabs, wts, wtf, rr, cc, outs_shifted in ((shifted, shift(dw), shift(dwf), shift(r), shift(dc), True), (aligned, shift(dw), shift(dwf), r, dc, False)):
            assert torch.equal(wround_dev(torch, ring, wts, tabs, terms, cc, nv, order), want), (name, order)
            outs = [shift(torch.full((x.numel() + 2 * w,), POISON_I64, dtype=torch.int64, device="cuda")) for x in want_folded] if outs_shifted else None
            msg, got, bufs = wfold_dev(torch, ring, wtf, tabs, terms, cc, nv, rr, order, outs=outs)
            assert torch.equal(msg, want_msg), (name, order)
            for g, x, b in zip(got, want_folded, bufs):
                assert torch.equal(g, x) and bool((b[g.numel():] == POISON_I64).all()), (name, order)


# ---- the workspace, the host-pointer forms, the class methods -------------------------------------------------------------------------------
def test_workspace_contents_do_not_matter_and_the_host_pointer_forms_agree(torch_cuda):
    torch = torch_cuda
    from stark_rings_amd import DenseMultilinearExtension as MLE, MLE_TRAILING, RingError, VirtualPolynomial

    for name, k, nv in (("goldilocks", 6, 10), ("stark", 4, 11), ("babybear72", 0, 3), ("frog16", 0, 13)):
        m, ring = model_for(name, k), ring_for(name, k)
        w, full = ring.words_per_elem, 1 << nv
        words = [t[:n * w] for t, n in zip(tables_for(name, k, nv), (full, full - 5, full // 2 + 1, full))]
        tabs = [dev(torch, t) for t in words]
        terms, cw = VP.R1CS, coeffs_for(name, k, "R1CS")
        dc = dev(torch, cw)
        ww, wf, r_words = weights_for(name, k, full // 2), weights_for(name, k, full // 4), m.uniform(0x4004, 1)
        dw, dwf, r = dev(torch, ww), dev(torch, wf), dev(torch, r_words)
        for order in ORDERS:
            a = wround_dev(torch, ring, dw, tabs, terms, dc, nv, order, work_fill=0)
            assert torch.equal(a, wround_dev(torch, ring, dw, tabs, terms, dc, nv, order, work_fill=POISON_I64))
            fa = wfold_dev(torch, ring, dwf, tabs, terms, dc, nv, r, order, work_fill=0)
            fb = wfold_dev(torch, ring, dwf, tabs, terms, dc, nv, r, order, work_fill=POISON_I64)
            assert torch.equal(fa[0], fb[0]) and all(torch.equal(x, y) for x, y in zip(fa[1], fb[1]))
            assert np.array_equal(ring.vpoly_wround_evals(ww, words, terms, cw, nv, order), host(a))
            assert np.array_equal(ring.vpoly_wround_evals(ww, words[:3], [[0, 1, 2]], None, nv, order),
                                  host(wround_dev(torch, ring, dw, tabs[:3], [[0, 1, 2]], None, nv, order)))
            msg, folded = ring.vpoly_wround_fold_evals(wf, words, terms, cw, nv, r_words, order)
            assert np.array_equal(msg, host(fa[0])) and all(np.array_equal(f, host(x)) for f, x in zip(folded, fa[1]))
            mles = [MLE(ring, nv, t) for t in tabs]
            g = VirtualPolynomial(ring, nv)
            g.add_mle_list([mles[0], mles[1], mles[2]], dc[:w])
            g.add_mle_list([mles[0], mles[3]], dc[w:])
            assert torch.equal(g.round_evals_weighted(dw, order), a)
            msg, h = g.fold_round_evals_weighted(r, dwf, order)
            assert torch.equal(msg, fa[0]) and h.num_vars == nv - 1 and h.terms == g.terms
            assert all(torch.equal(t.evaluations, x) for t, x in zip(h.tables, fa[1]))
            assert torch.equal(h.round_evals_weighted(dwf, order), fa[0])
        with pytest.raises(RingError):
            g.round_evals_weighted(dw, MLE_TRAILING + 1)
        with pytest.raises(RingError):
            g.fold_round_evals_weighted(r, dwf, MLE_TRAILING + 1)
        with pytest.raises(RingError):
            g.round_evals_weighted(dwf)  # half the weights


# ---- capture ----------------------------------------------------------------------------------------------------------------------------------
def test_capture_of_the_fused_call_on_a_fresh_context_and_replay_after_weights_and_challenge_change(torch_cuda):
    torch = torch_cuda
    from stark_rings_amd import CyclotomicRing

    name, k, nv = "goldilocks", 6, 10
    m = model_for(name, k)
    ring = CyclotomicRing(name, k, device=0)  # fresh: nothing has run on it, so nothing is warm
    try:
        w, terms, order = ring.words_per_elem, VP.R1CS, LEADING
        tabs = [dev(torch, t) for t in tables_for(name, k, nv)[:4]]
        r = challenge(torch, m, 0x6001)
        dc = dev(torch, coeffs_for(name, k, "R1CS"))
        dwf = dev(torch, weights_for(name, k, 1 << (nv - 2))).clone()
        out = torch.empty(4 * w, dtype=torch.int64, device="cuda")
        outs = [torch.empty(w << (nv - 1), dtype=torch.int64, device="cuda") for _ in range(4)]
        work_elems, launches = ring.vpoly_wround_fold_plan(nv, 4, 2, 3, order)
        assert work_elems and launches >= 2
        work = torch.full((work_elems * w,), POISON_I64, dtype=torch.int64, device="cuda")
        side = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            vpoly_wround_fold_evals_dev(ring, out, outs, dwf, tabs, terms, dc, nv, r, order, work, stream=side)
        graph.replay()
        torch.cuda.synchronize()
        want = wfold_dev(torch, ring_for(name, k), dwf, tabs, terms, dc, nv, r, order)
        assert torch.equal(out, want[0]) and all(torch.equal(a, b) for a, b in zip(outs, want[1]))
        dwf.copy_(dev(torch, weights_for(name, k, 1 << (nv - 2), seed=0x77)))
        r.copy_(challenge(torch, m, 0x6002))
        work.fill_(0x1111111111111111)
        graph.replay()
        torch.cuda.synchronize()
        want = wfold_dev(torch, ring_for(name, k), dwf, tabs, terms, dc, nv, r, order)
        assert torch.equal(out, want[0]) and all(torch.equal(a, b) for a, b in zip(outs, want[1]))
    finally:
        ring.close()


# ---- EqSumCheck -----------------------------------------------------------------------------------------------------------------------------
def claims(torch, ring, m, name, k, nv, kind):
    """(tables, add(g, mles)): the claim `kind` without eq over fresh uniform tables"""
    from stark_rings_amd import DenseMultilinearExtension as MLE

    n = {"product": 2, "r1cs": 3, "fraction": 4}[kind]
    tabs = [MLE(ring, nv, dev(torch, m.uniform(0xE900 + j, 1 << nv))) for j in range(n)]
    lam = dev(torch, m.uniform(0xE9FF, 1))
    minus_one = dev(torch, m.words([m.sub(m.zero(), one_of(m))]))

    def build(g, t):
        if kind == "product":
            g.add_mle_list([t[0], t[1]])
        elif kind == "r1cs":
            g.add_mle_list([t[0], t[1]])
            g.add_mle_list([t[2]], minus_one)
        else:
            g.add_mle_list([t[0], t[3]])
            g.add_mle_list([t[1], t[2]])
            g.add_mle_list([t[2], t[3]], lam)
        return g

    return tabs, build


@pytest.mark.parametrize("kind", ["product", "r1cs", "fraction"])
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name,k", SIX, ids=[c[0] for c in SIX])
def test_eq_sumcheck_sends_the_messages_of_the_explicit_prover(torch_cuda, name, k, order, kind):
    """the explicit prover: VirtualPolynomial with DenseMultilinearExtension.eq(ring, z) multiplied in, round_evals, then
    fold_round_evals (the fraction claim has 5 tables there: the 8-slot kernels)"""
    torch = torch_cuda
    from stark_rings_amd import DenseMultilinearExtension as MLE, EqSumCheck, VirtualPolynomial

    m, ring = model_for(name, k), ring_for(name, k)
    nv, w = 5, ring.words_per_elem
    tabs, build = claims(torch, ring, m, name, k, nv, kind)
    z = dev(torch, m.uniform(0x2E0, nv))
    rs = [challenge(torch, m, 0x7100 + i) for i in range(nv)]
    g = build(VirtualPolynomial(ring, nv), tabs)
    e = build(VirtualPolynomial(ring, nv), tabs).mul_by_mle(MLE.eq(ring, z))
    assert len(e.tables) == len(tabs) + 1 and e.degree == g.degree + 1
    prover = EqSumCheck(g, z, order)
    msg = e.round_evals(order)
    for j in range(nv):
        assert torch.equal(prover.message(), msg), (name, kind, order, j)
        prover.next(rs[j])
        if j + 1 < nv:
            msg, e = e.fold_round_evals(rs[j], order)
        else:
            e = e.fixed_variables(rs[j], order)
    finals, eq_r = prover.final()
    assert len(finals) == len(tabs)
    for a, b in zip(finals + [eq_r], [t.evaluations for t in e.tables]):
        assert torch.equal(a, b), (name, kind, order)
    assert all(torch.equal(t.evaluations, dev(torch, m.uniform(0xE900 + j, 1 << nv))) for j, t in enumerate(tabs))  # the inputs are intact


@pytest.mark.parametrize("name,k", SIX, ids=[c[0] for c in SIX])
def test_layer_claims_of_the_trees_start_at_the_layers_evaluation(torch_cuda, name, k):
    torch = torch_cuda
    from stark_rings_amd import FractionTree, ProductTree

    m, ring = model_for(name, k), ring_for(name, k)
    nv, w = 4, ring.words_per_elem
    leaves, nums = dev(torch, m.uniform(0x1EAF, 1 << nv)), dev(torch, m.uniform(0x1EB0, 1 << nv))
    lam = dev(torch, m.uniform(0x1A3, 1))
    pt, ft = ProductTree(ring, leaves, nv), FractionTree(ring, nums, leaves, nv)
    for layer in (1, 2, nv - 1):
        z = dev(torch, m.uniform(0x2E1 + layer, nv - layer))
        zl = z.clone()  # the layer has nv - layer variables; evaluate fixes variable 0 first, as eq_table indexes them
        claim = pt.layer_claim(layer, z)
        s = claim.message()
        got = s[:w].clone()
        ring.add_dev(got, s[w:2 * w])
        assert torch.equal(got, pt.layer(layer).evaluate(zl)), (name, layer)
        claim = ft.layer_claim(layer, z, lam)
        s = claim.message()
        got = s[:w].clone()
        ring.add_dev(got, s[w:2 * w])
        p, q = ft.layer(layer)
        want = q.evaluate(zl)
        ring.ntt_mul_dev(want, lam)
        ring.add_dev(want, p.evaluate(zl))
        assert torch.equal(got, want), (name, layer)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_every_device_refusal_names_its_reason_and_launches_nothing(torch_cuda):
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
    wt = torch.full((w * half,), 9, dtype=torch.int64, device="cuda")
    out = torch.full((3 * w,), canary, dtype=torch.int64, device="cuda")
    r = torch.full((8 * w,), 5, dtype=torch.int64, device="cuda")[:w]
    co = torch.full((8 * w,), 3, dtype=torch.int64, device="cuda")[:2 * w]
    need, _ = ring.vpoly_wround_fold_plan(nv, 2, 2, 2, LEADING)
    need_r, _ = ring.vpoly_wround_plan(nv, 2, 2, 2, LEADING)
    assert 0 < need <= 16 and 0 < need_r <= 16
    work = torch.full((16 * w,), canary, dtype=torch.int64, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    n_out = (ctypes.c_size_t * 8)()
    arr = (VPolyTerm * 8)()
    arr[0].n_factors, arr[0].table[0], arr[0].table[1] = 2, 0, 1
    arr[1].n_factors, arr[1].table[0] = 1, 1
    fp, f2p, gp, g2p, wtp, op, rp, cp, wp = (t.data_ptr() for t in (f, f2, g, g2, wt, out, r, co, work))
    eb = 8 * w
    pa, sa, oa = (ctypes.c_void_p * 8)(fp, f2p), (ctypes.c_size_t * 8)(full, full), (ctypes.c_void_p * 8)(gp, g2p)

    def rnd(out_p=op, wts=wtp, num_vars=nv, order=LEADING, work_p=wp, work_n=16, co_p=cp, tabs=pa, sizes=sa, terms=arr):
        rc = lib.sr_vpoly_wround_evals_dev(ctx, out_p, wts, tabs, sizes, 2, terms, 2, co_p, num_vars, order, work_p, work_n, st)
        return rc, _lib.last_error()

    def fold(out_p=op, wts=wtp, num_vars=nv, order=LEADING, work_p=wp, work_n=16, outs=oa, r_p=rp, co_p=cp, tabs=pa, sizes=sa, terms=arr):
        rc = lib.sr_vpoly_wround_fold_evals_dev(ctx, out_p, outs, n_out, wts, tabs, sizes, 2, terms, 2, co_p, num_vars, r_p, order, work_p, work_n, st)
        return rc, _lib.last_error()

    def terms_of(*lists):
        t = (VPolyTerm * 8)()
        for i, idx in enumerate(lists):
            t[i].n_factors = len(idx)
            for s, j in enumerate(idx[:4]):
                t[i].table[s] = j
        return t

    # what the two weighted families share with the sum-of-products checks: the same text under either prefix
    shared = [(dict(terms=terms_of([0, 1], [])), "n_factors must be 1 .. 4 (term 1)"), (dict(terms=terms_of([0, 1, 0, 1, 0], [1])), "n_factors must be"),
              (dict(terms=terms_of([0, 2], [1])), "table index outside 0 .. n_tables - 1 (term 0)"),
              (dict(terms=terms_of([0, 0], [0])), "a table that no term uses"),
              (dict(sizes=(ctypes.c_size_t * 8)(full, full + 1)), "n_evals exceeds 2^num_vars"),
              (dict(tabs=(ctypes.c_void_p * 8)(fp, None)), "null pointer (a table)"), (dict(work_p=None), "null pointer (d_work)")]

    for call, prefix, cases in (
            (rnd, "vpoly_wround: ", [(dict(wts=None), "null pointer (d_weights)"), (dict(order=2), "SR_MLE_ROUND_SUM"), (dict(order=3), "unknown order"),
                                     (dict(num_vars=0), "num_vars >= 1"), (dict(num_vars=48), "num_vars must be below 48"),
                                     (dict(out_p=None), "null pointer"), (dict(work_p=None), "null pointer"), (dict(work_n=need_r - 1), "workspace too small"),
                                     (dict(out_p=wtp + eb), "d_out overlaps d_weights"), (dict(work_p=wtp), "d_work overlaps d_weights"),
                                     (dict(out_p=fp + eb), "d_out overlaps a table"), (dict(out_p=wp + eb), "d_out overlaps d_work"),
                                     (dict(out_p=cp + eb), "d_out overlaps d_coeffs"), (dict(work_p=f2p), "d_work overlaps a table"),
                                     (dict(work_p=cp), "d_work overlaps d_coeffs"), (dict(co_p=f2p + eb), "d_coeffs overlaps a table")] + shared),
            (fold, "vpoly_wround_fold: ", [(dict(wts=None), "null pointer (d_weights)"), (dict(order=2), "unknown order"), (dict(num_vars=1), "num_vars >= 2"),
                                          (dict(r_p=None), "null pointer"), (dict(work_n=need - 1), "workspace too small"),
                                          (dict(out_p=wtp + eb), "d_out overlaps d_weights"), (dict(work_p=wtp), "d_work overlaps d_weights"),
                                          (dict(outs=(ctypes.c_void_p * 8)(gp, wtp)), "a folded table overlaps d_weights"),
                                          (dict(out_p=rp), "d_out overlaps d_r"), (dict(outs=(ctypes.c_void_p * 8)(gp, gp)), "two folded tables overlap"),
                                          (dict(outs=(ctypes.c_void_p * 8)(fp, g2p)), "only a trailing-order fold may run in place"),
                                          (dict(outs=(ctypes.c_void_p * 8)(fp, g2p), tabs=(ctypes.c_void_p * 8)(fp, fp), order=TRAILING),
                                           "appears twice cannot be folded in place"),
                                          (dict(out_p=wp + eb), "d_out overlaps d_work"), (dict(work_p=rp), "d_work overlaps d_r"),
                                          (dict(out_p=cp + eb), "d_out overlaps d_coeffs"), (dict(work_p=cp), "d_work overlaps d_coeffs"),
                                          (dict(r_p=cp + eb), "d_r overlaps d_coeffs"), (dict(co_p=f2p + eb), "d_coeffs overlaps a table"),
                                          (dict(co_p=g2p + eb), "d_coeffs overlaps a folded table"),
                                          (dict(out_p=fp + eb), "d_out overlaps a table"), (dict(work_p=f2p), "d_work overlaps a table"),
                                          (dict(r_p=fp + 3 * eb), "d_r overlaps a table"), (dict(out_p=gp + eb), "d_out overlaps a folded table"),
                                          (dict(work_p=g2p), "d_work overlaps a folded table"),
                                          (dict(r_p=g2p + eb), "d_r overlaps a folded table")] + shared)):
        for kw, msg in cases:
            rc, err = call(**kw)
            assert rc == 1 and msg in err and err.startswith(prefix), (kw, rc, err)
        rc, err = call(num_vars=47, sizes=(ctypes.c_size_t * 8)(1 << 45, 1 << 45))  # within 2^num_vars, beyond what a context addresses
        assert rc == 1 and err == "element count too large", (rc, err)
    torch.cuda.synchronize()
    for t in (out, work, g, g2):
        assert bool((t == canary).all())
    assert bool((f == 7).all()) and bool((wt == 9).all()) and list(n_out) == [0] * 8
    assert rnd()[0] == 0 and fold()[0] == 0 and fold(outs=pa, order=TRAILING)[0] == 0
    assert list(n_out)[:2] == [half, half]
    torch.cuda.synchronize()
