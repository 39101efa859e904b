"""GPU parity of the integer-column calls (sr_lincomb_index_dev, sr_lincomb_index) and of what is built on them (from_u64_dev,
identity_permutation[_mles], permutation_leaves_indexed) for all six ring ids.  Every comparison is bit-exact.  Expected values come
from tools/model_lincomb_index.py, where R::from(x) is x one() by doubling and adding in the ring (pinned by
tests/test_lincomb_index_host.py).  Every output has a guard behind (and, where shifted, before) it, every stored part of a table and
of a column has poison behind it, and every coefficient whose mask bit is clear holds 0xFF.. words.

Sizes are those of tests/test_lincomb_gpu.py.  (K, J, M) sit on both sides of every bound of the plan: K + J = 4 / 5, the outputs of
one launch +- 1, K = 0 with J = 1 and J = 8, K + J = 16."""
import json
import os
import sys

import numpy as np
import pytest

from test_mle_gpu import POISON, dev, host, model_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import model_lincomb as LC  # noqa: E402
import model_lincomb_index as LI  # noqa: E402

pytestmark = pytest.mark.gpu
# (ring, log2 D, n)
CASES = [("goldilocks", 0, 300), ("goldilocks", 6, 37), ("goldilocks", 16, 3), ("babybear", 5, 37), ("stark", 4, 21), ("stark", 12, 2),
         ("goldilocks24", 0, 70), ("babybear72", 0, 70), ("frog16", 0, 70)]
IDS = ["%s-%d-n%d" % c for c in CASES]
LARGER = {("goldilocks", 16), ("stark", 12)}
SMALL = [c for c in CASES if c[:2] not in LARGER]
SMALL_IDS = ["%s-%d-n%d" % c for c in SMALL]
GUARD = 0x6B6B6B6B6B6B6B6B
ONES = 0xFFFFFFFFFFFFFFFF
U64 = 1 << 64
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "lincomb_index_kats.json")))["cases"]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def i64(x):
    return x - (1 << 64) if x >= 1 << 63 else x


def edge_values(md):
    return LI.edge_values(md.p)


def stored(md, n, seed, n_evals=None):
    """a stored column of n_evals (default n) integers: the edge values of the ring mixed with random 64-bit ones"""
    rng = np.random.RandomState(seed)
    edges = edge_values(md)
    ne = n if n_evals is None else n_evals
    pool = [int(rng.randint(0, 1 << 62)) * 4 + int(rng.randint(0, 4)) for _ in range(5)]   # few, so that the model embeds few
    return [edges[(seed + 3 * i) % len(edges)] if i % 2 == 0 else pool[i % 5] for i in range(ne)]


_embedded = {}


def embed_for(md):
    """x -> R::from(x) of the model, each integer embedded once per ring: LI.from_u64 on the model's one() and add.  At the two
    large degrees (2^16, 2^12 coefficients per element) the closed form of the power-of-two rings instead, every coefficient x mod p,
    which tests/test_lincomb_index_host.py pins against from_u64."""
    memo = _embedded.setdefault((md.name, md.k), {})
    one, zero = md.elems(md.one())[0], md.zero()

    def embed(x):
        if x not in memo:
            if (md.name, md.k) in LARGER:
                memo[x] = np.array([x % md.p] * md.ring.degree, dtype=object)
            else:
                memo[x] = LI.from_u64(x, one, zero, md.add)
        return memo[x]

    return embed


def expected(md, tw, cols, cw, uses, n):
    """the model's outputs as memory words; tw: the stored words of each table, cols: LI columns, cw: the coefficient elements"""
    K, J, M = len(tw), len(cols), len(uses)
    T = K + J
    ce = md.elems(cw)
    rows = [[ce[m * (T + 1) + k] if uses[m] >> k & 1 else None for k in range(T + 1)] for m in range(M)]
    one = md.elems(md.one())[0]
    outs = LI.lincomb_index([md.elems(t) for t in tw], cols, rows, uses, n, md.zero(), one, md.add, md.mul, embed_for(md))
    return [md.words(o) for o in outs]


def draw(md, K, J, M, n, n_evals=None, seed=0x21C0):
    ne = list(n_evals) if n_evals is not None else [n] * K
    return [md.uniform(seed + k, ne[k]) for k in range(K)], md.uniform(seed + 0x80, M * (K + J + 1))


def mixed_columns(md, J, n, seed):
    """J columns: stored ones full of edge values, with progressions from 0 and up to 2^64 - 1 in between"""
    cols = []
    for j in range(J):
        if j % 3 == 1:
            cols.append(LI.Progression(0 if j % 2 else U64 - n))
        else:
            cols.append(stored(md, n, seed + j))
    return cols


def device_columns(torch, cols, shift):
    """IndexColumn for every model column: a stored one lies `shift` words past a 16-byte boundary with poison behind it"""
    from stark_rings_amd import IndexColumn

    out = []
    for c in cols:
        if isinstance(c, LI.Progression):
            out.append(IndexColumn(start=c.start))
            continue
        buf = torch.full((len(c) + 3,), i64(POISON), dtype=torch.int64, device="cuda")
        assert buf.data_ptr() % 16 == 0
        if c:
            buf[shift:shift + len(c)] = dev(torch, np.array(c, dtype=np.uint64))
        out.append(IndexColumn(buf[shift:shift + len(c)]))
    return out


def run(torch, md, tw, cols, cw, uses, n, shift=0, stream=None, want=None):
    """one device call on fresh buffers: poison behind every stored part, ONES in every coefficient whose bit is clear, guards around
    the outputs; compares with the model and checks the guards.  shift: every buffer starts `shift` words past a 16-byte boundary."""
    from stark_rings_amd import lincomb_index_dev

    ring, w = md.ring, md.w
    K, J, M = len(tw), len(cols), len(uses)
    T = K + J
    want = expected(md, tw, cols, cw, uses, n) if want is None else want
    tabs = []
    for t in tw:
        buf = torch.full((t.size + w + 2,), i64(POISON), dtype=torch.int64, device="cuda")
        assert buf.data_ptr() % 16 == 0
        buf[shift:shift + t.size] = dev(torch, t)
        tabs.append(buf[shift:shift + t.size])
    cp = cw.copy()
    for m in range(M):
        for k in range(T + 1):
            if not uses[m] >> k & 1:
                cp[(m * (T + 1) + k) * w:(m * (T + 1) + k + 1) * w] = np.uint64(ONES)
    cbuf = torch.zeros(cp.size + 2, dtype=torch.int64, device="cuda")
    cbuf[shift:shift + cp.size] = dev(torch, cp)
    whole = [torch.full((n * w + w + 2,), i64(GUARD), dtype=torch.int64, device="cuda") for _ in range(M)]
    outs = [b[shift:shift + n * w] for b in whole]
    dcols = device_columns(torch, cols, shift)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    lincomb_index_dev(ring, outs, tabs, dcols, cbuf[shift:shift + cp.size], uses, n, [t.size // w for t in tw], stream)
    torch.cuda.synchronize()
    for m in range(M):
        got = host(whole[m])
        assert np.array_equal(got[shift:shift + n * w], want[m]), (md.name, md.k, K, J, M, n, m, shift)
        assert (got[:shift] == np.uint64(GUARD)).all() and (got[shift + n * w:] == np.uint64(GUARD)).all(), "guard overwritten"
    return want


def shapes(md):
    if (md.name, md.k) in LARGER:
        return [(1, 2, 2), (4, 1, 1)]
    reg_m, run_m = LI.OUTPUTS[md.ring.ring]
    ms = sorted({m for m in (1, reg_m, reg_m + 1, run_m - 1, run_m, run_m + 1, 4) if 1 <= m <= 4})
    return [(K, J, M) for K, J in ((0, 1), (0, 8), (1, 2), (3, 1), (4, 1), (8, 8)) for M in ms]


@pytest.mark.parametrize("name,k,n", CASES, ids=IDS)
def test_every_shape_matches_the_model_with_and_without_the_constant(torch_cuda, name, k, n):
    """both kernels of every family and every split of the outputs over launches; the even outputs add their constant, the odd ones
    do not (their constants hold 0xFF.. words); every stored column carries the edge values 0, 1, 2^31 +- 1, 2^32 +- 1, 2^63,
    2^64 - 1 and p - 1, p, p + 1 where the prime is below 2^64"""
    from stark_rings_amd import lincomb_index_plan

    md = model_for(name, k)
    seen = set()
    for K, J, M in shapes(md):
        tw, cw = draw(md, K, J, M, n, seed=0x1000 + 64 * K + 4 * J + M)
        T = K + J
        uses = [(1 << T) - 1 | ((1 << T) if m % 2 == 0 else 0) for m in range(M)]
        run(torch_cuda, md, tw, mixed_columns(md, J, n, 0x50 + K), cw, uses, n)
        want = LI.plan(md.ring.ring, K, J, M)
        assert lincomb_index_plan(md.ring, K, J, M) == want[:2]
        seen.add(want)
    if (name, k) not in LARGER:
        assert {s[2] for s in seen} == ({True, False} if LI.OUTPUTS[md.ring.ring][0] else {False})
        assert max(s[0] for s in seen) == -(-4 // LI.OUTPUTS[md.ring.ring][1])


@pytest.mark.parametrize("name,k,n", SMALL, ids=SMALL_IDS)
def test_progressions_from_zero_to_the_last_that_does_not_wrap_and_across_p(torch_cuda, name, k, n):
    md = model_for(name, k)
    starts = [0, U64 - n, 1 << 32]
    if md.p < U64:
        starts.append(md.p - n // 2)   # crosses p (Goldilocks, frog16): the values p - .., p, p + 1, .. reduce
    else:
        starts.append((1 << 63) - 1)
    for s in starts:
        tw, cw = draw(md, 1, 1, 1, n, seed=0x1500)
        run(torch_cuda, md, tw, [LI.Progression(s)], cw, [0b111], n)
    tw, cw = draw(md, 0, 4, 2, n, seed=0x1600)
    run(torch_cuda, md, tw, [LI.Progression(s) for s in starts], cw, [0b11111, 0b01111], n)


@pytest.mark.parametrize("name,k,n", SMALL, ids=SMALL_IDS)
def test_masks_drop_columns_and_never_read_the_dropped_coefficients(torch_cuda, name, k, n):
    """a column used by one output only; a table used by one output only; an output of the constant alone"""
    md = model_for(name, k)
    for K, J, uses in ((1, 2, [0b1011, 0b1101]), (1, 2, [0b0001, 0b0110, 0b1000]), (3, 2, [0b110101, 0b001010]),
                       (2, 3, [0b000001, 0b111110, 0b100000, 0b010101]), (8, 8, [0x15555, 0x0AAAA])):
        tw, cw = draw(md, K, J, len(uses), n, seed=0x2000 + K)
        run(torch_cuda, md, tw, mixed_columns(md, J, n, 0x2100 + K), cw, uses, n)


@pytest.mark.parametrize("name,k,n", CASES, ids=IDS)
def test_truncated_columns_and_tables_with_poison_behind(torch_cuda, name, k, n):
    """n_evals of 0, 1 and n - 1 for columns, on both kernels, next to truncated tables"""
    md = model_for(name, k)
    for K, J, M, ne, cne in ((1, 3, 1, [n - 1], [0, 1, n - 1]), (2, 3, 1, [0, n], [n - 1, 0, 1]), (0, 2, 2, [], [1, n - 1]), (1, 1, 1, [1], [0])):
        tw, cw = draw(md, K, J, M, n, ne, seed=0x3000 + K)
        cols = [stored(md, n, 0x3100 + j, c) for j, c in enumerate(cne)]
        run(torch_cuda, md, tw, cols, cw, [(2 << (K + J)) - 1] * M, n)


@pytest.mark.parametrize("name,k,n", SMALL, ids=SMALL_IDS)
def test_the_worst_case_of_the_sums(torch_cuda, name, k, n):
    """every word p - 1 in eight tables and seventeen coefficients, every column value 2^64 - 1 (and p - 1): the largest sums"""
    md = model_for(name, k)
    n = min(n, 5)
    top = md.const(md.p - 1, 1)
    big = [U64 - 1] * n
    for K, J, M in ((8, 8, 1), (8, 8, LI.OUTPUTS[md.ring.ring][1]), (2, 2, max(LI.OUTPUTS[md.ring.ring][0], 1))):
        tw = [np.tile(top, n) for _ in range(K)]
        cols = [big if j % 2 == 0 else [(md.p - 1) % U64] * n for j in range(J)]
        run(torch_cuda, md, tw, cols, np.tile(top, M * (K + J + 1)), [(2 << (K + J)) - 1] * M, n)


@pytest.mark.parametrize("name,k,n", SMALL, ids=SMALL_IDS)
def test_every_buffer_off_by_eight_bytes(torch_cuda, name, k, n):
    """tables, coefficients, outputs and index arrays at an odd 8-byte pointer: the one-coefficient path, and the same values"""
    md = model_for(name, k)
    for K, J, M in ((1, 2, 2), (3, 2, 1), (0, 1, 1), (3, 3, 3)):
        tw, cw = draw(md, K, J, M, n, [n] * (K - 1) + [n - 1] if K else [], seed=0x4000 + K)
        cols = mixed_columns(md, J, n, 0x4100)
        cols[0] = stored(md, n, 0x4200, n - 1)
        want = run(torch_cuda, md, tw, cols, cw, [(2 << (K + J)) - 1] * M, n, shift=0)
        run(torch_cuda, md, tw, cols, cw, [(2 << (K + J)) - 1] * M, n, shift=1, want=want)


@pytest.mark.parametrize("name,k,n", CASES, ids=IDS)
def test_in_place_for_one_output(torch_cuda, name, k, n):
    torch = torch_cuda
    from stark_rings_amd import lincomb_index_dev

    md = model_for(name, k)
    w = md.w
    for K, J in ((1, 2), (3, 2)):
        tw, cw = draw(md, K, J, 1, n, seed=0x5000 + K)
        cols = mixed_columns(md, J, n, 0x5100)
        want = expected(md, tw, cols, cw, [(2 << (K + J)) - 1], n)
        which = K - 1
        tabs = [torch.cat([dev(torch, t), torch.full((w,), i64(GUARD), dtype=torch.int64, device="cuda")]) for t in tw]
        views = [t[:n * w] for t in tabs]
        lincomb_index_dev(md.ring, [views[which]], views, device_columns(torch, cols, 0), dev(torch, cw), None, n)
        torch.cuda.synchronize()
        for j in range(K):
            got = host(tabs[j])
            assert np.array_equal(got[:n * w], want[0] if j == which else tw[j]), (name, K, j)
            assert (got[n * w:] == np.uint64(GUARD)).all()


def test_refused_overlaps_leave_the_outputs_unchanged(torch_cuda):
    torch = torch_cuda
    from stark_rings_amd import IndexColumn, RingError, lincomb_index_dev

    md = model_for("goldilocks", 6)
    ring, w, n = md.ring, md.w, 8
    tw, cw = draw(md, 1, 1, 2, n, seed=0x6000)
    t0 = dev(torch, tw[0])
    coef = torch.cat([dev(torch, cw), torch.full((n * w,), i64(GUARD), dtype=torch.int64, device="cuda")])
    c = coef[:cw.size]
    big = torch.full((3 * n * w,), i64(GUARD), dtype=torch.int64, device="cuda")
    a, b = big[:n * w], big[2 * n * w:]
    col = IndexColumn(big[n * w:n * w + n])
    free = IndexColumn(torch.arange(n, dtype=torch.int64, device="cuda"))
    keep = [t.clone() for t in (t0, coef, big)]
    for outs, tables, cols, msg in (([t0, a], [t0], [free], "in place needs n_outputs == 1"),
                                    ([a, big[w:w + n * w]], [t0], [free], "two outputs overlap"),
                                    ([a, coef[w:w + n * w]], [t0], [free], "an output overlaps the coefficients"),
                                    ([a, big[w:w + n * w]], [t0], [col], "two outputs overlap"),
                                    ([a, big[n * w - w:2 * n * w - w]], [t0], [col], "two outputs overlap"),
                                    ([b, big[n * w:2 * n * w]], [t0], [col], "an output overlaps a column"),
                                    ([a, b], [big[w:w + n * w]], [free], "an output overlaps a table")):
        with pytest.raises(RingError, match=msg):
            lincomb_index_dev(ring, outs, tables, cols, c, None, n)
    torch.cuda.synchronize()
    for t, was in zip((t0, coef, big), keep):
        assert torch.equal(t, was)
    lincomb_index_dev(ring, [a], [t0], [IndexColumn(free.values, n_evals=0)], c[:3 * w], None, 0)   # n = 0 succeeds and writes nothing
    torch.cuda.synchronize()
    assert torch.equal(big, keep[2])


@pytest.mark.parametrize("name,k,n", CASES, ids=IDS)
def test_no_index_column_is_sr_lincomb_dev_bit_for_bit(torch_cuda, name, k, n):
    torch = torch_cuda
    from stark_rings_amd import lincomb_dev, lincomb_index_dev

    md = model_for(name, k)
    w = md.w
    for K, M in ((3, 2), (5, 1)):
        tw = [md.uniform(0x7000 + j, n) for j in range(K)]
        cw = md.uniform(0x7080, M * (K + 1))
        tabs, coef = [dev(torch, t) for t in tw], dev(torch, cw)
        a = [torch.zeros(n * w, dtype=torch.int64, device="cuda") for _ in range(M)]
        b = [torch.ones(n * w, dtype=torch.int64, device="cuda") for _ in range(M)]
        lincomb_dev(md.ring, a, tabs, coef, None, n)
        lincomb_index_dev(md.ring, b, tabs, [], coef, None, n)
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(a, b)), (name, K, M)


@pytest.mark.parametrize("name,k,n", SMALL, ids=SMALL_IDS)
def test_from_u64_is_the_forward_transform_of_the_constant_polynomial(torch_cuda, name, k, n):
    """R::from(x) == ntt((x mod p, 0, .., 0)) for the edge values, the polynomial built by monomial.from_ints"""
    torch = torch_cuda
    from stark_rings_amd import IndexColumn, from_u64_dev, monomial

    md = model_for(name, k)
    ring, w = md.ring, md.w
    xs = edge_values(md)
    got = from_u64_dev(ring, IndexColumn(dev(torch, np.array(xs, dtype=np.uint64))), len(xs))
    torch.cuda.synchronize()
    got = host(got)
    for i, x in enumerate(xs):
        poly = np.array(monomial.from_ints(ring, [x % md.p] + [0] * (ring.degree - 1)), dtype=np.uint64).reshape(-1)
        want = ring.elementwise_crt(poly)
        assert np.array_equal(got[i * w:(i + 1) * w], want), (name, x)


@pytest.mark.parametrize("name,k,n", SMALL, ids=SMALL_IDS)
def test_permutation_leaves_indexed_and_the_identity_fixtures(torch_cuda, name, k, n):
    torch = torch_cuda
    from stark_rings_amd import (IndexColumn, from_u64_dev, identity_permutation, identity_permutation_mles, permutation_leaves,
                                 permutation_leaves_indexed)

    md = model_for(name, k)
    ring, w = md.ring, md.w
    f = dev(torch, md.uniform(0x8000, n))
    beta, gamma = dev(torch, md.uniform(0x8001, 1)), dev(torch, md.uniform(0x8002, 1))
    rng = np.random.RandomState(0x8003)
    sigma = rng.permutation(n).astype(np.uint64) + np.uint64(n)   # positions of the second wire column
    sig = dev(torch, sigma)
    num, den = permutation_leaves_indexed(ring, f, sig, beta, gamma, id_start=n)
    ident_t = from_u64_dev(ring, IndexColumn(start=n), n, like=f)
    sigma_t = from_u64_dev(ring, sig, n)
    num2, den2 = permutation_leaves(ring, f, ident_t, sigma_t, beta, gamma)
    torch.cuda.synchronize()
    assert torch.equal(num, num2) and torch.equal(den, den2)
    # against the model
    b, g = md.elems(host(beta))[0], md.elems(host(gamma))[0]
    one = md.elems(md.one())[0]
    want = LI.permutation_leaves_indexed(md.elems(host(f)), n, [int(s) for s in sigma], b, g, one, md.zero(), md.add, md.mul, embed_for(md))
    assert np.array_equal(host(num), md.words(want[0])) and np.array_equal(host(den), md.words(want[1]))
    # the reference's fixtures: chunk i starts at i 2^num_vars
    nv, chunks = 2, 3
    whole = identity_permutation(ring, nv, chunks, f)
    mles = identity_permutation_mles(ring, nv, chunks, f)
    torch.cuda.synchronize()
    assert whole.numel() == (chunks << nv) * w and len(mles) == chunks
    zero, add = md.zero(), md.add
    for i, m in enumerate(mles):
        assert m.num_vars == nv and torch.equal(m.evaluations, whole[(i << nv) * w:((i + 1) << nv) * w])
        assert np.array_equal(host(m.evaluations)[:w], md.words([LI.from_u64(i << nv, one, zero, add)]))
    assert np.array_equal(host(whole)[-w:], md.words([LI.from_u64((chunks << nv) - 1, one, zero, add)]))


@pytest.mark.parametrize("name,k,n", [("goldilocks", 6, 37), ("frog16", 0, 70)], ids=["goldilocks", "frog16"])
def test_a_non_default_stream(torch_cuda, name, k, n):
    md = model_for(name, k)
    tw, cw = draw(md, 1, 2, 2, n, seed=0x9000)
    run(torch_cuda, md, tw, [LI.Progression(5), stored(md, n, 0x9001)], cw, [0b1011, 0b1101], n, stream=torch_cuda.cuda.Stream())


@pytest.mark.parametrize("name,k,n", [("goldilocks", 6, 37), ("stark", 4, 21), ("babybear72", 0, 70)], ids=["goldilocks", "stark", "babybear72"])
def test_capture_and_replay_on_a_fresh_context(torch_cuda, name, k, n):
    """one capture (a single stream, no parallel branch) on a context that has made no call before; the replay matches the model"""
    torch = torch_cuda
    from stark_rings_amd import CyclotomicRing, lincomb_index_dev

    md = model_for(name, k)
    fresh = CyclotomicRing(name, k, device=0)
    w = md.w
    tw, cw = draw(md, 1, 2, 2, n, seed=0xA000)
    cols = [LI.Progression(U64 - n), stored(md, n, 0xA001, n - 1)]
    uses = [0b1011, 0b1101]
    want = expected(md, tw, cols, cw, uses, n)
    tabs, coef, dcols = [dev(torch, t) for t in tw], dev(torch, cw), device_columns(torch, cols, 0)
    outs = [torch.full((n * w + w,), i64(GUARD), dtype=torch.int64, device="cuda") for _ in range(2)]
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        lincomb_index_dev(fresh, [o[:n * w] for o in outs], tabs, dcols, coef, uses, n, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    for o in outs:
        o.fill_(i64(GUARD))
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    for o, exp in zip(outs, want):
        assert np.array_equal(host(o)[:n * w], exp) and (host(o)[n * w:] == np.uint64(GUARD)).all(), name
    del g
    fresh.close()


@pytest.mark.parametrize("name,k,n", SMALL, ids=SMALL_IDS)
def test_the_host_pointer_form(torch_cuda, name, k, n):
    from stark_rings_amd import IndexColumn, RingError, lincomb_index

    md = model_for(name, k)
    for K, J, M, ne in ((1, 2, 2, None), (3, 3, 3, [n, 0, n - 1]), (0, 8, 1, None), (8, 8, 1, None)):
        tw, cw = draw(md, K, J, M, n, ne, seed=0xB000 + K)
        cols = mixed_columns(md, J, n, 0xB100)
        cols[0] = stored(md, n, 0xB200, n - 1)
        uses = [(2 << (K + J)) - 1] * M
        hc = [IndexColumn(start=c.start) if isinstance(c, LI.Progression) else IndexColumn(np.array(c, dtype=np.uint64)) for c in cols]
        got = lincomb_index(md.ring, tw, hc, cw, uses, n, n_evals=ne)
        for g, want in zip(got, expected(md, tw, cols, cw, uses, n)):
            assert np.array_equal(g, want), (name, K, J, M)
    tw, cw = draw(md, 1, 1, 1, n, seed=0xB300)
    col = IndexColumn(np.arange(n, dtype=np.uint64))
    for bad, msg in ((dict(uses=[0]), "empty mask"), (dict(uses=[0b1000]), "mask bit above"), (dict(uses=[0b101]), "column that no output uses"),
                     (dict(uses=[0b110]), "table that no output uses"), (dict(uses=[0b111], n_evals=[n + 1]), "exceeds n")):
        with pytest.raises(RingError, match=msg):
            lincomb_index(md.ring, tw, [col], cw, n=n, **bad)
    with pytest.raises(RingError, match="wraps"):
        lincomb_index(md.ring, tw, [IndexColumn(start=U64 - n + 1)], cw, [0b111], n)
    assert lincomb_index(md.ring, tw, [IndexColumn(col.values, n_evals=0)], cw, [0b111], 0)[0].size == 0


def test_the_pinned_vectors_on_the_device(torch_cuda):
    for c in KATS:
        md = model_for(c["ring"], c["log2_degree"])
        to_words = (lambda e: md.words([np.array(e, dtype=object)])) if c["form"] == "standard" else (lambda e: np.array(e, dtype=np.uint64))
        cat = lambda els: np.concatenate([to_words(e) for e in els]) if els else np.zeros(0, dtype=np.uint64)  # noqa: E731
        for key, s in c.items():
            if not isinstance(s, dict):
                continue
            tw = [cat(t) for t in s["tables"]]
            cols = [LI.Progression(d["start"]) if "start" in d else list(d["values"]) for d in s["columns"]]
            cw = cat([e for row in s["coef"] for e in row])
            run(torch_cuda, md, tw, cols, cw, s["uses"], s["n"], want=[cat(o) for o in s["outs"]])
