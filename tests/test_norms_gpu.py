"""GPU parity of sr_norm_batch_dev / sr_norm_batch (include/stark_rings_hip.h) for all six ring ids, bit for bit and word for word
against Python integers: tools/model_norms.py restates the reference's definition, oracle_lib.from_mont gives the standard form.
Every case compares the whole output; nothing is sampled."""
import ctypes
import os
import sys

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import model_norms as M  # noqa: E402

pytestmark = pytest.mark.gpu

LINF, L2SQ, BOTH = 1, 2, 3
# ring name, log2 D, the oracle's field name
RINGS = [("goldilocks", 10, "goldilocks"), ("babybear", 10, "babybear"), ("stark", 6, "stark"), ("goldilocks24", 0, "goldilocks"),
         ("babybear72", 0, "babybear"), ("frog16", 0, "frog")]
IDS = [r[0] for r in RINGS]
# one context per field family is enough where the ring's degree plays no part
FAMILIES = [RINGS[0], RINGS[1], RINGS[2], RINGS[5]]
FAM_IDS = [r[0] for r in FAMILIES]
_rings = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "the gpu-marked tests need a HIP device"
    yield torch
    for r in _rings.values():
        r.close()
    _rings.clear()


class Case:
    """a ring context and the field facts the model needs"""

    def __init__(self, name, k, field):
        from stark_rings_amd import CyclotomicRing

        if (name, k) not in _rings:
            _rings[(name, k)] = CyclotomicRing(name, k, device=0)
        self.ring = _rings[(name, k)]
        self.field = O.FIELD_ID[field]
        self.p = self.ring.modulus
        self.limbs = self.ring.limbs
        self.half = (self.p - 1) // 2
        self.lw, self.sw = (1, 3) if self.limbs == 1 else (4, 9)

    def wpg(self, which):
        return (self.lw if which & LINF else 0) + (self.sw if which & L2SQ else 0)

    def uniform(self, seed, n):
        return O.fill_uniform(self.field, seed, 0, n)

    def images(self, values):
        return O.to_mont(self.field, [v % self.p for v in values])

    def expect(self, arr, group, which):
        xs = O.from_mont(self.field, arr)
        return np.array(M.records(xs, self.p, group, which, self.limbs), dtype=np.uint64)

    def expect_values(self, linf, l2sq, which):
        return np.array((M.words(linf, self.lw) if which & LINF else []) + (M.words(l2sq, self.sw) if which & L2SQ else []), dtype=np.uint64)


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def run_dev(torch, c, t_coeffs, group, which, work=None):
    """the records of the device call on a device tensor of coefficients, as numpy words; the workspace is the plan's unless given"""
    n = t_coeffs.numel() // c.limbs
    g = group if group is not None else max(n, 1)
    wpg, need, launches = c.ring.norm_plan(n, g, which)
    assert wpg == c.wpg(which) and 1 <= launches <= 2
    out = torch.full((max(n // g, 1) * wpg,), -1, dtype=torch.int64, device="cuda")
    if work is None and need:
        work = torch.empty(need, dtype=torch.int64, device="cuda")
    c.ring.norm_batch_dev(out, t_coeffs, g, which, work)
    torch.cuda.synchronize()
    return host(out)


def check(torch, c, arr, group, which, what):
    got = run_dev(torch, c, dev(torch, arr), group, which)
    want = c.expect(arr, group if group is not None else max(arr.size // c.limbs, 1), which)
    assert got.shape == want.shape and np.array_equal(got, want), what


@pytest.mark.parametrize("name,k,field", RINGS, ids=IDS)
def test_uniform_data_every_group_shape_and_mask(torch_cuda, name, k, field):
    c = Case(name, k, field)
    d = c.ring.degree
    n = 9 * d if k else 432   # a multiple of 16, 24, 72, D and 3 D for every ring
    arr = c.uniform(0x4E01, n)
    t = dev(torch_cuda, arr)
    for group in (1, d, 3 * d, None, 24, 72, 16):
        g = group or n
        single = {}
        for which in (LINF, L2SQ, BOTH):
            got = run_dev(torch_cuda, c, t, group, which)
            assert np.array_equal(got, c.expect(arr, g, which)), (name, group, which)
            single[which] = got
        # one fused pass = the two single calls, record by record
        fused = single[BOTH].reshape(-1, c.lw + c.sw)
        assert np.array_equal(fused[:, :c.lw].ravel(), single[LINF]) and np.array_equal(fused[:, c.lw:].ravel(), single[L2SQ]), (name, group)
    # the convenience forms return Python integers
    xs = O.from_mont(c.field, arr)
    assert c.ring.norms_dev(t) == (M.linf(xs, c.p), M.l2sq(xs, c.p))
    assert c.ring.linf_norm_dev(t, d) == [M.linf(g, c.p) for g in M.groups(xs, d)]
    assert c.ring.l2_norm_squared_dev(t, d) == [M.l2sq(g, c.p) for g in M.groups(xs, d)]


@pytest.mark.parametrize("name,k,field", FAMILIES, ids=FAM_IDS)
def test_mid_size_slices_take_both_launches(torch_cuda, name, k, field):
    """3 * 2^18 coefficients (Stark: 3 * 2^14): whole slice (partial records and the second launch), wide groups with one workgroup each, wide
    groups with several, and narrow groups."""
    c = Case(name, k, field)
    n = 3 << (18 if c.limbs == 1 else 14)
    arr = c.uniform(0x4E02, n)
    assert c.ring.norm_plan(n, n, BOTH)[2] == 2
    for group in (None, 1 << 10, n // 3, 3 << 10, 48):
        check(torch_cuda, c, arr, group, BOTH, (name, group))
    check(torch_cuda, c, arr, None, LINF, name)
    check(torch_cuda, c, arr, None, L2SQ, name)


@pytest.mark.parametrize("name,k,field", FAMILIES, ids=FAM_IDS)
def test_odd_counts_single_coefficient_and_odd_word_offset(torch_cuda, name, k, field):
    c = Case(name, k, field)
    for n in (1, 2, 3, 63, 65, 1023, 1025, 4097, 4099, 8193):
        arr = c.uniform(0x4E03 + n, n)
        pool = torch_cuda.zeros((n + 1) * c.limbs, dtype=torch_cuda.int64, device="cuda")
        for off in (0, 1):   # in u64 words: the source starts on an even or an odd word (8-byte aligned only)
            view = pool[off:off + n * c.limbs]
            assert view.data_ptr() % 16 == 8 * off
            view.copy_(dev(torch_cuda, arr))
            for group in (None, 1):
                for which in (LINF, L2SQ, BOTH):
                    got = run_dev(torch_cuda, c, view, group, which)
                    assert np.array_equal(got, c.expect(arr, group or n, which)), (name, n, off, group, which)


@pytest.mark.parametrize("name,k,field", FAMILIES, ids=FAM_IDS)
def test_edge_coefficients(torch_cuda, name, k, field):
    c = Case(name, k, field)
    vals = [0, 1, c.p - 1, c.half, c.half + 1]
    arr = c.images(vals)
    got = run_dev(torch_cuda, c, dev(torch_cuda, arr), 1, BOTH).reshape(5, -1)
    for row, s in zip(got, (0, 1, 1, c.half, c.half)):
        assert np.array_equal(row, c.expect_values(s, s * s, BOTH)), (name, s)
    assert np.array_equal(run_dev(torch_cuda, c, dev(torch_cuda, arr), None, BOTH), c.expect_values(c.half, 2 + 2 * c.half**2, BOTH))
    assert np.array_equal(run_dev(torch_cuda, c, dev(torch_cuda, arr[:c.limbs]), None, BOTH), c.expect_values(0, 0, BOTH))


def carry_lengths(c):
    """the lengths at which a slice of all (p - 1) / 2 first carries into the next output word (checked with integers), one below, and 2^20"""
    h2 = c.half**2
    third = -(-(1 << 128) // h2)   # the sum first needs the third word
    if c.p == 2013265921:
        second = -(-(1 << 64) // h2)
        assert second == 19 and (1 << 20) * h2 < 1 << 128   # the third word stays zero
        return [second - 1, second, 1 << 20]
    assert third == (5 if c.p == 2**64 - 2**32 + 1 else 6)
    return [third - 1, third, 1 << 20]


@pytest.mark.parametrize("name,k,field", [RINGS[0], RINGS[1], RINGS[5]], ids=["goldilocks", "babybear", "frog16"])
def test_all_largest_magnitude_one_limb_carries(torch_cuda, name, k, field):
    c = Case(name, k, field)
    img = c.images([c.half])
    for n in carry_lengths(c):
        arr = np.tile(img, n)
        for group in (None,) + ((1 << 12, 64) if n == 1 << 20 else ()):
            g = group or n
            got = run_dev(torch_cuda, c, dev(torch_cuda, arr), group, BOTH).reshape(n // g, -1)
            want = c.expect_values(c.half, g * c.half**2, BOTH)
            assert all(np.array_equal(row, want) for row in got), (name, n, group)
        assert np.array_equal(run_dev(torch_cuda, c, dev(torch_cuda, arr), None, L2SQ), c.expect_values(0, n * c.half**2, L2SQ)), (name, n)
    # alternating (p - 1) / 2 and (p + 1) / 2: the same magnitudes from both signs
    arr = np.tile(c.images([c.half, c.half + 1]), 1 << 19)
    assert np.array_equal(run_dev(torch_cuda, c, dev(torch_cuda, arr), None, BOTH), c.expect_values(c.half, (1 << 20) * c.half**2, BOTH))


def test_all_largest_magnitude_stark_fills_nine_words(torch_cuda):
    c = Case(*RINGS[2])
    img = c.images([c.half])
    for n in (1, 3, 1 << 10, 1 << 16, (1 << 20) + 1):
        arr = np.tile(img, n)
        want = c.expect_values(c.half, n * c.half**2, BOTH)
        if n >= 1 << 16:
            assert want[-1] != 0   # the ninth word of l2sq is in use
        assert np.array_equal(run_dev(torch_cuda, c, dev(torch_cuda, arr), None, BOTH), want), n
    n = 1 << 16
    got = run_dev(torch_cuda, c, dev(torch_cuda, np.tile(img, n)), 1 << 11, BOTH).reshape(32, -1)
    assert all(np.array_equal(row, c.expect_values(c.half, (1 << 11) * c.half**2, BOTH)) for row in got)


@pytest.mark.parametrize("name,k,field", FAMILIES, ids=FAM_IDS)
def test_the_single_largest_coefficient_at_every_boundary(torch_cuda, name, k, field):
    """Small coefficients everywhere and (p - 1) / 2 at one index: index 0, the last, and both sides of every boundary the launcher has -- the
    pair a lane loads (2 i, 2 i + 1; one more with the one-coefficient head of an odd word offset), the wave (64 lanes), the workgroup (256
    lanes), the eight loads a lane has in flight, the span of a workgroup (a partial record) -- for a whole slice (wide, several partial
    records, both word offsets) and for every index of two narrow groups."""
    torch = torch_cuda
    c = Case(name, k, field)
    one = c.limbs == 1
    rng = np.random.RandomState(7)

    def sweep(n, group, positions, off):
        small = [int(v) for v in rng.randint(0, 1000, size=n)]
        signed = [v if v % 2 == 0 else -v for v in small]
        arr = c.images(signed)
        pool = torch.zeros((n + 1) * c.limbs, dtype=torch.int64, device="cuda")
        view = pool[off:off + n * c.limbs]
        view.copy_(dev(torch, arr))
        big = dev(torch, c.images([c.half]))
        g = group or n
        base = [sum(v * v for v in small[i:i + g]) for i in range(0, n, g)]
        base_max = [max(small[i:i + g]) for i in range(0, n, g)]
        for pos in positions:
            keep = view[pos * c.limbs:(pos + 1) * c.limbs].clone()
            view[pos * c.limbs:(pos + 1) * c.limbs] = big
            got = run_dev(torch, c, view, group, BOTH).reshape(n // g, -1)
            for gi in range(n // g):
                hit = gi == pos // g
                want = c.expect_values(c.half if hit else base_max[gi], base[gi] + (c.half**2 - small[pos]**2 if hit else 0), BOTH)
                assert np.array_equal(got[gi], want), (name, n, group, pos, gi, off)
            view[pos * c.limbs:(pos + 1) * c.limbs] = keep

    n = 20000 if one else 2500
    wpg, work, launches = c.ring.norm_plan(n, n, BOTH)
    parts = work // wpg
    assert launches == 2 and parts >= 3
    per_load = 2 if one else 1
    span = -(-(n // per_load) // parts) * per_load   # coefficients of one workgroup's span (norms.hpp: per = ceil(loads / parts))
    marks = {0, 1, 2, 3, n - 3, n - 2, n - 1}
    for b in (64 * per_load, 256 * per_load, 256 * per_load * (8 if one else 2)):
        marks |= {b - 2, b - 1, b, b + 1, b + 2}
    for j in range(1, parts):
        marks |= {j * span - 2, j * span - 1, j * span, j * span + 1, j * span + 2}
    marks = sorted(m for m in marks if 0 <= m < n)
    for off in ((0, 1) if one else (0,)):
        sweep(n, None, marks, off)
    sweep(144, 72, range(144), 0)
    sweep(96, 24, range(96), 1 if one else 0)


@pytest.mark.parametrize("name,k,field", FAMILIES, ids=FAM_IDS)
def test_workspace_contents_do_not_matter_and_a_short_one_is_refused(torch_cuda, name, k, field):
    torch = torch_cuda
    from stark_rings_amd import RingError, _lib

    c = Case(name, k, field)
    n = 3 << 15
    arr = c.uniform(0x4E05, n)
    t = dev(torch, arr)
    for group in (None, n // 3):
        wpg, need, launches = c.ring.norm_plan(n, group or n, BOTH)
        assert launches == 2 and need > 0
        want = c.expect(arr, group or n, BOTH)
        for poison in (0, -1, 0x0123456789ABCDEF):
            work = torch.full((need + 8,), poison, dtype=torch.int64, device="cuda")
            assert np.array_equal(run_dev(torch, c, t, group, BOTH, work), want), (name, group, poison)
            assert bool((work[need:] == poison).all()), "words beyond the plan's workspace were written"
        # twice on the same workspace: nothing is accumulated across calls
        work = torch.zeros(need, dtype=torch.int64, device="cuda")
        run_dev(torch, c, t, group, BOTH, work)
        assert np.array_equal(run_dev(torch, c, t, group, BOTH, work), want)
        out = torch.full((want.size,), 0x55, dtype=torch.int64, device="cuda")
        with pytest.raises(RingError, match="workspace too small"):
            c.ring.norm_batch_dev(out, t, group, BOTH, work[:need - 1])
        with pytest.raises(RingError, match="null buffer"):
            c.ring.norm_batch_dev(out, t, group, BOTH, None)
        torch.cuda.synchronize()
        assert bool((out == 0x55).all()), "a refused call wrote its output"


def test_every_refusal_names_its_reason(torch_cuda):
    torch = torch_cuda
    from stark_rings_amd import _lib

    c = Case(*RINGS[0])
    lib, ctx = c.ring._lib, c.ring._ctx
    pool = torch.zeros(1 << 16, dtype=torch.int64, device="cuda")
    base = pool.data_ptr()
    at = lambda words: ctypes.c_void_p(base + 8 * words)
    n = 1 << 14
    wpg, need, _ = c.ring.norm_plan(n, n, BOTH)
    coeffs, out, work = at(0), at(n), at(n + 64)
    cases = [
        ((None, coeffs, n, n, BOTH, work, need), "null buffer"),
        ((out, None, n, n, BOTH, work, need), "null buffer"),
        ((out, coeffs, n, n, BOTH, None, 0), "null buffer"),
        ((out, coeffs, n, n, 0, work, need), "which"),
        ((out, coeffs, n, n, 4, work, need), "which"),
        ((out, coeffs, n, 0, BOTH, work, need), "group must be at least 1"),
        ((out, coeffs, n, 24, BOTH, work, need), "group must divide"),
        ((out, coeffs, 0, 1, LINF, work, need), "empty slice"),
        ((out, coeffs, 0, 1, BOTH, work, need), "empty slice"),
        ((out, coeffs, n, n, BOTH, work, need - 1), "workspace too small"),
        ((at(n - 1), coeffs, n, n, BOTH, work, need), "d_out overlaps d_coeffs"),
        ((at(8), coeffs, n, 1, LINF, work, need), "d_out overlaps d_coeffs"),
        ((at(n + 64 + need - 1), coeffs, n, n, BOTH, work, need), "d_out overlaps d_work"),
        ((out, coeffs, n, n, BOTH, at(n - 20), need), "d_coeffs overlaps d_work"),
    ]
    for args, msg in cases:
        assert lib.sr_norm_batch_dev(ctx, *args, None) == 1, args
        assert msg in _lib.last_error(), (args, _lib.last_error())
    torch.cuda.synchronize()
    assert not bool(pool.any()), "a refused call wrote device memory"
    # the host-pointer form refuses the same arguments
    a = np.zeros(64, dtype=np.uint64)
    p = a.ctypes.data_as(_lib.u64p)
    for args, msg in (((None, p, 48, 24, BOTH), "null buffer"), ((p, None, 48, 24, BOTH), "null buffer"), ((p, p, 48, 24, 8), "which"),
                      ((p, p, 48, 0, BOTH), "group must be at least 1"), ((p, p, 48, 36, BOTH), "group must divide"),
                      ((p, p, 0, 1, LINF), "empty slice")):
        assert lib.sr_norm_batch(ctx, *args) == 1, args
        assert msg in _lib.last_error(), (args, _lib.last_error())
    # the empty slice has a squared l2 norm: zero, on both paths
    assert c.ring.l2_norm_squared(np.zeros(0, dtype=np.uint64)) == 0
    assert c.ring.l2_norm_squared_dev(torch.zeros(0, dtype=torch.int64, device="cuda")) == 0


@pytest.mark.parametrize("name,k,field", FAMILIES, ids=FAM_IDS)
def test_capturable_on_a_fresh_context_and_replayed_on_new_data(torch_cuda, name, k, field):
    """Captured on a non-default stream by a context that has never run anything, with a caller-supplied (poisoned) workspace; replayed after
    the input changed.  Whole slice (two launches) and narrow groups (one) in the same graph, one after the other."""
    torch = torch_cuda
    from stark_rings_amd import CyclotomicRing

    c = Case(name, k, field)
    fresh = CyclotomicRing(name, k, device=0)
    n = 3 << 14
    t = dev(torch, c.uniform(0x4E06, n))
    wpg, need, launches = fresh.norm_plan(n, n, BOTH)
    assert launches == 2
    work = torch.full((need,), -1, dtype=torch.int64, device="cuda")
    out_whole = torch.zeros(wpg, dtype=torch.int64, device="cuda")
    out_narrow = torch.zeros(n // 24 * wpg, dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        fresh.norm_batch_dev(out_whole, t, None, BOTH, work, stream=torch.cuda.current_stream())
        fresh.norm_batch_dev(out_narrow, t, 24, BOTH, None, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    for seed in (0x4E07, 0x4E08):
        arr = c.uniform(seed, n)
        t.copy_(dev(torch, arr))
        out_whole.zero_()
        out_narrow.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(host(out_whole), c.expect(arr, n, BOTH)), (name, seed)
        assert np.array_equal(host(out_narrow), c.expect(arr, 24, BOTH)), (name, seed)
    del g
    fresh.close()


@pytest.mark.parametrize("name,k,field", FAMILIES, ids=FAM_IDS)
def test_host_pointer_call_streams_in_chunks_and_groups_straddle_them(torch_cuda, name, k, field):
    """SR_HOST_CHUNK_MB = 1 (sr_plan.host_chunk_mb): 5.25 chunks of 1 MiB; groups of a seventh of the slice begin and end inside chunks, the
    whole slice spans all of them, and 48-coefficient groups fill every chunk with whole groups (one straddling where 48 does not divide the
    chunk).  Equal to the device call and to the model."""
    torch = torch_cuda
    from stark_rings_amd import CyclotomicRing, _lib

    c = Case(name, k, field)
    plan = _lib.plan_from_env(c.ring.ring)
    plan.host_chunk_mb = 1
    chunked = CyclotomicRing(name, k, device=0, plan=plan)
    chunk = (1 << 20) // (8 * c.limbs)
    n = 21 * chunk // 4
    assert n > 2 * chunk and -(-n // chunk) >= 3 and (n // 7) % chunk != 0 and chunk % 48 != 0
    arr = c.uniform(0x4E09, n)
    xs = O.from_mont(c.field, arr)
    t = dev(torch, arr)
    for group in (n // 7, None, 48):
        g = group or n
        want = [(M.linf(v, c.p), M.l2sq(v, c.p)) for v in M.groups(xs, g)]
        got = chunked.norms(arr, group)
        assert (got if group else [got]) == want, (name, group)
        dev_got = c.ring.norms_dev(t, group)
        assert (dev_got if group else [dev_got]) == want, (name, group)
    assert chunked.linf_norm(arr) == max(w[0] for w in want) and chunked.l2_norm_squared(arr) == sum(w[1] for w in want)
    assert chunked.linf_norm(arr, n // 7) == [M.linf(v, c.p) for v in M.groups(xs, n // 7)]
    # a slice small enough for one staging copy takes the same path's short form
    assert chunked.norms(arr[:1000 * c.limbs]) == (M.linf(xs[:1000], c.p), M.l2sq(xs[:1000], c.p))
    chunked.close()


@pytest.mark.parametrize("name,k,field", RINGS, ids=IDS)
@pytest.mark.parametrize("basis", [2, 1 << 16, 10])
def test_digits_of_the_balanced_decomposition_are_short(torch_cuda, name, k, field, basis):
    """A property of what already exists, nothing of the reference is read: every digit of sr_decompose_balanced_batch is at most b / 2 in
    absolute value (the linf norm on the device says so for each digit element), and the digits recompose to the input."""
    torch = torch_cuda
    c = Case(name, k, field)
    d, w = c.ring.degree, c.ring.words_per_elem
    batch = 3
    digits_needed = 1
    while basis**digits_needed <= 2 * c.p:
        digits_needed += 1
    a = dev(torch, c.uniform(0x4E0A, batch * d))
    digits = torch.empty(batch * digits_needed * w, dtype=torch.int64, device="cuda")
    c.ring.gadget_decompose_dev(digits, a, basis, digits_needed)
    assert c.ring.decompose_overflow_count() == 0
    per_element = c.ring.linf_norm_dev(digits, d)
    assert len(per_element) == batch * digits_needed and max(per_element) <= basis // 2, (name, basis, max(per_element))
    assert c.ring.linf_norm_dev(digits) == max(per_element)
    xs = O.from_mont(c.field, host(digits))
    assert per_element == [M.linf(g, c.p) for g in M.groups(xs, d)]
    assert c.ring.l2_norm_squared_dev(digits) == M.l2sq(xs, c.p)
    back = torch.empty_like(a)
    c.ring.gadget_recompose_dev(back, digits, basis, digits_needed)
    torch.cuda.synchronize()
    assert np.array_equal(host(back), host(a))
