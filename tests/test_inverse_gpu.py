"""GPU parity of the batch inversion (sr_inverse_batch[_dev], sr_inverse_zero_count) for all six ring ids.  Every comparison is
bit-exact and no expected value comes from the code under test:
  * power-of-two rings: the inverse of the standard-form Python integer (pow(x, -1, p), which is pow(x, p - 2, p) by another algorithm)
    times the numerator, converted back to the memory image;
  * goldilocks24 / babybear72 / frog16: every device output y satisfies mul(y, den) == num on the non-zero slots with the Fq3 / Fq9 / Fq4
    products of oracle/pyref.py on standard-form integers -- in a field that determines y.
Zero slots come back zero and are counted."""
import ctypes
import random

import numpy as np
import pytest

import oracle_lib as O
import pyref as P
from stark_rings_amd import inverse_dev
from test_host_fields import FIELD_EDGES
from test_mle_gpu import POISON, dev, host, model_for, ring_for

pytestmark = pytest.mark.gpu

CASES = [("goldilocks", 0), ("goldilocks", 6), ("goldilocks", 16), ("babybear", 5), ("stark", 4), ("stark", 12), ("goldilocks24", 0),
         ("babybear72", 0), ("frog16", 0)]
IDS = ["%s-%d" % c for c in CASES]
BIG = {("goldilocks", 16): 3, ("stark", 12): 2}   # the cap on n, unless the chunk forces more
SLOT = {"goldilocks24": ("goldilocks", 3, lambda x, y: P.fq3_mul("goldilocks", x, y)), "babybear72": ("babybear", 9, P.fq9_mul),
        "frog16": ("frog", 4, P.fq4_mul)}
GUARD = 5   # words before and behind every buffer


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def edges(name):
    base = SLOT[name][0] if name in SLOT else name
    p = P.PRIMES[base][0]
    vals = [v for v in FIELD_EDGES[base] if v] + [(p + 1) // 2]
    if base == "goldilocks":
        vals += [2**32 - 1, 2**32, 2**64 - 2**32]
    return vals


def units_of(m):
    """(units of an element, words of a unit): coefficients of a power-of-two ring, slots of the reference's own rings"""
    if m.pow2:
        return m.ring.degree, m.ring.limbs
    sw = SLOT[m.name][1]
    return m.w // sw, sw


def table(m, seed, n):
    """n elements: uniform, with the field's edge values sprinkled in; never a zero unit (those are planted)"""
    words = m.uniform(seed, n)
    rng = random.Random(seed)
    ev = edges(m.name)
    L = m.ring.limbs
    n_coeffs = words.size // L
    for _ in range(min(n_coeffs, 64)):
        at = rng.randrange(n_coeffs)
        words[at * L:(at + 1) * L] = O.to_mont(m.F, [rng.choice(ev)])
    nu, uw = units_of(m)
    flat = words.reshape(n * nu, uw)
    dead = ~flat.any(axis=1)
    flat[dead, 0] = O.to_mont(m.F, [1])[0]
    return words


def plant(m, words, positions):
    """zero the units (element, unit)"""
    nu, uw = units_of(m)
    flat = words.reshape(-1, uw)
    for e, u in positions:
        flat[e * nu + u] = 0
    return words


def check(m, got, den, num):
    """got == num / den on every non-zero unit, zero on the others"""
    nu, uw = units_of(m)
    n = den.size // m.w
    g, d = got.reshape(n * nu, uw), den.reshape(n * nu, uw)
    dead = ~d.any(axis=1)
    assert not g[dead].any(), "a zero unit did not come back as zero"
    p = m.p
    if m.pow2:
        xs = O.from_mont(m.F, den)
        ns = O.from_mont(m.F, num) if num is not None else None
        want = [0 if x == 0 else pow(x, -1, p) * (ns[i] if ns is not None else 1) % p for i, x in enumerate(xs)]
        assert np.array_equal(got, O.to_mont(m.F, want))
        return
    base, sw, mul = SLOT[m.name]
    ys, xs = O.from_mont(m.F, got), O.from_mont(m.F, den)
    ns = O.from_mont(m.F, num) if num is not None else None
    one = [1] + [0] * (sw - 1)
    assert all(y < p for y in ys), "an output word is not canonical"
    for s in range(n * nu):
        if dead[s]:
            continue
        want = ns[s * sw:(s + 1) * sw] if ns is not None else one
        assert mul(ys[s * sw:(s + 1) * sw], xs[s * sw:(s + 1) * sw]) == want, (m.name, s)


class Placed:
    """a device buffer with GUARD poison words before and behind it; odd: it starts 8 bytes past a 16-byte boundary"""

    def __init__(self, torch, words, odd):
        off = GUARD + (1 - GUARD % 2 if odd else GUARD % 2)   # odd offset: an odd number of words from the (256-byte aligned) base
        self.off, self.n = off, words.size
        raw = np.full(off + words.size + GUARD, POISON, dtype=np.uint64)
        raw[off:off + words.size] = words
        self.raw = dev(torch, raw)
        self.t = self.raw[off:off + words.size]
        assert (self.t.data_ptr() % 16 == 8) == bool(odd)

    def guards_intact(self):
        r = host(self.raw)
        return bool((r[:self.off] == POISON).all() and (r[self.off + self.n:] == POISON).all())


def sizes(name, k, c):
    if (name, k) in BIG:
        return sorted({1, BIG[(name, k)], c + 1})
    out = {1, max(c - 1, 1), c, c + 1, 3 * c + 1}
    if k <= 6:
        out.add(37 * c + 5)   # several lane-groups in a workgroup and a partial last wave
    return sorted(out)


@pytest.mark.parametrize("has_num", (False, True), ids=("inverse", "divide"))
@pytest.mark.parametrize("name,k", CASES, ids=IDS)
def test_every_size_around_the_chunk_matches_the_integers(torch_cuda, name, k, has_num):
    torch = torch_cuda
    m = model_for(name, k)
    work, launches, c = m.ring.inverse_plan(1, has_num)
    assert work == 0 and launches == 1 and c >= 1
    m.ring.inverse_zero_count()   # whatever an earlier test left is cleared by this read
    for j, n in enumerate(sizes(name, k, c)):
        den, num = table(m, 0x1A00 + j, n), (table(m, 0x1B00 + j, n) if has_num else None)
        out = Placed(torch, np.full(n * m.w, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64), odd=False)
        t_den, t_num = Placed(torch, den, False), (Placed(torch, num, False) if has_num else None)
        inverse_dev(m.ring, out.t, t_den.t, t_num.t if has_num else None)
        torch.cuda.synchronize()
        check(m, host(out.t), den, num)
        assert out.guards_intact(), (name, n)
        assert np.array_equal(host(t_den.t), den), "the denominators were written"
        assert m.ring.inverse_zero_count() == 0, (name, n)


@pytest.mark.parametrize("has_num", (False, True), ids=("inverse", "divide"))
@pytest.mark.parametrize("name,k", CASES, ids=IDS)
def test_planted_zeros_come_back_zero_and_are_counted(torch_cuda, name, k, has_num):
    torch = torch_cuda
    m = model_for(name, k)
    c = m.ring.inverse_plan(1, has_num)[2]
    nu, uw = units_of(m)
    n = BIG.get((name, k), 0) and c + 1 or 3 * c + 1
    first = c if n > 2 * c else 0                       # the chunk the zeros go into: the second where there is one
    last = min(first + c, n) - 1
    rng = random.Random("zeros %s %d" % (name, k))
    u = [rng.randrange(nu) for _ in range(4)]
    planted = {(first, u[0]), ((first + last) // 2, u[1]), (last, u[2])}          # head, middle, tail of a lane's chunk
    whole = 2 * c if n > 3 * c else 0                                          # a lane whose whole chunk is zero
    planted |= {(e, u[3]) for e in range(whole, min(whole + c, n))}
    m.ring.inverse_zero_count()
    den = plant(m, table(m, 0x2A00, n), planted)
    num = table(m, 0x2B00, n) if has_num else None
    out = Placed(torch, np.full(n * m.w, 0x77, dtype=np.uint64), odd=False)
    inverse_dev(m.ring, out.t, dev(torch, den), dev(torch, num) if has_num else None)
    torch.cuda.synchronize()
    check(m, host(out.t), den, num)
    assert out.guards_intact()
    assert m.ring.inverse_zero_count() == len(planted)
    assert m.ring.inverse_zero_count() == 0, "the read did not clear the count"
    # an all-zero table: every unit counted, every output zero
    n0 = min(n, c + 1)
    z = dev(torch, np.zeros(n0 * m.w, dtype=np.uint64))
    o = dev(torch, np.full(n0 * m.w, 0x33, dtype=np.uint64))
    inverse_dev(m.ring, o, z, dev(torch, num[:n0 * m.w]) if has_num else None)
    torch.cuda.synchronize()
    assert not host(o).any()
    assert m.ring.inverse_zero_count() == n0 * nu


@pytest.mark.parametrize("name,k", CASES, ids=IDS)
def test_odd_pointers_poison_behind_the_inputs_and_in_place(torch_cuda, name, k):
    """each buffer once at an odd 8-byte offset (the one-coefficient lane of the one-limb fields), poison around every input and guards
    around the output; then in place on den and in place on num"""
    torch = torch_cuda
    m = model_for(name, k)
    c = m.ring.inverse_plan(1, True)[2]
    n = 2 if (name, k) in BIG else 3 * c + 1
    den, num = table(m, 0x3A00, n), table(m, 0x3B00, n)
    m.ring.inverse_zero_count()
    for odd in ((True, False, False), (False, True, False), (False, False, True), (True, True, True)):
        out = Placed(torch, np.full(n * m.w, 0x11, dtype=np.uint64), odd[0])
        t_den, t_num = Placed(torch, den, odd[1]), Placed(torch, num, odd[2])
        inverse_dev(m.ring, out.t, t_den.t, t_num.t)
        torch.cuda.synchronize()
        check(m, host(out.t), den, num)
        assert out.guards_intact() and t_den.guards_intact() and t_num.guards_intact(), (name, odd)
        out2 = Placed(torch, np.full(n * m.w, 0x11, dtype=np.uint64), odd[0])
        inverse_dev(m.ring, out2.t, t_den.t)
        torch.cuda.synchronize()
        check(m, host(out2.t), den, None)
        assert out2.guards_intact()
    for odd in (False, True):
        a, b = Placed(torch, den, odd), Placed(torch, num, odd)
        inverse_dev(m.ring, a.t, a.t, b.t)                    # in place on den
        torch.cuda.synchronize()
        check(m, host(a.t), den, num)
        assert a.guards_intact() and np.array_equal(host(b.t), num)
        a = Placed(torch, den, odd)
        inverse_dev(m.ring, b.t, a.t, b.t)                    # in place on num
        torch.cuda.synchronize()
        check(m, host(b.t), den, num)
        assert b.guards_intact() and np.array_equal(host(a.t), den)
        inverse_dev(m.ring, a.t, a.t)                         # in place, no numerator
        torch.cuda.synchronize()
        check(m, host(a.t), den, None)
    assert m.ring.inverse_zero_count() == 0


@pytest.mark.parametrize("name,k", [("goldilocks", 6), ("goldilocks24", 0)], ids=["goldilocks-6", "goldilocks24-0"])
def test_host_pointer_form_streams_in_chunks(torch_cuda, name, k):
    """SR_HOST_CHUNK_MB = 1 (sr_plan.host_chunk_mb): more than two staging chunks and a ragged last one whose length is no multiple of the
    lane's chunk; equal to the device call (checked against the integers above) and, for the power-of-two ring, to the integers"""
    torch = torch_cuda
    from stark_rings_amd import CyclotomicRing, _lib

    m = model_for(name, k)
    plan = _lib.plan_from_env(m.ring.ring)
    plan.host_chunk_mb = 1
    chunked = CyclotomicRing(name, k, device=0, plan=plan)
    chunk = (1 << 20) // (8 * m.w)
    n = 2 * chunk + chunk // 3 + 3
    assert n > 2 * chunk
    nu, uw = units_of(m)
    den = plant(m, table(m, 0x4A00, n), {(0, 0), (chunk, nu - 1), (n - 1, 0)})
    num = table(m, 0x4B00, n)
    for nm in (None, num):
        got = chunked.inverse(den, nm)
        assert chunked.inverse_zero_count() == 3
        o = dev(torch, np.zeros(n * m.w, dtype=np.uint64))
        inverse_dev(m.ring, o, dev(torch, den), dev(torch, nm) if nm is not None else None)
        torch.cuda.synchronize()
        assert m.ring.inverse_zero_count() == 3
        assert np.array_equal(got, host(o)), (name, nm is not None)
        if m.pow2:
            check(m, got, den, nm)
    small = chunked.inverse(den[:5 * m.w], num[:5 * m.w])      # one staging copy: the same path's short form
    check(m, small, den[:5 * m.w], num[:5 * m.w])
    assert chunked.inverse_zero_count() == 1
    assert chunked.inverse(np.zeros(0, dtype=np.uint64)).size == 0     # n == 0 succeeds
    empty = torch.zeros(0, dtype=torch.int64, device="cuda")
    some = torch.zeros(m.w, dtype=torch.int64, device="cuda")
    inverse_dev(m.ring, some, some, n=0)
    assert chunked._lib.sr_inverse_batch_dev(chunked._ctx, some.data_ptr(), None, some.data_ptr(), 0, None, 0, None) == 0
    torch.cuda.synchronize()
    assert not host(some).any() and empty.numel() == 0 and chunked.inverse_zero_count() == 0
    chunked.close()


@pytest.mark.parametrize("name,k", [("goldilocks", 6), ("stark", 4), ("goldilocks24", 0), ("frog16", 0)],
                         ids=["goldilocks-6", "stark-4", "goldilocks24-0", "frog16-0"])
def test_the_call_is_capturable_on_a_fresh_context(torch_cuda, name, k):
    """Captured into a graph on a non-default stream on a context that has never run anything eagerly; replayed twice on new values in the
    same buffers.  The count of the replays is read afterwards."""
    torch = torch_cuda
    from stark_rings_amd import CyclotomicRing

    m = model_for(name, k)
    fresh = CyclotomicRing(name, k, device=0)
    c = fresh.inverse_plan(1, True)[2]
    n = 5 * c + 1
    t_den = dev(torch, table(m, 0x5A00, n))
    t_num = dev(torch, table(m, 0x5B00, n))
    out = torch.zeros(n * m.w, dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        inverse_dev(fresh, out, t_den, t_num, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    for seed in (0x5C00, 0x5D00):
        den = plant(m, table(m, seed, n), {(1, 0)})
        t_den.copy_(dev(torch, den))
        want = torch.zeros_like(out)
        inverse_dev(m.ring, want, t_den, t_num)     # eager, on the long-lived context
        torch.cuda.synchronize()
        out.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(host(out), host(want)), (name, seed)
    check(m, host(out), den, host(t_num))
    assert fresh.inverse_zero_count() == 2
    m.ring.inverse_zero_count()
    del g
    fresh.close()


def test_every_refusal_names_its_reason(torch_cuda):
    torch = torch_cuda
    from stark_rings_amd import RingError, _lib

    ring = ring_for("goldilocks", 6)
    lib, ctx, w = ring._lib, ring._ctx, ring.words_per_elem
    pool = torch.ones(64 * w, dtype=torch.int64, device="cuda")
    base, E = pool.data_ptr(), w * 8
    out, num, den = base, base + 16 * E, base + 32 * E

    def call(o, nm, d, n, wk=None, wn=0):
        rc = lib.sr_inverse_batch_dev(ctx, o, nm, d, n, wk, wn, None)
        return rc, _lib.last_error()

    assert call(out, num, den, 8)[0] == 0
    assert call(den, num, den, 8)[0] == 0 and call(num, num, den, 8)[0] == 0     # in place on either input
    for args, msg in (
        ((None, num, den, 8), "null output buffer"),
        ((out, num, None, 8), "null denominators"),
        ((den + E, num, den, 8), "d_out overlaps d_den"),
        ((den - E, None, den, 8), "d_out overlaps d_den"),
        ((num + 7 * E, num, den, 8), "d_out overlaps d_num"),
        ((out, num, den, 1 << 46), "element count too large"),
    ):
        rc, err = call(*args)
        assert rc == 1 and msg in err, (args, rc, err)
    assert lib.sr_inverse_batch(None, None, None, None, 0) == 1 and "null context" in _lib.last_error()
    cnt = ctypes.c_ulonglong()
    assert lib.sr_inverse_zero_count(ctx, None, None) == 1 and "null buffer" in _lib.last_error()
    assert lib.sr_inverse_zero_count(ctx, ctypes.byref(cnt), None) == 0
    torch.cuda.synchronize()
    with pytest.raises(RingError, match="fewer than n elements"):
        inverse_dev(ring, pool[:3 * w], pool[:4 * w])
    with pytest.raises(RingError, match="num holds fewer"):
        inverse_dev(ring, pool[:4 * w], pool[4 * w:8 * w], pool[8 * w:11 * w])
    with pytest.raises(RingError, match="differ in length"):
        ring.inverse(np.ones(2 * w, dtype=np.uint64), np.ones(w, dtype=np.uint64))


def test_the_slot_wise_inverse_is_the_inverse_in_the_ring(torch_cuda):
    """("goldilocks", 6): for a in coefficient form, ring.mul(a, icrt(inverse(crt(a)))) is the ring's one"""
    m = model_for("goldilocks", 6)
    ring = m.ring
    n = 5
    a = m.uniform(0x6A00, n)
    a_ntt = ring.elementwise_crt(a.copy())
    assert a_ntt.reshape(-1).all(), "a random element with a zero slot: pick another seed"
    inv = ring.elementwise_icrt(ring.inverse(a_ntt))
    assert ring.inverse_zero_count() == 0
    prod = ring.mul(a.copy(), inv)
    one = np.zeros(n * m.w, dtype=np.uint64)
    one[::ring.degree] = O.to_mont(m.F, [1])[0]
    assert np.array_equal(prod, one)
