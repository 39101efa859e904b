"""GPU parity of the symmetric-matrix calls (sr_gram_ntt[_dev], sr_symm_recompose[_dev]) for all six ring ids.  Every comparison is
bit-exact.  Expected values come from tools/model_symmetric.py, the line-by-line restatement of symmetric_matrix.rs:17-62 and
balanced_decomposition/mod.rs:358-386 (pinned against full dense matrices by tests/test_symm_host.py): on standard-form Python
integers for the power-of-two rings, on the oracle's Fq3 / Fq9 / Fq4 slot products plus integer addition for the reference's own
rings.  The independent device path for the Gram matrix is the lower triangle of sr_matmul_ntt_dev(A, A^T), A^T built on the host."""
import ctypes
import os
import sys

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import model_symmetric as M  # noqa: E402

pytestmark = pytest.mark.gpu
RINGS = [("goldilocks", 6), ("goldilocks", 16), ("babybear", 5), ("stark", 4), ("goldilocks24", 0), ("babybear72", 0), ("frog16", 0)]
IDS = ["%s-%d" % r for r in RINGS]
SLOT_RINGS = [r for r in RINGS if r[1] == 0]
BASE = {"goldilocks24": "goldilocks", "babybear72": "babybear", "frog16": "frog"}
SLOT_MUL = {"goldilocks24": "sro_g24_ntt_mul", "babybear72": "sro_bb72_ntt_mul", "frog16": "sro_frog16_ntt_mul"}
POISON = 0xDEADBEEFCAFEF00D  # not canonical in any of the fields: a kernel that read it would show it
RECOMPOSE_SHAPES = [(1, 1), (3, 2), (2, 3), (4, 1)]


def gram_shapes(k):
    """n = 9 is one past BabyBear's 8-row block, 5 crosses every other block; at D = 2^16 one small shape"""
    return [(3, 2)] if k == 16 else [(n, m) for n in (1, 2, 5, 9) for m in (0, 1, 3, 17)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


_rings, _models = {}, {}


def ring_for(name, k):
    from stark_rings_amd import CyclotomicRing

    if (name, k) not in _rings:
        _rings[(name, k)] = CyclotomicRing(name, k, device=0)
    return _rings[(name, k)]


class Model:
    """the restatement's element type and operations for one ring"""

    def __init__(self, name, k):
        self.name, self.k = name, k
        self.ring = ring_for(name, k)
        self.F = O.FIELD_ID[BASE.get(name, name)]
        self.w = self.ring.words_per_elem
        self.pow2 = name not in SLOT_MUL
        p = self.ring.modulus
        if self.pow2:  # elements: numpy object arrays of D standard-form integers
            self.add = lambda a, b: (a + b) % p
            self.mul = lambda a, b: (a * b) % p
            self.zero = np.array([0] * self.ring.degree, dtype=object)
        else:          # elements: uint64 memory images; the product is the oracle's slot product
            fn = SLOT_MUL[name]
            self.add = lambda a, b: ((a.astype(object) + b.astype(object)) % p).astype(np.uint64)
            self.mul = lambda a, b: O.small(fn, a, b)
            self.zero = np.zeros(self.w, dtype=np.uint64)

    def elems(self, words):
        words = np.ascontiguousarray(words, dtype=np.uint64)
        if self.pow2:
            ints = np.array(O.from_mont(self.F, words), dtype=object) if words.size else np.zeros(0, dtype=object)
            return [ints[i * self.ring.degree:(i + 1) * self.ring.degree] for i in range(words.size // self.w)]
        return [words[i * self.w:(i + 1) * self.w].copy() for i in range(words.size // self.w)]

    def words(self, elems):
        if not elems:
            return np.zeros(0, dtype=np.uint64)
        if self.pow2:
            return O.to_mont(self.F, [int(x) for e in elems for x in e])
        return np.concatenate(elems)

    def uniform(self, seed, n_elems):
        return O.fill_uniform(self.F, seed, 0, n_elems * self.ring.degree)

    def gram(self, a, n, m):
        return self.words(M.gram(self.elems(a), n, m, self.add, self.mul, self.zero).packed())

    def recompose(self, mat, n, d, powers):
        sym = M.SymmetricMatrix.from_packed(n * d, self.elems(mat))
        return self.words(M.recompose_left_right_symmetric_matrix(sym, self.elems(powers), self.add, self.mul, self.zero).packed())


def model_for(name, k):
    if (name, k) not in _models:
        _models[(name, k)] = Model(name, k)
    return _models[(name, k)]


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def poison(torch, n_words):
    return dev(torch, np.full(n_words, POISON, dtype=np.uint64))


def packed(n):
    return n * (n + 1) // 2


def gram_dev(torch, ring, t_a, n, m, extra_work=0, stream=None):
    """the _dev call on a poisoned output with one poisoned element behind it and a poisoned workspace of the planned size (plus
    extra_work elements); returns the packed result after checking the guard element"""
    w = ring.words_per_elem
    buf = poison(torch, (packed(n) + 1) * w)
    need, launches = ring.gram_plan(n, m)
    work = poison(torch, (need + extra_work) * w) if need + extra_work else None
    ring.gram_ntt_dev(buf[:packed(n) * w], t_a, n, m, work, stream)
    torch.cuda.synchronize()
    got = host(buf)
    assert (got[packed(n) * w:] == POISON).all(), "the element behind the output was written"
    return got[:packed(n) * w], launches


def recompose_dev(torch, ring, t_mat, n, d, t_powers, extra_work=0):
    w = ring.words_per_elem
    buf = poison(torch, (packed(n) + 1) * w)
    need, launches = ring.symm_recompose_plan(n, d)
    assert (need, launches) == (d * d, 2)
    work = poison(torch, (need + extra_work) * w)
    ring.symm_recompose_dev(buf[:packed(n) * w], t_mat, n, d, t_powers, work)
    torch.cuda.synchronize()
    got = host(buf)
    assert (got[packed(n) * w:] == POISON).all(), "the element behind the output was written"
    return got[:packed(n) * w]


def lower_triangle_of_a_at(torch, ring, a, n, m):
    """sr_matmul_ntt_dev(A, A^T), A^T built on the host, then the entries (i, j), j <= i, in packed order"""
    w = ring.words_per_elem
    at = np.ascontiguousarray(a.reshape(n, m, w).transpose(1, 0, 2)).reshape(-1)
    y = torch.zeros(n * n * w, dtype=torch.int64, device="cuda")
    ring.matmul_ntt_dev(y, dev(torch, a), dev(torch, at), n, m, n)
    torch.cuda.synchronize()
    full = host(y).reshape(n, n, w)
    return np.concatenate([full[i, j] for i in range(n) for j in range(i + 1)])


@pytest.mark.parametrize("name,k", RINGS, ids=IDS)
def test_gram_matches_the_restatement_and_the_matrix_product(torch_cuda, name, k):
    torch = torch_cuda
    m_ = model_for(name, k)
    ring, w = m_.ring, m_.w
    for n, m in gram_shapes(k):
        a = m_.uniform(0x1000 + 37 * n + m, n * m)
        t_a = dev(torch, a) if m else torch.zeros(0, dtype=torch.int64, device="cuda")
        got, _ = gram_dev(torch, ring, t_a, n, m)
        where = "%s n %d m %d" % (name, n, m)
        want = m_.gram(a, n, m)
        print("%s: %d of %d words differ from the restatement" % (where, int((got != want).sum()), want.size))
        assert np.array_equal(got, want), where
        if m == 0:
            assert not got.any(), where
        else:
            assert np.array_equal(got, lower_triangle_of_a_at(torch, ring, a, n, m)), where + " against sr_matmul_ntt_dev(A, A^T)"
            assert np.array_equal(host(t_a), a), "the input was written"
        assert np.array_equal(ring.gram_ntt(a, n, m), want), where + " host-pointer form"
    # n == 0 writes nothing
    guard = poison(torch, w)
    ring.gram_ntt_dev(guard[:0], guard[:0], 0, 5)
    torch.cuda.synchronize()
    assert (host(guard) == POISON).all()
    assert ring.gram_ntt(np.zeros(0, dtype=np.uint64), 0, 5).size == 0


@pytest.mark.parametrize("name,k", RINGS, ids=IDS)
def test_gram_split_path(torch_cuda, name, k):
    """n = 2: the first power of two m <= 2^12 for which sr_gram_plan reports two launches; a slot ring must have one"""
    torch = torch_cuda
    m_ = model_for(name, k)
    ring, n = m_.ring, 2
    split = [m for m in (1 << e for e in range(13)) if ring.gram_plan(n, m)[1] == 2]
    if not split:
        assert (name, k) not in SLOT_RINGS, "sr_gram_plan never splits n = 2 on a slot ring"
        return
    m = split[0]
    need, _ = ring.gram_plan(n, m)
    assert need >= 2 * packed(n) and need % packed(n) == 0
    a = m_.uniform(0x2000 + k, n * m)
    t_a = dev(torch, a)
    want = lower_triangle_of_a_at(torch, ring, a, n, m)
    if k != 16:
        assert np.array_equal(m_.gram(a, n, m), want), "the restatement against sr_matmul_ntt_dev(A, A^T)"
    for extra in (0, 5):
        got, launches = gram_dev(torch, ring, t_a, n, m, extra_work=extra)
        assert launches == 2
        assert np.array_equal(got, want), "%s m %d, workspace + %d elements" % (name, m, extra)
    assert np.array_equal(ring.gram_ntt(a, n, m), want), "host-pointer form"
    # an odd m just above: the last span is shorter than the others
    m2 = m + 3
    if k != 16 and ring.gram_plan(n, m2)[1] == 2:
        a2 = m_.uniform(0x2100 + k, n * m2)
        got, _ = gram_dev(torch, ring, dev(torch, a2), n, m2)
        assert np.array_equal(got, lower_triangle_of_a_at(torch, ring, a2, n, m2)), "%s m %d" % (name, m2)


@pytest.mark.parametrize("name,k", RINGS, ids=IDS)
def test_recompose_matches_the_restatement(torch_cuda, name, k):
    torch = torch_cuda
    m_ = model_for(name, k)
    ring = m_.ring
    for n, d in RECOMPOSE_SHAPES:
        mat = m_.uniform(0x3000 + 10 * n + d, packed(n * d))
        powers = m_.uniform(0x3100 + 10 * n + d, d)
        t_mat, t_powers = dev(torch, mat), dev(torch, powers)
        want = m_.recompose(mat, n, d, powers)
        for extra in (0, 3):
            got = recompose_dev(torch, ring, t_mat, n, d, t_powers, extra_work=extra)
            print("%s n %d d %d: %d of %d words differ" % (name, n, d, int((got != want).sum()), want.size))
            assert np.array_equal(got, want), "%s n %d d %d" % (name, n, d)
        assert ring.count_noncanonical_dev(dev(torch, got)) == 0
        assert np.array_equal(host(t_mat), mat) and np.array_equal(host(t_powers), powers), "an input was written"
        assert np.array_equal(ring.symm_recompose(mat, n, d, powers), want), "host-pointer form"
        if name == "goldilocks" and k == 6 and (n, d) == (3, 2):   # buffers 8 bytes off a 16-byte boundary: the one-coefficient path
            w = m_.w
            off = lambda words: dev(torch, np.concatenate([np.zeros(1, dtype=np.uint64), words]))[1:]  # noqa: E731
            out = poison(torch, packed(n) * w + 1)[1:]
            work = poison(torch, d * d * w + 1)[1:]
            ring.symm_recompose_dev(out, off(mat), n, d, off(powers), work)
            torch.cuda.synchronize()
            assert np.array_equal(host(out), want), "unaligned buffers"
    guard = poison(torch, m_.w)
    ring.symm_recompose_dev(guard[:0], guard[:0], 0, 1, guard, guard)   # n == 0 writes nothing
    torch.cuda.synchronize()
    assert (host(guard) == POISON).all()


@pytest.mark.parametrize("name,k", RINGS, ids=IDS)
def test_recompose_of_a_gram_matrix_is_the_gram_matrix_of_the_recomposed_rows(torch_cuda, name, k):
    """recompose(gram(A), powers) == gram(B), B[i] = sum_a powers[a] A[i d + a], B built from sr_mul_elem_batch_dev and
    sr_add_batch_dev"""
    torch = torch_cuda
    m_ = model_for(name, k)
    ring, w = m_.ring, m_.w
    for n, d in RECOMPOSE_SHAPES:
        m = 3
        a = m_.uniform(0x4000 + 10 * n + d, n * d * m)
        powers = m_.uniform(0x4100 + 10 * n + d, d)
        t_a, t_powers = dev(torch, a), dev(torch, powers)
        rows = t_a.view(n, d, m * w)
        b = torch.zeros(n * m * w, dtype=torch.int64, device="cuda")
        for q in range(d):
            term = rows[:, q, :].clone(memory_format=torch.contiguous_format).view(-1)   # a copy: the product below works in place and must not touch A
            ring.mul_elem_dev(term, t_powers[q * w:(q + 1) * w].clone())
            ring.add_dev(b, term)
        g, _ = gram_dev(torch, ring, t_a, n * d, m)
        lhs = recompose_dev(torch, ring, dev(torch, g), n, d, t_powers)
        rhs, _ = gram_dev(torch, ring, b, n, m)
        assert np.array_equal(lhs, rhs), "%s n %d d %d" % (name, n, d)


def test_every_refusal_names_its_reason_and_writes_nothing(torch_cuda):
    torch = torch_cuda
    from stark_rings_amd import _lib

    ring = ring_for("goldilocks24", 0)
    lib, ctx, w = ring._lib, ring._ctx, ring.words_per_elem
    E = w * 8
    n, m = 2, 4096
    need, launches = ring.gram_plan(n, m)
    assert launches == 2
    pool = poison(torch, (n * m + 3 + need + 64) * w)
    base = pool.data_ptr()
    a, out, work = base, base + n * m * E, base + (n * m + 3 + 8) * E
    st = ring._stream(None)

    def refused(rc, text):
        torch.cuda.synchronize()
        assert rc == 1 and text in _lib.last_error(), (rc, _lib.last_error())
        assert (host(pool) == POISON).all(), "a refused call wrote something"

    g = lib.sr_gram_ntt_dev
    refused(g(None, out, a, n, m, work, need, st), "null context")
    refused(g(ctx, None, a, n, m, work, need, st), "null buffer")
    refused(g(ctx, out, None, n, m, work, need, st), "null buffer")
    refused(g(ctx, out, a, n, m, None, need, st), "null buffer")
    refused(g(ctx, out, a, n, m, work, need - 1, st), "workspace too small")
    refused(g(ctx, out, a, n, m, work, 0, st), "workspace too small")
    refused(g(ctx, a, a, n, m, work, need, st), "d_out overlaps d_a")
    refused(g(ctx, a + (n * m - 1) * E, a, n, m, work, need, st), "d_out overlaps d_a")
    refused(g(ctx, out, out + 2 * E, n, m, work, need, st), "d_out overlaps d_a")
    refused(g(ctx, work, a, n, m, work, need, st), "d_out overlaps d_work")
    refused(g(ctx, work + (need - 1) * E, a, n, m, work, need, st), "d_out overlaps d_work")
    refused(g(ctx, out, a, n, m, a + E, need, st), "d_a overlaps d_work")
    refused(g(ctx, out, a, (1 << 64) - 1, m, work, need, st), "overflows")
    refused(g(ctx, out, a, 1 << 20, 1, work, need, st), "exceeds one launch")

    r = lib.sr_symm_recompose_dev
    n, d = 2, 2                                        # mat: packed(4) = 10 elements, out 3, work 4, powers 2
    mat, out, work, powers = base, base + 12 * E, base + 15 * E, base + 30 * E
    refused(r(None, out, mat, n, d, powers, work, 4, st), "null context")
    refused(r(ctx, None, mat, n, d, powers, work, 4, st), "null buffer")
    refused(r(ctx, out, None, n, d, powers, work, 4, st), "null buffer")
    refused(r(ctx, out, mat, n, d, None, work, 4, st), "null buffer")
    refused(r(ctx, out, mat, n, d, powers, None, 4, st), "null buffer")
    refused(r(ctx, out, mat, n, 0, powers, work, 4, st), "d == 0")
    refused(r(ctx, out, mat, 0, 0, powers, work, 4, st), "d == 0")
    refused(r(ctx, out, mat, n, d, powers, work, 3, st), "workspace too small")
    refused(r(ctx, mat + 9 * E, mat, n, d, powers, work, 4, st), "d_out overlaps d_mat")
    refused(r(ctx, mat, mat, n, d, powers, work, 4, st), "d_out overlaps d_mat")
    refused(r(ctx, powers + E, mat, n, d, powers, work, 4, st), "d_out overlaps d_powers")
    refused(r(ctx, out, mat, n, d, out + 2 * E, work, 4, st), "d_out overlaps d_powers")
    refused(r(ctx, out, mat, n, d, powers, out + 2 * E, 4, st), "d_out overlaps d_work")
    refused(r(ctx, work + 3 * E, mat, n, d, powers, work, 4, st), "d_out overlaps d_work")
    refused(r(ctx, out, mat, n, d, powers, mat + 8 * E, 4, st), "d_mat overlaps d_work")
    refused(r(ctx, out, mat, n, d, powers, powers - 3 * E, 4, st), "d_powers overlaps d_work")
    refused(r(ctx, out, mat, 1 << 40, 1 << 40, powers, work, 4, st), "overflows")
    # host-pointer forms: null pointers and d == 0
    z = np.zeros(16 * w, dtype=np.uint64)
    zp = z.ctypes.data_as(_lib.u64p)
    refused(lib.sr_gram_ntt(ctx, None, zp, 2, 2), "null buffer")
    refused(lib.sr_gram_ntt(ctx, zp, None, 2, 2), "null buffer")
    refused(lib.sr_symm_recompose(ctx, zp, zp, 2, 0, zp), "d == 0")
    refused(lib.sr_symm_recompose(ctx, zp, None, 2, 1, zp), "null buffer")
    assert not z.any()


@pytest.mark.parametrize("name,k", [RINGS[0], RINGS[3], RINGS[4], RINGS[6]], ids=[IDS[0], IDS[3], IDS[4], IDS[6]])
def test_both_calls_are_capturable_on_a_fresh_context(torch_cuda, name, k):
    """One of each call captured into a graph on a single non-default stream, on a context that has never run anything eagerly (no
    warm-up); replayed twice on changed inputs in the same buffers.  The Gram shape is one the plan splits where it can."""
    torch = torch_cuda
    from stark_rings_amd import CyclotomicRing

    m_ = model_for(name, k)
    fresh = CyclotomicRing(name, k, device=0)
    w = m_.w
    n, d = 2, 2
    split = [m for m in (1 << e for e in range(13)) if fresh.gram_plan(n * d, m)[1] == 2]
    m = split[0] if split else 5
    t_a = dev(torch, m_.uniform(0x5000, n * d * m))
    t_powers = dev(torch, m_.uniform(0x5001, d))
    g_work = torch.zeros(max(fresh.gram_plan(n * d, m)[0], 1) * w, dtype=torch.int64, device="cuda")
    r_work = torch.zeros(d * d * w, dtype=torch.int64, device="cuda")
    t_g = torch.zeros(packed(n * d) * w, dtype=torch.int64, device="cuda")
    out = torch.zeros(packed(n) * w, dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=s):
        fresh.gram_ntt_dev(t_g, t_a, n * d, m, g_work, stream=torch.cuda.current_stream())
        fresh.symm_recompose_dev(out, t_g, n, d, t_powers, r_work, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    for seed in (0x5100, 0x5200):
        a, powers = m_.uniform(seed, n * d * m), m_.uniform(seed + 1, d)
        t_a.copy_(dev(torch, a))
        t_powers.copy_(dev(torch, powers))
        want_g, _ = gram_dev(torch, m_.ring, t_a, n * d, m)                        # eager, on the long-lived context
        want = recompose_dev(torch, m_.ring, dev(torch, want_g), n, d, t_powers)
        out.zero_()
        t_g.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(host(t_g), want_g), (name, seed)
        assert np.array_equal(host(out), want), (name, seed)
    assert np.array_equal(want_g, lower_triangle_of_a_at(torch, m_.ring, a, n * d, m))
    del graph
    fresh.close()


@pytest.mark.parametrize("name,k", [RINGS[0], RINGS[2], RINGS[3], RINGS[5]], ids=[IDS[0], IDS[2], IDS[3], IDS[5]])
def test_python_mirror_and_wire_round_trip_on_device_results(torch_cuda, name, k):
    torch = torch_cuda
    from stark_rings_amd import RingError, SymmetricMatrixNTT, recompose_left_right_symmetric_matrix, wire

    m_ = model_for(name, k)
    ring, w = m_.ring, m_.w
    n, d, m = 2, 2, 3
    a = m_.uniform(0x6000, n * d * m)
    powers = m_.uniform(0x6001, d)
    on_dev = SymmetricMatrixNTT.gram(ring, dev(torch, a), n * d, m)
    on_host = SymmetricMatrixNTT.gram(ring, a, n * d, m)
    torch.cuda.synchronize()
    want = m_.gram(a, n * d, m)
    assert on_dev.size() == on_host.size() == n * d
    assert np.array_equal(host(on_dev.words), want) and np.array_equal(on_host.words, want)
    model = M.SymmetricMatrix.from_packed(n * d, [want[e * w:(e + 1) * w] for e in range(packed(n * d))])
    for i in range(n * d):
        for j in range(n * d):
            assert np.array_equal(host(on_dev.at(i, j)), model.at(i, j)), (i, j)
            assert np.array_equal(on_host.at(i, j), model.at(i, j)), (i, j)
    assert all(np.array_equal(host(x), y) for x, y in zip(on_dev.diag(), model.diag()))
    assert [r.numel() for r in on_dev.rows()] == [(i + 1) * w for i in range(n * d)]
    small_dev = recompose_left_right_symmetric_matrix(on_dev, dev(torch, powers))
    small_host = on_host.recompose_left_right(powers)
    torch.cuda.synchronize()
    want_small = m_.recompose(want, n, d, powers)
    assert small_dev.size() == small_host.size() == n
    assert np.array_equal(host(small_dev.words), want_small) and np.array_equal(small_host.words, want_small)
    with pytest.raises(RingError):
        on_host.recompose_left_right(m_.uniform(1, 3))               # 3 does not divide 4
    zero = SymmetricMatrixNTT.zero(ring, 3, device=True)
    assert zero.size() == 3 and not host(zero.words).any()
    # wire: the derived Vec<Vec<F>> framing around the device codec
    data = wire.serialize_symmetric(ring, on_host)
    eb = wire.elem_bytes(ring)
    assert data.size == 8 + n * d * 8 + packed(n * d) * eb
    assert int.from_bytes(data[:8].tobytes(), "little") == n * d and int.from_bytes(data[8:16].tobytes(), "little") == 1
    coeff = O.wire_bytes(m_.F)
    framed = M.wire_frame(model.rows(), lambda e: O.serialize(m_.F, e).tobytes())
    assert eb == ring.degree * coeff and data.tobytes() == framed
    rows = wire.deserialize_symmetric(ring, data)
    back = SymmetricMatrixNTT.from_rows(ring, rows)
    assert back.size() == n * d and np.array_equal(back.words, want)
    ragged = [want[:w], want[:3 * w], want[:0]]                       # accepted by deserialize, as in the reference; refused by from_rows
    again = wire.deserialize_symmetric(ring, wire.serialize_symmetric(ring, ragged))
    assert [r.size for r in again] == [w, 3 * w, 0] and np.array_equal(again[1], want[:3 * w])
    with pytest.raises(RingError, match="wrong number of entries"):
        SymmetricMatrixNTT.from_rows(ring, again)
    with pytest.raises(RingError, match="unexpected end"):
        wire.deserialize_symmetric(ring, data[:-1])
    assert wire.deserialize_symmetric(ring, wire.serialize_symmetric(ring, [])) == []
