"""GPU parity tests: the HIP path (through the C ABI) vs the oracle, bit-exact.

Shapes follow the reference's tests: literal KATs (stark_prime/ntt.rs:377-545), crt/icrt round trips
(crt.rs:85-147), NTT-mul == schoolbook (stark_prime/mod.rs:161-177), crt(1) = 1 (mod.rs:125-137),
reduce (mod.rs:139-159), plus ragged/edge batches.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle_lib as O
import pyref as P

I = lambda v: [int(x) for x in v]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


_rings = {}


def ring_for(name, k):
    from stark_rings_amd import CyclotomicRing

    key = (name, k)
    if key not in _rings:
        _rings[key] = CyclotomicRing(name, k, device=0)
    return _rings[key]


def edge_and_random(F, k, batch, seed):
    """batch elements: all-zero, all-(p-1), 1, X^(D-1), then uniform -- the LAST element always stays uniform (a batch of one is
    one uniform element: a lone zero polynomial would let any linear kernel through)."""
    name = [n for n, f in O.FIELD_ID.items() if f == F][0]
    p = P.PRIMES[name][0]
    L = O.LIMBS[F]
    d = 1 << k
    data = O.fill_uniform(F, seed, 0, batch * d).reshape(batch, d * L)
    specials = []
    specials.append([0] * d)
    specials.append([p - 1] * d)
    specials.append([1] + [0] * (d - 1))
    specials.append([0] * (d - 1) + [1])
    for i, s in enumerate(specials):
        if i + 1 < batch:
            data[i] = O.to_mont(F, s)
    return np.ascontiguousarray(data.reshape(-1))


CASES = [("goldilocks", k) for k in (0, 1, 2, 5, 10, 12, 13, 16)] + \
        [("babybear", k) for k in (0, 1, 4, 10, 12, 14)] + \
        [("stark", k) for k in (0, 1, 4, 8, 10, 12)]


@pytest.mark.parametrize("name,k", CASES)
def test_host_api_fwd_inv_mul_match_oracle(torch_cuda, name, k):
    F = O.FIELD_ID[name]
    ring = ring_for(name, k)
    batch = 5 if k >= 12 else 37   # ragged: not a multiple of anything convenient
    a = edge_and_random(F, k, batch, 0xA0 + k)
    b = edge_and_random(F, k, batch, 0xB0 + k)[::-1].copy() if False else O.fill_uniform(F, 0xB0 + k, 0, batch << k)
    fa = ring.elementwise_crt(a.copy())
    assert np.array_equal(fa, O.pow2_fwd(F, a, k, batch)), "crt mismatch"
    assert np.array_equal(ring.elementwise_icrt(fa.copy()), a), "icrt(crt(x)) != x"
    assert np.array_equal(ring.elementwise_icrt(b.copy()), O.pow2_inv(F, b, k, batch)), "icrt mismatch"
    fb = O.pow2_fwd(F, b, k, batch)
    assert np.array_equal(ring.ntt_mul(fa.copy(), fb), O.pow2_pointwise(F, fa, fb)), "slot product mismatch"
    assert np.array_equal(ring.mul(a, b), O.pow2_ring_mul(F, a, b, k, batch, 4)), "ring mul mismatch"


@pytest.mark.parametrize("name,k", [("goldilocks", 16), ("goldilocks", 13), ("babybear", 16), ("stark", 12), ("stark", 4)])
def test_device_api_matches_oracle(torch_cuda, name, k):
    torch = torch_cuda
    F = O.FIELD_ID[name]
    ring = ring_for(name, k)
    batch = 3
    n = batch << k
    a = O.fill_uniform(F, 1, 0, n)
    b = O.fill_uniform(F, 2, 0, n)
    ta = torch.from_numpy(a.view(np.int64)).cuda()
    tb = torch.from_numpy(b.view(np.int64)).cuda()
    # device generator == oracle generator
    tg = torch.empty_like(ta)
    ring.fill_uniform_dev(tg, 1, 0)
    assert np.array_equal(tg.cpu().numpy().view(np.uint64), a)
    assert ring.count_noncanonical_dev(tg) == 0
    out = torch.empty_like(ta)
    ring.mul_dev(out, ta, tb)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), O.pow2_ring_mul(F, a, b, k, batch, 4))
    # a is untouched
    assert np.array_equal(ta.cpu().numpy().view(np.uint64), a)
    # in place (out aliases a)
    tb2 = torch.from_numpy(b.view(np.int64)).cuda()
    ring.mul_dev(ta, ta, tb2)
    assert torch.equal(ta, out)


def test_stark16_reference_kats_on_gpu(torch_cuda, kats):
    # stark_prime/ntt.rs:377-545 through the C ABI (SR_RING_STARK_POW2, log2_degree = 4)
    F = O.STARK
    ring = ring_for("stark", 4)
    for k in kats["stark16"]["kats"]:
        c, e = I(k["coeffs"]), I(k["evals"])
        assert O.from_mont(F, ring.elementwise_crt(O.to_mont(F, c))) == e, k["name"]
        assert O.from_mont(F, ring.elementwise_icrt(O.to_mont(F, e))) == c, k["name"]


@pytest.mark.parametrize("name", ["goldilocks", "babybear", "stark"])
def test_crt_of_one_and_mul_equals_schoolbook(torch_cuda, name):
    F = O.FIELD_ID[name]
    k = 6
    d = 1 << k
    ring = ring_for(name, k)
    one = O.to_mont(F, [1] + [0] * (d - 1))
    assert O.from_mont(F, ring.elementwise_crt(one.copy())) == [1] * d
    a = O.fill_uniform(F, 5, 0, d)
    b = O.fill_uniform(F, 6, 0, d)
    sb = O.schoolbook(F, a, b, d)
    red = ring.reduce(sb, 2 * d - 1, 1)
    assert np.array_equal(red, O.pow2_reduce(F, sb, 2 * d - 1, k))
    assert np.array_equal(ring.mul(a, b), red)


@pytest.mark.parametrize("name", ["goldilocks", "babybear", "stark"])
def test_reduce_ragged_lengths(torch_cuda, name):
    F = O.FIELD_ID[name]
    L = O.LIMBS[F]
    k = 4
    d = 16
    ring = ring_for(name, k)
    for in_len in (0, 1, 15, 16, 17, 31, 32):
        batch = 3
        src = O.fill_uniform(F, 9 + in_len, 0, batch * in_len) if in_len else np.zeros(0, dtype=np.uint64)
        got = ring.reduce(src, in_len, batch)
        for e in range(batch):
            want = O.pow2_reduce(F, src[e * in_len * L:(e + 1) * in_len * L] if in_len else np.zeros(1, dtype=np.uint64), in_len, k)
            assert np.array_equal(got[e * d * L:(e + 1) * d * L], want), (in_len, e)


def test_errors(torch_cuda):
    from stark_rings_amd import CyclotomicRing, RingError

    ring = ring_for("goldilocks", 4)
    with pytest.raises(RingError):
        ring.elementwise_crt(np.zeros(17, dtype=np.uint64))  # not a multiple of D ("Wrong length")
    with pytest.raises(RingError):
        ring.reduce(np.zeros(33, dtype=np.uint64), 33, 1)     # more than 2D coefficients
    with pytest.raises(RingError):
        CyclotomicRing("goldilocks", 40)
    with pytest.raises(RingError):
        CyclotomicRing("babybear", 27)                         # 2D-th roots need 2-adicity >= k+1
    empty = np.zeros(0, dtype=np.uint64)
    assert ring.elementwise_crt(empty).size == 0               # empty batch is a no-op


# ----------------------------------------------------------------------------- reference-native small rings
def _small(name):
    if name == "goldilocks24":
        return O.GOLDILOCKS, 24, "sro_g24_", P.g24_reduce
    return O.BABYBEAR, 72, "sro_bb72_", P.bb72_reduce


def test_goldilocks24_reference_kats_on_gpu(torch_cuda, kats):
    # goldilocks/ntt.rs:563-787: crt then dehomogenize == literal residues; homogenize then icrt == coefficients
    F = O.GOLDILOCKS
    ring = ring_for("goldilocks24", 0)
    for k in kats["goldilocks24"]["kats"]:
        c, r = I(k["coeffs"]), I(k["residues"])
        got = ring.elementwise_crt(O.to_mont(F, c))
        assert O.from_mont(F, O.small("sro_g24_dehomogenize", got)) == r, k["name"]
        got = ring.elementwise_icrt(O.small("sro_g24_homogenize", O.to_mont(F, r)))
        assert O.from_mont(F, got) == c, k["name"]


def test_babybear72_reference_kat_on_gpu(torch_cuda, kats):
    # babybear/ntt.rs:866-1019
    F = O.BABYBEAR
    ring = ring_for("babybear72", 0)
    for k in kats["babybear72"]["kats"]:
        c, r = I(k["coeffs"]), I(k["residues"])
        got = ring.elementwise_icrt(O.small("sro_bb72_homogenize", O.to_mont(F, r)))
        assert O.from_mont(F, got) == c
        got = ring.elementwise_crt(O.to_mont(F, c))
        assert O.from_mont(F, O.small("sro_bb72_dehomogenize", got)) == r


@pytest.mark.parametrize("name", ["goldilocks24", "babybear72"])
def test_small_rings_match_oracle(torch_cuda, name):
    F, D, pre, pyreduce = _small(name)
    ring = ring_for(name, 0)
    batch = 301  # ragged vs the 64-lane workgroups
    a = O.fill_uniform(F, 21, 0, batch * D)
    b = O.fill_uniform(F, 22, 0, batch * D)
    p = P.PRIMES["goldilocks" if D == 24 else "babybear"][0]
    a[:D] = O.to_mont(F, [0] * D)
    a[D:2 * D] = O.to_mont(F, [p - 1] * D)
    a[2 * D:3 * D] = O.to_mont(F, [1] + [0] * (D - 1))
    ca = ring.elementwise_crt(a.copy())
    want_ca = O.small(pre + "crt", a)
    assert np.array_equal(ca, want_ca)
    # crt(1) = 1: goldilocks/mod.rs:179-191
    W = D // 8
    assert O.from_mont(F, ca[2 * D:3 * D]) == ([1] + [0] * (W - 1)) * 8
    assert np.array_equal(ring.elementwise_icrt(ca.copy()), a)               # crt.rs:85-147 round trip
    assert np.array_equal(ring.elementwise_icrt(b.copy()), O.small(pre + "icrt", b))
    cb = O.small(pre + "crt", b)
    prod = ring.ntt_mul(ca.copy(), cb)
    assert np.array_equal(prod, O.small(pre + "ntt_mul", want_ca, cb))     # Fq3 / Fq9 slot products
    want = O.small(pre + "icrt", prod)
    assert np.array_equal(ring.mul(a, b), want)                            # fused ring product
    # test_mul_crt (goldilocks/mod.rs:231-247): NTT product == schoolbook product reduced mod Phi
    for e in (3, 17, 300):
        sb = O.schoolbook(F, a[e * D:(e + 1) * D], b[e * D:(e + 1) * D], D)
        red = ring.reduce(sb, 2 * D - 1, 1)
        assert np.array_equal(red, want[e * D:(e + 1) * D])
        std = O.from_mont(F, sb)
        assert O.from_mont(F, red) == pyreduce(std)
    # ragged reduce lengths (reduce_in_place uses .get(..).unwrap_or(ZERO))
    for in_len in (0, 5, D, D + 3, 2 * D - 1, 2 * D):
        src = O.fill_uniform(F, 77 + in_len, 0, 2 * in_len) if in_len else np.zeros(0, dtype=np.uint64)
        got = ring.reduce(src, in_len, 2)
        for e in range(2):
            std = O.from_mont(F, src[e * in_len:(e + 1) * in_len]) if in_len else []
            assert O.from_mont(F, got[e * D:(e + 1) * D]) == pyreduce(std), (in_len, e)


# ----------------------------------------------------------------------------- tuned Goldilocks path
@pytest.mark.parametrize("k,batch", [(8, 21), (9, 13), (10, 5), (11, 3), (12, 7), (14, 3), (15, 2), (16, 3), (17, 2), (18, 1), (19, 1),
                                      (20, 1)])
def test_goldilocks_tuned_path_all_plans(torch_cuda, k, batch):
    """Every plan of the tuned path: 256 <= D <= 4096 (several ring elements per tile, ragged last tile, twist inside the
    rows kernel), D = 2^13..2^15 (strided register passes + 4096-point rows) and 2^16 <= D <= 2^20 (the shift-only 8-stage
    column pass + 256..4096-point rows), vs the oracle and vs the generic kernels (SR_GOLDILOCKS_GENERIC=1 routes the same ring through them)."""
    import os

    from stark_rings_amd import CyclotomicRing

    F = O.GOLDILOCKS
    ring = ring_for("goldilocks", k)
    a = edge_and_random(F, k, batch, 0xC0 + k)
    b = O.fill_uniform(F, 0xD0 + k, 0, batch << k)
    fa = ring.elementwise_crt(a.copy())
    assert np.array_equal(fa, O.pow2_fwd(F, a, k, batch, 4))
    assert np.array_equal(ring.elementwise_icrt(fa.copy()), a)
    want = O.pow2_ring_mul(F, a, b, k, batch, 4)
    assert np.array_equal(ring.mul(a, b), want)
    os.environ["SR_GOLDILOCKS_GENERIC"] = "1"
    try:
        generic = CyclotomicRing("goldilocks", k, device=0)
    finally:
        del os.environ["SR_GOLDILOCKS_GENERIC"]
    assert np.array_equal(generic.elementwise_crt(a.copy()), fa)
    assert np.array_equal(generic.mul(a, b), want)
    generic.close()


@pytest.mark.parametrize("k,batch", [(16, 3), (17, 2), (20, 1)])
def test_goldilocks_older_plan_equals_cols256_plan(torch_cuda, k, batch):
    """SR_GL_COLS256=0 selects the plan these sizes ran before the shift-only column pass existed (register strided
    passes / the general-twiddle 256-leg pass + 4096-point rows): same bytes out."""
    import os

    from stark_rings_amd import CyclotomicRing

    F = O.GOLDILOCKS
    a = edge_and_random(F, k, batch, 0xE0 + k)
    b = O.fill_uniform(F, 0xF0 + k, 0, batch << k)
    ring = ring_for("goldilocks", k)
    os.environ["SR_GL_COLS256"] = "0"
    try:
        older = CyclotomicRing("goldilocks", k, device=0)
    finally:
        del os.environ["SR_GL_COLS256"]
    fa = ring.elementwise_crt(a.copy())
    assert np.array_equal(older.elementwise_crt(a.copy()), fa)
    assert np.array_equal(older.elementwise_icrt(fa.copy()), a)
    want = O.pow2_ring_mul(F, a, b, k, batch, 4)
    assert np.array_equal(ring.mul(a, b), want)
    assert np.array_equal(older.mul(a, b), want)
    older.close()


def test_goldilocks_chunked_launches_equal_single_launch(torch_cuda):
    import os

    from stark_rings_amd import CyclotomicRing

    torch = torch_cuda
    F = O.GOLDILOCKS
    k, batch = 13, 11
    a = O.fill_uniform(F, 31, 0, batch << k)
    b = O.fill_uniform(F, 32, 0, batch << k)
    want = O.pow2_ring_mul(F, a, b, k, batch, 4)
    os.environ["SR_CHUNK_POLYS"] = "4"   # 4 + 4 + 3: ragged last chunk
    try:
        ring = CyclotomicRing("goldilocks", k, device=0)
    finally:
        del os.environ["SR_CHUNK_POLYS"]
    assert np.array_equal(ring.mul(a, b), want)
    ring.close()


# ----------------------------------------------------------------------------- register-tiled path (BabyBear; Goldilocks cross-check)
@pytest.mark.parametrize("name,k,batch", [("babybear", 12, 5), ("babybear", 13, 3), ("babybear", 15, 2), ("babybear", 16, 3),
                                          ("babybear", 17, 2), ("babybear", 18, 1), ("babybear", 20, 1),
                                          ("goldilocks", 12, 3), ("goldilocks", 14, 2), ("goldilocks", 16, 2)])
def test_register_tiled_path_matches_oracle_and_generic(torch_cuda, name, k, batch):
    import os

    from stark_rings_amd import CyclotomicRing

    F = O.FIELD_ID[name]
    env_on = {"goldilocks": "SR_GOLDILOCKS_REGTILE"}.get(name)      # BabyBear uses the register-tiled path by default
    env_generic = {"babybear": "SR_BABYBEAR_GENERIC", "goldilocks": "SR_GOLDILOCKS_GENERIC"}[name]
    if env_on:
        os.environ[env_on] = "1"
    try:
        ring = CyclotomicRing(name, k, device=0)
    finally:
        if env_on:
            del os.environ[env_on]
    a = edge_and_random(F, k, batch, 0xE0 + k)
    b = O.fill_uniform(F, 0xF0 + k, 0, batch << k)
    fa = ring.elementwise_crt(a.copy())
    assert np.array_equal(fa, O.pow2_fwd(F, a, k, batch, 4))
    assert np.array_equal(ring.elementwise_icrt(fa.copy()), a)
    assert np.array_equal(ring.elementwise_icrt(b.copy()), O.pow2_inv(F, b, k, batch, 4))
    want = O.pow2_ring_mul(F, a, b, k, batch, 4)
    assert np.array_equal(ring.mul(a, b), want)
    ring.close()
    os.environ[env_generic] = "1"
    try:
        generic = CyclotomicRing(name, k, device=0)
    finally:
        del os.environ[env_generic]
    assert np.array_equal(generic.mul(a, b), want)
    generic.close()


@pytest.mark.parametrize("k,batch", [(16, 3), (20, 1)])
def test_babybear_older_plan_equals_cols256_plan(torch_cuda, k, batch):
    """SR_RT_COLS256=0 selects the 4-stage register column passes + twelve-stage rows these sizes ran before the 8-stage
    column pass existed: same bytes out."""
    import os

    from stark_rings_amd import CyclotomicRing

    F = O.BABYBEAR
    a = edge_and_random(F, k, batch, 0x1E0 + k)
    b = O.fill_uniform(F, 0x1F0 + k, 0, batch << k)
    ring = ring_for("babybear", k)
    fa = ring.elementwise_crt(a.copy())
    want = O.pow2_ring_mul(F, a, b, k, batch, 4)
    assert np.array_equal(ring.mul(a, b), want)
    os.environ["SR_RT_COLS256"] = "0"
    try:
        older = CyclotomicRing("babybear", k, device=0)
        assert np.array_equal(older.elementwise_crt(a.copy()), fa)
        assert np.array_equal(older.elementwise_icrt(fa.copy()), a)
        assert np.array_equal(older.mul(a, b), want)
        older.close()
    finally:
        del os.environ["SR_RT_COLS256"]


@pytest.mark.parametrize("k,batch", [(1, 9), (3, 70), (4, 37), (4, 131), (5, 33), (6, 17), (7, 9), (8, 5), (9, 7), (10, 3), (11, 3), (12, 5),
                                     (13, 2), (14, 2), (15, 1), (16, 1)])
def test_stark_three_kernel_families_agree(torch_cuda, k, batch):
    """Stark rings run on three kernel families that must produce the same bytes: the register-tiled kernels on 28-bit lazy limbs
    (ntt_stark.hpp, k >= 4: several small ring elements share a workgroup -- the batches leave ragged last workgroups --, one
    tile per element up to D = 2048, strided passes of 1, 2 or 3 stages above: k = 12..16 walks every combination), the generic
    LDS kernels on the same arithmetic (SR_STARK_TUNED=0, every k >= 1) and the generic kernels on 8 x 32-bit limbs
    (SR_STARK_LAZY=0, what every size ran before).  Inputs include all-zero, all-(p-1), 1 and X^(D-1); the oracle pins the values."""
    import os

    from stark_rings_amd import CyclotomicRing

    F = O.STARK
    a = edge_and_random(F, k, batch, 0x2A0 + k)
    b = np.ascontiguousarray(edge_and_random(F, k, batch, 0x2B0 + k).reshape(batch, -1)[::-1]).reshape(-1)   # edge elements last
    ring = ring_for("stark", k)
    fa = ring.elementwise_crt(a.copy())
    prod = ring.mul(a, b)
    assert np.array_equal(ring.elementwise_icrt(fa.copy()), a)
    if k <= 12:
        assert np.array_equal(fa, O.pow2_fwd(F, a, k, batch, 4))
        assert np.array_equal(prod, O.pow2_ring_mul(F, a, b, k, batch, 4))
    else:
        e = batch - 1
        d4 = 4 << k
        assert np.array_equal(fa[e * d4:(e + 1) * d4], O.pow2_fwd(F, a[e * d4:(e + 1) * d4], k, 1))
        assert np.array_equal(prod[e * d4:(e + 1) * d4], O.pow2_ring_mul(F, a[e * d4:(e + 1) * d4], b[e * d4:(e + 1) * d4], k, 1))
    variants = [("SR_STARK_TUNED", "0"), ("SR_STARK_LAZY", "0")]
    if 10 <= k <= 12:   # one tile per ring element, or strided passes + 512-coefficient tiles: both ways for these degrees
        variants += [("SR_ST_WHOLE_MAX", "9"), ("SR_ST_WHOLE_MAX", "12")]
    for var, val in variants:
        os.environ[var] = val
        try:
            other = CyclotomicRing("stark", k, device=0)
            assert np.array_equal(other.elementwise_crt(a.copy()), fa), var
            assert np.array_equal(other.elementwise_icrt(fa.copy()), a), var
            assert np.array_equal(other.mul(a, b), prod), var
            other.close()
        finally:
            del os.environ[var]


# ----------------------------------------------------------------------------- maximum sizes and BASELINE full sizes
@pytest.mark.parametrize("name,k", [("goldilocks", 22), ("goldilocks", 24), ("babybear", 24), ("stark", 18), ("stark", 20)])
def test_maximum_degrees_single_element(torch_cuda, name, k):
    """Largest degrees each kernel family accepts (tuned Goldilocks <= 2^22, generic / register-tiled <= 2^24, Stark <= 2^20)."""
    F = O.FIELD_ID[name]
    ring = ring_for(name, k)
    a = O.fill_uniform(F, 0x11 + k, 0, 1 << k)
    b = O.fill_uniform(F, 0x22 + k, 0, 1 << k)
    fa = ring.elementwise_crt(a.copy())
    assert np.array_equal(fa, O.pow2_fwd(F, a, k, 1))
    assert np.array_equal(ring.elementwise_icrt(fa), a)
    assert np.array_equal(ring.mul(a, b), O.pow2_ring_mul(F, a, b, k, 1))
    _rings.pop((name, k)).close()   # free the large tables


@pytest.mark.parametrize("name,k,batch", [("goldilocks", 16, 1 << 14), ("babybear", 16, 1 << 14), ("stark", 12, 1 << 12)])
def test_full_size_properties(torch_cuda, name, k, batch):
    """BASELINE configs 2, 3, 5 at full size, through size-independent properties (the oracle would take minutes):
    round trip, multiplication by 1, commutativity, the negacyclic wrap X^(D-1) * X = -1, canonical outputs,
    plus sampled elements against the oracle."""
    torch = torch_cuda
    F = O.FIELD_ID[name]
    L = O.LIMBS[F]
    d = 1 << k
    p = P.PRIMES[name][0]
    ring = ring_for(name, k)
    n = batch * d * L
    a = torch.empty(n, dtype=torch.int64, device="cuda")
    b = torch.empty(n, dtype=torch.int64, device="cuda")
    ring.fill_uniform_dev(a, 0xAA, 0)
    ring.fill_uniform_dev(b, 0xBB, 0)
    a0, b0 = a.clone(), b.clone()
    # icrt(crt(a)) == a   (crt.rs:85-147 at full size)
    ring.elementwise_crt_dev(a)
    assert not torch.equal(a, a0)
    ring.elementwise_icrt_dev(a)
    assert torch.equal(a, a0)
    # a * b == b * a, and a few elements against the oracle
    ab = torch.empty_like(a)
    ring.mul_dev(ab, a, b)            # b may now hold crt-side scratch
    b.copy_(b0)
    ba = torch.empty_like(a)
    ring.mul_dev(ba, b, a)
    a.copy_(a0)
    assert torch.equal(ab, ba)
    assert ring.count_noncanonical_dev(ab) == 0
    w = d * L
    for e in (0, batch // 2 + 1, batch - 1):
        ea = O.fill_uniform(F, 0xAA, e * d, d)
        eb = O.fill_uniform(F, 0xBB, e * d, d)
        assert np.array_equal(ab[e * w:(e + 1) * w].cpu().numpy().view(np.uint64), O.pow2_ring_mul(F, ea, eb, k))
    # a * 1 == a ;  X^(D-1) * X == -1
    one = torch.zeros(n, dtype=torch.int64, device="cuda")
    one_elem = torch.from_numpy(O.to_mont(F, [1] + [0] * (d - 1)).view(np.int64)).cuda()
    one.view(batch, w)[:] = one_elem
    out = torch.empty_like(a)
    b.copy_(one)
    ring.mul_dev(out, a, b)
    assert torch.equal(out, a0)
    x1 = torch.from_numpy(O.to_mont(F, [0, 1] + [0] * (d - 2)).view(np.int64)).cuda()
    xd = torch.from_numpy(O.to_mont(F, [0] * (d - 1) + [1]).view(np.int64)).cuda()
    minus_one = O.to_mont(F, [p - 1] + [0] * (d - 1))
    small = 4
    ta = xd.repeat(small).contiguous()
    tb = x1.repeat(small).contiguous()
    to = torch.empty_like(ta)
    ring.mul_dev(to, ta, tb)
    assert np.array_equal(to[:w].cpu().numpy().view(np.uint64), minus_one)


# ----------------------------------------------------------------------------- add / sub, and the first "next" row: Matrix<RqNTT> * vec
@pytest.mark.parametrize("name,k", [("goldilocks", 6), ("babybear", 6), ("stark", 4), ("goldilocks24", 0), ("babybear72", 0)])
def test_add_sub_match_integer_arithmetic(torch_cuda, name, k):
    base = {"goldilocks24": "goldilocks", "babybear72": "babybear"}.get(name, name)
    F = O.FIELD_ID[base]
    p = P.PRIMES[base][0]
    ring = ring_for(name, k)
    batch = 9
    n = batch * ring.degree
    a = O.fill_uniform(F, 41, 0, n)
    b = O.fill_uniform(F, 42, 0, n)
    a[:ring.words_per_elem] = O.to_mont(F, [p - 1] * ring.degree)      # force wrap-around on add, borrow on sub
    sa, sb = O.from_mont(F, a), O.from_mont(F, b)
    assert O.from_mont(F, ring.add(a.copy(), b)) == [(x + y) % p for x, y in zip(sa, sb)]
    assert O.from_mont(F, ring.sub(a.copy(), b)) == [(x - y) % p for x, y in zip(sa, sb)]
    assert np.array_equal(ring.sub(ring.add(a.copy(), b), b), a)


@pytest.mark.parametrize("name,k,nrows,ncols", [("goldilocks", 5, 7, 9), ("babybear", 6, 5, 3), ("stark", 4, 6, 5), ("goldilocks", 12, 3, 4)])
def test_matvec_ntt_matches_row_by_row_products(torch_cuda, name, k, nrows, ncols):
    """Matrix<RqNTT>::checked_mul_vec (linear_algebra/src/matrix.rs:168-178; test_matrix_mul_vec :233-244):
    y[r] = sum_c M[r][c] * v[c], against the oracle's slot products and integer sums."""
    torch = torch_cuda
    from stark_rings_amd import RingError

    F = O.FIELD_ID[name]
    L = O.LIMBS[F]
    p = P.PRIMES[name][0]
    ring = ring_for(name, k)
    w = ring.words_per_elem
    m = O.fill_uniform(F, 51, 0, nrows * ncols << k)
    v = O.fill_uniform(F, 52, 0, ncols << k)
    want = []
    for r in range(nrows):
        acc = [0] * (1 << k)
        for c in range(ncols):
            prod = O.from_mont(F, O.pow2_pointwise(F, m[(r * ncols + c) * w:(r * ncols + c + 1) * w], v[c * w:(c + 1) * w]))
            acc = [(x + y) % p for x, y in zip(acc, prod)]
        want += acc
    tm = torch.from_numpy(m.view(np.int64)).cuda()
    tv = torch.from_numpy(v.view(np.int64)).cuda()
    ty = torch.empty(nrows * w, dtype=torch.int64, device="cuda")
    ring.matvec_ntt_dev(ty, tm, tv, nrows, ncols)
    assert O.from_mont(F, ty.cpu().numpy().view(np.uint64)) == want
    with pytest.raises(RingError, match="DifferentLengths"):
        ring.matvec_ntt_dev(ty, tm, tv, nrows, ncols + 1)


def _slot_products(F, p, k, w, pairs):
    """sum of slot-wise products of (a, b) ring-element pairs through the oracle, as standard-form integers"""
    acc = [0] * (1 << k)
    for a, b in pairs:
        prod = O.from_mont(F, O.pow2_pointwise(F, a, b))
        acc = [(x + y) % p for x, y in zip(acc, prod)]
    return acc


@pytest.mark.parametrize("name,k,nrows,ncols", [("goldilocks", 5, 6, 9), ("babybear", 6, 4, 5), ("stark", 4, 5, 4)])
def test_spmv_ntt_matches_oracle_row_sums(torch_cuda, name, k, nrows, ncols):
    """SparseMatrix<RqNTT>::checked_mul_vec (linear_algebra/src/sparse_matrix.rs:201-211): per row the sum over its stored
    (value, column) entries of value * v[column]; an empty row is zero; repeated columns in a row both count.  Device (CSR)
    and host-pointer entry points against the oracle's slot products."""
    torch = torch_cuda
    from stark_rings_amd import RingError

    F = O.FIELD_ID[name]
    p = P.PRIMES[name][0]
    ring = ring_for(name, k)
    w = ring.words_per_elem
    v = O.fill_uniform(F, 62, 0, ncols << k)
    rng = np.random.default_rng(7 + k)
    rows, seed = [], 100
    for r in range(nrows):
        nz = 0 if r == 2 else int(rng.integers(1, ncols + 2))      # row 2 is empty; some rows hold a column twice
        row = []
        for _ in range(nz):
            seed += 1
            row.append((O.fill_uniform(F, seed, 0, 1 << k), int(rng.integers(0, ncols))))
        rows.append(row)
    want = []
    for row in rows:
        want += _slot_products(F, p, k, w, [(val, v[c * w:(c + 1) * w]) for val, c in row])
    got = ring.spmv_ntt(rows, v, ncols)
    assert O.from_mont(F, got) == want
    # device CSR
    nnz = sum(len(r) for r in rows)
    vals = np.concatenate([val for row in rows for val, _ in row]) if nnz else np.zeros(0, dtype=np.uint64)
    cols = np.array([c for row in rows for _, c in row], dtype=np.int32)
    ptr = np.zeros(nrows + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    ty = torch.empty(nrows * w, dtype=torch.int64, device="cuda")
    tv = torch.from_numpy(v.view(np.int64)).cuda()
    tvals, tcols, tptr = torch.from_numpy(vals.view(np.int64)).cuda(), torch.from_numpy(cols).cuda(), torch.from_numpy(ptr).cuda()
    ring.spmv_ntt_dev(ty, tvals, tcols, tptr, tv, nrows, ncols)
    assert O.from_mont(F, ty.cpu().numpy().view(np.uint64)) == want
    assert ring.spmv_bad_index_count() == 0
    # out-of-range column: host form refuses (the reference panics on v[col]); device form skips the entry and counts it
    bad_rows = [list(r) for r in rows]
    bad_rows[0] = bad_rows[0] + [(O.fill_uniform(F, 999, 0, 1 << k), ncols)]
    with pytest.raises(RingError, match="out of range"):
        ring.spmv_ntt(bad_rows, v, ncols)
    bad_cols = cols.copy()
    bad_cols[0] = ncols + 3
    ring.spmv_ntt_dev(ty, tvals, torch.from_numpy(bad_cols).cuda(), tptr, tv, nrows, ncols)
    assert ring.spmv_bad_index_count() == 1 and ring.spmv_bad_index_count() == 0
    with pytest.raises(RingError, match="DifferentLengths"):
        ring.spmv_ntt(rows, v[w:], ncols)


@pytest.mark.parametrize("name,k,n,m,p_", [("goldilocks", 5, 5, 7, 3), ("babybear", 6, 3, 4, 5), ("stark", 4, 4, 3, 2), ("goldilocks", 12, 2, 3, 2)])
def test_matmul_ntt_matches_oracle(torch_cuda, name, k, n, m, p_):
    """Matrix<RqNTT>::checked_mul_mat (linear_algebra/src/matrix.rs:148-166): Y[i][j] = sum_t A[i][t] * B[t][j], slot-wise."""
    torch = torch_cuda
    from stark_rings_amd import RingError

    F = O.FIELD_ID[name]
    p = P.PRIMES[name][0]
    ring = ring_for(name, k)
    w = ring.words_per_elem
    a = O.fill_uniform(F, 71, 0, n * m << k)
    b = O.fill_uniform(F, 72, 0, m * p_ << k)
    want = []
    for i in range(n):
        for j in range(p_):
            want += _slot_products(F, p, k, w, [(a[(i * m + t) * w:(i * m + t + 1) * w], b[(t * p_ + j) * w:(t * p_ + j + 1) * w])
                                                for t in range(m)])
    assert O.from_mont(F, ring.matmul_ntt(a, b, n, m, p_)) == want
    ta, tb = torch.from_numpy(a.view(np.int64)).cuda(), torch.from_numpy(b.view(np.int64)).cuda()
    ty = torch.empty(n * p_ * w, dtype=torch.int64, device="cuda")
    ring.matmul_ntt_dev(ty, ta, tb, n, m, p_)
    assert O.from_mont(F, ty.cpu().numpy().view(np.uint64)) == want
    # a matrix times a one-column matrix is the matrix-vector product
    tv = tb[:m * w].clone() if p_ == 1 else torch.from_numpy(O.fill_uniform(F, 73, 0, m << k).view(np.int64)).cuda()
    y1 = torch.empty(n * w, dtype=torch.int64, device="cuda")
    y2 = torch.empty(n * w, dtype=torch.int64, device="cuda")
    ring.matmul_ntt_dev(y1, ta, tv, n, m, 1)
    ring.matvec_ntt_dev(y2, ta, tv, n, m)
    assert torch.equal(y1, y2)
    assert np.array_equal(ring.matvec_ntt(a, tv.cpu().numpy().view(np.uint64), n, m), y2.cpu().numpy().view(np.uint64))
    with pytest.raises(RingError, match="DifferentLengths"):
        ring.matmul_ntt(a, b, n, m + 1, p_)


# ----------------------------------------------------------------------------- second "next" row: balanced gadget decomposition
def _signed_std(F, arr, p):
    return [v - p if v > (p - 1) // 2 else v for v in O.from_mont(F, arr)]


def test_decomposition_reference_kats_on_gpu(torch_cuda, kats):
    """stark_prime/decomposition.rs:72-99 and balanced_decomposition/mod.rs:469-514 through the C ABI."""
    kat = kats["decomposition"]["stark_prime_fq"]
    p = P.PRIMES["stark"][0]
    ring = ring_for("stark", 4)
    x = [int(kat["x"])] + [0] * 15
    digits = ring.gadget_decompose(O.to_mont(O.STARK, x), kat["basis"], kat["padding"])
    got = _signed_std(O.STARK, digits, p)
    assert [got[j * 16] for j in range(kat["padding"])] == [int(v) for v in kat["digits"]]
    assert all(got[j * 16 + i] == 0 for j in range(kat["padding"]) for i in range(1, 16))
    assert O.from_mont(O.STARK, ring.gadget_recompose(digits, kat["basis"], kat["padding"])) == x
    kat = kats["decomposition"]["goldilocks24_gadget"]
    p = P.PRIMES["goldilocks"][0]
    ring = ring_for("goldilocks24", 0)
    vals = kat["input_coefficient_values"]
    a = O.to_mont(O.GOLDILOCKS, [v % p for v in vals for _ in range(24)])
    digits = ring.gadget_decompose(a, kat["basis"], kat["padding"])
    assert _signed_std(O.GOLDILOCKS, digits, p) == [v for v in kat["expected_coefficient_values"] for _ in range(24)]
    assert np.array_equal(ring.gadget_recompose(digits, kat["basis"], kat["padding"]), a)   # test_gadget_recompose


@pytest.mark.parametrize("name,k", [("goldilocks", 7), ("babybear", 7), ("stark", 4), ("goldilocks24", 0), ("babybear72", 0)])
@pytest.mark.parametrize("basis", [2, 4, 16, 1 << 16, 10, 1 << 32, (1 << 32) + 2, 1 << 40, 3 * (1 << 40) + 10, 1 << 63, (1 << 64) - 2])
def test_decomposition_matches_oracle(torch_cuda, name, k, basis):
    """test_decompose_balanced / _vec / _polyring (mod.rs:409-467) shapes on every ring: digits equal the oracle's,
    |digit| <= b/2, recompose(decompose(v)) == v; edge coefficients 0, 1, p-1, (p-1)/2, (p-1)/2 + 1."""
    torch = torch_cuda
    base = {"goldilocks24": "goldilocks", "babybear72": "babybear"}.get(name, name)
    F = O.FIELD_ID[base]
    p = P.PRIMES[base][0]
    ring = ring_for(name, k)
    d, w, batch = ring.degree, ring.words_per_elem, 5
    a = O.fill_uniform(F, 0x77 + basis % 97, 0, batch * d)
    edge = O.to_mont(F, [0, 1, p - 1, (p - 1) // 2, (p - 1) // 2 + 1, 2, p - 2, basis % p, (basis // 2) % p, (basis // 2 + 1) % p])
    a[:edge.size] = edge
    pad = 1
    while (basis // 2) * (basis ** pad - 1) // (basis - 1) < (p - 1) // 2:
        pad += 1
    pad += 1
    want, over = O.decompose_balanced(F, a, d, batch, basis, pad)
    assert not over
    got = ring.gadget_decompose(a, basis, pad)
    assert np.array_equal(got, want)
    assert all(abs(v) <= basis // 2 for v in _signed_std(F, got[:2 * pad * w], p))
    assert np.array_equal(ring.gadget_recompose(got, basis, pad), a)
    assert np.array_equal(O.recompose(F, got, d, batch, basis, pad), a)
    # device-resident forms
    ta = torch.from_numpy(a.view(np.int64)).cuda()
    tout = torch.empty(batch * pad * w, dtype=torch.int64, device="cuda")
    ring.gadget_decompose_dev(tout, ta, basis, pad)
    assert np.array_equal(tout.cpu().numpy().view(np.uint64), want)
    assert ring.decompose_overflow_count() == 0
    tback = torch.empty_like(ta)
    ring.gadget_recompose_dev(tback, tout, basis, pad)
    assert torch.equal(tback, ta)


def test_decomposition_errors(torch_cuda):
    """panics of the reference as errors: basis 0 / 1 ("cannot decompose in basis 0 or 1"), odd basis ("must be even"),
    out[i] out of bounds when padding_size digits do not suffice."""
    torch = torch_cuda
    from stark_rings_amd import RingError

    ring = ring_for("goldilocks", 7)
    F, p = O.GOLDILOCKS, P.PRIMES["goldilocks"][0]
    a = O.fill_uniform(F, 9, 0, 2 * ring.degree)
    for bad, msg in ((0, "basis 0 or 1"), (1, "basis 0 or 1"), (7, "must be even"), ((1 << 63) + 1, "must be even")):
        with pytest.raises(RingError, match=msg):
            ring.gadget_decompose(a, bad, 8)
    with pytest.raises(RingError, match="more than padding_size"):
        ring.gadget_decompose(a, 2, 8)
    ta = torch.from_numpy(a.view(np.int64)).cuda()
    tout = torch.empty(a.size * 8, dtype=torch.int64, device="cuda")
    ring.gadget_decompose_dev(tout, ta, 2, 8)
    n_over = ring.decompose_overflow_count()
    want_over = sum(1 for v in O.from_mont(F, a) if abs(v - p if v > (p - 1) // 2 else v) >= 2 ** 8)
    assert n_over == want_over and ring.decompose_overflow_count() == 0
    with pytest.raises(RingError, match="multiple of padding_size"):
        ring.gadget_recompose(a, 2, 3)


def test_linear_algebra_many_rows(torch_cuda):
    """more rows than a 16-bit grid dimension holds: the launches are flat over (row, slot chunk)"""
    torch = torch_cuda
    F, p = O.GOLDILOCKS, P.PRIMES["goldilocks"][0]
    k, nrows, ncols = 3, 70001, 3
    ring = ring_for("goldilocks", k)
    w = ring.words_per_elem
    m = O.fill_uniform(F, 81, 0, nrows * ncols << k)
    v = O.fill_uniform(F, 82, 0, ncols << k)
    tm, tv = torch.from_numpy(m.view(np.int64)).cuda(), torch.from_numpy(v.view(np.int64)).cuda()
    ty = torch.empty(nrows * w, dtype=torch.int64, device="cuda")
    ring.matvec_ntt_dev(ty, tm, tv, nrows, ncols)
    y = ty.cpu().numpy().view(np.uint64)
    for r in (0, 1, 65535, 65536, nrows - 1):
        want = _slot_products(F, p, k, w, [(m[(r * ncols + c) * w:(r * ncols + c + 1) * w], v[c * w:(c + 1) * w]) for c in range(ncols)])
        assert O.from_mont(F, y[r * w:(r + 1) * w]) == want
    # sparse: one stored entry per row, column r mod ncols, values = the first column of m
    cols = torch.arange(nrows, dtype=torch.int32, device="cuda") % ncols
    ptr = torch.arange(nrows + 1, dtype=torch.int64, device="cuda")
    vals = tm.view(nrows, ncols * w)[:, :w].contiguous().view(-1)
    ring.spmv_ntt_dev(ty, vals, cols, ptr, tv, nrows, ncols)
    y = ty.cpu().numpy().view(np.uint64)
    for r in (0, 65535, 65536, nrows - 1):
        c = r % ncols
        assert O.from_mont(F, y[r * w:(r + 1) * w]) == _slot_products(F, p, k, w, [(m[r * ncols * w:(r * ncols + 1) * w], v[c * w:(c + 1) * w])])
    # mat-mat with 70001 x 3 times 3 x 1 equals the mat-vec
    y2 = torch.empty(nrows * w, dtype=torch.int64, device="cuda")
    ring.matmul_ntt_dev(y2, tm, tv, nrows, ncols, 1)
    ring.matvec_ntt_dev(ty, tm, tv, nrows, ncols)
    assert torch.equal(y2, ty)


# ----------------------------------------------------------------------------- "next" row 4: the frog ring X^16 + 1 -> 4 x Fq4
def test_frog16_reference_kats_on_gpu(torch_cuda, kats):
    """frog_ring/ntt.rs:387-563 through the C ABI: crt then (oracle) dehomogenize == expected residues; (oracle) homogenize then
    icrt == expected coefficients."""
    ring = ring_for("frog16", 0)
    F = O.FROG
    for k in kats["frog16"]["kats"]:
        c, r = [int(v) for v in k["coeffs"]], [int(v) for v in k["residues"]]
        if k["kind"] == "crt_then_dehomogenize":
            got = ring.elementwise_crt(O.to_mont(F, c))
            assert O.from_mont(F, O.small("sro_frog16_dehomogenize", got)) == r
        else:
            got = ring.elementwise_icrt(O.small("sro_frog16_homogenize", O.to_mont(F, r)))
            assert O.from_mont(F, got) == c


def test_frog16_matches_oracle(torch_cuda):
    """test_crt_one / test_icrt_one / test_mul_crt / test_reduce of frog_ring/mod.rs:143-219 as batch parity against the oracle:
    crt, icrt, Fq4 slot products, the fused ring product (== schoolbook reduced), reduce with ragged lengths, add / sub, and the
    balanced decomposition over the frog prime."""
    ring = ring_for("frog16", 0)
    F, p, D = O.FROG, P.FROG_P, 16
    batch = 301
    a = O.fill_uniform(F, 0xF1, 0, batch * D)
    b = O.fill_uniform(F, 0xF2, 0, batch * D)
    a[:D] = O.to_mont(F, [1] + [0] * 15)
    a[D:2 * D] = O.to_mont(F, [p - 1] * 16)
    fa = ring.elementwise_crt(a.copy())
    assert np.array_equal(fa, O.small("sro_frog16_crt", a))
    assert O.from_mont(F, fa[:D]) == [1, 0, 0, 0] * 4                      # crt(ONE) == ONE
    assert np.array_equal(ring.elementwise_icrt(fa.copy()), a)
    fb = ring.elementwise_crt(b.copy())
    prod = ring.ntt_mul(fa.copy(), fb)
    assert np.array_equal(prod, O.small("sro_frog16_ntt_mul", fa, fb))
    c = ring.mul(a, b)
    assert np.array_equal(c, ring.elementwise_icrt(prod.copy()))
    for e in (0, 1, 7, batch - 1):
        sb = O.schoolbook(F, a[e * D:(e + 1) * D], b[e * D:(e + 1) * D], D)
        assert O.from_mont(F, c[e * D:(e + 1) * D]) == P.frog16_reduce(O.from_mont(F, sb))
    for in_len in (0, 5, 16, 19, 31, 32):
        src = O.fill_uniform(F, 0xF3 + in_len, 0, 2 * in_len) if in_len else np.zeros(0, dtype=np.uint64)
        got = ring.reduce(src, in_len, 2)
        for e in range(2):
            std = O.from_mont(F, src[e * in_len:(e + 1) * in_len]) if in_len else []
            assert O.from_mont(F, got[e * D:(e + 1) * D]) == P.frog16_reduce(std)
    sa, sb_ = O.from_mont(F, a), O.from_mont(F, b)
    assert O.from_mont(F, ring.add(a.copy(), b)) == [(x + y) % p for x, y in zip(sa, sb_)]
    assert O.from_mont(F, ring.sub(a.copy(), b)) == [(x - y) % p for x, y in zip(sa, sb_)]
    for basis, pad in ((2, 65), (1 << 16, 5), (10, 21)):
        want, over = O.decompose_balanced(F, a, D, batch, basis, pad)
        assert not over
        got = ring.gadget_decompose(a, basis, pad)
        assert np.array_equal(got, want)
        assert np.array_equal(ring.gadget_recompose(got, basis, pad), a)


# ----------------------------------------------------------------------------- Cyclotomic::rot
@pytest.mark.parametrize("name,k", [("goldilocks", 6), ("babybear", 5), ("stark", 4), ("goldilocks24", 0), ("babybear72", 0), ("frog16", 0)])
def test_rot_matches_oracle_and_monomial_products(torch_cuda, name, k):
    """test_cyclotomic (goldilocks/mod.rs:249-262, babybear/mod.rs:259-272, stark_prime/mod.rs:179-192, frog_ring/mod.rs:221-234):
    rot^i(a) == a * X^i with the product taken by the ring's own multiplication; rot == the oracle's on a batch."""
    torch = torch_cuda
    base = {"goldilocks24": "goldilocks", "babybear72": "babybear", "frog16": "frog"}.get(name, name)
    F = O.FIELD_ID[base]
    ring = ring_for(name, k)
    d, w, batch = ring.degree, ring.words_per_elem, 6
    tri = name in ("goldilocks24", "babybear72")
    a = O.fill_uniform(F, 0x90, 0, batch * d)
    assert np.array_equal(ring.rot(a.copy()), O.rot(F, a, d, tri))
    ta = torch.from_numpy(a.view(np.int64)).cuda()
    tout = torch.empty_like(ta)
    ring.rot_dev(tout, ta)
    assert np.array_equal(tout.cpu().numpy().view(np.uint64), O.rot(F, a, d, tri))
    cur = a[:w].copy()
    for i in range(1, min(d, 20)):
        cur = ring.rot(cur)
        xi = O.to_mont(F, [1 if j == i else 0 for j in range(d)])
        assert np.array_equal(cur, ring.mul(a[:w].copy(), xi))


# ----------------------------------------------------------------------------- threading (Send + Sync, rayon callers)
def test_concurrent_calls_on_shared_and_private_contexts(torch_cuda):
    """The reference's ring types are Send + Sync and rayon workers multiply concurrently (matrix.rs:174): several host threads
    call the host-pointer entry points at once, four on ONE shared context (serialised by the context's mutex) and four on
    contexts of their own; every result must equal the oracle's."""
    import threading

    from stark_rings_amd import CyclotomicRing

    F, k, batch = O.GOLDILOCKS, 13, 5
    shared = CyclotomicRing("goldilocks", k, device=0)
    jobs, errors = [], []
    for i in range(8):
        a = O.fill_uniform(F, 0x300 + i, 0, batch << k)
        b = O.fill_uniform(F, 0x400 + i, 0, batch << k)
        jobs.append((a, b, O.pow2_ring_mul(F, a, b, k, batch, 4)))

    def work(i):
        try:
            ring = shared if i < 4 else CyclotomicRing("goldilocks", k, device=0)
            a, b, want = jobs[i]
            for _ in range(3):
                if not np.array_equal(ring.mul(a, b), want):
                    errors.append("thread %d: product differs" % i)
                if not np.array_equal(ring.elementwise_icrt(ring.elementwise_crt(a.copy())), a):
                    errors.append("thread %d: round trip differs" % i)
            if ring is not shared:
                ring.close()
        except Exception as exc:  # noqa: BLE001 - reported below
            errors.append("thread %d: %r" % (i, exc))

    threads = [threading.Thread(target=work, args=(i,)) for i in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    shared.close()
    assert not errors, errors


@pytest.mark.parametrize("name,k,batch", [("goldilocks", 13, 83), ("babybear", 13, 83), ("stark", 8, 301), ("goldilocks24", 0, 30000)])
def test_host_pointer_pipeline_chunks_equal_one_shot(torch_cuda, name, k, batch):
    """SR_HOST_CHUNK_MB=1 cuts the host batches of the transform / product entry points into many chunks (ragged last one) that
    alternate between two staging lanes while a helper thread copies results out: same bytes as the oracle and as one shot."""
    import os

    base = {"goldilocks24": "goldilocks"}.get(name, name)
    F = O.FIELD_ID[base]
    ring = ring_for(name, k)
    n = batch * ring.degree
    a = O.fill_uniform(F, 0x501, 0, n)
    b = O.fill_uniform(F, 0x502, 0, n)
    one_fwd = ring.elementwise_crt(a.copy())
    one_mul = ring.mul(a, b)
    one_add = ring.add(a.copy(), b)
    os.environ["SR_HOST_CHUNK_MB"] = "1"
    try:
        fa = ring.elementwise_crt(a.copy())
        assert np.array_equal(fa, one_fwd)
        assert np.array_equal(ring.elementwise_icrt(fa.copy()), a)
        assert np.array_equal(ring.mul(a, b), one_mul)
        inplace = a.copy()
        assert np.array_equal(ring.mul(inplace, b, inplace), one_mul)       # out aliases a
        assert np.array_equal(ring.add(a.copy(), b), one_add)
        assert np.array_equal(ring.ntt_mul(fa.copy(), ring.elementwise_crt(b.copy())), ring.elementwise_crt(one_mul.copy()))
    finally:
        del os.environ["SR_HOST_CHUNK_MB"]
    if k:
        assert np.array_equal(one_mul, O.pow2_ring_mul(F, a, b, k, batch, 4))


def test_device_calls_on_two_streams_share_one_context(torch_cuda):
    """Two HIP streams interleave device-resident BabyBear products (D = 2^16: the register-tiled path keeps packed
    intermediates in context-owned scratch) on ONE context: the scratch hand-over between streams is ordered by an event."""
    torch = torch_cuda
    F, k, batch = O.BABYBEAR, 16, 6
    ring = ring_for("babybear", k)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    data = []
    for i in range(6):
        a = O.fill_uniform(F, 0x600 + i, 0, batch << k)
        b = O.fill_uniform(F, 0x700 + i, 0, batch << k)
        data.append((torch.from_numpy(a.view(np.int64)).cuda(), torch.from_numpy(b.view(np.int64)).cuda(),
                     O.pow2_ring_mul(F, a, b, k, batch, 4)))
    torch.cuda.synchronize()
    outs = []
    for i, (ta, tb, _) in enumerate(data):
        st = streams[i & 1]
        out = torch.empty_like(ta)
        ring.mul_dev(out, ta, tb, stream=st)
        outs.append(out)
    torch.cuda.synchronize()
    for out, (_, _, want) in zip(outs, data):
        assert np.array_equal(out.cpu().numpy().view(np.uint64), want)


# ----------------------------------------------------------------------------- "next" row 3: ark-serialize wire format
WIRE_CASES = [("goldilocks", 6), ("goldilocks", 0), ("babybear", 5), ("babybear", 1), ("babybear", 0), ("stark", 4), ("stark", 0),
              ("goldilocks24", 0),
              ("babybear72", 0), ("frog16", 0)]


def _base_field(name):
    return O.FIELD_ID[{"goldilocks24": "goldilocks", "babybear72": "babybear", "frog16": "frog"}.get(name, name)]


@pytest.mark.parametrize("name,k", WIRE_CASES)
def test_wire_format_matches_oracle(torch_cuda, name, k):
    """CanonicalSerialize / CanonicalDeserialize of ring elements (coeff_form.rs:154-189, ntt_form.rs:24) through the C ABI, host and
    device entry points, against the oracle's restatement of the ark-serialize bytes; round trip; InvalidData for an integer >= p."""
    from stark_rings_amd import RingError

    torch = torch_cuda
    F = _base_field(name)
    ring = ring_for(name, k)
    d, wb, batch = ring.degree, ring.wire_coeff_bytes, 37
    assert wb == O.wire_bytes(F)
    p = ring.modulus
    a = O.fill_uniform(F, 0xA1, 0, batch * d)
    a[:O.LIMBS[F] * min(d, 4)] = O.to_mont(F, [0, p - 1, 1, (p - 1) // 2][:min(d, 4)])
    want = O.serialize(F, a)
    got = ring.serialize(a)
    assert got.dtype == np.uint8 and got.size == batch * d * wb
    assert np.array_equal(got, want)
    assert np.array_equal(ring.deserialize(got), a)
    ta = torch.from_numpy(a.view(np.int64)).cuda()
    tw = torch.empty(batch * d * wb, dtype=torch.uint8, device="cuda")
    ring.serialize_dev(tw, ta)
    assert np.array_equal(tw.cpu().numpy(), want)
    tb = torch.zeros_like(ta)
    ring.deserialize_dev(tb, tw)
    assert torch.equal(ta, tb) and ring.wire_invalid_count() == 0
    # empty batch
    assert ring.serialize(np.zeros(0, dtype=np.uint64)).size == 0 and ring.deserialize(np.zeros(0, dtype=np.uint8)).size == 0
    # coefficients that are not below the modulus: the host form refuses, the device form reads 0 and counts them
    bad = want.copy()
    for coeff, v in ((1, p), (d * batch - 1, (1 << (8 * wb)) - 1)):
        bad[coeff * wb:(coeff + 1) * wb] = np.frombuffer(v.to_bytes(wb, "little"), dtype=np.uint8)
    with pytest.raises(RingError):
        ring.deserialize(bad)
    ring.deserialize_dev(tb, torch.from_numpy(bad).cuda())
    n_bad = 2 if d * batch - 1 != 1 else 1
    assert ring.wire_invalid_count() == n_bad and ring.wire_invalid_count() == 0
    ref, obad = O.deserialize(F, bad)
    assert obad == n_bad and np.array_equal(tb.cpu().numpy().view(np.uint64), ref)
    with pytest.raises(RingError):
        ring.deserialize(want[:-1])          # not a whole number of elements


@pytest.mark.parametrize("name,k", [("goldilocks", 5), ("babybear", 4), ("stark", 4), ("frog16", 0)])
def test_wire_container_framing(torch_cuda, name, k):
    """Vec<R>, Matrix<R> and SparseMatrix<R> (matrix.rs:111-145, sparse_matrix.rs:158-200) against the Python model's bytes; the
    device-resident sparse writer (elements encoded at their framed offsets) produces the same bytes."""
    from stark_rings_amd import wire

    torch = torch_cuda
    base = {"frog16": "frog"}.get(name, name)
    F = O.FIELD_ID[base]
    ring = ring_for(name, k)
    d, w = ring.degree, ring.words_per_elem
    n = 6
    a = O.fill_uniform(F, 0xA2, 0, n * d)
    std = O.from_mont(F, a)
    elems = [std[e * d:(e + 1) * d] for e in range(n)]
    v = wire.serialize_vec(ring, a)
    assert v.tobytes() == P.serialize_vec(base, elems)
    back, end = wire.deserialize_vec(ring, v)
    assert end == v.size and np.array_equal(back, a)
    m = wire.serialize_matrix(ring, a, 2, 3)
    assert m.tobytes() == P.serialize_matrix(base, [elems[0:3], elems[3:6]])
    mb, nr, nc = wire.deserialize_matrix(ring, m)
    assert (nr, nc) == (2, 3) and np.array_equal(mb, a)
    assert wire.serialize_matrix(ring, a[:0], 0, 0).tobytes() == (0).to_bytes(8, "little")
    rows = [[(a[0:w], 5), (a[w:2 * w], 0)], [], [(a[2 * w:3 * w], 11)], [(a[3 * w:4 * w], 2), (a[4 * w:5 * w], 3), (a[5 * w:6 * w], 4)]]
    model_rows = [[(elems[0], 5), (elems[1], 0)], [], [(elems[2], 11)], [(elems[3], 2), (elems[4], 3), (elems[5], 4)]]
    s = wire.serialize_sparse(ring, 4, 12, rows)
    assert s.tobytes() == P.serialize_sparse(base, 4, 12, model_rows)
    nr, nc, back_rows = wire.deserialize_sparse(ring, s)
    assert (nr, nc) == (4, 12) and [[c for _, c in r] for r in back_rows] == [[c for _, c in r] for r in rows]
    assert all(np.array_equal(x[0], y[0]) for rx, ry in zip(back_rows, rows) for x, y in zip(rx, ry))
    vals = torch.from_numpy(a.view(np.int64)).cuda()
    cols = torch.tensor([5, 0, 11, 2, 3, 4], dtype=torch.int32, device="cuda")
    row_ptr = torch.tensor([0, 2, 2, 3, 6], dtype=torch.int64, device="cuda")
    sd = wire.serialize_sparse_dev(ring, 4, 12, vals, cols, row_ptr)
    assert sd.cpu().numpy().tobytes() == s.tobytes()
    assert ring.wire_invalid_count() == 0
    # a misaligned element offset is refused on the device (counted, element skipped)
    offs = torch.tensor([0, 4 if name != "babybear" else 2], dtype=torch.int64, device="cuda")
    buf = torch.zeros(4 * d * ring.wire_coeff_bytes, dtype=torch.uint8, device="cuda")
    ring.serialize_dev(buf, vals[:2 * w], offsets=offs)
    assert ring.wire_invalid_count() == 1


# ----------------------------------------------------------------------------- "next" row 4: monomial helpers
def test_monomial_reference_kats_on_gpu(torch_cuda, kats):
    """test_monomial_ops / test_monomial_range_check (crates/ring/src/monomial.rs:100-137) on the ring they use (frog, D = 16),
    with the product taken by the ring multiplication of the C ABI."""
    from stark_rings_amd import RingError, monomial as M

    ring = ring_for("frog16", 0)
    kat = kats["monomial"]
    p = ring.modulus
    for a, ok in kat["range_check"]["cases"]:
        if ok:
            M.psi_range_check(ring, a % p)
        else:
            with pytest.raises(RingError):
                M.psi_range_check(ring, a % p)
    zero, one = M.zero_monomial(ring), M.unit_monomial(ring, 0)
    assert np.array_equal(ring.add(zero.copy(), one), one)
    x2 = M.monomial(ring, kat["ops"]["monomial_degrees"]["x2"], 1)
    x15 = M.monomial(ring, kat["ops"]["monomial_degrees"]["x15"], 1)
    assert M.to_ints(ring, ring.add(x2.copy(), x2))[2] == 2
    assert M.to_ints(ring, ring.mul(x2, x15))[1] == p - 1


@pytest.mark.parametrize("name,k", [("goldilocks", 6), ("babybear", 5), ("stark", 4), ("frog16", 0), ("goldilocks", 10)])
def test_monomial_helpers_match_model(torch_cuda, name, k):
    """psi, exp, exp_signed and the batched range check against the Python model (monomial.rs:36-93)."""
    from stark_rings_amd import RingError, monomial as M

    base = {"frog16": "frog"}.get(name, name)
    ring = ring_for(name, k)
    p, d = ring.modulus, ring.degree
    assert M.to_ints(ring, M.psi(ring)) == P.psi_table(d, p)
    for a in (0, 1, 5, d // 2 - 1, d // 2, d - 1, p - 1, p - 3, p - d // 2, p - d):
        assert M.to_ints(ring, M.exp(ring, a)) == P.exp_monomial(d, a, p)
        if P.center(a, p) < d:
            assert M.to_ints(ring, M.exp_signed(ring, a)) == P.exp_signed(d, a, p)
    with pytest.raises(RingError):
        M.exp(ring, d + 2)                    # the reference indexes past the coefficient array and panics
    log2d = d.bit_length() - 1
    vals = list(range(0, d)) + [p - v for v in range(1, d + 1)]
    got = M.psi_range_check_batch(ring, vals)
    assert got == [abs(v if v < d + 1 else v - p) < d // 2 for v in vals]
    if d <= 64:
        assert got == [P.psi_range_check(base, log2d, v) for v in vals]


def test_absurd_element_counts_are_refused(torch_cuda):
    """Counts whose byte size would wrap size_t are rejected before any size arithmetic (SR_E_INVALID), not launched."""
    from stark_rings_amd import _lib

    ring = ring_for("goldilocks", 10)
    lib = _lib.load()
    buf = np.zeros(1024, dtype=np.uint64)
    ptr = buf.ctypes.data_as(_lib.u64p)
    huge = (1 << 63) // 1024
    assert lib.sr_ntt_fwd_batch(ring._ctx, ptr, huge) != 0
    assert lib.sr_ring_mul_batch(ring._ctx, ptr, ptr, ptr, huge) != 0
    assert lib.sr_decompose_balanced_batch(ring._ctx, ptr, ptr, 4, 1 << 40, 1 << 30) != 0
    assert lib.sr_matvec_ntt(ring._ctx, ptr, ptr, ptr, 1 << 40, 1 << 30) != 0
    assert "too large" in _lib.last_error()
    assert np.array_equal(ring.elementwise_icrt(ring.elementwise_crt(buf.copy())), buf)   # the context is still usable


@pytest.mark.parametrize("name,k", [("stark", 3), ("stark", 0), ("babybear", 3), ("goldilocks", 3)])
def test_long_sums_of_extreme_products(torch_cuda, name, k):
    """The linear-algebra kernels sum pre(a, b) terms and apply post() once (Stark: uncarried 28-bit limbs, weakly reduced every
    four terms).  Inner dimension 41 with every entry p - 1, then p - 1 against 1, then random: dense mat-vec, mat-mat and a
    sparse row whose bad column indices are skipped must all equal the integer sums; SR_STARK_LAZY=0 (8 x 32-bit limbs) agrees."""
    import os

    from stark_rings_amd import CyclotomicRing

    torch = torch_cuda
    F, p = O.FIELD_ID[name], P.PRIMES[name][0]
    ring = ring_for(name, k)
    d, w, L = ring.degree, ring.words_per_elem, O.LIMBS[F]
    rinv = pow(pow(2, 64 * L, p), -1, p)
    nrows, ncols = 5, 41
    for case in range(3):
        if case == 0:
            mi, vi = [p - 1] * (nrows * ncols * d), [p - 1] * (ncols * d)
        elif case == 1:
            mi, vi = [p - 1] * (nrows * ncols * d), [1] * (ncols * d)
        else:
            mi = O.from_mont(F, O.fill_uniform(F, 0x7A, 0, nrows * ncols * d))
            vi = O.from_mont(F, O.fill_uniform(F, 0x7B, 0, ncols * d))
        m, v = O.to_mont(F, mi), O.to_mont(F, vi)
        want = []
        for r in range(nrows):
            for s_ in range(d):
                want.append(sum(mi[(r * ncols + c) * d + s_] * vi[c * d + s_] for c in range(ncols)) % p)
        got = ring.matvec_ntt(m, v, nrows, ncols)
        assert O.from_mont(F, got) == want, case
        # the same numbers as a (5 x 41) (41 x 1) matrix product
        assert np.array_equal(ring.matmul_ntt(m, v, nrows, ncols, 1), got)
        # sparse row 0 = dense row 0 with three out-of-range columns mixed in (skipped and counted on the device)
        tv = torch.from_numpy(v.view(np.int64)).cuda()
        cols = list(range(ncols))
        vals = [m[c * w:(c + 1) * w] for c in range(ncols)]
        for at in (3, 7, 40):
            cols.insert(at, ncols + 5)
            vals.insert(at, m[:w])
        tvals = torch.from_numpy(np.concatenate(vals).view(np.int64)).cuda()
        tcols = torch.tensor(cols, dtype=torch.int32, device="cuda")
        tptr = torch.tensor([0, len(cols)], dtype=torch.int64, device="cuda")
        ty = torch.empty(w, dtype=torch.int64, device="cuda")
        ring.spmv_ntt_dev(ty, tvals, tcols, tptr, tv, 1, ncols)
        assert ring.spmv_bad_index_count() == 3
        assert np.array_equal(ty.cpu().numpy().view(np.uint64), got[:w])
        if name == "stark" and k > 0:
            os.environ["SR_STARK_LAZY"] = "0"
            try:
                other = CyclotomicRing("stark", k, device=0)
                assert np.array_equal(other.matvec_ntt(m, v, nrows, ncols), got)
                other.close()
            finally:
                del os.environ["SR_STARK_LAZY"]
    assert rinv  # (Montgomery images cancel: products of images are taken by the kernels' own boundary product)


# ----------------------------------------------------------------------------- round 2: operands are never written; constant-operand product
def _plan(**kw):
    from stark_rings_amd import _lib

    p = _lib.Plan()
    for key, val in kw.items():
        setattr(p, key, val)
    return p


_PLANS_INTACT = [
    ("goldilocks", 13, {}), ("goldilocks", 16, {}), ("goldilocks", 17, {}), ("goldilocks", 16, {"flags": 2}),   # 2 = SR_PLAN_GL_NO_COLS256
    ("goldilocks", 14, {"flags": 1}), ("goldilocks", 16, {"flags": 8}),                                         # generic kernels; register-tiled
    ("babybear", 16, {}), ("babybear", 14, {}), ("babybear", 13, {"flags": 1}), ("babybear", 16, {"flags": 4}),
    ("stark", 12, {}), ("stark", 13, {}), ("stark", 12, {"flags": 32}), ("stark", 11, {"flags": 16}), ("stark", 12, {"stark_whole_max": 12}),
]


@pytest.mark.parametrize("name,k,plan", _PLANS_INTACT)
def test_ring_mul_leaves_both_operands_intact(torch_cuda, name, k, plan):
    """coeff_form.rs:250-258: `a * &b` never mutates an operand.  Every prime, D above one tile, every kernel plan: a and b are
    bit-identical after the call, and ONE b multiplied into several a gives the oracle's products each time."""
    torch = torch_cuda
    from stark_rings_amd import CyclotomicRing

    F = O.FIELD_ID[name]
    ring = CyclotomicRing(name, k, device=0, plan=_plan(**plan))
    batch = 3
    n = batch << k
    b = O.fill_uniform(F, 77, 0, n)
    tb = torch.from_numpy(b.view(np.int64)).cuda()
    for seed in (5, 6):
        a = O.fill_uniform(F, seed, 0, n)
        ta = torch.from_numpy(a.view(np.int64)).cuda()
        out = torch.empty_like(ta)
        ring.mul_dev(out, ta, tb)
        torch.cuda.synchronize()
        assert np.array_equal(tb.cpu().numpy().view(np.uint64), b), "b was written"
        assert np.array_equal(ta.cpu().numpy().view(np.uint64), a), "a was written"
        assert np.array_equal(out.cpu().numpy().view(np.uint64), O.pow2_ring_mul(F, a, b, k, batch, 4))
    # host form, same contract
    a = O.fill_uniform(F, 9, 0, n)
    a0, b0 = a.copy(), b.copy()
    got = ring.mul(a, b)
    assert np.array_equal(a, a0) and np.array_equal(b, b0)
    assert np.array_equal(got, O.pow2_ring_mul(F, a, b, k, batch, 4))
    ring.close()


@pytest.mark.parametrize("name,k", [("goldilocks", 16), ("goldilocks", 13), ("stark", 12), ("babybear", 13)])
def test_ring_mul_in_chunks_of_the_operand_scratch(torch_cuda, name, k):
    """A scratch cap below the batch (sr_plan.scratch_limit_bytes / chunk_polys) cuts the product into chunks: same results,
    ragged last chunk included; sr_ctx_reserve_scratch pre-sizes the scratch."""
    torch = torch_cuda
    from stark_rings_amd import CyclotomicRing

    F = O.FIELD_ID[name]
    L = O.LIMBS[F]
    batch = 7
    elem_bytes = (8 * L) << k
    flags = 1 if name == "babybear" else 0   # BabyBear's register-tiled path owns packed scratch of its own: test the generic path here
    for plan in (_plan(flags=flags, scratch_limit_bytes=3 * elem_bytes), _plan(flags=flags, chunk_polys=2)):
        ring = CyclotomicRing(name, k, device=0, plan=plan)
        ring.reserve_scratch(batch)
        n = batch << k
        a = O.fill_uniform(F, 21, 0, n)
        b = O.fill_uniform(F, 22, 0, n)
        ta = torch.from_numpy(a.view(np.int64)).cuda()
        tb = torch.from_numpy(b.view(np.int64)).cuda()
        out = torch.empty_like(ta)
        ring.mul_dev(out, ta, tb)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint64), O.pow2_ring_mul(F, a, b, k, batch, 4))
        assert np.array_equal(tb.cpu().numpy().view(np.uint64), b)
        ring.close()


_RHS_CASES = [("goldilocks", k) for k in (4, 8, 10, 12, 13, 16, 17)] + [("babybear", 10), ("babybear", 16), ("stark", 4), ("stark", 12),
                                                                       ("goldilocks24", 0), ("babybear72", 0), ("frog16", 0)]


@pytest.mark.parametrize("name,k", _RHS_CASES)
def test_ring_mul_with_ntt_form_rhs(torch_cuda, name, k):
    """sr_ring_mul_ntt_rhs_batch_dev: out = icrt(crt(a) (.) b_ntt) == a * b for b_ntt = crt(b) -- the constant-operand product
    (one transform fewer); fused on the tuned Goldilocks path, composed elsewhere.  a and b_ntt are only read; ragged batch."""
    torch = torch_cuda
    ring = ring_for(name, k)
    w = ring.words_per_elem
    batch = 5
    base = {"goldilocks24": "goldilocks", "babybear72": "babybear", "frog16": "frog"}.get(name, name)
    F = O.FIELD_ID[base]
    a = O.fill_uniform(F, 31, 0, batch * ring.degree)
    b = O.fill_uniform(F, 32, 0, batch * ring.degree)
    ta = torch.from_numpy(a.view(np.int64)).cuda()
    tb = torch.from_numpy(b.view(np.int64)).cuda()
    want = torch.empty_like(ta)
    ring.mul_dev(want, ta, tb)
    tbn = tb.clone()
    ring.elementwise_crt_dev(tbn)
    keep = tbn.clone()
    out = torch.empty_like(ta)
    ring.mul_ntt_rhs_dev(out, ta, tbn)
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    assert torch.equal(tbn, keep), "b_ntt was written"
    assert np.array_equal(ta.cpu().numpy().view(np.uint64), a), "a was written"
    # in place on a
    ring.mul_ntt_rhs_dev(ta, ta, tbn)
    assert torch.equal(ta, want)
    assert w * batch == ta.numel()
    # host-pointer form
    assert np.array_equal(ring.mul_ntt_rhs(a, ring.elementwise_crt(b.copy())), want.cpu().numpy().view(np.uint64))


def test_plan_struct_is_validated_and_env_free(torch_cuda):
    """sr_ctx_create_ex refuses malformed plans; the library exports no behaviour switch through the environment."""
    from stark_rings_amd import CyclotomicRing, RingError

    for bad in (_plan(flags=1 << 9), _plan(log_tile=7), _plan(log_tile=13), _plan(stark_whole_max=8), _plan(lanes=3)):
        with pytest.raises(RingError):
            CyclotomicRing("goldilocks", 10, device=0, plan=bad)
    import glob
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for path in glob.glob(os.path.join(root, "stark_rings_amd", "csrc", "*")):
        assert "getenv" not in open(path).read(), path


# ----------------------------------------------------------------------------- round 2: linear algebra over the reference's own RqNTT types
_SMALL_LA = [("goldilocks24", "goldilocks", "sro_g24_ntt_mul"), ("babybear72", "babybear", "sro_bb72_ntt_mul"), ("frog16", "frog", "sro_frog16_ntt_mul")]


def _oracle_slot_dot(fn, F, p, rows_m, vec, d):
    """sum_c M[c] * v[c] for ring elements in NTT form: oracle slot products (Fq3 / Fq9 / Fq4), coefficient-wise integer sums."""
    acc = [0] * d
    for mc, vc in zip(rows_m, vec):
        prod = O.from_mont(F, O.small(fn, mc, vc))
        acc = [(x + y) % p for x, y in zip(acc, prod)]
    return acc


@pytest.mark.parametrize("name,base,fn", _SMALL_LA)
def test_linear_algebra_over_the_reference_rings(torch_cuda, name, base, fn):
    """Matrix<R>::checked_mul_vec / checked_mul_mat (matrix.rs:148-178) and SparseMatrix<R>::checked_mul_vec
    (sparse_matrix.rs:201-212) for R = the RqNTT types the reference actually ships (Fq3 / Fq9 / Fq4 slots): every output is the
    oracle's slot products summed as integers.  Inner dimension 41 with every coefficient p - 1, then random."""
    torch = torch_cuda
    F = O.FIELD_ID[base]
    p = P.PRIMES[base][0]
    ring = ring_for(name, 0)
    d = ring.degree
    nrows, ncols = 3, 41
    for case in range(2):
        if case == 0:
            m = O.to_mont(F, [p - 1] * (nrows * ncols * d))
            v = O.to_mont(F, [p - 1] * (ncols * d))
        else:
            m = O.fill_uniform(F, 0x51, 0, nrows * ncols * d)
            v = O.fill_uniform(F, 0x52, 0, ncols * d)
        el = lambda buf, i: buf[i * d:(i + 1) * d]
        want = []
        for r in range(nrows):
            want += _oracle_slot_dot(fn, F, p, [el(m, r * ncols + c) for c in range(ncols)], [el(v, c) for c in range(ncols)], d)
        got = ring.matvec_ntt(m, v, nrows, ncols)
        assert O.from_mont(F, got) == want, (name, case)
        assert np.array_equal(ring.matmul_ntt(m, v, nrows, ncols, 1), got)
        # (2 x 41) (41 x 3): B's columns are v, 2v (= v + v) and v again
        v2 = ring.add(v.copy(), v)
        b = np.concatenate([np.concatenate([el(v, c), el(v2, c), el(v, c)]) for c in range(ncols)])
        y = ring.matmul_ntt(m[:2 * ncols * d], b, 2, ncols, 3)
        for i in range(2):
            row = O.from_mont(F, got[i * d:(i + 1) * d])
            assert O.from_mont(F, el(y, i * 3 + 0)) == row and O.from_mont(F, el(y, i * 3 + 2)) == row
            assert O.from_mont(F, el(y, i * 3 + 1)) == [(2 * x) % p for x in row]
        # sparse: row 0 = dense row 0 with bad columns mixed in (skipped + counted), row 1 empty, row 2 = two entries
        tv = torch.from_numpy(v.view(np.int64)).cuda()
        cols = list(range(ncols))
        vals = [el(m, c) for c in range(ncols)]
        for at in (2, 17):
            cols.insert(at, ncols + 1)
            vals.insert(at, el(m, 0))
        cols += [5, 40]
        vals += [el(m, 7), el(m, 9)]
        tvals = torch.from_numpy(np.concatenate(vals).view(np.int64)).cuda()
        tcols = torch.tensor(cols, dtype=torch.int32, device="cuda")
        tptr = torch.tensor([0, ncols + 2, ncols + 2, ncols + 4], dtype=torch.int64, device="cuda")
        ty = torch.empty(3 * d, dtype=torch.int64, device="cuda")
        ring.spmv_ntt_dev(ty, tvals, tcols, tptr, tv, 3, ncols)
        assert ring.spmv_bad_index_count() == 2
        sy = ty.cpu().numpy().view(np.uint64)
        assert np.array_equal(sy[:d], got[:d])
        assert not sy[d:2 * d].any()
        assert O.from_mont(F, sy[2 * d:]) == _oracle_slot_dot(fn, F, p, [el(m, 7), el(m, 9)], [el(v, 5), el(v, 40)], d)
    # host sparse form refuses an out-of-range column (the reference panics on v[col]); empty shapes
    from stark_rings_amd import RingError
    with pytest.raises(RingError):
        ring.spmv_ntt([[(el(m, 0), ncols)]], v, ncols)
    assert ring.matvec_ntt(np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint64), 0, 0).size == 0
    z = ring.matvec_ntt(np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint64), 2, 0)
    assert z.size == 2 * d and not z.any()


@pytest.mark.parametrize("name,base,fn", _SMALL_LA)
def test_small_ring_linear_algebra_long_rows_and_ragged_blocks(torch_cuda, name, base, fn):
    """Round 3: the small-ring products sum slot products as INTEGERS (96-bit accumulators per power of X, one Montgomery step and
    one fold by the non-residue at the end, csrc/small_linalg.hpp), a short-and-wide mat-vec is cut into row parts over several
    workgroups, and mat-mat works on 2 x 2 output blocks.  Pinned here: 2 rows x 700 columns with every coefficient p - 1 (the
    largest integer sums; row parts in use) and random, against the oracle's slot products; mat-mat with odd n and p (ragged
    blocks) and an inner dimension that is not a multiple of the term groups, against mat-vec column by column."""
    F = O.FIELD_ID[base]
    p = P.PRIMES[base][0] if base in P.PRIMES else P.FROG_P
    ring = ring_for(name, 0)
    d = ring.degree
    el = lambda buf, i: buf[i * d:(i + 1) * d]
    nrows, ncols = 2, 700
    for case in range(2):
        if case == 0:
            m = O.to_mont(F, [p - 1] * (nrows * ncols * d))
            v = O.to_mont(F, [p - 1] * (ncols * d))
        else:
            m = O.fill_uniform(F, 0x61, 0, nrows * ncols * d)
            v = O.fill_uniform(F, 0x62, 0, ncols * d)
        got = ring.matvec_ntt(m, v, nrows, ncols)
        for r in range(nrows):
            want = _oracle_slot_dot(fn, F, p, [el(m, r * ncols + c) for c in range(ncols)], [el(v, c) for c in range(ncols)], d)
            assert O.from_mont(F, el(got, r)) == want, (name, case, r)
    # (5 x 23) (23 x 3): every output against the mat-vec of its row block with its column
    n, mm, pp = 5, 23, 3
    a = O.fill_uniform(F, 0x63, 0, n * mm * d)
    b = O.fill_uniform(F, 0x64, 0, mm * pp * d)
    a[:d] = O.to_mont(F, [p - 1] * d)
    y = ring.matmul_ntt(a, b, n, mm, pp)
    for j in range(pp):
        col = np.concatenate([el(b, t * pp + j) for t in range(mm)])
        yj = ring.matvec_ntt(a, col, n, mm)
        for i in range(n):
            assert np.array_equal(el(y, i * pp + j), el(yj, i)), (name, i, j)
    want00 = _oracle_slot_dot(fn, F, p, [el(a, t) for t in range(mm)], [el(b, t * pp) for t in range(mm)], d)
    assert O.from_mont(F, el(y, 0)) == want00


# ----------------------------------------------------------------------------- round 2: GadgetDecompose for Matrix / SparseMatrix
@pytest.mark.parametrize("name,k,basis,pad", [("goldilocks", 4, 4, 33), ("babybear", 3, 16, 9), ("goldilocks24", 0, 1 << 16, 5), ("stark", 2, 1 << 32, 9)])
def test_matrix_and_sparse_matrix_gadget_decompose(torch_cuda, name, k, basis, pad):
    """balanced_decomposition/mod.rs:276-352: Matrix<R> n x m -> n x (k m) row by row; SparseMatrix<R> entry (e, c) ->
    (digit_i, c k + i) with zero digits dropped; recompose inverts both.  Digits are the oracle's."""
    base = {"goldilocks24": "goldilocks"}.get(name, name)
    F = O.FIELD_ID[base]
    p = P.PRIMES[base][0]
    ring = ring_for(name, k)
    d, w = ring.degree, ring.words_per_elem
    nrows, ncols = 3, 4
    mat = O.fill_uniform(F, 0x91, 0, nrows * ncols * d)
    small = O.to_mont(F, [1] + [0] * (d - 1))          # the constant 1: exactly one non-zero digit in any basis
    mat[5 * w:6 * w] = small
    dec, r2, c2 = ring.matrix_gadget_decompose(mat, nrows, ncols, basis, pad)
    assert (r2, c2) == (nrows, ncols * pad)
    want, over = O.decompose_balanced(F, mat, d, nrows * ncols, basis, pad)
    assert not over and np.array_equal(dec, want)
    # entry (r, c) of the input is the recomposition of entries (r, c k .. c k + k - 1) of the output
    back, r3, c3 = ring.matrix_gadget_recompose(dec, r2, c2, basis, pad)
    assert (r3, c3) == (nrows, ncols) and np.array_equal(back, mat)
    # sparse: rows with 2, 0 and 3 stored entries
    el = lambda i: mat[i * w:(i + 1) * w]
    rows = [[(el(0), 1), (el(1), 3)], [], [(el(4), 0), (el(5), 2), (el(6), 3)]]
    srows, sc = ring.sparse_gadget_decompose(rows, ncols, basis, pad)
    assert sc == ncols * pad and len(srows) == 3 and srows[1] == []
    for row, srow in zip(rows, srows):
        exp = []
        for e, c in row:
            dg, _ = O.decompose_balanced(F, np.ascontiguousarray(e), d, 1, basis, pad)
            exp += [(dg[i * w:(i + 1) * w], c * pad + i) for i in range(pad) if dg[i * w:(i + 1) * w].any()]
        assert len(srow) == len(exp)
        for (g, gc), (x, xc) in zip(srow, exp):
            assert gc == xc and np.array_equal(g, x)
    assert len([1 for e, c in srows[2] if c // pad == 2]) == 1      # the small element keeps ONE non-zero digit
    rrows, rc = ring.sparse_gadget_recompose(srows, sc, basis, pad)
    assert rc == ncols
    for row, rrow in zip(rows, rrows):
        assert len(row) == len(rrow)
        for (e, c), (g, gc) in zip(row, rrow):
            assert c == gc and np.array_equal(e, g)


def test_context_group_shares_one_twiddle_block(torch_cuda):
    """sr_ctx_create_group: n contexts whose tables are peer copies of the first one's, and sr_shard_range == sharding.shard_range.
    The test widens itself: on a box with several visible GPUs the group spans min(count, 8) DISTINCT devices -- the
    twiddle block then really crosses xGMI (hipMemcpyPeer between two devices), every context computes on ITS device's buffers from
    a host thread of its own (contexts on different devices run concurrently; what a single-process Rust host with one rayon worker
    per GPU does), and every shard is checked against the oracle.  With one GPU the ids are {0, 0}: the same call
    path, both contexts on device 0.  The id selection itself is unit-tested on the CPU (tests/test_sharding_gloo.py)."""
    import ctypes
    import threading

    torch = torch_cuda
    from stark_rings_amd import _lib
    from stark_rings_amd.sharding import group_device_ids, shard_range

    lib = _lib.load()
    dev_ids = group_device_ids(torch.cuda.device_count())
    n = len(dev_ids)
    ids = (ctypes.c_int * n)(*dev_ids)
    ctxs = (ctypes.c_void_p * n)()
    k, batch = 13, 5 if n == 2 else 3 * n + 1
    assert lib.sr_ctx_create_group(0, k, ids, n, None, ctxs) == 0, _lib.last_error()
    try:
        F = O.GOLDILOCKS
        a = O.fill_uniform(F, 3, 0, batch << k)
        b = O.fill_uniform(F, 4, 0, batch << k)
        want = O.pow2_ring_mul(F, a, b, k, batch, 4)
        got, errors = [None] * n, []

        def work(i):
            try:
                first, count = ctypes.c_size_t(), ctypes.c_size_t()
                assert lib.sr_shard_range(batch, n, i, ctypes.byref(first), ctypes.byref(count)) == 0
                assert (first.value, count.value) == shard_range(batch, n, i)
                lo, hi = first.value << k, (first.value + count.value) << k
                dev = torch.device("cuda", dev_ids[i])
                with torch.cuda.device(dev):
                    ta = torch.from_numpy(a[lo:hi].copy().view(np.int64)).to(dev)
                    tb = torch.from_numpy(b[lo:hi].copy().view(np.int64)).to(dev)
                    out = torch.empty_like(ta)
                    st = torch.cuda.current_stream(dev)
                    rc = lib.sr_ring_mul_batch_dev(ctxs[i], ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(ta.data_ptr()),
                                                   ctypes.c_void_p(tb.data_ptr()), count.value, ctypes.c_void_p(st.cuda_stream))
                    assert rc == 0, _lib.last_error()
                    st.synchronize()
                    got[i] = (lo, hi, out.cpu().numpy().view(np.uint64))
            except BaseException as e:  # noqa: BLE001 -- reported by the main thread
                errors.append((i, repr(e)))

        threads = [threading.Thread(target=work, args=(i,)) for i in range(n)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        for i, (lo, hi, part) in enumerate(got):
            assert np.array_equal(part, want[lo:hi]), "shard %d (device %d)" % (i, dev_ids[i])
        assert sum(hi - lo for lo, hi, _ in got) == batch << k
        first, count = ctypes.c_size_t(), ctypes.c_size_t()
        assert lib.sr_shard_range(5, 2, 2, ctypes.byref(first), ctypes.byref(count)) != 0
    finally:
        for c in ctxs:
            lib.sr_ctx_destroy(c)


@pytest.mark.parametrize("name,k,batch", [("goldilocks", 13, 70), ("goldilocks", 16, 67), ("babybear", 16, 67), ("babybear", 13, 70)])
def test_ring_mul_in_default_chunks(torch_cuda, name, k, batch):
    """Default plan of the tuned Goldilocks path and of the register-tiled BabyBear path for batches >= 64 above one tile: eight chunks of launches through a scratch of one
    chunk (ragged last chunk here); a plan with chunk_polys = batch runs one set of launches.  Same products, operands intact, and
    work queued behind the call on the caller's stream sees the results."""
    torch = torch_cuda
    from stark_rings_amd import CyclotomicRing

    F = O.FIELD_ID[name]
    n = batch << k
    a = O.fill_uniform(F, 0x61, 0, n)
    b = O.fill_uniform(F, 0x62, 0, n)
    want = O.pow2_ring_mul(F, a, b, k, batch, 8)
    for plan in (_plan(), _plan(chunk_polys=batch)):
        ring = CyclotomicRing(name, k, device=0, plan=plan)
        ta = torch.from_numpy(a.view(np.int64)).cuda()
        tb = torch.from_numpy(b.view(np.int64)).cuda()
        out = torch.empty_like(ta)
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            ring.mul_dev(out, ta, tb, stream=st)
            copy = out.clone()            # queued on the caller's stream right behind the call
        st.synchronize()
        assert np.array_equal(copy.cpu().numpy().view(np.uint64), want)
        assert np.array_equal(tb.cpu().numpy().view(np.uint64), b)
        with torch.cuda.stream(st):
            ring.mul_dev(out, out, tb, stream=st)
            ring.mul_ntt_rhs_dev(ta, ta, ring.elementwise_crt_dev(tb.clone(), stream=st), stream=st)
        st.synchronize()
        assert torch.equal(ta, copy)
        ring.close()


@pytest.mark.parametrize("name,k,batch", [("goldilocks", 16, 9), ("goldilocks", 16, 24), ("goldilocks", 17, 5), ("goldilocks", 18, 3), ("goldilocks", 20, 1),
                                          ("babybear", 16, 9), ("babybear", 16, 16), ("babybear", 20, 1)])
def test_column_pass_tile_order_covers_every_tile(torch_cuda, name, k, batch):
    """The column passes hand runs of 16 (8 on the register-tiled path) consecutive tiles to one XCD (xcd_tile, csrc/fields.hpp); launches whose
    tile count is not a multiple of 8 runs keep the plain order for the rest.  One set of launches per call (chunk_polys = batch), batches
    with and without such a rest: every coefficient of every element must still be transformed exactly once -- product, forward and inverse
    transform against the oracle."""
    torch = torch_cuda
    from stark_rings_amd import CyclotomicRing

    F = O.FIELD_ID[name]
    n = batch << k
    a = O.fill_uniform(F, 0x71, 0, n)
    b = O.fill_uniform(F, 0x72, 0, n)
    ring = CyclotomicRing(name, k, device=0, plan=_plan(chunk_polys=batch))
    ta = torch.from_numpy(a.view(np.int64)).cuda()
    tb = torch.from_numpy(b.view(np.int64)).cuda()
    out = torch.empty_like(ta)
    ring.mul_dev(out, ta, tb)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), O.pow2_ring_mul(F, a, b, k, batch, 8))
    ring.elementwise_crt_dev(ta)
    torch.cuda.synchronize()
    assert np.array_equal(ta.cpu().numpy().view(np.uint64), O.pow2_fwd(F, a, k, batch, 8))
    ring.elementwise_icrt_dev(ta)
    torch.cuda.synchronize()
    assert np.array_equal(ta.cpu().numpy().view(np.uint64), a)
    ring.close()


@pytest.mark.parametrize("k,batch,plan_kw", [(16, 460, {}), (16, 300, {"chunk_polys": 64}), (16, 131, {"chunk_polys": 1}), (17, 7, {"chunk_polys": 2}),
                                             (20, 3, {"chunk_polys": 1}), (16, 300, {"lanes": 1}), (16, 129, {"scratch_limit_bytes": 16 << 20})])
def test_goldilocks_product_on_two_lanes(torch_cuda, k, batch, plan_kw):
    """Tuned Goldilocks product above one chunk: chunks dealt to two internal streams, each with its own scratch pair (gl_fast_ring_mul_chunk);
    ragged last chunks, chunk of one element, a scratch cap that shrinks the chunk, and the one-stream plan (lanes = 1) for comparison.  Against the
    oracle: out of place with operands intact, then in place over a (out == a) and squaring (a and b the same buffer), and a second call on ANOTHER
    caller stream right behind the first (the scratch is ordered across streams by an event)."""
    torch = torch_cuda
    from stark_rings_amd import CyclotomicRing

    F = O.GOLDILOCKS
    n = batch << k
    a = O.fill_uniform(F, 0x81, 0, n)
    b = O.fill_uniform(F, 0x82, 0, n)
    want = O.pow2_ring_mul(F, a, b, k, batch, 8)
    ring = CyclotomicRing("goldilocks", k, device=0, plan=_plan(**plan_kw))
    ta = torch.from_numpy(a.view(np.int64)).cuda()
    tb = torch.from_numpy(b.view(np.int64)).cuda()
    out = torch.empty_like(ta)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        ring.mul_dev(out, ta, tb, stream=s1)
    with torch.cuda.stream(s2):
        out2 = torch.empty_like(ta)
        ring.mul_dev(out2, tb, ta, stream=s2)  # commutes; queued on another stream while the first call's lanes still run
    s1.synchronize()
    s2.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), want)
    assert np.array_equal(out2.cpu().numpy().view(np.uint64), want)
    assert np.array_equal(ta.cpu().numpy().view(np.uint64), a) and np.array_equal(tb.cpu().numpy().view(np.uint64), b)
    ring.mul_dev(ta, ta, tb)   # in place over a
    torch.cuda.synchronize()
    assert np.array_equal(ta.cpu().numpy().view(np.uint64), want)
    ring.mul_dev(out, tb, tb)  # squaring (a and b the same buffer)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), O.pow2_ring_mul(F, b, b, k, batch, 8))
    # the stand-alone transforms take the same lanes (in place, two launches per chunk)
    tt = torch.from_numpy(a.view(np.int64)).cuda()
    ring.elementwise_crt_dev(tt)
    torch.cuda.synchronize()
    assert np.array_equal(tt.cpu().numpy().view(np.uint64), O.pow2_fwd(F, a, k, batch, 8))
    ring.elementwise_icrt_dev(tt)
    torch.cuda.synchronize()
    assert np.array_equal(tt.cpu().numpy().view(np.uint64), a)
    del tt
    # the constant-operand product takes the same lanes (three launches per chunk)
    ta = torch.from_numpy(a.view(np.int64)).cuda()
    tbn = tb.clone()
    ring.elementwise_crt_dev(tbn)
    keep = tbn.clone()
    ring.mul_ntt_rhs_dev(out, ta, tbn)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), want)
    assert torch.equal(tbn, keep) and np.array_equal(ta.cpu().numpy().view(np.uint64), a)
    ring.close()


@pytest.mark.parametrize("name,k,batch,plan_kw", [("babybear", 16, 600, {}), ("babybear", 16, 300, {"chunk_polys": 64}), ("babybear", 14, 70, {"chunk_polys": 8}),
                                                  ("babybear", 20, 3, {"chunk_polys": 1}), ("babybear", 16, 300, {"lanes": 1}),
                                                  ("goldilocks", 16, 300, {"flags": 8, "chunk_polys": 64})])  # 8 = SR_PLAN_GL_REGTILE
def test_register_tiled_product_on_two_lanes(torch_cuda, name, k, batch, plan_kw):
    """The register-tiled product (BabyBear; Goldilocks by plan flag) in chunks on the context's two streams, each lane with its own pair of
    packed scratch buffers: against the oracle, operands intact, in place over a, and a second call queued on another stream."""
    torch = torch_cuda
    from stark_rings_amd import CyclotomicRing

    F = O.FIELD_ID[name]
    n = batch << k
    a = O.fill_uniform(F, 0x91, 0, n)
    b = O.fill_uniform(F, 0x92, 0, n)
    want = O.pow2_ring_mul(F, a, b, k, batch, 8)
    ring = CyclotomicRing(name, k, device=0, plan=_plan(**plan_kw))
    ta = torch.from_numpy(a.view(np.int64)).cuda()
    tb = torch.from_numpy(b.view(np.int64)).cuda()
    out = torch.empty_like(ta)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        ring.mul_dev(out, ta, tb, stream=s1)
    with torch.cuda.stream(s2):
        out2 = torch.empty_like(ta)
        ring.mul_dev(out2, tb, ta, stream=s2)
    s1.synchronize()
    s2.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), want)
    assert np.array_equal(out2.cpu().numpy().view(np.uint64), want)
    assert np.array_equal(ta.cpu().numpy().view(np.uint64), a) and np.array_equal(tb.cpu().numpy().view(np.uint64), b)
    ring.mul_dev(ta, ta, tb)
    torch.cuda.synchronize()
    assert np.array_equal(ta.cpu().numpy().view(np.uint64), want)
    # the stand-alone transforms take the same lanes (a packed scratch buffer per lane)
    tt = torch.from_numpy(a.view(np.int64)).cuda()
    ring.elementwise_crt_dev(tt)
    torch.cuda.synchronize()
    assert np.array_equal(tt.cpu().numpy().view(np.uint64), O.pow2_fwd(F, a, k, batch, 8))
    ring.elementwise_icrt_dev(tt)
    torch.cuda.synchronize()
    assert np.array_equal(tt.cpu().numpy().view(np.uint64), a)
    ring.close()


@pytest.mark.parametrize("name,k", [("stark", 3), ("goldilocks", 4), ("babybear", 3), ("frog16", 0)])
@pytest.mark.parametrize("basis", [1 << 64, (1 << 64) + 2, 3 * (1 << 70) + 6, 1 << 100, (1 << 127) - 2])
def test_decomposition_with_u128_bases(torch_cuda, name, k, basis):
    """decompose_balanced_in_place takes b: u128 (balanced_decomposition/mod.rs:62-117).  Bases of 2^64 and more through the _wide entry
    points against the big-integer model (oracle/pyref.py): for the 252-bit prime a real multi-digit decomposition, for the one-limb
    fields digit 0 = the coefficient and zeros behind it.  recompose(decompose(x)) == x; |digit| <= b / 2."""
    torch = torch_cuda
    base = {"frog16": "frog"}.get(name, name)
    F = O.FIELD_ID[base]
    p = P.PRIMES[base][0] if base in P.PRIMES else P.FROG_P
    ring = ring_for(name, k)
    d, w, batch = ring.degree, ring.words_per_elem, 3
    vals = O.from_mont(F, O.fill_uniform(F, 0xD1, 0, batch * d))
    edge = [0, 1, p - 1, (p - 1) // 2, (p - 1) // 2 + 1, basis % p, (basis // 2) % p, (basis // 2 + 1) % p, (p - basis // 2) % p]
    vals[:len(edge)] = edge
    a = O.to_mont(F, vals)
    pad = 1
    while (basis // 2) * (basis ** pad - 1) // (basis - 1) < (p - 1) // 2:
        pad += 1
    pad += 1
    got = ring.gadget_decompose(a, basis, pad)
    digits = O.from_mont(F, got)
    for e in range(batch):
        for i in range(d):
            want = P.decompose_balanced(vals[e * d + i], p, basis, pad)
            mine = [digits[(e * pad + j) * d + i] for j in range(pad)]
            assert [x % p for x in want] == mine, (name, basis, vals[e * d + i])
            assert all(abs(x) <= basis // 2 for x in want)
    assert np.array_equal(ring.gadget_recompose(got, basis, pad), a)
    ta = torch.from_numpy(a.view(np.int64)).cuda()
    tout = torch.empty(batch * pad * w, dtype=torch.int64, device="cuda")
    ring.gadget_decompose_dev(tout, ta, basis, pad)
    assert np.array_equal(tout.cpu().numpy().view(np.uint64), got)
    assert ring.decompose_overflow_count() == 0
    tback = torch.empty_like(ta)
    ring.gadget_recompose_dev(tback, tout, basis, pad)
    assert torch.equal(tback, ta)
    if name == "stark":   # too few digits: counted on the device, refused by the host form
        from stark_rings_amd import RingError
        with pytest.raises(RingError, match="more than padding_size"):
            ring.gadget_decompose(O.to_mont(F, [p - 1 - (1 << 200)] + [0] * (d - 1)), basis, 1)


def test_decomposition_basis_range_is_validated(torch_cuda):
    """The reference takes b: u128 and casts it `as i128` (balanced_decomposition/mod.rs:62, 73): a basis of 2^127 or more is negative
    there, so decomposition refuses it (mirror and C ABI alike) instead of computing something the reference does not; nothing outside
    [0, 2^128) is silently truncated on its way through ctypes; recomposition (no cast in the reference) takes the whole u128 range."""
    torch = torch_cuda
    from stark_rings_amd import RingError
    ring = ring_for("goldilocks", 4)
    F = O.FIELD_ID["goldilocks"]
    a = O.to_mont(F, list(range(16)))
    ta = torch.from_numpy(a.view(np.int64)).cuda()
    tout = torch.empty(2 * 16, dtype=torch.int64, device="cuda")
    for bad in (-2, 1 << 128, (1 << 128) + 2):
        with pytest.raises(RingError, match="u128"):
            ring.gadget_decompose(a, bad, 2)
        with pytest.raises(RingError, match="u128"):
            ring.gadget_recompose(np.concatenate([a, a]), bad, 2)
        with pytest.raises(RingError, match="u128"):
            ring.gadget_decompose_dev(tout, ta, bad, 2)
        with pytest.raises(RingError, match="u128"):
            ring.gadget_recompose_dev(ta, tout, bad, 2)
    for neg in (1 << 127, (1 << 128) - 2):
        with pytest.raises(RingError, match="2\\^127"):
            ring.gadget_decompose(a, neg, 2)
        with pytest.raises(RingError, match="2\\^127"):
            ring.gadget_decompose_dev(tout, ta, neg, 2)
    # the C ABI refuses it as well (a caller that bypasses the mirror)
    lib = ring._lib
    out = np.zeros(32, dtype=np.uint64)
    rc = lib.sr_decompose_balanced_batch_wide(ring._ctx, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                              a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), 0, 1 << 63, 2, 1)
    assert rc != 0
    # recomposition: basis (2^128 - 2) mod p through R::from(b)
    digits = np.concatenate([a, a])
    p = P.PRIMES["goldilocks"][0]
    got = O.from_mont(F, ring.gadget_recompose(digits, (1 << 128) - 2, 2))
    assert list(got) == [(i + ((1 << 128) - 2) % p * i) % p for i in range(16)]




def test_baseline_config0_literally(torch_cuda):
    """BASELINE.json configs[0]: Goldilocks, D = 2^10, batch = 1 -- one ring product through the HOST entry point
    (sr_ring_mul_batch, the plumbing case) and through the device entry point, bit for bit against the oracle; crt / icrt of the
    single element as well (crt.rs:58-74 on one element)."""
    torch = torch_cuda
    F = O.GOLDILOCKS
    k, d = 10, 1024
    ring = ring_for("goldilocks", k)
    a = O.fill_uniform(F, 0x5EED0001, 0, d)
    b = O.fill_uniform(F, 0x5EED0002, 0, d)
    want = O.pow2_ring_mul(F, a, b, k, 1)
    got = ring.mul(a.copy(), b)
    assert np.array_equal(got, want)
    ta, tb = torch.from_numpy(a.view(np.int64)).cuda(), torch.from_numpy(b.view(np.int64)).cuda()
    out = torch.empty_like(ta)
    ring.mul_dev(out, ta, tb)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), want)
    assert np.array_equal(ta.cpu().numpy().view(np.uint64), a) and np.array_equal(tb.cpu().numpy().view(np.uint64), b)
    fa = ring.elementwise_crt(a.copy())
    assert np.array_equal(fa, O.pow2_fwd(F, a, k, 1))
    assert np.array_equal(ring.elementwise_icrt(fa), a)


def test_library_settles_the_lanes_plan_itself(torch_cuda):
    """sr_plan.lanes = 0 is AUTO: with six more streams alive in the process (what a framework or RCCL adds, and what used to push both
    lanes onto one hardware queue) the library times two lanes against one stream inside sr_ctx_reserve_scratch, keeps the faster and
    says so through sr_ctx_plan_in_use; the product then runs at the winner's pace and is bit-exact either way."""
    torch = torch_cuda
    import time
    from stark_rings_amd import CyclotomicRing
    from stark_rings_amd._lib import Plan

    extra = [torch.cuda.Stream() for _ in range(6)]
    x = torch.zeros(1 << 20, device="cuda")
    for s in extra:       # make every one of them a live queue user
        with torch.cuda.stream(s):
            x.add_(1)
    torch.cuda.synchronize()
    k, batch = 16, 2048
    ring = CyclotomicRing("goldilocks", k, plan=Plan())
    plan0, probe0 = ring.plan_in_use()
    assert plan0.lanes == 0 and probe0 is None           # not settled before the first chunked product / reserve
    ring.reserve_scratch(batch)
    plan, probe = ring.plan_in_use()
    assert plan.lanes in (1, 2) and probe is not None and probe["elems"] == 2048
    assert (plan.lanes == 1) == (probe["one_stream_ms"] < probe["two_lanes_ms"])   # the faster steady state wins, no margin (capi.hip)
    F = O.GOLDILOCKS
    d = 1 << k
    ta = torch.empty(batch * d, dtype=torch.int64, device="cuda")
    tb = torch.empty(batch * d, dtype=torch.int64, device="cuda")
    ring.fill_uniform_dev(ta, 0x77, 0)
    ring.fill_uniform_dev(tb, 0x78, 0)
    out = torch.empty_like(ta)
    ring.mul_dev(out, ta, tb)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(4):
        ring.mul_dev(out, ta, tb)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / 4 * 1e3
    best = min(probe["two_lanes_ms"], probe["one_stream_ms"])
    worst = max(probe["two_lanes_ms"], probe["one_stream_ms"])
    assert ms < 1.25 * best, (ms, probe)                 # the plan in use is the one the probe found faster ...
    sample = [0, 1, 777, batch - 1]
    ea = np.concatenate([O.fill_uniform(F, 0x77, e * d, d) for e in sample])
    eb = np.concatenate([O.fill_uniform(F, 0x78, e * d, d) for e in sample])
    want = O.pow2_ring_mul(F, ea, eb, k, len(sample), 4)
    for i, e in enumerate(sample):
        assert np.array_equal(out[e * d:(e + 1) * d].cpu().numpy().view(np.uint64), want[i * d:(i + 1) * d])
    # ... and an explicit plan is honoured and reported without a probe
    for lanes in (1, 2):
        pl = Plan()
        pl.lanes = lanes
        r2 = CyclotomicRing("goldilocks", k, plan=pl)
        r2.reserve_scratch(batch)
        p2, pr2 = r2.plan_in_use()
        assert p2.lanes == lanes and pr2 is None
        o2 = torch.empty_like(ta)
        r2.mul_dev(o2, ta, tb)
        torch.cuda.synchronize()
        assert torch.equal(o2, out)
        r2.close()
    ring.close()
    del extra, worst


@pytest.mark.gpu
@pytest.mark.parametrize("name,k,batch", [("goldilocks", 16, 16384), ("babybear", 16, 16384), ("goldilocks", 20, 1024)])
def test_probe_measures_the_plan_it_picks(torch_cuda, name, k, batch):
    """the probe runs each plan the way it runs a batch (up to 32 chunks, warmed up, on the context's own streams), so
    its one-stream / two-lane ratio must be the ratio the full batch shows when each plan is forced -- BASELINE configs 2 and 3 at
    full size, config 4's degree on 1024 elements.  A context that never reserves scratch never probes: two lanes, unmeasured, and
    its first product does not block on a measurement.  A context created while six foreign streams exist (and have run work: their
    hardware queues are mapped) still picks the faster plan."""
    torch = torch_cuda
    import time
    from stark_rings_amd import CyclotomicRing
    from stark_rings_amd._lib import Plan

    d = 1 << k
    ring = CyclotomicRing(name, k, plan=Plan())
    ta = torch.empty(batch * d, dtype=torch.int64, device="cuda")
    tb = torch.empty(batch * d, dtype=torch.int64, device="cuda")
    out = torch.empty_like(ta)
    ring.fill_uniform_dev(ta, 0x91, 0)
    ring.fill_uniform_dev(tb, 0x92, 0)
    lazy = CyclotomicRing(name, k, plan=Plan())
    lazy.mul_dev(out, ta, tb)                                  # no reserve_scratch: no probe, ever
    torch.cuda.synchronize()
    pl, pr = lazy.plan_in_use()
    assert pl.lanes == 0 and pr is None
    lazy.close()
    ring.reserve_scratch(batch)
    plan, probe = ring.plan_in_use()
    assert probe is not None and probe["elems"] > 0
    ring.close()

    def full(lanes):
        p = Plan()
        p.lanes = lanes
        r = CyclotomicRing(name, k, plan=p)
        r.reserve_scratch(batch)
        r.mul_dev(out, ta, tb)
        torch.cuda.synchronize()
        best = None
        for _ in range(4):      # the best of four samples of two back-to-back batches each
            t0 = time.perf_counter()
            r.mul_dev(out, ta, tb)
            r.mul_dev(out, ta, tb)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / 2
            best = ms if best is None or ms < best else best
        r.close()
        return best

    two, one = full(2), full(1)
    ratio_full, ratio_probe = one / two, probe["one_stream_ms"] / probe["two_lanes_ms"]
    print("probe %s D=2^%d: probe one/two = %.4f (%.3f / %.3f ms per %d), full batch one/two = %.4f (%.3f / %.3f ms per %d); picked %d lanes"
          % (name, k, ratio_probe, probe["one_stream_ms"], probe["two_lanes_ms"], probe["elems"], ratio_full, one, two, batch, plan.lanes))
    # typically within 2 %; 6 % here: one box in a dozen showed 4.7 % between two separately timed runs of the same plan
    assert abs(ratio_probe - ratio_full) < 0.06 * ratio_full, (ratio_probe, ratio_full)
    assert (plan.lanes == 2) == (ratio_probe > 1.0)
    if abs(ratio_full - 1.0) > 0.06:
        assert (plan.lanes == 2) == (ratio_full > 1.0), "the probe picked the slower plan"
    foreign = [torch.cuda.Stream() for _ in range(6)]
    for st in foreign:
        with torch.cuda.stream(st):
            torch.zeros(1 << 20, device="cuda").add_(1)
    torch.cuda.synchronize()
    crowded = CyclotomicRing(name, k, plan=Plan())
    crowded.reserve_scratch(batch)
    plan_c, probe_c = crowded.plan_in_use()
    crowded.close()
    print("  beside six foreign streams: one/two = %.4f, picked %d lanes" % (probe_c["one_stream_ms"] / probe_c["two_lanes_ms"], plan_c.lanes))
    if abs(ratio_full - 1.0) > 0.06:
        assert (plan_c.lanes == 2) == (ratio_full > 1.0), "beside six foreign streams the probe picked the slower plan"
    del foreign


@pytest.mark.parametrize("k,batch", [(0, 7), (4, 5), (10, 37), (12, 5), (13, 3), (14, 2), (16, 5), (17, 1)])
def test_babybear_packed32_boundary_matches_the_oracle(torch_cuda, k, batch):
    """BASELINE configs[2] says "packed 32-bit modmul": the opt-in sr_*_packed32_* entry points take the low half of the reference's
    Fp64 limb (babybear/mod.rs:18-26: a * 2^64 mod p < 2^31 in a u64) as a uint32.  Against the oracle on the 8-byte images:
    unpack(f_packed(pack(x))) == f(x) for the ring product, crt, icrt, slot product, add and sub; operands are never written;
    pack / unpack are inverse on canonical images.  D < 4096 takes the widened route, D >= 4096 the register-tiled kernels on
    packed words (k = 12 one launch, 13 / 14 / 17 strided passes, 16 the cols256 + rows256 pair)."""
    torch = torch_cuda
    F = O.BABYBEAR
    ring = ring_for("babybear", k)
    n = batch << k
    a = edge_and_random(F, k, batch, 0xC0 + k)
    b = O.fill_uniform(F, 0xD0 + k, 0, n)
    assert int(a.max()) < (1 << 31) and int(b.max()) < (1 << 31)

    def pack(x64):
        t64 = torch.from_numpy(x64.view(np.int64)).cuda()
        t32 = torch.full((x64.size,), -1, dtype=torch.int32, device="cuda")
        ring.pack32_dev(t32, t64)
        return t32

    def unpack(t32):
        t64 = torch.full((t32.numel(),), -1, dtype=torch.int64, device="cuda")
        ring.unpack32_dev(t64, t32)
        torch.cuda.synchronize()
        return t64.cpu().numpy().view(np.uint64)

    pa, pb = pack(a), pack(b)
    assert np.array_equal(pa.cpu().numpy().view(np.uint32), a.astype(np.uint32))
    assert np.array_equal(unpack(pa), a) and np.array_equal(unpack(pb), b)
    # ring product, out of place and in place over a
    out = torch.full_like(pa, -1)
    ring.mul_packed32_dev(out, pa, pb)
    want = O.pow2_ring_mul(F, a, b, k, batch)
    assert np.array_equal(unpack(out), want), "packed ring product"
    assert np.array_equal(unpack(pa), a) and np.array_equal(unpack(pb), b), "operands written"
    pa2 = pa.clone()
    ring.mul_packed32_dev(pa2, pa2, pb)
    assert np.array_equal(unpack(pa2), want), "packed ring product in place"
    # transforms
    fa = pa.clone()
    ring.elementwise_crt_packed32_dev(fa)
    want_f = O.pow2_fwd(F, a, k, batch)
    assert np.array_equal(unpack(fa), want_f), "packed crt"
    back = fa.clone()
    ring.elementwise_icrt_packed32_dev(back)
    assert np.array_equal(unpack(back), a), "packed icrt(crt)"
    ib = pb.clone()
    ring.elementwise_icrt_packed32_dev(ib)
    assert np.array_equal(unpack(ib), O.pow2_inv(F, b, k, batch)), "packed icrt"
    # slot product and sums
    fb = pack(O.pow2_fwd(F, b, k, batch))
    prod = fa.clone()
    ring.ntt_mul_packed32_dev(prod, fb)
    assert np.array_equal(unpack(prod), O.pow2_pointwise(F, want_f, O.pow2_fwd(F, b, k, batch))), "packed slot product"
    s_ = pa.clone()
    ring.add_packed32_dev(s_, pb)
    p = P.PRIMES["babybear"][0]
    m = min(n, 2048)          # the oracle's integers on a prefix, the 8-byte entry points on everything
    av, bv = O.from_mont(F, a[:m]), O.from_mont(F, b[:m])
    assert np.array_equal(unpack(s_)[:m], O.to_mont(F, [(x + y) % p for x, y in zip(av, bv)])), "packed add vs integers"
    d_ = pa.clone()
    ring.sub_packed32_dev(d_, pb)
    ta, tb = torch.from_numpy(a.view(np.int64)).cuda(), torch.from_numpy(b.view(np.int64)).cuda()
    ring.add_dev(ta, tb)       # the 8-byte entry points (themselves checked against the oracle elsewhere) as the wide reference
    torch.cuda.synchronize()
    assert np.array_equal(unpack(s_), ta.cpu().numpy().view(np.uint64)), "packed add"
    ta = torch.from_numpy(a.view(np.int64)).cuda()
    ring.sub_dev(ta, tb)
    torch.cuda.synchronize()
    assert np.array_equal(unpack(d_), ta.cpu().numpy().view(np.uint64)), "packed sub"


def test_packed32_entry_points_refuse_other_rings(torch_cuda):
    torch = torch_cuda
    from stark_rings_amd import RingError
    ring = ring_for("goldilocks", 4)
    t32 = torch.zeros(16, dtype=torch.int32, device="cuda")
    t64 = torch.zeros(16, dtype=torch.int64, device="cuda")
    with pytest.raises(RingError, match="BabyBear"):
        ring.pack32_dev(t32, t64)
    with pytest.raises(RingError, match="BabyBear"):
        ring.mul_packed32_dev(t32, t32.clone(), t32.clone())
    bb = ring_for("babybear", 4)
    with pytest.raises(RingError, match="alias"):
        bb.mul_packed32_dev(t32, t32.clone(), t32)



# ----------------------------------------------------------------------------- lazy butterflies: representatives that land on p
@pytest.mark.gpu
@pytest.mark.parametrize("k,batch", [(16, 2), (17, 1), (13, 3), (20, 1)])
def test_goldilocks_inverse_with_lazy_sums_landing_on_p(torch_cuda, k, batch):
    """The inverse rows kernels run decimation-in-time butterflies whose sums and differences are lazy 64-bit representatives
    (ntt_goldilocks.hpp, SR_GL_LAZY_DIT).  A representative differs from the canonical value only when a sum lands in [p, 2^64) --
    probability 2^-32 per value on uniform data, certain on inputs built for it: here every 256-block of the NTT-domain operand
    starts with sixteen words for which one output of the first 16-point network is 0 mod p with non-zero legs, so that the lazy sum
    is p itself, in the very slot that reaches the next network WITHOUT a table product in front (factor 1) -- the value
    G::canon exists for.  D = 2^13 and 2^20 run 4096-point tiles (three networks): there the first 256-block of every tile is built
    so that the SECOND-level networks leave p where the third takes it (tools/model_fast_goldilocks.py: crafted_inverse_block256).
    Whole transforms against the oracle, every word; plus the product of such operands.  The build without the canonicalisation
    (-DSR_GL_LAZY_CANON=0) fails this test."""
    import os
    import random
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import model_fast_goldilocks as M

    F = O.GOLDILOCKS
    d = 1 << k
    ring = ring_for("goldilocks", k)
    rng = random.Random(0x1A2 + k)
    raw = O.fill_uniform(F, 0x51 + k, 0, batch * d).copy()
    hits = 0
    for blk in range(batch * d // 256):
        slot = 1 + blk % 15
        words = M.crafted_inverse_block(rng, slot)
        hits += M.dft16_inv_lazy(words)[slot] == M.p
        raw[blk * 256:blk * 256 + 16] = np.array(words, dtype=np.uint64)
    if k in (13, 20):
        T = M.tables(13)
        for tile in range(batch * d // 4096):
            slots = [1 + (i0 * 7 + tile) % 15 for i0 in range(16)]
            raw[tile * 4096:tile * 4096 + 256] = np.array(M.crafted_inverse_block256(rng, T, slots), dtype=np.uint64)
    assert hits > batch * d // 256 // 4, "the crafted blocks do not leave the representative p (%d)" % hits
    want = O.pow2_inv(F, raw, k, batch, 4)
    got = ring.elementwise_icrt(raw.copy())
    assert np.array_equal(got, want)
    assert np.array_equal(ring.elementwise_crt(got.copy()), raw)
    # the fused product runs the same inverse networks on crt(a) (.) crt(b): choose a = icrt(raw), b = icrt(R^2-image of 1 in every slot)
    # so that the slot product hands the inverse exactly `raw` again (mul_boundary(x, R) = x)
    one = O.to_mont(F, [1] * (batch * d))           # Montgomery image of 1 in every NTT slot
    b = O.pow2_inv(F, one, k, batch, 4)
    assert np.array_equal(ring.mul(want, b), want)


def _structured_operands(F, name, k, seed):
    """ring elements whose transforms are full of coincidences (equal legs, zero differences, sums that land on 0 or p): small and
    signed-small coefficients, monomials, constants, alternating signs, a geometric sequence of a root of unity, sparse supports"""
    import random

    p = P.PRIMES[name][0]
    d = 1 << k
    rng = random.Random(seed)
    els = []
    els.append([1] * d)                                                    # constant 1 in every coefficient
    els.append([(p - 1) if i & 1 else 1 for i in range(d)])                # +-1 alternating
    els.append([rng.choice((0, 1, p - 1)) for _ in range(d)])              # ternary
    els.append([rng.randrange(4) for _ in range(d)])                       # tiny
    mono = [0] * d
    mono[d // 2] = 1
    els.append(mono)                                                       # X^(D/2)
    sparse = [0] * d
    for i in rng.sample(range(d), min(d, 5)):
        sparse[i] = rng.choice((1, p - 1, 2, p - 2))
    els.append(sparse)
    w = pow(7, (p - 1) // (2 * d), p) if (p - 1) % (2 * d) == 0 else 3
    geo, acc = [], 1
    for i in range(d):
        geo.append(acc)
        acc = acc * w % p
    els.append(geo)                                                        # psi^i: its transform is a single spike (or nearly)
    els.append([(p - v) % p for v in geo])                                 # and its negative
    half = [rng.randrange(p) for _ in range(d // 2)]
    els.append(half + half)                                                # period D/2
    els.append([p - 1] * d)
    return els


@pytest.mark.gpu
@pytest.mark.parametrize("name,k", [("goldilocks", 10), ("goldilocks", 12), ("goldilocks", 13), ("goldilocks", 16), ("goldilocks", 17),
                                    ("goldilocks", 20), ("babybear", 12), ("babybear", 16), ("stark", 10)])
def test_structured_operands_through_every_tuned_plan(torch_cuda, name, k):
    """Uniform data hardly ever produces equal butterfly legs, zero differences or sums that land exactly on 0 or p; these operands
    do, all the time.  Transforms, inverse transforms and products (each operand with each) against the oracle, every word."""
    F = O.FIELD_ID[name]
    ring = ring_for(name, k)
    els = _structured_operands(F, name, k, 0x5EED + k)
    n = len(els)
    a = O.to_mont(F, [v for e in els for v in e])
    fa = ring.elementwise_crt(a.copy())
    assert np.array_equal(fa, O.pow2_fwd(F, a, k, n, 4))
    assert np.array_equal(ring.elementwise_icrt(fa.copy()), a)
    L = O.LIMBS[F]
    a2 = a.reshape(n, -1)
    for shift in (0, 1, 3, 7):
        b = np.ascontiguousarray(np.roll(a2, shift, axis=0)).reshape(-1)
        assert np.array_equal(ring.mul(a, b), O.pow2_ring_mul(F, a, b, k, n, 4)), "shift %d" % shift


# ----------------------------------------------------------------------------- round 4: context-owned temporaries under several caller streams
@pytest.mark.gpu
def test_context_temporaries_are_ordered_between_caller_streams(torch_cuda):
    """the row-part buffer of a short-and-wide small-ring mat-vec and the staging buffers of the packed-u32 entry points
    below D = 4096 are ONE set per context, while _dev calls may arrive on any stream.  Calls issued back to back on two streams,
    with different operands, must each see their own temporaries: the users are ordered by the same event as the operand scratch
    (ScratchUse in capi.hip).  Many alternations, results against single-stream runs of the same calls."""
    torch = torch_cuda
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    # (a) Goldilocks-24 mat-vec, 2 rows x 3000 columns: row parts in use
    ring = ring_for("goldilocks24", 0)
    d = ring.degree
    nrows, ncols = 2, 3000
    F = O.GOLDILOCKS
    ms = [torch.from_numpy(O.fill_uniform(F, 0x300 + i, 0, nrows * ncols * d).view(np.int64)).cuda() for i in range(2)]
    vs = [torch.from_numpy(O.fill_uniform(F, 0x310 + i, 0, ncols * d).view(np.int64)).cuda() for i in range(2)]
    ref = []
    for i in range(2):
        y = torch.empty(nrows * d, dtype=torch.int64, device="cuda")
        ring.matvec_ntt_dev(y, ms[i], vs[i], nrows, ncols)
        torch.cuda.synchronize()
        ref.append(y.clone())
    ys = [[torch.empty(nrows * d, dtype=torch.int64, device="cuda") for _ in range(16)] for _ in range(2)]
    torch.cuda.synchronize()
    for r in range(16):
        ring.matvec_ntt_dev(ys[0][r], ms[0], vs[0], nrows, ncols, stream=s1)
        ring.matvec_ntt_dev(ys[1][r], ms[1], vs[1], nrows, ncols, stream=s2)
    torch.cuda.synchronize()
    for r in range(16):
        assert torch.equal(ys[0][r], ref[0]) and torch.equal(ys[1][r], ref[1]), "mat-vec round %d" % r
    # (b) packed BabyBear product at D = 2^10 (the widened route through the context's staging buffers)
    k, batch = 10, 512
    bb = ring_for("babybear", k)
    n = batch << k
    ops = []
    for i in range(2):
        a = torch.from_numpy(O.fill_uniform(O.BABYBEAR, 0x320 + i, 0, n).astype(np.uint32).view(np.int32)).cuda()
        b = torch.from_numpy(O.fill_uniform(O.BABYBEAR, 0x330 + i, 0, n).astype(np.uint32).view(np.int32)).cuda()
        ops.append((a, b))
    refp = []
    for a, b in ops:
        o = torch.empty_like(a)
        bb.mul_packed32_dev(o, a, b)
        torch.cuda.synchronize()
        refp.append(o.clone())
    outs = [[torch.empty_like(ops[0][0]) for _ in range(16)] for _ in range(2)]
    torch.cuda.synchronize()
    for r in range(16):
        bb.mul_packed32_dev(outs[0][r], ops[0][0], ops[0][1], stream=s1)
        bb.mul_packed32_dev(outs[1][r], ops[1][0], ops[1][1], stream=s2)
    torch.cuda.synchronize()
    for r in range(16):
        assert torch.equal(outs[0][r], refp[0]) and torch.equal(outs[1][r], refp[1]), "packed product round %d" % r
    # and the single-stream reference itself is the oracle's product
    want = O.pow2_ring_mul(O.BABYBEAR, O.fill_uniform(O.BABYBEAR, 0x320, 0, n), O.fill_uniform(O.BABYBEAR, 0x330, 0, n), k, batch)
    assert np.array_equal(refp[0].cpu().numpy().view(np.uint32).astype(np.uint64), want)


# ----------------------------------------------------------------------------- round 4: Neg, Mul<scalar>, Add<scalar> of RqPoly / RqNTT
@pytest.mark.gpu
@pytest.mark.parametrize("name,k", [("goldilocks", 6), ("goldilocks", 16), ("babybear", 5), ("stark", 4), ("goldilocks24", 0), ("babybear72", 0), ("frog16", 0)])
def test_neg_scale_and_add_scalar_match_integer_arithmetic(torch_cuda, name, k):
    """The unary operators of the reference's element types, every ring id, host and device entry points, against
    Python integers on the standard-form values: Neg (coeff_form.rs:270-278, ntt_form.rs:191-203); Mul<Fp> / Mul<u64 ...>
    (coeff_form.rs:390-408, 610-650; ntt_form.rs:373-425: every coefficient / slot component times the scalar); Add<u64 ...>
    (coeff_form.rs:652-700: coefficient 0 of every element; ntt_form.rs:427-505: component 0 of every slot).  Edge values: 0, 1,
    p - 1 as data and as scalar; a scalar word >= p is refused."""
    torch = torch_cuda
    base = {"goldilocks24": "goldilocks", "babybear72": "babybear", "frog16": "frog"}.get(name, name)
    F = O.FIELD_ID[base]
    p = P.PRIMES[base][0] if base in P.PRIMES else P.FROG_P
    L = O.LIMBS[F]
    ring = ring_for(name, k)
    d, batch = ring.degree, 5
    slot = {"goldilocks24": 3, "babybear72": 9, "frog16": 4}.get(name, 1)
    a = O.fill_uniform(F, 0x700 + k, 0, batch * d)
    std = O.from_mont(F, a)
    std[0:4] = [0, 1, p - 1, p - 2]
    a = O.to_mont(F, std)

    def dev(fn, *args):
        t = torch.from_numpy(a.copy().view(np.int64)).cuda()
        fn(t, *args)
        torch.cuda.synchronize()
        return t.cpu().numpy().view(np.uint64)

    want = O.to_mont(F, [(p - v) % p for v in std])
    assert np.array_equal(ring.neg(a.copy()), want) and np.array_equal(dev(ring.neg_dev), want)
    for sc in (0, 1, p - 1, 2**32 % p, 0xDEADBEEFCAFE % p, (p + 1) // 2):
        s_img = O.to_mont(F, [sc])
        want = O.to_mont(F, [v * sc % p for v in std])
        assert np.array_equal(ring.scale(a.copy(), s_img), want), ("scale", sc)
        assert np.array_equal(dev(ring.scale_dev, s_img), want), ("scale_dev", sc)
        w0 = list(std)
        for e in range(batch):
            w0[e * d] = (w0[e * d] + sc) % p
        assert np.array_equal(ring.add_scalar(a.copy(), s_img, False), O.to_mont(F, w0)), ("add_scalar coeff", sc)
        assert np.array_equal(dev(ring.add_scalar_dev, s_img, False), O.to_mont(F, w0))
        w1 = [(v + sc) % p if i % slot == 0 else v for i, v in enumerate(std)]
        assert np.array_equal(ring.add_scalar(a.copy(), s_img, True), O.to_mont(F, w1)), ("add_scalar ntt", sc)
        assert np.array_equal(dev(ring.add_scalar_dev, s_img, True), O.to_mont(F, w1))
    # consistency with the ring's own product: a * from_scalar(s) == scale(a, s) for the power-of-two rings (coeff_form.rs:396)
    if slot == 1:
        sc = 0x1234567 % p
        const = O.to_mont(F, ([sc] + [0] * (d - 1)) * batch)
        assert np.array_equal(ring.mul(a.copy(), const), ring.scale(a.copy(), O.to_mont(F, [sc])))
    bad = O.ints_to_limbs([p], L)   # the modulus itself is not a canonical image
    with pytest.raises(Exception, match="canonical"):
        ring.scale(a.copy(), bad)
    with pytest.raises(Exception, match="limb"):
        ring.scale(a.copy(), np.zeros(L + 1, dtype=np.uint64))
    if base == "babybear":   # bits above the 31-bit residue: not an Fp64 image of a BabyBear element
        with pytest.raises(Exception, match="canonical"):
            ring.scale(a.copy(), np.array([(1 << 32) + 5], dtype=np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("name,k,batch", [("goldilocks", 6, 5), ("goldilocks", 16, 3), ("babybear", 5, 9), ("stark", 4, 7), ("stark", 12, 2),
                                          ("goldilocks24", 0, 131), ("babybear72", 0, 67), ("frog16", 0, 200)])
def test_matrix_times_one_ring_element(torch_cuda, name, k, batch):
    """`MulAssign<&R> for Matrix<R>` (linear_algebra/src/matrix.rs:207-211) and `for SparseMatrix<R>` (sparse_matrix.rs:303-307):
    every entry of the matrix's flat storage times ONE ring element, slot-wise (Fq3 / Fq9 / Fq4 slot products on the reference's own
    rings; batches that leave ragged last workgroups).  Against the slot product with the element repeated (itself pinned to the
    oracle by the tests above), against the oracle directly on the power-of-two rings, host and device entry points; edge
    multipliers 0 and 1; a multiplier that is not one element or lies inside the batch is refused."""
    torch = torch_cuda
    from stark_rings_amd import RingError

    base = {"goldilocks24": "goldilocks", "babybear72": "babybear", "frog16": "frog"}.get(name, name)
    F = O.FIELD_ID[base]
    ring = ring_for(name, k)
    w = ring.words_per_elem
    a = O.fill_uniform(F, 0x7A0 + k, 0, batch * ring.degree)
    r = O.fill_uniform(F, 0x7B0 + k, 0, ring.degree)
    want = ring.ntt_mul(a.copy(), np.tile(r, batch))
    assert np.array_equal(ring.mul_elem(a.copy(), r), want)
    ta = torch.from_numpy(a.copy().view(np.int64)).cuda()
    tr = torch.from_numpy(r.view(np.int64)).cuda()
    ring.mul_elem_dev(ta, tr)
    torch.cuda.synchronize()
    assert np.array_equal(ta.cpu().numpy().view(np.uint64), want)
    if name in ("goldilocks", "babybear", "stark"):
        for e in (0, batch - 1):
            assert np.array_equal(want[e * w:(e + 1) * w], O.pow2_pointwise(F, a[e * w:(e + 1) * w], r)), e
    one = O.to_mont(F, [1] * ring.degree) if name in ("goldilocks", "babybear", "stark") else None
    if one is not None:     # the multiplicative identity of the fully split rings: 1 in every slot
        assert np.array_equal(ring.mul_elem(a.copy(), one), a)
    assert not ring.mul_elem(a.copy(), np.zeros(w, dtype=np.uint64)).any()
    assert ring.mul_elem(np.zeros(0, dtype=np.uint64), r).size == 0
    with pytest.raises(RingError, match="one ring element"):
        ring.mul_elem(a.copy(), np.tile(r, 2))
    with pytest.raises(RingError, match="inside the batch"):
        ring.mul_elem_dev(ta, ta[w:2 * w] if batch > 1 else ta)


@pytest.mark.gpu
@pytest.mark.parametrize("name,k,batch", [("goldilocks", 16, 460), ("goldilocks", 16, 100), ("goldilocks", 20, 30), ("goldilocks", 10, 64), ("babybear", 16, 1000),
                                          ("stark", 12, 8), ("stark", 14, 3)])
def test_device_calls_can_be_captured_into_a_hip_graph(torch_cuda, name, k, batch):
    """A caller that replays the same batch shape many times can capture the `_dev` calls into a HIP graph: after
    sr_ctx_reserve_scratch nothing in them allocates, synchronises or probes, and the two internal lanes fork from / join to the
    caller's stream with events, which is the capturable form.  Captured once (product, forward transform, constant-operand product),
    replayed on NEW operand values in the same buffers: every replay equals the eager result bit for bit.  (Small batches gain: 1 024
    Goldilocks products of degree 2^16 replay in 0.95 ms against 1.09 ms eager; a full config-2 batch is unchanged.)"""
    torch = torch_cuda
    from stark_rings_amd import CyclotomicRing

    ring = CyclotomicRing(name, k, device=0)
    n = batch * ring.words_per_elem
    a = torch.empty(n, dtype=torch.int64, device="cuda")
    b = torch.empty(n, dtype=torch.int64, device="cuda")
    ring.fill_uniform_dev(a, 0x61, 0)
    ring.fill_uniform_dev(b, 0x62, 0)
    ring.reserve_scratch(batch)
    out, fa, out2 = torch.empty_like(a), torch.empty_like(a), torch.empty_like(a)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):           # once eagerly on the capture stream: lazily created lanes and buffers exist afterwards
        ring.mul_dev(out, a, b, stream=s)
        fa.copy_(b)
        ring.elementwise_crt_dev(fa, stream=s)
        ring.mul_ntt_rhs_dev(out2, a, fa, stream=s)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        cur = torch.cuda.current_stream()
        ring.mul_dev(out, a, b, stream=cur)
        fa.copy_(b)
        ring.elementwise_crt_dev(fa, stream=cur)
        ring.mul_ntt_rhs_dev(out2, a, fa, stream=cur)
    torch.cuda.synchronize()
    for seed in (0x71, 0x81):
        ring.fill_uniform_dev(a, seed, 0)          # new values, same buffers
        ring.fill_uniform_dev(b, seed + 1, 0)
        want = torch.empty_like(a)
        ring.mul_dev(want, a, b)
        torch.cuda.synchronize()
        out.zero_()
        out2.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want), seed
        assert torch.equal(out2, want), seed
        wf = b.clone()
        ring.elementwise_crt_dev(wf)
        torch.cuda.synchronize()
        assert torch.equal(fa, wf), seed
    ring.close()


# ----------------------------------------------------------------------------- round 4: the column pass that keeps its twist factors
@pytest.mark.gpu
@pytest.mark.parametrize("k,batch,chunk", [(16, 456, 0), (16, 264, 64), (16, 40, 8), (16, 48, 24), (16, 32, 16), (16, 200, 40),
                                           (17, 232, 0), (18, 120, 0), (20, 33, 0), (20, 17, 8)])
def test_keep_and_plain_column_passes_agree(torch_cuda, k, batch, chunk):
    """Round 4: on the two-lane plans a column-pass workgroup owns one column chunk and walks over the ring elements of the launch
    with its 16 twist factors in registers (cols256_keep_kernel; launches whose element count is a multiple of 8 -- the rest, here
    the ragged last chunk, runs the plain kernel).  The (XCD, column chunk, group) -> ring element walk must cover every tile of every
    element exactly once: product, constant-operand product, forward and inverse transform against the plain-kernel plan
    (SR_PLAN_GL_PLAIN_COLS) bit for bit, and sampled elements against the oracle."""
    torch = torch_cuda
    from stark_rings_amd import CyclotomicRing

    F = O.GOLDILOCKS
    d = 1 << k
    n = batch * d
    ta = torch.empty(n, dtype=torch.int64, device="cuda")
    tb = torch.empty(n, dtype=torch.int64, device="cuda")
    res = []
    for flags in (0, 128):   # 128 = SR_PLAN_GL_PLAIN_COLS
        ring = CyclotomicRing("goldilocks", k, device=0, plan=_plan(flags=flags, lanes=2, chunk_polys=chunk))
        ring.fill_uniform_dev(ta, 0xE1, 0)
        ring.fill_uniform_dev(tb, 0xE2, 0)
        out = torch.empty_like(ta)
        ring.mul_dev(out, ta, tb)
        fb = tb.clone()
        ring.elementwise_crt_dev(fb)
        out2 = torch.empty_like(ta)
        ring.mul_ntt_rhs_dev(out2, ta, fb)
        fa = ta.clone()
        ring.elementwise_crt_dev(fa)
        back = fa.clone()
        ring.elementwise_icrt_dev(back)
        torch.cuda.synchronize()
        assert torch.equal(out, out2) and torch.equal(back, ta)
        assert ring.count_noncanonical_dev(out) == 0 and ring.count_noncanonical_dev(fa) == 0
        res.append((out, fa))
        ring.close()
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    sample = sorted({0, 1, 7, 8, batch // 2, batch - 9, batch - 8, batch - 1})
    ea = np.concatenate([O.fill_uniform(F, 0xE1, e * d, d) for e in sample])
    eb = np.concatenate([O.fill_uniform(F, 0xE2, e * d, d) for e in sample])
    want = O.pow2_ring_mul(F, ea, eb, k, len(sample), 4)
    wf = O.pow2_fwd(F, ea, k, len(sample), 4)
    for i, e in enumerate(sample):
        assert np.array_equal(res[0][0][e * d:(e + 1) * d].cpu().numpy().view(np.uint64), want[i * d:(i + 1) * d]), e
        assert np.array_equal(res[0][1][e * d:(e + 1) * d].cpu().numpy().view(np.uint64), wf[i * d:(i + 1) * d]), e


@pytest.mark.gpu
@pytest.mark.parametrize("name,k", [("goldilocks24", 0), ("babybear72", 0), ("frog16", 0), ("stark", 4), ("goldilocks", 10)])
def test_primitive_ops_like_the_reference(torch_cuda, name, k):
    """coeff_form.rs:736-746 `test_primitive_ops` (on the Goldilocks ring there), for every ring family: R::one() + 1u32 == R::one() + R::one(),
    R::one() * 1u32 == R::one(), R::one() * 0u32 == R::zero(), R::one() - 0u32 == R::one(), R::one() - 1u32 == R::zero() -- and the NTT-form
    counterparts through crt (ntt_form.rs:373-505: adding a primitive to an RqNTT adds it to every slot, which is crt of adding it to
    coefficient 0)."""
    base = {"goldilocks24": "goldilocks", "babybear72": "babybear", "frog16": "frog"}.get(name, name)
    F = O.FIELD_ID[base]
    p = P.PRIMES[base][0] if base in P.PRIMES else P.FROG_P
    ring = ring_for(name, k)
    d = ring.degree
    one = O.to_mont(F, [1] + [0] * (d - 1))
    zero = O.to_mont(F, [0] * d)
    img = lambda v: O.to_mont(F, [v % p])
    assert np.array_equal(ring.add_scalar(one.copy(), img(1), False), ring.add(one.copy(), one))
    assert np.array_equal(ring.scale(one.copy(), img(1)), one)
    assert np.array_equal(ring.scale(one.copy(), img(0)), zero)
    assert np.array_equal(ring.add_scalar(one.copy(), img(-0), False), one)          # one - 0
    assert np.array_equal(ring.add_scalar(one.copy(), img(-1), False), zero)         # one - 1: Sub passes the negated scalar
    assert np.array_equal(ring.neg(one.copy()), ring.sub(zero.copy(), one))
    # the NTT-form operators are the coefficient-form ones seen through crt
    a = O.fill_uniform(F, 0x515, 0, 3 * d)
    for v in (1, 7, p - 1):
        lhs = ring.add_scalar(ring.elementwise_crt(a.copy()), img(v), True)
        rhs = ring.elementwise_crt(ring.add_scalar(a.copy(), img(v), False))
        assert np.array_equal(lhs, rhs), v
        assert np.array_equal(ring.scale(ring.elementwise_crt(a.copy()), img(v)), ring.elementwise_crt(ring.scale(a.copy(), img(v))))
    assert np.array_equal(ring.neg(ring.elementwise_crt(a.copy())), ring.elementwise_crt(ring.neg(a.copy())))


_FOLD_ORACLE = {"goldilocks24": "sro_g24_ntt_mul", "babybear72": "sro_bb72_ntt_mul", "frog16": "sro_frog16_ntt_mul"}


@pytest.mark.gpu
@pytest.mark.parametrize("name,k,sizes", [("goldilocks", 6, (0, 1, 2, 3, 31, 32, 33, 67, 1100)), ("goldilocks", 16, (3, 70)),
                                          ("babybear", 5, (0, 1, 5, 40, 1063)), ("stark", 4, (0, 1, 2, 45, 1100)), ("stark", 9, (3, 37)),
                                          ("goldilocks24", 0, (0, 1, 2, 3, 64, 65, 1001)), ("babybear72", 0, (0, 1, 7, 130)),
                                          ("frog16", 0, (0, 1, 4, 9, 515))])
def test_sum_and_product_over_a_slice_of_ring_elements(torch_cuda, name, k, sizes):
    """`impl Sum` / `impl Product` of the element types rows a2 / a3 name: `iter.fold(zero(), |acc, x| acc + x)` for
    RqPoly and RqNTT (coeff_form.rs:507-521, ntt_form.rs:640-654) and `iter.fold(one(), |acc, x| acc * x)` for RqNTT
    (ntt_form.rs:656-670), every ring id, host and device entry points.  Sum against Python integers on the standard-form values;
    Product against the oracle's slot product folded LEFT TO RIGHT exactly as the reference folds (the device uses a tree: same
    value, the fold being associative and commutative on canonical results).  Empty slices give zero() / one(); slice lengths cover
    one, two and three stages of the device fold, odd lengths of the halving tree, and an all-(p - 1) element."""
    torch = torch_cuda
    from stark_rings_amd import RingError

    base = {"goldilocks24": "goldilocks", "babybear72": "babybear", "frog16": "frog"}.get(name, name)
    F = O.FIELD_ID[base]
    p = P.PRIMES[base][0] if base in P.PRIMES else P.FROG_P
    ring = ring_for(name, k)
    d, w = ring.degree, ring.words_per_elem
    slot = {"goldilocks24": 3, "babybear72": 9, "frog16": 4}.get(name, 1)
    one_std = [1 if i % slot == 0 else 0 for i in range(d)]

    def slot_mul(x, y):
        if name in _FOLD_ORACLE:
            return O.small(_FOLD_ORACLE[name], x, y)
        return O.pow2_pointwise(F, x, y)

    for n in sizes:
        a = O.fill_uniform(F, 0x900 + 7 * k + n, 0, max(n, 1) * d)[:n * w]
        if n >= 2:
            a[w:2 * w] = O.to_mont(F, [p - 1] * d)
        std = O.from_mont(F, a) if n else []
        want_sum = O.to_mont(F, [sum(std[e * d + i] for e in range(n)) % p for i in range(d)])
        assert np.array_equal(ring.sum(a), want_sum), ("sum", n)
        acc = O.to_mont(F, one_std)
        for e in range(n):
            acc = slot_mul(acc, a[e * w:(e + 1) * w])
        assert np.array_equal(ring.product(a), acc), ("product", n)
        ta = torch.from_numpy(a.copy().view(np.int64)).cuda() if n else torch.empty(0, dtype=torch.int64, device="cuda")
        out = torch.full((w,), -1, dtype=torch.int64, device="cuda")
        ring.sum_dev(out, ta)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint64), want_sum), ("sum_dev", n)
        out.fill_(-1)
        ring.product_dev(out, ta)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint64), acc), ("product_dev", n)
        if n:
            assert np.array_equal(ta.cpu().numpy().view(np.uint64), a), "the input slice was written"
    # Product for RqPoly (coeff_form.rs:523-537: the fold of ring products) = icrt(product(crt(x_i))), against the oracle's ring product
    if slot == 1 and k >= 1:
        n = 5
        a = O.fill_uniform(F, 0x9F0 + k, 0, n * d)
        acc = a[:w].copy()
        for e in range(1, n):
            acc = O.pow2_ring_mul(F, acc, a[e * w:(e + 1) * w], k)
        assert np.array_equal(ring.product_poly(a), acc)
        ta = torch.from_numpy(a.copy().view(np.int64)).cuda()
        out = torch.empty(w, dtype=torch.int64, device="cuda")
        ring.product_poly_dev(out, ta)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint64), acc)
        one_poly = O.to_mont(F, [1] + [0] * (d - 1))
        assert np.array_equal(ring.product_poly(np.zeros(0, dtype=np.uint64)), one_poly)   # one() of RqPoly: icrt of the all-ones slots
    if slot > 1:   # the reference's own rings: Product for RqPoly against the fold of the ring's fused product (pinned to the oracle above)
        n = 4
        a = O.fill_uniform(F, 0x9E0 + slot, 0, n * d)
        acc = a[:w].copy()
        for e in range(1, n):
            acc = ring.mul(acc, a[e * w:(e + 1) * w].copy())
        assert np.array_equal(ring.product_poly(a), acc)
        one_poly = O.to_mont(F, [1] + [0] * (d - 1))
        assert np.array_equal(ring.product_poly(np.zeros(0, dtype=np.uint64)), one_poly)
    # out inside the slice is refused
    ta = torch.from_numpy(O.fill_uniform(F, 1, 0, 3 * d).view(np.int64)).cuda()
    with pytest.raises(RingError, match="overlap"):
        ring.sum_dev(ta[w:2 * w], ta)
    with pytest.raises(RingError, match="one ring element"):
        ring.product_dev(ta[:2 * w], ta)


@pytest.mark.gpu
def test_reserve_covers_transforms_between_four_and_eight_lane_chunks(torch_cuda):
    """sr_ctx_reserve_scratch sized the register-tiled scratch for the PRODUCT only (two lanes from 3.5 lane chunks
    on: four chunk buffers), while a stand-alone transform takes the lanes from eight chunks on and below that runs on the caller's
    stream through ONE buffer of the whole batch -- so at BabyBear D = 2^16, batch 1025 .. 2047, the first transform after reserve
    synchronised the device and reallocated.  Here: batch 1500 (5.9 chunks of 256), reserve, then crt, product and icrt are captured
    into a graph WITHOUT any eager warm-up -- a capture tolerates neither an allocation nor a synchronisation -- and the replay equals
    what a second, eager context computes."""
    torch = torch_cuda
    from stark_rings_amd import CyclotomicRing

    batch, k = 1500, 16
    ring = CyclotomicRing("babybear", k, device=0)
    n = batch * ring.words_per_elem
    a = torch.empty(n, dtype=torch.int64, device="cuda")
    b = torch.empty(n, dtype=torch.int64, device="cuda")
    ring.fill_uniform_dev(a, 0x51, 0)
    ring.fill_uniform_dev(b, 0x52, 0)
    ring.reserve_scratch(batch)
    fa, out = a.clone(), torch.empty_like(a)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        cur = torch.cuda.current_stream()
        ring.elementwise_crt_dev(fa, stream=cur)       # one stream, whole-batch packed scratch: must already be there
        ring.mul_dev(out, a, b, stream=cur)            # two lanes, four chunk buffers
        ring.elementwise_icrt_dev(fa, stream=cur)
    g.replay()
    torch.cuda.synchronize()
    ref = CyclotomicRing("babybear", k, device=0)
    want = torch.empty_like(a)
    ref.mul_dev(want, a, b)
    torch.cuda.synchronize()
    assert torch.equal(out, want) and torch.equal(fa, a)
    # the packed-u32 twins share the scratch and the rule
    a32 = torch.empty(n, dtype=torch.int32, device="cuda")
    ring.pack32_dev(a32, a)
    f32 = a32.clone()
    torch.cuda.synchronize()
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2, stream=s):
        cur = torch.cuda.current_stream()
        ring.elementwise_crt_packed32_dev(f32, stream=cur)
        ring.elementwise_icrt_packed32_dev(f32, stream=cur)
    g2.replay()
    torch.cuda.synchronize()
    assert torch.equal(f32, a32)
    ring.close()
    ref.close()


@pytest.mark.gpu
def test_captured_graph_freezes_the_scratch(torch_cuda):
    """ADVICE r4 (medium), the limits of the graph-capture guarantee made enforceable: a captured graph holds the context's scratch
    addresses, so once a `_dev` call has been seen on a capturing stream no `_dev` call moves a context buffer any more -- a larger
    batch that would have to grow the scratch is refused (SR_E_INVALID, "reserve") instead of freeing memory the graph still writes
    to; sr_ctx_reserve_scratch remains the one, explicit way to grow.  A capture on a context that never reserved is refused the
    same way (the growth would have to synchronise the device in the middle of the capture)."""
    torch = torch_cuda
    from stark_rings_amd import CyclotomicRing, RingError

    k, small, big = 13, 8, 96
    F = O.GOLDILOCKS
    ring = CyclotomicRing("goldilocks", k, device=0)
    w = ring.words_per_elem
    a = torch.from_numpy(O.fill_uniform(F, 0x31, 0, big << k).view(np.int64)).cuda()
    b = torch.from_numpy(O.fill_uniform(F, 0x32, 0, big << k).view(np.int64)).cuda()
    out = torch.empty_like(a)
    ring.reserve_scratch(small)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ring.mul_dev(out[:small * w], a[:small * w], b[:small * w], stream=torch.cuda.current_stream())
    g.replay()
    torch.cuda.synchronize()
    want = O.pow2_ring_mul(F, a[:small * w].cpu().numpy().view(np.uint64), b[:small * w].cpu().numpy().view(np.uint64), k, small, 4)
    assert np.array_equal(out[:small * w].cpu().numpy().view(np.uint64), want)
    with pytest.raises(RingError, match="reserve"):
        ring.mul_dev(out, a, b)                       # 96 elements need a larger operand scratch: refused, nothing freed
    g.replay()                                        # the graph still runs on intact memory
    torch.cuda.synchronize()
    assert np.array_equal(out[:small * w].cpu().numpy().view(np.uint64), want)
    del g
    ring.reserve_scratch(big)                         # the explicit way to grow (graphs captured before are invalid from here on)
    ring.mul_dev(out, a, b)
    torch.cuda.synchronize()
    e = big - 1
    assert np.array_equal(out[e * w:].cpu().numpy().view(np.uint64),
                          O.pow2_ring_mul(F, a[e * w:].cpu().numpy().view(np.uint64), b[e * w:].cpu().numpy().view(np.uint64), k, 1))
    fresh = CyclotomicRing("goldilocks", k, device=0)  # never reserved: its first product under capture would have to allocate
    g3 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g3, stream=s):
        with pytest.raises(RingError, match="reserve"):
            fresh.mul_dev(out[:small * w], a[:small * w], b[:small * w], stream=torch.cuda.current_stream())
    ring.close()
    fresh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k,batch,lanes", [(13, 20, 0), (15, 9, 0), (16, 40, 1), (16, 460, 2), (18, 37, 2), (20, 30, 2), (20, 5, 1)])
def test_split_rows_plan_equals_the_fused_product(torch_cuda, k, batch, lanes):
    """VERDICT r4 #5, the A/B plan SR_PLAN_GL_SPLIT_ROWS: the fused rows kernel of a Goldilocks ring product above one tile as two
    launches -- crt of b's tiles in place in the scratch (rows<0>), then the constant-operand product (rows<3>) -- on the one-stream
    and the two-lane plans.  Bit for bit the default plan's product, operands intact, sampled elements against the oracle.  (Measured
    slower on config 4: 158.2-159.0 against 156.1-156.6 ms per shard; it stays as a differential test of the rows kernels.)"""
    torch = torch_cuda
    from stark_rings_amd import CyclotomicRing

    F = O.GOLDILOCKS
    d = 1 << k
    ta = torch.empty(batch * d, dtype=torch.int64, device="cuda")
    tb = torch.empty_like(ta)
    outs = []
    for flags in (0, 256):   # 256 = SR_PLAN_GL_SPLIT_ROWS
        ring = CyclotomicRing("goldilocks", k, device=0, plan=_plan(flags=flags, lanes=lanes))
        ring.fill_uniform_dev(ta, 0xD1, 0)
        ring.fill_uniform_dev(tb, 0xD2, 0)
        a0, b0 = ta.clone(), tb.clone()
        out = torch.empty_like(ta)
        ring.mul_dev(out, ta, tb)
        torch.cuda.synchronize()
        assert torch.equal(ta, a0) and torch.equal(tb, b0), "operands written"
        assert ring.count_noncanonical_dev(out) == 0
        outs.append(out)
        ring.close()
    assert torch.equal(outs[0], outs[1])
    sample = sorted({0, batch // 2, batch - 1})
    ea = np.concatenate([O.fill_uniform(F, 0xD1, e * d, d) for e in sample])
    eb = np.concatenate([O.fill_uniform(F, 0xD2, e * d, d) for e in sample])
    want = O.pow2_ring_mul(F, ea, eb, k, len(sample), 4)
    for i, e in enumerate(sample):
        assert np.array_equal(outs[1][e * d:(e + 1) * d].cpu().numpy().view(np.uint64), want[i * d:(i + 1) * d]), e


@pytest.mark.gpu
@pytest.mark.parametrize("name,k,n", [("goldilocks", 16, 16384), ("babybear", 16, 4099), ("stark", 12, 4096), ("goldilocks24", 0, 1 << 17)])
def test_sum_and_product_at_batch_sizes_of_the_baseline_configs(torch_cuda, name, k, n):
    """Sum / Product over slices as long as the BASELINE batches (config 2: 16 384 elements of degree 2^16 = 8 GiB; a ragged BabyBear
    slice; config 5; 2^17 elements of the reference's own Goldilocks-24 ring): the device fold runs its full ladder of stages (and the
    halving tree of the small ring seventeen levels deep).  Checked on 64 sampled word positions -- gathered on the device, summed as Python
    integers, multiplied left to right by the oracle's slot product -- and, for the sum, by linearity on the whole element:
    sum(a) + sum(a) == sum over the slice of (a + a)."""
    torch = torch_cuda
    base = {"goldilocks24": "goldilocks"}.get(name, name)
    F = O.FIELD_ID[base]
    p = P.PRIMES[base][0]
    L = O.LIMBS[F]
    ring = ring_for(name, k)
    d, w = ring.degree, ring.words_per_elem
    a = torch.empty(n * w, dtype=torch.int64, device="cuda")
    ring.fill_uniform_dev(a, 0xF00D + k, 0)
    s = torch.empty(w, dtype=torch.int64, device="cuda")
    ring.sum_dev(s, a)
    torch.cuda.synchronize()
    slot = 3 if name == "goldilocks24" else 1
    rng = np.random.default_rng(7)
    pos = sorted({0, d - 1} | {int(x) for x in rng.integers(0, d, 62)})
    if slot > 1:   # whole slots, so that the slot product can be folded on the sample
        pos = sorted({q - q % slot + j for q in pos for j in range(slot)})
    idx = torch.tensor([q * L + l for q in pos for l in range(L)], dtype=torch.int64, device="cuda")
    cols = a.view(n, w)[:, idx].contiguous().cpu().numpy().view(np.uint64)          # (n, len(pos) * L) memory images
    std = O.from_mont(F, cols.reshape(-1))
    m = len(pos)
    want = O.to_mont(F, [sum(std[e * m + i] for e in range(n)) % p for i in range(m)])
    got = s[idx].cpu().numpy().view(np.uint64)
    assert np.array_equal(got, want), "sum"
    if name != "goldilocks24":   # linearity on every word: sum(a) + sum(a) == sum(a + a)
        twice = s.clone()
        ring.add_dev(twice, s)
        ring.add_dev(a, a)   # a += a: the kernel reads both operands of a word before it writes that word
        s2 = torch.empty_like(s)
        ring.sum_dev(s2, a)
        torch.cuda.synchronize()
        assert torch.equal(s2, twice), "linearity"
        ring.fill_uniform_dev(a, 0xF00D + k, 0)
    prod = torch.empty(w, dtype=torch.int64, device="cuda")
    ring.product_dev(prod, a)
    torch.cuda.synchronize()
    if slot == 1:
        acc = cols[0].copy()
        for e in range(1, n):
            acc = O.pow2_pointwise(F, acc, cols[e])
    else:   # 24-word blocks of whole slots: pad the sample to whole ring elements for the oracle's 8-slot product
        pad = (-m) % 24
        blk = np.concatenate([cols, np.tile(O.to_mont(F, [1, 0, 0] * (pad // 3)), (n, 1))], axis=1) if pad else cols
        acc = blk[0].copy()
        for e in range(1, n):
            acc = O.small("sro_g24_ntt_mul", acc, blk[e])
        acc = acc[:m]
    assert np.array_equal(prod[idx].cpu().numpy().view(np.uint64), acc), "product"
