"""CPU checks of the batch inversion (include/stark_rings_hip.h: sr_inverse_plan, sr_inverse_batch_dev, sr_inverse_batch,
sr_inverse_zero_count): the exports and the plan, the refusals that need no device, and the restatement tools/model_inverse.py -- the
chunked walk against the direct inverse over Z_97, Goldilocks and an Fq3, zeros at every position of a chunk with their count; every
chain against its exponent (integer bookkeeping) and against pow() on a small field; the op-count table against an instrumented mul."""
import ctypes
import os
import random
import re
import sys

import pytest

from stark_rings_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import model_inverse as MI  # noqa: E402

NEW = ("sr_inverse_plan", "sr_inverse_batch_dev", "sr_inverse_batch", "sr_inverse_zero_count")
RINGS = [(0, 10), (1, 16), (2, 12), (3, 0), (4, 0), (5, 0)]
CHUNKS = (1, 2, 3, 8, 17)
# (order, zero, one, mul) and a draw of one non-zero element
MODELS = {
    "z97": (MI.prime_model(97), lambda rng: rng.randrange(1, 97)),
    "goldilocks": (MI.prime_model(MI.GOLDILOCKS_P), lambda rng: rng.choice((1, 2, MI.GOLDILOCKS_P - 1, 2**32, rng.randrange(1, MI.GOLDILOCKS_P)))),
    # 2 is no cube modulo 7 (the cubes are 1 and 6), so u^3 - 2 is irreducible: a field of 343 elements
    "fq3_7": (MI.fq3_model(7, 2), lambda rng: rng.choice([(a, b, c) for a in range(7) for b in range(7) for c in range(7)][1:])),
    # the slot field of goldilocks24: NONRESIDUE = 2^40 (oracle/pyref.py: fq3_mul)
    "fq3_goldilocks": (MI.fq3_model(MI.GOLDILOCKS_P, 2**40), lambda rng: tuple(rng.randrange(MI.GOLDILOCKS_P) for _ in range(3))[:2] + (1,)),
}


def test_header_library_and_ctypes_table_carry_the_new_names():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "stark_rings_hip.h")).read()
    declared = set(re.findall(r"\b(sr_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared, "%s is not declared in the header" % name
        assert name in _lib.SYMBOLS, "%s is missing from _lib.SYMBOLS" % name
        assert hasattr(lib, name), "the library does not export %s" % name
    block = header[header.index("Batch inversion (csrc/inverse.hpp)"):header.index("int sr_inverse_plan")]
    for word in ("batch_inversion", "Field::inverse", "sr_inverse_zero_count", "in place"):
        assert word in block, word


def test_the_package_exports_the_mirrors():
    import stark_rings_amd as S
    from stark_rings_amd import inverse as mod

    assert S.inverse is mod and callable(mod.inverse)   # the host-pointer form keeps the module's name: inverse.inverse
    for name in ("inverse_plan", "inverse_dev", "inverse_zero_count"):
        assert getattr(S, name) is getattr(mod, name)
    # the ring carries the plan, the host-pointer form and the count; the device form is the module's function, as lincomb_dev is
    for name in ("inverse_plan", "inverse", "inverse_zero_count"):
        assert callable(getattr(S.CyclotomicRing, name))


def _plan(ring, k, n, has_num):
    lib = _lib.load()
    work, launches, chunk = ctypes.c_size_t(99), ctypes.c_int(-1), ctypes.c_size_t(0)
    rc = lib.sr_inverse_plan(ring, k, n, has_num, ctypes.byref(work), ctypes.byref(launches), ctypes.byref(chunk))
    return rc, work.value, launches.value, chunk.value


@pytest.mark.parametrize("ring,k", RINGS)
def test_the_plan_is_host_arithmetic_and_matches_the_models_table(ring, k):
    fam = [f for f, i in MI.RING_IDS.items() if i == ring][0]
    for has_num in (0, 1):
        assert _plan(ring, k, 0, has_num) == (0, 0, 0, MI.CHOSEN[fam][has_num])
        for n in (1, 7, 1 << 20):
            assert _plan(ring, k, n, has_num) == (0, 0, 1, MI.CHOSEN[fam][has_num])
    src = open(os.path.join(ROOT, "stark_rings_amd", "csrc", "inverse.hpp")).read()
    assert "constexpr int kRun = %d;" % MI.RUN in src


def test_the_plan_refuses_with_a_reason():
    lib = _lib.load()
    work, launches, chunk = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_size_t()
    args = (ctypes.byref(work), ctypes.byref(launches), ctypes.byref(chunk))
    assert lib.sr_inverse_plan(6, 0, 1, 0, *args) != 0 and "unknown ring id" in _lib.last_error()
    assert lib.sr_inverse_plan(0, 25, 1, 0, *args) != 0 and "log2_degree out of range" in _lib.last_error()
    assert lib.sr_inverse_plan(0, 4, 1 << 47, 0, *args) != 0 and "element count too large" in _lib.last_error()
    assert lib.sr_inverse_plan(0, 4, 1, 0, None, ctypes.byref(launches), ctypes.byref(chunk)) != 0 and "null result pointer" in _lib.last_error()
    out = ctypes.c_ulonglong()
    assert lib.sr_inverse_batch_dev(None, None, None, None, 0, None, 0, None) != 0 and "null context" in _lib.last_error()
    assert lib.sr_inverse_batch(None, None, None, None, 0) != 0 and "null context" in _lib.last_error()
    assert lib.sr_inverse_zero_count(None, ctypes.byref(out), None) != 0 and "null context" in _lib.last_error()


# ---- the walk ----------------------------------------------------------------------------------------------------------------------
def _tables(name, chunk):
    """(den, label) for every n and zero placement the issue lists, around this chunk length"""
    (order, zero, one, mul), draw = MODELS[name]
    rng = random.Random("inverse host %s %d" % (name, chunk))
    for n in sorted({1, max(chunk - 1, 1), chunk, chunk + 1, 3 * chunk + 1}):
        yield [draw(rng) for _ in range(n)], "n=%d" % n
    n = 3 * chunk + 1
    base = [draw(rng) for _ in range(n)]
    for where, at in (("first", chunk), ("middle", chunk + chunk // 2), ("last", 2 * chunk - 1)):   # of the second chunk
        den = list(base)
        den[at] = zero
        yield den, "zero at the %s position" % where
    den = list(base)
    den[chunk:2 * chunk] = [zero] * chunk
    yield den, "a whole chunk of zeros"
    yield [zero] * n, "all zeros"


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("name", sorted(MODELS))
def test_the_chunked_walk_equals_the_direct_inverse_and_counts_the_zeros(name, chunk):
    (order, zero, one, mul), draw = MODELS[name]
    rng = random.Random("inverse host numerators " + name)
    for den, label in _tables(name, chunk):
        for num in (None, [draw(rng) for _ in den]):
            got, zeros = MI.batch_inverse(den, num, chunk, order, zero, one, mul)
            want, want_zeros = MI.direct_inverse(den, num, order, zero, one, mul)
            assert got == want, (label, num is not None)
            assert zeros == want_zeros == sum(1 for d in den if d == zero), label
            for d, g, e in zip(den, got, range(len(den))):   # and by the defining property: out * den == num
                assert g == zero if d == zero else mul(g, d) == (one if num is None else num[e]), label


def test_the_small_prime_inverse_is_pythons():
    order, zero, one, mul = MI.prime_model(97)
    den = list(range(97))
    got, zeros = MI.batch_inverse(den, None, 8, order, zero, one, mul)
    assert zeros == 1 and got == [0] + [pow(x, -1, 97) for x in range(1, 97)]


# ---- the chains ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", sorted(MI.FIELDS))
def test_every_chain_computes_the_fermat_exponent(fam):
    order = MI.FIELDS[fam]
    steps = MI.chain(order - 2)
    assert MI.chain_exponent(steps) == order - 2
    # the value, on a small field: the chain is a recipe for x^e whatever the modulus, so Z_p with a small p checks the recipe
    for p in (97, 65537):
        for x in (1, 2, 3, p - 1, 57):
            assert MI.run_chain(steps, x, lambda a, b: a * b % p) == pow(x, order - 2, p), (fam, p, x)
    counted = [0]

    def mul(a, b):
        counted[0] += 1
        return a * b % 97

    MI.run_chain(steps, 5, mul)
    assert counted[0] == MI.chain_products(steps)
    # a run of eight ones never costs more than eight squarings and a product, so the chain is at most ten products (u) worse than
    # square-and-multiply, and far better where |F| - 2 is mostly ones
    assert MI.chain_products(steps) <= MI.square_and_multiply_products(order - 2) + 10
    if fam in ("goldilocks", "babybear", "stark"):
        assert MI.chain_products(steps) == {"goldilocks": 86, "babybear": 48, "stark": 286}[fam]


def test_the_kernels_exponents_are_the_models():
    """csrc/inverse.hpp spells |F| - 2 as 64-bit words; they are the model's integers"""
    src = open(os.path.join(ROOT, "stark_rings_amd", "csrc", "inverse.hpp")).read()
    names = {"Goldilocks": "goldilocks", "BabyBear": "babybear", "Stark": "stark", "SlotG24": "goldilocks24", "SlotB72": "babybear72",
             "SlotFrog": "frog16"}
    for cpp, fam in names.items():
        body = src[src.index("struct Exponent<%s>" % cpp):]
        body = body[:body.index("};")]
        e = MI.FIELDS[fam] - 2
        assert int(re.search(r"kBits = (\d+);", body).group(1)) == e.bit_length(), fam
        words = [int(w, 16) for w in re.findall(r"0x([0-9A-F]{16})ull", body)]
        if fam == "stark":   # three words of ones are written as ~0ull
            assert "i < 3 ? ~0ull" in body
            words = [2**64 - 1] * 3 + words
        assert sum(w << (64 * i) for i, w in enumerate(words)) == e, fam


@pytest.mark.parametrize("chunk", MI.CHUNKS)
def test_the_op_count_table_is_what_an_instrumented_mul_counts(chunk):
    table = MI.op_table()
    for fam, order in MI.FIELDS.items():
        # the walk's products do not depend on the field, only the chain does: run the walk on Z_97 with this family's chain length
        inv = MI.chain_products(MI.chain(order - 2))
        for has_num in (False, True):
            assert table[fam, chunk, has_num] * chunk == MI.walk_products(chunk, has_num, inv)
    counted = [0]

    def mul(a, b):
        counted[0] += 1
        return a * b % 97

    rng = random.Random(chunk)
    den = [rng.randrange(1, 97) for _ in range(chunk)]
    inv97 = MI.chain_products(MI.chain(95))
    for num in (None, den):
        counted[0] = 0
        MI.batch_inverse(den, num, chunk, 97, 0, 1, mul)
        assert counted[0] == MI.walk_products(chunk, num is not None, inv97)
    for fam, (c0, c1) in MI.CHOSEN.items():
        assert c0 in MI.CHUNKS and c1 in MI.CHUNKS and c1 <= c0, fam
