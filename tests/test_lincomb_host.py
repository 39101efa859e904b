"""CPU checks of the linear-combination entry points (include/stark_rings_hip.h: sr_lincomb_plan, sr_lincomb_dev, sr_lincomb): the
exports, the plan for every ring and every (K, M) in range against the model's table, the refusals that need no device with their
messages, and the term-at-a-time restatement (tools/model_lincomb.py, the oracle of tests/test_lincomb_gpu.py) against its second
formulation -- the chain of operators the call replaces -- and against closed forms; the permutation product identity and the
cross-multiplied logUp identity on the model, a zero denominator included; the pinned vectors of tests/golden/lincomb_kats.json
regenerate byte for byte."""
import ctypes
import json
import os
import random
import re
import sys

import numpy as np
import pytest

from stark_rings_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import model_frac_tree as FT  # noqa: E402
import model_lincomb as LC  # noqa: E402
import model_prod_tree as PT  # noqa: E402

NEW = ("sr_lincomb_plan", "sr_lincomb_dev", "sr_lincomb")
RINGS = [(0, 10), (1, 16), (2, 12), (3, 0), (4, 0), (5, 0)]
PRIMES = [0xFFFFFFFF00000001, 2013265921, 0x800000000000011000000000000000000000000000000000000000000000001, 15912092521325583641]
PRIME_IDS = ["goldilocks", "babybear", "stark", "frog"]


def test_header_library_and_ctypes_table_carry_the_new_names():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "stark_rings_hip.h")).read()
    declared = set(re.findall(r"\b(sr_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared, "%s is not declared in the header" % name
        assert name in _lib.SYMBOLS, "%s is missing from _lib.SYMBOLS" % name
        assert hasattr(lib, name), "the library does not export %s" % name
    assert re.search(r"SR_LINCOMB_MAX_TABLES = 16, SR_LINCOMB_MAX_OUTPUTS = 4", header)
    for cite in ("dense.rs:288-317", ":370-374", ":386-395"):   # the three reference operators the call composes
        assert cite in header[header.index("Linear combinations (csrc/lincomb.hpp)"):header.index("int sr_lincomb_plan")], cite


def test_the_package_exports_the_mirrors():
    import stark_rings_amd as S
    from stark_rings_amd import lincomb as mod
    from stark_rings_amd import lookup

    assert S.lincomb is mod and callable(mod.lincomb)   # the host-pointer form keeps the module's name: lincomb.lincomb
    for name in ("lincomb_plan", "lincomb_dev"):
        assert getattr(S, name) is getattr(mod, name)
    for name in ("fingerprint", "permutation_leaves", "PermutationCheck", "LookupCheck"):
        assert getattr(S, name) is getattr(lookup, name)
    assert callable(S.DenseMultilinearExtension.linear_combination)
    assert not [n for n in dir(S.CyclotomicRing) if "lincomb" in n]


def _plan(ring, k, n_tables, n_outputs):
    lib = _lib.load()
    launches, per = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib.sr_lincomb_plan(ring, k, n_tables, n_outputs, ctypes.byref(launches), ctypes.byref(per))
    return rc, launches.value, per.value


@pytest.mark.parametrize("ring,k", RINGS)
def test_plan_for_every_ring_and_every_shape(ring, k):
    for K in range(1, 17):
        for M in range(1, 5):
            rc, launches, per = _plan(ring, k, K, M)
            want = LC.plan(ring, K, M)
            assert rc == 0 and (launches, per) == want[:2], (ring, K, M, launches, per, want)
            assert launches == -(-M // per) and 1 <= per <= M


def test_the_plan_splits_where_the_registers_say_so():
    """the table itself (tests/test_lincomb_isa.py holds the register counts behind it): a fingerprint (K <= 4, M <= 2) is one
    launch on the one-limb fields; Stark and the reference's own rings produce one output per launch"""
    assert LC.OUTPUTS == {0: (2, 3), 1: (2, 4), 2: (1, 1), 3: (1, 1), 4: (0, 1), 5: (0, 1)} and LC.REG_TABLES == 4
    assert LC.plan(0, 3, 2) == (1, 2, True) and LC.plan(1, 3, 2) == (1, 2, True)
    assert LC.plan(0, 5, 2) == (1, 2, False) and LC.plan(0, 3, 3) == (1, 3, False) and LC.plan(0, 16, 4) == (2, 3, False)
    assert LC.plan(1, 16, 4) == (1, 4, False)
    assert LC.plan(2, 3, 1) == (1, 1, True) and LC.plan(2, 3, 2) == (2, 1, False) and LC.plan(3, 4, 1) == (1, 1, True)
    for ring in (4, 5):
        assert LC.plan(ring, 3, 2) == (2, 1, False) and LC.plan(ring, 1, 1) == (1, 1, False)


def test_plan_refuses_bad_arguments():
    lib = _lib.load()
    a, b = ctypes.c_int(), ctypes.c_int()
    for args, msg in (((6, 0, 1, 1), "unknown ring"), ((-1, 0, 1, 1), "unknown ring"), ((0, 25, 1, 1), "log2_degree"), ((0, -1, 1, 1), "log2_degree"),
                      ((0, 10, 0, 1), "n_tables outside 1 .. 16"), ((0, 10, 17, 1), "n_tables outside 1 .. 16"),
                      ((0, 10, 1, 0), "n_outputs outside 1 .. 4"), ((0, 10, 1, 5), "n_outputs outside 1 .. 4")):
        assert lib.sr_lincomb_plan(*args, ctypes.byref(a), ctypes.byref(b)) == 1, args
        assert msg in _lib.last_error(), (args, _lib.last_error())
    assert lib.sr_lincomb_plan(0, 10, 1, 1, None, ctypes.byref(b)) == 1 and "null" in _lib.last_error()
    assert lib.sr_lincomb_plan(0, 10, 1, 1, ctypes.byref(a), None) == 1 and "null" in _lib.last_error()


def _call(fn, ctx, outs, tables, n_evals, coef, uses, n, n_outputs=None, n_tables=None):
    lib = _lib.load()
    M = len(outs) if n_outputs is None else n_outputs
    K = len(tables) if n_tables is None else n_tables
    po = (ctypes.c_void_p * max(len(outs), 1))(*outs) if outs is not None else None
    pt = (ctypes.c_void_p * max(len(tables), 1))(*tables) if tables is not None else None
    pe = (ctypes.c_size_t * len(n_evals))(*n_evals) if n_evals is not None else None
    pu = (ctypes.c_uint32 * len(uses))(*uses) if uses is not None else None
    args = [ctx, po, M, pt, pe, K, coef, pu, n]
    if fn == "sr_lincomb_dev":
        args.append(None)
    rc = getattr(lib, fn)(*args)
    return rc, _lib.last_error()


@pytest.mark.parametrize("fn", ["sr_lincomb_dev", "sr_lincomb"])
def test_every_host_checkable_refusal_names_its_reason(fn):
    """These refusals are decided on the arguments alone, before the context is read and before any device work, so they need no
    device: the context here is a block of zeros that is never dereferenced.  A null context is refused first, whatever else is
    wrong."""
    buf = np.zeros(64, dtype=np.uint64)
    d = buf.ctypes.data
    coef = buf.ctypes.data_as(_lib.u64p) if fn == "sr_lincomb" else d
    fake = np.zeros(4096, dtype=np.uint64)
    ctx = fake.ctypes.data
    ok = dict(outs=[d], tables=[d + 64, d + 128], n_evals=None, coef=coef, uses=[0b111], n=1)

    def refused(msg, ctx=ctx, **change):
        rc, err = _call(fn, ctx, **dict(ok, **change))
        assert rc == 1 and msg in err, (change, rc, err)

    refused("null context", ctx=None)
    refused("null context", ctx=None, tables=[], uses=[0], outs=[])   # first, whatever else is wrong
    refused("n_tables outside 1 .. 16", tables=[], uses=[0b1])
    refused("n_tables outside 1 .. 16", tables=[d + 64] * 17, uses=[0b1])
    refused("n_outputs outside 1 .. 4", outs=[])
    refused("n_outputs outside 1 .. 4", outs=[d] * 5, uses=[0b111] * 5)
    refused("null argument", outs=None, n_outputs=1)
    refused("null argument", tables=None, n_tables=2)
    refused("null argument", coef=None)
    refused("null argument", uses=None)
    refused("an output with an empty mask", outs=[d, d + 256], uses=[0b111, 0])
    refused("a mask bit above n_tables", uses=[0b1111])
    refused("a table that no output uses", uses=[0b101])
    refused("n must be below 2^48", n=1 << 48)
    refused("n_evals exceeds n", n_evals=[1, 2])
    refused("null table", tables=[d + 64, None])
    refused("null output", outs=[None])
    assert not fake.any()


# ---- the restatement the GPU tests use as their oracle, pinned on integers modulo each prime --------------------------------------
def _ops(p):
    return 0, (lambda a, b: (a + b) % p), (lambda r, a: r * a % p)


@pytest.mark.parametrize("p", PRIMES, ids=PRIME_IDS)
def test_the_model_matches_its_second_formulation_and_closed_forms(p):
    zero, add, mul = _ops(p)
    rng = random.Random(p)
    draw = lambda: rng.choice((0, 1, p - 1, rng.randrange(p), rng.randrange(p)))  # noqa: E731
    for K in (1, 2, 3, 4, 5, 16):
        for M in (1, 2, 4):
            for n in (0, 1, 5):
                n_evals = [rng.choice((0, 1, max(n - 1, 0), n)) if n else 0 for _ in range(K)]
                tables = [[draw() for _ in range(ne)] for ne in n_evals]
                coef = [[draw() for _ in range(K + 1)] for _ in range(M)]
                uses = [LC.full_mask(K)] + [rng.randrange(1, 2 << K) for _ in range(M - 1)]
                got = LC.lincomb(tables, coef, uses, n, zero, add, mul)
                assert got == LC.composition(tables, coef, uses, n, zero, add, mul), (K, M, n)
                for m in range(M):
                    for e in range(n):
                        want = sum(coef[m][k] * (tables[k][e] if e < n_evals[k] else 0) for k in range(K) if uses[m] >> k & 1)
                        want += coef[m][K] if uses[m] >> K & 1 else 0
                        assert got[m][e] == want % p, (K, M, n, m, e)
                # an entry whose bit is clear is never touched
                holes = [[c if uses[m] >> k & 1 else None for k, c in enumerate(row)] for m, row in enumerate(coef)]
                assert LC.lincomb(tables, holes, uses, n, zero, add, mul) == got
    # the constant goes to every one of the n elements, the truncated part included
    assert LC.lincomb([[5]], [[2, 7]], [0b11], 3, zero, add, mul) == [[17, 7, 7]]
    assert LC.lincomb([[5]], [[2, 7]], [0b10], 3, zero, add, mul) == [[7, 7, 7]]
    assert LC.lincomb([[5]], [[2, 7]], [0b01], 3, zero, add, mul) == [[10, 0, 0]]


def test_the_traffic_model():
    for K in range(1, 17):
        for M in range(1, 5):
            one, comp = LC.traffic(K, M, 10)
            assert one == (K + M) * 10 and comp == M * (3 * K + 3) * 10
    assert LC.traffic(3, 2) == (5, 24) and LC.traffic(4, 1) == (5, 15) and LC.traffic(8, 1) == (9, 27) and LC.traffic(16, 1) == (17, 51)
    one, comp = LC.traffic(16, 1)
    assert 3 * one == comp   # a third of the traffic at M = 1, whatever K


@pytest.mark.parametrize("p", PRIMES, ids=PRIME_IDS)
def test_the_permutation_product_identity(p):
    """three wire columns of 2^5 rows, sigma a permutation of the 96 positions that keeps the wire values: the two grand products
    over all leaves agree, and differ after one sigma entry is changed"""
    zero, add, mul = _ops(p)
    rng = random.Random(p + 2)
    rows, cols = 32, 3
    total = rows * cols
    # positions in cycles of equal wire value
    perm = list(range(total))
    classes = [rng.randrange(12) for _ in range(total)]
    values = [rng.randrange(p) for _ in range(12)]
    for c in range(12):
        members = [i for i in range(total) if classes[i] == c]
        for a, b in zip(members, members[1:] + members[:1]):
            perm[a] = b
    f = [values[classes[i]] for i in range(total)]
    ident = list(range(1, total + 1))
    sigma = [ident[perm[i]] for i in range(total)]
    beta, gamma = rng.randrange(p), rng.randrange(p)

    def roots(sigma):
        num, den = [], []
        for c in range(cols):
            s = slice(c * rows, (c + 1) * rows)
            a, b = LC.permutation_leaves(f[s], ident[s], sigma[s], beta, gamma, 1, zero, add, mul)
            num += a
            den += b
        assert num == [(beta + x + gamma * i) % p for x, i in zip(f, ident)]
        assert den == [(beta + x + gamma * s) % p for x, s in zip(f, sigma)]
        return PT.layers(num, 7, 1, 1, lambda a, b: a * b % p)[-1][0], PT.layers(den, 7, 1, 1, lambda a, b: a * b % p)[-1][0]

    a, b = roots(sigma)
    assert a == b
    bad = list(sigma)
    bad[17] = bad[17] % total + 1
    a, b = roots(bad)
    assert a != b


@pytest.mark.parametrize("p", PRIMES, ids=PRIME_IDS)
def test_the_cross_multiplied_logup_identity(p):
    """2^6 witness rows drawn from a 2^4-row table of two columns, fingerprints beta - (c_0 + gamma c_1) from the model, true
    multiplicities: P_w Q_t == P_t Q_w, also for a beta that makes a table denominator zero (where no inverse exists); not after
    one multiplicity is off by one"""
    zero, add, mul = _ops(p)
    rng = random.Random(p + 3)
    table = [(rng.randrange(1000), rng.randrange(1000)) for _ in range(16)]
    picks = [rng.randrange(16) for _ in range(64)]
    gamma = rng.randrange(p)
    mults = [picks.count(j) for j in range(16)]

    def cross(beta, mults):
        minus = p - 1
        coef = [[minus, (minus * gamma) % p, beta]]
        q_t = LC.lincomb([[r[0] for r in table], [r[1] for r in table]], coef, [0b111], 16, zero, add, mul)[0]
        wit = [table[j] for j in picks]
        q_w = LC.lincomb([[r[0] for r in wit], [r[1] for r in wit]], coef, [0b111], 64, zero, add, mul)[0]
        assert q_t == [(beta - a - gamma * b) % p for a, b in table]
        pw, qw = FT.layers(None, q_w, 6, 1, 0, 1, add, lambda a, b: a * b % p)
        pt, qt = FT.layers([m % p for m in mults], q_t, 4, 1, 0, 1, add, lambda a, b: a * b % p)
        return pw[-1][0] * qt[-1][0] % p == pt[-1][0] * qw[-1][0] % p, q_t

    ok, q_t = cross(rng.randrange(1 << 20, p), mults)
    assert ok and 0 not in q_t
    used = next(j for j in range(16) if mults[j])
    ok, q_t = cross((table[used][0] + gamma * table[used][1]) % p, mults)   # beta equal to a table fingerprint
    assert ok and q_t[used] == 0
    off = list(mults)
    off[used] += 1
    assert not cross(rng.randrange(1 << 20, p), off)[0]


def test_the_pinned_vectors_regenerate_byte_for_byte():
    path = os.path.join(ROOT, "tests", "golden", "lincomb_kats.json")
    assert open(path).read() == LC.dump_kats()
    assert os.path.getsize(path) < 256 << 10
    cases = json.load(open(path))["cases"]
    assert sorted(c["ring_id"] for c in cases) == list(range(6))
    for c in cases:
        shapes = {k: v for k, v in c.items() if isinstance(v, dict)}
        assert sorted((s["n_tables"], s["n_outputs"]) for s in shapes.values()) == [(1, 1), (3, 2), (3, 2), (3, 2), (16, 1)]
        assert shapes["k3_m2_truncated"]["n_evals"] == [0, 1, 2] and shapes["k3_m2_masked"]["uses"] == [0b1011, 0b0101]
        for s in shapes.values():
            assert len(s["outs"]) == s["n_outputs"] and all(len(o) == s["n"] for o in s["outs"])
            assert len(s["coef"]) == s["n_outputs"] and all(len(r) == s["n_tables"] + 1 for r in s["coef"])
