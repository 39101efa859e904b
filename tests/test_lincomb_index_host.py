"""CPU checks of the integer-column entry points (include/stark_rings_hip.h: sr_lincomb_index_plan, sr_lincomb_index_dev,
sr_lincomb_index, sr_index_count_dev, sr_index_count): the exports, the plan for every ring and every (K, J, M) in range against the
model's table and the constants of csrc/lincomb_index.hpp, the refusals that need no device with their messages, and the restatement
(tools/model_lincomb_index.py, the oracle of tests/test_lincomb_index_gpu.py): R::from(x) by doubling and adding against x additions
and against the closed form, the linear combination against integers modulo each prime, the multiplicities against a plain count;
the pinned vectors of tests/golden/lincomb_index_kats.json regenerate byte for byte."""
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
import model_lincomb as LC  # noqa: E402
import model_lincomb_index as LI  # noqa: E402

NEW = ("sr_lincomb_index_plan", "sr_lincomb_index_dev", "sr_lincomb_index", "sr_index_count_dev", "sr_index_count")
RINGS = [(0, 10), (1, 16), (2, 12), (3, 0), (4, 0), (5, 0)]
PRIMES = [0xFFFFFFFF00000001, 2013265921, 0x800000000000011000000000000000000000000000000000000000000000001, 15912092521325583641]
PRIME_IDS = ["goldilocks", "babybear", "stark", "frog"]
U64 = 1 << 64


def test_header_library_and_ctypes_table_carry_the_new_names():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "stark_rings_hip.h")).read()
    declared = set(re.findall(r"\b(sr_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared, "%s is not declared in the header" % name
        assert name in _lib.SYMBOLS, "%s is missing from _lib.SYMBOLS" % name
        assert hasattr(lib, name), "the library does not export %s" % name
    assert re.search(r"SR_LINCOMB_MAX_INDEX_COLUMNS = 8", header)
    assert re.search(r"typedef struct sr_index_column \{\s*const uint64_t \*values;[^}]*size_t n_evals;[^}]*uint64_t start;[^}]*\} sr_index_column;", header)
    assert "multilinear_polynomial.rs:79-133" in header


def test_the_package_exports_the_mirrors():
    import stark_rings_amd as S
    from stark_rings_amd import index_columns as mod
    from stark_rings_amd import lookup

    for name in ("IndexColumn", "lincomb_index_plan", "lincomb_index_dev", "lincomb_index", "from_u64_dev", "identity_permutation",
                 "identity_permutation_mles", "index_count_dev", "index_count"):
        assert getattr(S, name) is getattr(mod, name), name
    for name in ("permutation_leaves_indexed", "fingerprint_indexed"):
        assert getattr(S, name) is getattr(lookup, name)
    assert callable(S.LookupCheck.from_indices)
    assert not [n for n in dir(S.CyclotomicRing) if n.startswith("index_count") or "lincomb" in n or "from_u64" in n]
    assert ctypes.sizeof(mod.sr_index_column) == 24
    # the column object's own checks
    col = S.IndexColumn(start=7)
    assert col.is_progression and col.start == 7
    stored = S.IndexColumn(np.arange(5, dtype=np.uint64), n_evals=3)
    assert not stored.is_progression and stored.n_evals == 3
    for bad in (dict(values=np.arange(5, dtype=np.uint64), start=1), dict(start=U64), dict(start=-1), dict(n_evals=2),
                dict(values=np.arange(5, dtype=np.uint64), n_evals=6)):
        with pytest.raises(S.RingError):
            S.IndexColumn(**bad)


def _plan(ring, k, n_tables, n_index, n_outputs):
    lib = _lib.load()
    launches, per = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib.sr_lincomb_index_plan(ring, k, n_tables, n_index, n_outputs, ctypes.byref(launches), ctypes.byref(per))
    return rc, launches.value, per.value


@pytest.mark.parametrize("ring,k", RINGS)
def test_plan_for_every_ring_and_every_shape(ring, k):
    for K in range(0, 17):
        for J in range(0, 9):
            if not 1 <= K + J <= 16:
                continue
            for M in range(1, 5):
                rc, launches, per = _plan(ring, k, K, J, M)
                want = LI.plan(ring, K, J, M)
                assert rc == 0 and (launches, per) == want[:2], (ring, K, J, M, launches, per, want)
                assert launches == -(-M // per) and 1 <= per <= M
                if J == 0:   # sr_lincomb's plan
                    a, b = ctypes.c_int(), ctypes.c_int()
                    assert _lib.load().sr_lincomb_plan(ring, k, K, M, ctypes.byref(a), ctypes.byref(b)) == 0
                    assert (a.value, b.value) == (launches, per)


def test_the_plan_table_equals_the_constants_of_the_header():
    src = open(os.path.join(ROOT, "stark_rings_amd", "csrc", "lincomb_index.hpp")).read()
    assert re.search(r"constexpr int kRegTerms = %d;" % LI.REG_TERMS, src)
    assert re.search(r"kRegOutputs = std::is_same<T, Goldilocks>::value \|\| std::is_same<T, BabyBear>::value \? 2 : "
                     r"std::is_same<T, SlotG24>::value \? 1 : 0;", src)
    assert re.search(r"kRunOutputs = std::is_same<T, BabyBear>::value \? 4 : std::is_same<T, Goldilocks>::value \? 3 : 1;", src)
    assert re.search(r"constexpr size_t kLdsBins = %d;" % LI.LDS_BINS, src)
    assert re.search(r"MAX_COLUMNS = 8, MAX_TERMS = 16", src)
    assert LI.OUTPUTS == {0: (2, 3), 1: (2, 4), 2: (0, 1), 3: (1, 1), 4: (0, 1), 5: (0, 1)}
    from stark_rings_amd import index_columns

    assert index_columns.LDS_BINS == LI.LDS_BINS and index_columns.MAX_INDEX_COLUMNS == LI.MAX_COLUMNS
    # a column of permutation leaves (K = 1, J = 2, M = 2) is one launch on the one-limb fields
    assert LI.plan(0, 1, 2, 2) == (1, 2, True) and LI.plan(1, 1, 2, 2) == (1, 2, True)
    assert LI.plan(2, 1, 2, 2) == (2, 1, False) and LI.plan(3, 1, 2, 1) == (1, 1, True) and LI.plan(3, 1, 2, 2) == (2, 1, False)
    assert LI.plan(0, 3, 2, 2) == (1, 2, False) and LI.plan(0, 8, 8, 4) == (2, 3, False) and LI.plan(1, 0, 8, 4) == (1, 4, False)
    assert LI.traffic() == (3, 5)


def test_plan_refuses_bad_arguments():
    lib = _lib.load()
    a, b = ctypes.c_int(), ctypes.c_int()
    for args, msg in (((6, 0, 1, 1, 1), "unknown ring"), ((0, 25, 1, 1, 1), "log2_degree"), ((0, 10, -1, 1, 1), "n_tables outside 0 .. 16"),
                      ((0, 10, 17, 0, 1), "n_tables outside 0 .. 16"), ((0, 10, 1, 9, 1), "n_index outside 0 .. 8"),
                      ((0, 10, 1, -1, 1), "n_index outside 0 .. 8"), ((0, 10, 0, 0, 1), "n_tables + n_index outside 1 .. 16"),
                      ((0, 10, 9, 8, 1), "n_tables + n_index outside 1 .. 16"), ((0, 10, 1, 1, 0), "n_outputs outside 1 .. 4"),
                      ((0, 10, 1, 1, 5), "n_outputs outside 1 .. 4")):
        assert lib.sr_lincomb_index_plan(*args, ctypes.byref(a), ctypes.byref(b)) == 1, args
        assert msg in _lib.last_error(), (args, _lib.last_error())
    assert lib.sr_lincomb_index_plan(0, 10, 1, 1, 1, None, ctypes.byref(b)) == 1 and "null" in _lib.last_error()
    assert lib.sr_lincomb_index_plan(0, 10, 1, 1, 1, ctypes.byref(a), None) == 1 and "null" in _lib.last_error()


def _call(fn, ctx, outs, tables, n_evals, columns, coef, uses, n, n_outputs=None, n_tables=None, n_index=None):
    from stark_rings_amd.index_columns import sr_index_column

    lib = _lib.load()
    M = len(outs) if n_outputs is None else n_outputs
    K = len(tables) if n_tables is None else n_tables
    J = len(columns) if n_index is None else n_index
    po = (ctypes.c_void_p * max(len(outs), 1))(*outs) if outs is not None else None
    pt = (ctypes.c_void_p * max(len(tables), 1))(*tables) if tables is not None else None
    pe = (ctypes.c_size_t * len(n_evals))(*n_evals) if n_evals is not None else None
    pc = (sr_index_column * max(len(columns), 1))(*[sr_index_column(*c) for c in columns]) if columns is not None else None
    pu = (ctypes.c_uint32 * len(uses))(*uses) if uses is not None else None
    args = [ctx, po, M, pt, pe, K, pc, J, coef, pu, n]
    if fn == "sr_lincomb_index_dev":
        args.append(None)
    rc = getattr(lib, fn)(*args)
    return rc, _lib.last_error()


@pytest.mark.parametrize("fn", ["sr_lincomb_index_dev", "sr_lincomb_index"])
def test_every_host_checkable_refusal_names_its_reason(fn):
    """These refusals are decided on the arguments alone, before the context is read and before any device work, so they need no
    device: the context here is a block of zeros that is never dereferenced.  A null context is refused first."""
    buf = np.zeros(64, dtype=np.uint64)
    d = buf.ctypes.data
    coef = buf.ctypes.data_as(_lib.u64p) if fn == "sr_lincomb_index" else d
    fake = np.zeros(4096, dtype=np.uint64)
    ctx = fake.ctypes.data
    # one table, a stored column and a progression
    ok = dict(outs=[d], tables=[d + 64], n_evals=None, columns=[(d + 128, 1, 0), (None, 0, 5)], coef=coef, uses=[0b1111], n=1)

    def refused(msg, ctx=ctx, **change):
        rc, err = _call(fn, ctx, **dict(ok, **change))
        assert rc == 1 and msg in err, (change, rc, err)

    refused("null context", ctx=None)
    refused("null context", ctx=None, tables=[], columns=[], uses=[0], outs=[])   # first, whatever else is wrong
    refused("n_tables outside 0 .. 16", tables=[d + 64] * 17, columns=[], uses=[0b1])
    refused("n_tables outside 0 .. 16", n_tables=-1)
    refused("n_index outside 0 .. 8", columns=[(None, 0, 0)] * 9, uses=[0b1])
    refused("n_index outside 0 .. 8", n_index=-1)
    refused("n_tables + n_index outside 1 .. 16", tables=[], columns=[], uses=[0b1])
    refused("n_tables + n_index outside 1 .. 16", tables=[d + 64] * 12, columns=[(None, 0, 0)] * 5, uses=[0b1])
    refused("n_outputs outside 1 .. 4", outs=[])
    refused("n_outputs outside 1 .. 4", outs=[d] * 5, uses=[0b1111] * 5)
    refused("null argument", outs=None, n_outputs=1)
    refused("null argument", tables=None, n_tables=1)
    refused("null argument", columns=None, n_index=2)
    refused("null argument", coef=None)
    refused("null argument", uses=None)
    refused("an output with an empty mask", outs=[d, d + 256], uses=[0b1111, 0])
    refused("a mask bit above n_tables + n_index", uses=[0b11111])
    refused("a table that no output uses", uses=[0b1110])
    refused("a column that no output uses", uses=[0b1101])
    refused("a column that no output uses", uses=[0b1011])
    refused("n must be below 2^48", n=1 << 48)
    refused("n_evals exceeds n", n_evals=[2])
    refused("a column's n_evals exceeds n", columns=[(d + 128, 2, 0), (None, 0, 5)])
    refused("a stored column with a non-zero start", columns=[(d + 128, 1, 9), (None, 0, 5)])
    refused("a progression wraps", columns=[(d + 128, 1, 0), (None, 0, U64 - 1)], n=2)
    refused("a progression wraps", columns=[(d + 128, 1, 0), (None, 0, U64 - 4)], n=6, n_evals=[1])
    refused("null table", tables=[None])
    refused("null output", outs=[None])
    assert not fake.any()


@pytest.mark.parametrize("fn", ["sr_index_count_dev", "sr_index_count"])
def test_index_count_refusals(fn):
    lib = _lib.load()
    buf = np.zeros(16, dtype=np.uint64)
    d = buf.ctypes.data
    fake = np.zeros(4096, dtype=np.uint64)
    ptr = (lambda a: ctypes.cast(a, _lib.u64p)) if fn == "sr_index_count" else (lambda a: a)
    tail = [None] if fn == "sr_index_count_dev" else []
    for args, msg in (((None, ptr(d), ptr(d + 64), 1, 1), "null context"),
                      ((fake.ctypes.data, ptr(d), ptr(d + 64), 1 << 48, 1), "n must be below 2^48"),
                      ((fake.ctypes.data, ptr(d), ptr(d + 64), 1, 1 << 48), "n_bins must be below 2^48"),
                      ((fake.ctypes.data, None, ptr(d + 64), 1, 1), "null counts"),
                      ((fake.ctypes.data, ptr(d), None, 1, 1), "null indices"),
                      ((fake.ctypes.data, ptr(d), ptr(d + 8), 4, 4), "counts overlaps the indices")):
        assert getattr(lib, fn)(*args, *tail) == 1, args
        assert msg in _lib.last_error(), (args, _lib.last_error())
    assert not fake.any()


# ---- the restatement the GPU tests use as their oracle, pinned on integers modulo each prime --------------------------------------
def _ops(p):
    return 0, (lambda a, b: (a + b) % p), (lambda r, a: r * a % p)


@pytest.mark.parametrize("p", PRIMES, ids=PRIME_IDS)
def test_from_u64_by_doubling_matches_repeated_addition_and_the_closed_form(p):
    zero, add, mul = _ops(p)
    for x in range(41):
        assert LI.from_u64(x, 1, zero, add) == LI.from_u64_repeated(x, 1, zero, add) == x % p
    for x in LI.edge_values(p) + [random.Random(p).randrange(U64) for _ in range(50)]:
        assert LI.from_u64(x, 1, zero, add) == x % p, x
    # on ring elements of a power-of-two ring: every coefficient x mod p; on a slot image: component 0 of every slot
    vadd = lambda a, b: tuple((x + y) % p for x, y in zip(a, b))  # noqa: E731
    one, z = (1, 1, 1, 1), (0, 0, 0, 0)
    for x in (0, 1, 40, U64 - 1) + ((p, p + 1) if p < U64 else ()):
        assert LI.from_u64(x, one, z, vadd) == (x % p,) * 4
        if x <= 40:
            assert LI.from_u64_repeated(x, one, z, vadd) == (x % p,) * 4
    r = 12345 % p   # a slot ring's one(): (R, 0, 0) per slot
    assert LI.from_u64(U64 - 1, (r, 0, 0, r, 0, 0), (0,) * 6, vadd) == ((U64 - 1) * r % p, 0, 0, (U64 - 1) * r % p, 0, 0)


@pytest.mark.parametrize("p", PRIMES, ids=PRIME_IDS)
def test_the_model_matches_closed_forms(p):
    zero, add, mul = _ops(p)
    rng = random.Random(p + 5)
    draw = lambda: rng.choice((0, 1, p - 1, rng.randrange(p), rng.randrange(p)))  # noqa: E731
    edges = LI.edge_values(p)
    for K, J in ((0, 1), (0, 8), (1, 2), (2, 2), (3, 1), (4, 1), (8, 8), (15, 1)):
        for M in (1, 2, 4):
            for n in (0, 1, 5):
                T = K + J
                n_evals = [rng.choice((0, 1, max(n - 1, 0), n)) if n else 0 for _ in range(K)]
                tables = [[draw() for _ in range(ne)] for ne in n_evals]
                cols, ints = [], []
                for j in range(J):
                    if rng.random() < 0.4:
                        start = rng.choice((0, U64 - n if n else 0, p - 2 if p < U64 else 7, rng.randrange(U64 - n)))
                        cols.append(LI.Progression(start))
                        ints.append([start + e for e in range(n)])
                    else:
                        ne = rng.choice((0, 1, max(n - 1, 0), n)) if n else 0
                        vals = [rng.choice(edges + [rng.randrange(U64)]) for _ in range(ne)]
                        cols.append(vals)
                        ints.append(vals + [0] * (n - ne))
                coef = [[draw() for _ in range(T + 1)] for _ in range(M)]
                uses = [(2 << T) - 1] + [rng.randrange(1, 2 << T) for _ in range(M - 1)]
                got = LI.lincomb_index(tables, cols, coef, uses, n, zero, 1, add, mul)
                for m in range(M):
                    for e in range(n):
                        want = sum(coef[m][k] * (tables[k][e] if e < n_evals[k] else 0) for k in range(K) if uses[m] >> k & 1)
                        want += sum(coef[m][K + j] * ints[j][e] for j in range(J) if uses[m] >> (K + j) & 1)
                        want += coef[m][T] if uses[m] >> T & 1 else 0
                        assert got[m][e] == want % p, (K, J, M, n, m, e)
                holes = [[c if uses[m] >> k & 1 else None for k, c in enumerate(row)] for m, row in enumerate(coef)]
                assert LI.lincomb_index(tables, cols, holes, uses, n, zero, 1, add, mul) == got
                if J and K:   # the columns as tables of R::from: sr_lincomb's model gives the same
                    as_tables = tables + [[x % p for x in c] for c in ints]
                    assert LC.lincomb(as_tables, coef, uses, n, zero, add, mul) == got
    assert LI.lincomb_index([], [[5]], [[2, 7]], [0b11], 3, zero, 1, add, mul) == [[17, 7, 7]]
    assert LI.lincomb_index([], [LI.Progression(4)], [[2, 7]], [0b01], 3, zero, 1, add, mul) == [[8, 10, 12]]
    with pytest.raises(AssertionError):
        LI.column_values(LI.Progression(U64 - 1), 2)
    # the leaves of a permutation argument from integers are those from tables of R::from
    f = [draw() for _ in range(6)]
    sigma = [3, 5, 0, 1, 2, 4]
    beta, gamma = draw(), draw()
    assert LI.permutation_leaves_indexed(f, 10, sigma, beta, gamma, 1, zero, add, mul) == \
        LC.permutation_leaves(f, [10 + e for e in range(6)], sigma, beta, gamma, 1, zero, add, mul)


def test_the_count_of_the_model():
    rng = random.Random(7)
    idx = [rng.randrange(12) for _ in range(500)]
    counts, skipped = LI.index_count(idx, 10)
    assert counts == [idx.count(t) for t in range(10)] and skipped == idx.count(10) + idx.count(11)
    assert LI.index_count([], 3) == ([0, 0, 0], 0) and LI.index_count([U64 - 1], 0) == ([], 1)


def test_the_pinned_vectors_regenerate_byte_for_byte():
    path = os.path.join(ROOT, "tests", "golden", "lincomb_index_kats.json")
    assert open(path).read() == LI.dump_kats()
    assert os.path.getsize(path) < 256 << 10
    cases = json.load(open(path))["cases"]
    assert sorted(c["ring_id"] for c in cases) == list(range(6))
    for c in cases:
        shapes = {k: v for k, v in c.items() if isinstance(v, dict)}
        assert sorted((s["n_tables"], s["n_index"], s["n_outputs"]) for s in shapes.values()) == [(0, 1, 1), (0, 8, 1), (1, 2, 2), (2, 2, 1), (3, 2, 2)]
        assert shapes["k1_j2_m2_leaves"]["uses"] == [0b1011, 0b1101]
        for s in shapes.values():
            assert len(s["outs"]) == s["n_outputs"] and all(len(o) == s["n"] for o in s["outs"])
            assert len(s["coef"]) == s["n_outputs"] and all(len(r) == s["n_tables"] + s["n_index"] + 1 for r in s["coef"])
            assert len(s["columns"]) == s["n_index"]
