"""Every field's DEVICE arithmetic against exact integers.  tools/ubench/field_ops_device.hip reads operand pairs, runs each
(field, op) in a kernel -- once plainly, once with odd and even lanes in the two arms of a branch -- and on the host build of the
same templates; this file writes the operands, runs the program once and compares every word of every array with Python integers
(moduli and Montgomery constants from oracle/pyref.py, expected values as in tests/test_host_fields.py).  Nothing has a tolerance.

For Stark::mont_mul (inline-asm product scanning on the device, CIOS on the host), StarkL::mul_tw (generated asm columns on the
device, a C++ loop on the host) and the slow path of StarkL::canonical the operands are chosen to reach the branches that matter;
test_operands_reach_the_branches_that_matter shows on the CPU, with integers alone, that they do.  Edge, crafted and uniform
pairs are shuffled together and n is no multiple of 64, so no wave is uniform and the last one is partial."""
import functools
import os
import random
import shutil
import struct
import subprocess

import pytest

import pyref as P
from test_host_fields import (FIELD_EDGES, GOLDILOCKS_MUL_SPECIALS, KAPPA_BITS, NAMES, STARK_LAZY_BOUNDARIES, STARK_LAZY_EDGES,
                              STARK_LAZY_SLOW_PAIRS)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stark_rings_amd", "csrc")
SRC = os.path.join(ROOT, "tools", "ubench", "field_ops_device.hip")
EXE = os.path.join(ROOT, "tools", "ubench", "field_ops_device")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("fields.hpp", "stark_lazy.hpp", "stark_mul_cols.inc")]

N = 4133                      # 64 waves and 37 lanes: the last wave is partial, the last workgroup too
SPECIAL_SHARE = 4             # at least one pair in SPECIAL_SHARE is an edge or crafted one
STARK_L = 4                   # field id of StarkL; 0..3 are NAMES
PLAIN_OPS = (0, 1, 2, 3, 4, 16, 17)
LAZY_OPS = (0, 1, 3, 4, 5, 6, 7, 8, 17, 18, 19, 20)
SP = P.STARK_P
M28, M32, M64, M256 = (1 << 28) - 1, (1 << 32) - 1, (1 << 64) - 1, (1 << 256) - 1
NEED = 8                      # pairs wanted in every class of the coverage test


# ---------------------------------------------------------------- operands
def _stark_borders():
    """Values on both sides of every limb border of the two Stark representations (eight 32-bit, nine 28-bit limbs)."""
    out = []
    for w, top in ((32, 7), (28, 8)):
        for i in range(1, top + 1):
            out += [2**(w * i) - 1, 2**(w * i), 2**(w * i) + 1, SP - 2**(w * i)]
    out += [2**251 - 1, 17 * 2**192 - 1, 17 * 2**192 + 1, (SP - 1) // 2, (SP + 1) // 2]
    assert all(0 <= v < SP for v in out)
    return sorted(set(out))


QUOTIENT_TARGETS = ([M32 << (32 * k) for k in range(8)] + [M256] + [M256 ^ (M32 << (32 * k)) for k in range(8)] + [1 << 255, M32])


def _quotient_pairs(rng, per_target):
    """Pairs (a, b), both below p, whose Montgomery quotient m = -a b p^-1 mod 2^256 is a chosen word pattern: a odd,
    b = -m p a^-1 mod 2^256, kept if below p.  An odd a cannot give m = 2^255 (b would be 2^255): there a b = 2^255 (mod 2^256)
    is met by splitting the power of two between the operands."""
    out = []
    for m in QUOTIENT_TARGETS:
        got = 0
        while got < per_target:
            if m == 1 << 255:
                s = rng.randrange(8, 248)
                a, b = (rng.randrange(1 << (250 - s)) | 1) << s, (rng.randrange(1 << (s - 5)) | 1) << (255 - s)
            else:
                a = rng.randrange(SP) | 1
                b = -m * SP * pow(a, -1, 1 << 256) & M256
            if b < SP:                      # about one try in 32
                assert a < SP and -a * b * pow(SP, -1, 1 << 256) & M256 == m
                out.append((a, b))
                got += 1
    return out


def _result_pairs(rng, r_bits, per_target):
    """Pairs whose Montgomery product a b 2^-r_bits is 0, 1, 2, p - 2 or p - 1."""
    out = []
    for t in (0, 1, 2, SP - 2, SP - 1):
        for _ in range(per_target):
            a = rng.randrange(1, SP)
            out.append((a, t * pow(2, r_bits, SP) * pow(a, -1, SP) % SP))
    return out


def _combination_pairs(rng, ca, cb, per_class):
    """Pairs (a, b) below p whose exact ca a - cb b (StarkL ops 7 and 8: 3a - 5b, 7a - 2b; what canonical() is handed, uncarried)
    is a chosen integer V = q 2^251 + e: fold() subtracts q p, so with c = p - 2^251
      e < q c (q > 0)                      -> the folded value is negative;
      2^251 - e' with e' <= (|q| - 1) c    -> it is p or more, the subtraction of p is kept;
      2^251 - e' with (|q| - 1) c < e'     -> it is in [2^251, p): the subtraction is tried and dropped;
      low limb below q (q > 0) or at least 2^28 + q (q < 0), value elsewhere in range -> limb 0 leaves [0, 2^28)."""
    c = SP - 2**251
    targets = []
    for k in range(per_class):
        qpos = 1 + k % (ca - 1)                       # V < ca p
        qneg = -(1 + k % (cb - 1))                    # V > -cb p
        qneg2 = -(2 + k % max(1, cb - 2))
        small = (0, 1, c - 1)[k % 3] if k < 3 else rng.randrange(c)
        targets.append(qpos * 2**251 + (small if qpos == 1 else rng.randrange(qpos * c)))              # negative
        targets.append((qneg + 1) * 2**251 - ((-qneg - 1) * c + 1 + rng.randrange(c)))                 # [2^251, p): dropped
        targets.append((qneg2 + 1) * 2**251 - (1 + rng.randrange((-qneg2 - 1) * c)))                   # >= p: kept
        mid = rng.randrange(2**220) << 28
        targets.append(qpos * 2**251 + 2**250 + mid + rng.randrange(qpos))                             # limb 0 borrows
        targets.append(qneg * 2**251 + 2**250 + mid + (1 << 28) - 1 - rng.randrange(-qneg))            # limb 0 carries
    out = []
    for v in targets:
        while True:
            b = rng.randrange(SP)
            if (v + cb * b) % ca == 0 and 0 <= (v + cb * b) // ca < SP:
                out.append(((v + cb * b) // ca, b))
                break
    return out


def _mixed(specials, p, rng):
    """N pairs: the special ones shuffled among uniform ones."""
    assert N // SPECIAL_SHARE <= len(specials) <= N // 2, len(specials)
    assert all(0 <= a < p and 0 <= b < p for a, b in specials)
    tagged = [(a, b, True) for a, b in specials] + [(rng.randrange(p), rng.randrange(p), False) for _ in range(N - len(specials))]
    rng.shuffle(tagged)
    return tagged


def _edge_pairs(edges, p, rng, want):
    """Edge x edge (strided when there are many), then edge beside uniform operands on either side until `want` pairs exist."""
    n = len(edges)
    out = [(a, b) for a in edges for b in edges] if n * n <= want // 2 else \
          [(e, e) for e in edges] + [(edges[i], edges[(i * k + 3) % n]) for k in (1, 7) for i in range(n)]
    i = 0
    while len(out) < want:
        e, r = edges[i % n], rng.randrange(p)
        out.append((e, r) if i & 1 else (r, e))
        i += 1
    return out


@functools.lru_cache(maxsize=None)
def operands(field):
    """[(a, b, special)] * N for a field id, the same for each of its ops."""
    rng = random.Random(20240 + field)
    if field == STARK_L:
        edges = sorted(set(STARK_LAZY_EDGES + _stark_borders()))
        bnd = STARK_LAZY_BOUNDARIES
        sp = list(STARK_LAZY_SLOW_PAIRS) + [(b, a) for a, b in STARK_LAZY_SLOW_PAIRS]
        sp += [(bnd[i], bnd[j]) for i in range(len(bnd)) for j in range(len(bnd)) if (i * len(bnd) + j) % 23 == 0]
        sp += _combination_pairs(rng, 3, 5, 12) + _combination_pairs(rng, 7, 2, 12)
        sp += _result_pairs(rng, 280, 16)
        sp += _edge_pairs(edges, SP, rng, 1300 - len(sp))
        return _mixed(sp, SP, rng)
    name = NAMES[field]
    p = P.PRIMES[name][0]
    edges = list(FIELD_EDGES[name])
    sp = []
    if name == "goldilocks":
        edges = sorted(set(edges + [v % p for v in GOLDILOCKS_MUL_SPECIALS]))
    if name == "stark":
        edges = sorted(set(edges + _stark_borders()))
        sp += _quotient_pairs(rng, 10) + _result_pairs(rng, 256, 16)
    sp += _edge_pairs(edges, p, rng, 1300 - len(sp))
    return _mixed(sp, p, rng)


def requests():
    return [(f, op) for f in range(4) for op in PLAIN_OPS] + [(STARK_L, op) for op in LAZY_OPS]


# ---------------------------------------------------------------- expected values
@functools.lru_cache(maxsize=None)
def formula(field, op):
    """(a, b) -> the exact value of the op, before reduction modulo p; the formulas of tests/test_host_fields.py."""
    if field == STARK_L:
        rinv, r256inv = pow(pow(2, 280, SP), -1, SP), pow(pow(2, 256, SP), -1, SP)
        return {0: lambda a, b: a + b, 1: lambda a, b: a - b, 3: lambda a, b: a * b * rinv, 4: lambda a, b: (a & M64) << 280,
                5: lambda a, b: (a + 6 * b) * b * rinv + (a - 6 * b) * (a + 6 * b) * rinv, 6: lambda a, b: 256 * a,
                7: lambda a, b: 3 * a - 5 * b, 8: lambda a, b: 7 * a - 2 * b, 17: lambda a, b: a * a * rinv, 18: lambda a, b: a * b * rinv,
                19: lambda a, b: a, 20: lambda a, b: a * b * r256inv}[op]
    name = NAMES[field]
    p, _, limbs = P.PRIMES[name]
    rb_inv = pow(pow(2, 64 * limbs, p), -1, p)
    kap_inv = pow(pow(2, KAPPA_BITS[name], p), -1, p)
    kap = KAPPA_BITS[name]
    return {0: lambda a, b: a + b, 1: lambda a, b: a - b, 2: lambda a, b: a * b * rb_inv, 3: lambda a, b: a * b * kap_inv,
            4: lambda a, b: ((a & M64) % p) << kap, 16: lambda a, b: -a, 17: lambda a, b: a * a * kap_inv}[op]


def expected(field, op, a, b):
    return formula(field, op)(a, b) % (SP if field == STARK_L else P.PRIMES[NAMES[field]][0])


# ---------------------------------------------------------------- StarkL in integers: load, relax, fold, canonical as stark_lazy.hpp has them
def lz_load(v):
    return [(v >> (28 * i)) & M28 for i in range(8)] + [v >> 224]


def lz_value(x):
    return sum(l << (28 * i) for i, l in enumerate(x))


def lz_relax(x):
    x = list(x)
    for i in range(8):
        c = x[i] >> 28
        x[i] &= M28
        x[i + 1] += c
    return x


def lz_fold(x):
    x = list(x)
    q = x[8] >> 27
    x[8] &= (1 << 27) - 1
    x[7] -= q
    x[6] -= q << 24
    x[0] -= q
    return x


def lz_canonical(x):
    """(canonical limbs, the set of arms taken)"""
    x = lz_fold(lz_relax(x))
    for i in (6, 7):
        c = x[i] >> 28
        x[i] &= M28
        x[i + 1] += c
    arms = set()
    if not 0 <= x[0] <= M28 or not 0 <= x[8] < (1 << 27):
        arms.add("slow")
        if not 0 <= x[0] <= M28:
            arms.add("limb0")
        x = lz_relax(x)
        if x[8] < 0:
            arms.add("negative")
            x = lz_relax([x[0] + 1] + x[1:6] + [x[6] + (1 << 24), x[7] + 1, x[8] + (1 << 27)])
        elif x[8] >= (1 << 27):
            y = lz_relax([x[0] - 1] + x[1:6] + [x[6] - (1 << 24), x[7] - 1, x[8] - (1 << 27)])
            arms.add("kept" if y[8] >= 0 else "dropped")
            if y[8] >= 0:
                x = y
    else:
        arms.add("fast")
    return x, arms


def lz_combination(op, a, b):
    """The uncarried limbs StarkL ops 7 and 8 hand to store(): 3a - 5b and 7a - 2b limb by limb."""
    ca, cb = {7: (3, 5), 8: (7, 2)}[op]
    return [ca * x - cb * y for x, y in zip(lz_load(a), lz_load(b))]


def _assert_invariants(x):
    assert all(abs(l) < 2**31 - 16 for l in x) and abs(lz_value(x)) < 16 * SP, x


def test_operands_reach_the_branches_that_matter():
    """Integers only.  Every operand is canonical, every lazy state of the StarkL ops stays inside the documented invariants
    (|limb| < 2^31 - 16, |value| < 16 p), no wave of 64 is all edge or all uniform, and at least NEED pairs of the set reach:
    Stark::mont_mul with and without its final subtraction, with a zero word and with an all-ones word in the quotient; for
    StarkL ops 7 and 8, the fast path and every arm of the slow path of canonical()."""
    for field in range(5):
        ops = operands(field)
        p = SP if field == STARK_L else P.PRIMES[NAMES[field]][0]
        assert len(ops) == N and N % 64 != 0
        assert all(0 <= a < p and 0 <= b < p for a, b, _ in ops)
        for w in range(0, N, 64):
            kinds = {s for _, _, s in ops[w:w + 64]}
            assert kinds == {True, False}, "wave %d is uniform" % (w // 64)

    count = dict.fromkeys(("taken", "not taken", "zero word", "ones word"), 0)
    for a, b, _ in operands(2):
        m = -a * b * pow(SP, -1, 1 << 256) & M256
        assert (a * b + m * SP) & M256 == 0
        count["taken" if (a * b + m * SP) >> 256 >= SP else "not taken"] += 1
        words = [(m >> (32 * k)) & M32 for k in range(8)]
        count["zero word"] += 0 in words and a * b != 0
        count["ones word"] += M32 in words
    assert min(count.values()) >= NEED, count

    for a, b, _ in operands(STARK_L):
        for x, y in ((a, b), (b, a)):
            s, d = lz_load(x), lz_load(x)
            for _ in range(6):                                   # op 5
                s = [u + v for u, v in zip(s, lz_load(y))]
                d = [u - v for u, v in zip(d, lz_load(y))]
                _assert_invariants(s)
                _assert_invariants(d)
            r = lz_load(x)
            for _ in range(4):                                   # op 6
                r = [4 * l for l in r]
                _assert_invariants(r)
                r = lz_fold(lz_relax(r))
                _assert_invariants(r)
    for op in (7, 8):
        count = dict.fromkeys(("fast", "slow", "limb0", "negative", "kept", "dropped"), 0)
        for a, b, _ in operands(STARK_L):
            for x, y in ((a, b), (b, a)):                        # the divergent launch swaps the even lanes' operands
                state = lz_combination(op, x, y)
                _assert_invariants(state)
                c, arms = lz_canonical(state)
                assert lz_value(c) == expected(STARK_L, op, x, y) and all(0 <= l <= M28 for l in c)
                for arm in arms:
                    count[arm] += 1
        assert min(count.values()) >= NEED, (op, count)


# ---------------------------------------------------------------- the driver
def _build():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    if not hipcc:
        pytest.fail("hipcc not found: cannot build tools/ubench/field_ops_device")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-o", EXE, SRC], check=True, cwd=ROOT, stdout=subprocess.PIPE,
                   stderr=subprocess.PIPE, timeout=900)


def _words(v):
    return v.to_bytes(32, "little")


def write_requests(path):
    reqs = requests()
    with open(path, "wb") as f:
        f.write(b"SRFOPRQ1" + struct.pack("<II", len(reqs), 0))
        for field, op in reqs:
            f.write(struct.pack("<IIII", field, op, N, 0))
            f.write(b"".join(_words(a) + _words(b) for a, b, _ in operands(field)))


def run_driver(tmp_path, host_only):
    """One run of the driver over every request -> {(field, op): [array of N integers] * (2 or 4)}"""
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in DEPS):
        _build()
    req, res = str(tmp_path / "requests.bin"), str(tmp_path / "results.bin")
    write_requests(req)
    r = subprocess.run([EXE] + (["--host-only"] if host_only else []) + [req, res], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    data = open(res, "rb").read()
    count, with_device = struct.unpack_from("<II", data, 8)
    assert data[:8] == b"SRFOPRS1" and count == len(requests()) and with_device == (0 if host_only else 1)
    arrays = 2 if host_only else 4
    out, off = {}, 16
    for field, op in requests():
        assert struct.unpack_from("<IIII", data, off) == (field, op, N, 0)
        off += 16
        out[(field, op)] = [[int.from_bytes(data[off + 32 * (k * N + i):off + 32 * (k * N + i + 1)], "little") for i in range(N)]
                            for k in range(arrays)]
        off += 32 * arrays * N
    assert off == len(data)
    return out


ARRAY_NAMES = ("host build, plain", "host build, divergent order", "device, plain launch", "device, divergent launch")


def compare(results):
    wrong = []
    for (field, op), arrays in results.items():
        ops = operands(field)
        plain = [expected(field, op, a, b) for a, b, _ in ops]
        swapped = [plain[i] if i & 1 else expected(field, op, b, a) for i, (a, b, _) in enumerate(ops)]
        for k, got in enumerate(arrays):
            want = swapped if k & 1 else plain
            bad = [i for i in range(N) if got[i] != want[i]]
            if bad:
                i = bad[0]
                wrong.append("field %d op %d, %s: %d of %d wrong, first at %d: a=%#x b=%#x got %#x want %#x"
                             % (field, op, ARRAY_NAMES[k], len(bad), N, i, ops[i][0], ops[i][1], got[i], want[i]))
    assert not wrong, "\n".join(wrong[:20])


def test_host_build_of_the_driver_equals_integers(tmp_path):
    """--host-only: no HIP call is made.  The op definitions of the driver are right before any GPU sees them."""
    compare(run_driver(tmp_path, host_only=True))


@pytest.mark.gpu
def test_device_field_arithmetic_equals_integers(tmp_path):
    """Kernels and host build, plain and divergent launch, every word against Python integers."""
    results = run_driver(tmp_path, host_only=False)
    assert all(len(arrays) == 4 for arrays in results.values())
    compare(results)
