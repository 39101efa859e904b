"""Every `_dev` call that predates the polynomial work, at every placement of its pointer arguments.

include/stark_rings_hip.h promises one layout for every entry point: no padding, 8-byte aligned (4-byte for the packed BabyBear
boundary).  The streaming kernels choose between a 16-byte body (two coefficients per lane) and a one-coefficient body from the
pointer bits and the parity of the count; whole torch allocations (256-byte aligned, nothing in front, nothing behind) only ever
reach the first.  Here every pointer of every call is placed 0 and 8 bytes behind a 16-byte boundary (0 .. 12 bytes in steps of 4
for the packed words; 0, 4, 8 for the wire bytes) inside one allocation with guard words in front of and behind it, and after every
call
  1. the output equals the expected words (Python integers on the oracle's standard-form values, the oracle's slot products,
     transforms, decomposition and wire bytes -- never the call under test at another placement),
  2. every guard word in front of and behind every output is intact,
  3. every input is unchanged word for word, including the poison behind it (POISON of test_mle_gpu.py),
  4. count_noncanonical_dev(out) == 0 where the output holds ring words,
  5. the output is the same at every placement.
GROUPS below is the case table as data; tests/test_dev_boundaries_host.py checks without a GPU that it names every `_dev` method and
that its size rules yield the counts they claim."""
import itertools

import numpy as np
import pytest

import oracle_lib as O
import pyref as P
from test_mle_gpu import POISON, SLOT_MUL, host, model_for

pytestmark = pytest.mark.gpu
GUARD = 0x6B6B6B6B6B6B6B6B
PAD = 32  # guard bytes in front of the payload's 16-byte boundary, and behind the payload
PRE = {"goldilocks24": "sro_g24_", "babybear72": "sro_bb72_", "frog16": "sro_frog16_"}
SMALL_D = {"goldilocks24": 24, "babybear72": 72, "frog16": 16}

# ---- the case table -------------------------------------------------------------------------------------------------------------
POW2 = [("goldilocks", 0), ("goldilocks", 1), ("goldilocks", 6), ("babybear", 0), ("babybear", 1), ("babybear", 5), ("stark", 0), ("stark", 4)]
SMALL = [("goldilocks24", 0), ("babybear72", 0), ("frog16", 0)]
RINGS = POW2 + SMALL
REDUCE_RINGS = [(n, k) for n, k in POW2 if k >= 1]
PACKED_RINGS = [("babybear", 0), ("babybear", 1), ("babybear", 5)]
PACKED_NTT_RINGS = [("babybear", 0), ("babybear", 4), ("babybear", 12)]
NTT_RINGS = [("goldilocks", 6), ("goldilocks", 13), ("goldilocks", 16), ("babybear", 5), ("babybear", 12), ("babybear", 16), ("stark", 4),
             ("stark", 12)] + SMALL
LINALG_RINGS = [("goldilocks", 5), ("babybear", 6), ("stark", 4)] + SMALL
FOLD_LENGTHS = (1, 2, 3, 33, 67)
BASES = (2, 10, 1 << 16, (1 << 32) + 2)
WIDE_BASIS = (1 << 64) + 2


def degree(name, k):
    return SMALL_D.get(name, 1 << k)


def stream_batches(d, span=512):
    """Batches of a ring of degree d whose coefficient counts b * d are the smallest at which the bodies of a streaming kernel
    differ: 1, 2 and 3 coefficients (the nearest batches), the largest count not above span - 2, exactly span (one workgroup of 256
    lanes in the widest body) where d divides it, the first count above span, and the first above 2 span that is no multiple of span."""
    out = {1, 2, 3, span // d + 1}
    if (span - 2) // d:
        out.add((span - 2) // d)
    if span % d == 0:
        out.add(span // d)
    b = 2 * span // d + 1
    while (b * d) % span == 0:
        b += 1
    out.add(b)
    return sorted(out)


def quad_batches(d):
    """the same for the packed words: four per lane, 1024 per workgroup; 4 and 5 coefficients for the quad's own tail"""
    return sorted(set(stream_batches(d, 1024)) | {(4 + d - 1) // d, (5 + d - 1) // d})


SIZE_RULES = {"stream": (stream_batches, 512), "quads": (quad_batches, 1024)}
# group -> the methods it covers, its rings and the size rule of its batches (None: the shapes are the group's own, named in its test)
GROUPS = {
    "binary": {"calls": ["add_dev", "sub_dev", "ntt_mul_dev"], "rings": RINGS, "sizes": "stream"},
    "unary": {"calls": ["neg_dev", "scale_dev", "add_scalar_dev"], "rings": RINGS, "sizes": "stream"},
    "broadcast": {"calls": ["mul_elem_dev", "mul_elem_add_dev"], "rings": RINGS, "sizes": "stream"},
    "folds": {"calls": ["sum_dev", "product_dev", "product_poly_dev"], "rings": RINGS, "sizes": None},
    "rot": {"calls": ["rot_dev"], "rings": RINGS, "sizes": "stream"},
    "reduce": {"calls": ["reduce_dev"], "rings": REDUCE_RINGS, "sizes": "stream"},
    "gadget": {"calls": ["gadget_decompose_dev", "gadget_recompose_dev"], "rings": RINGS, "sizes": "stream"},
    "wire": {"calls": ["serialize_dev", "deserialize_dev"], "rings": RINGS, "sizes": "stream"},
    "pack32": {"calls": ["pack32_dev", "unpack32_dev"], "rings": PACKED_RINGS, "sizes": "quads"},
    "packed32_elementwise": {"calls": ["add_packed32_dev", "sub_packed32_dev", "ntt_mul_packed32_dev"], "rings": PACKED_RINGS, "sizes": "quads"},
    "packed32_transforms": {"calls": ["elementwise_crt_packed32_dev", "elementwise_icrt_packed32_dev", "mul_packed32_dev"],
                            "rings": PACKED_NTT_RINGS, "sizes": None},
    "transforms": {"calls": ["elementwise_crt_dev", "elementwise_icrt_dev", "mul_dev", "mul_ntt_rhs_dev"], "rings": NTT_RINGS, "sizes": None},
    "linalg": {"calls": ["matvec_ntt_dev", "spmv_ntt_dev", "matmul_ntt_dev"], "rings": LINALG_RINGS, "sizes": None},
    # the helpers every check above leans on: run at the shifted pointers by the groups that use them
    "helpers": {"calls": ["fill_uniform_dev", "count_noncanonical_dev"], "rings": RINGS, "sizes": None},
}
ids = lambda rings: ["%s-%d" % r for r in rings]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


# ---- placement ------------------------------------------------------------------------------------------------------------------
def _pattern(value, nbytes):
    return np.full((nbytes + 7) // 8, value, dtype=np.uint64).view(np.uint8)[:nbytes]


def image(words, shift, tail):
    """the bytes of one allocation: guard, the payload `shift` units (of the payload's item size) behind a 16-byte boundary, `tail`"""
    return np.concatenate([_pattern(GUARD, PAD + shift * words.itemsize), np.ascontiguousarray(words).view(np.uint8).reshape(-1),
                           _pattern(tail, PAD)])


def placed(torch, words, shift, tail=GUARD):
    """(view, whole buffer): `words` inside one allocation, guard words in front, `tail` words behind (GUARD behind an output, POISON
    behind an input), the view starting `shift` items behind a 16-byte boundary"""
    kinds = {8: torch.int64, 4: torch.int32, 1: torch.uint8}
    whole = torch.from_numpy(image(words, shift, tail)).cuda()
    off = PAD + shift * words.itemsize
    view = whole[off:off + words.nbytes].view(kinds[words.itemsize])
    assert whole.data_ptr() % 16 == 0 and view.data_ptr() % 16 == words.itemsize * shift and view.numel() == words.size
    return view, whole


def check(whole, want, shift, tail, what, payload=True):
    """checks 1 - 3 on one buffer: the guard in front, the payload (an input's own words, an output's expected ones), the words behind"""
    got, img = whole.cpu().numpy(), image(want, shift, tail)
    off = PAD + shift * want.itemsize
    end = off + want.nbytes
    assert got.size == img.size
    assert np.array_equal(got[:off], img[:off]), "%s: the words in front were written" % (what,)
    assert np.array_equal(got[end:], img[end:]), "%s: the words behind were written" % (what,)
    if payload:
        bad = np.flatnonzero(got[off:end] != img[off:end])
        assert bad.size == 0, "%s: %d wrong bytes, the first in item %d of %d" % (what, bad.size, bad[0] // want.itemsize if bad.size else -1, want.size)


def sweep(torch, ring, operands, call, want, what, shifts=(0, 1), canonical=True):
    """operands: (name, words, kind) with kind "in" (only read: poison behind it), "out" or "io" (written: guards around it), in the
    order `call` takes them; want: name -> expected words of every written operand (None: not compared, see the caller).  Runs the
    call at every combination of shifts and applies the five checks; returns the outputs of the first placement."""
    first = None
    per = [shifts if isinstance(shifts, tuple) else shifts[nm] for nm, _, _ in operands]
    for combo in itertools.product(*per):
        bufs = [placed(torch, words, s, POISON if kind == "in" else GUARD) for (nm, words, kind), s in zip(operands, combo)]
        call(*[v for v, _ in bufs])
        outs = {}
        for (nm, words, kind), s, (view, whole) in zip(operands, combo, bufs):
            label = "%s, %s at shifts %s" % (what, nm, combo)
            if kind == "in":
                check(whole, words, s, POISON, label + " (input)")
                continue
            w = want[nm]
            check(whole, words if w is None else w, s, GUARD, label, payload=w is not None)
            if canonical:
                assert ring.count_noncanonical_dev(view) == 0, label
            outs[nm] = view.cpu().numpy().copy()
        if first is None:
            first = outs
        for nm in outs:
            assert np.array_equal(outs[nm], first[nm]), "%s: %s differs between placements %s" % (what, nm, combo)
    return first


# ---- models ---------------------------------------------------------------------------------------------------------------------
def data(m, seed, batch):
    """uniform elements with p - 1, 0, 1 in the first coefficients and p - 1 in the last"""
    a = m.uniform(seed, batch)
    n, L = batch * m.ring.degree, m.ring.limbs
    e = O.to_mont(m.F, [m.p - 1, 0, 1][:min(n, 3)])
    a[:e.size] = e
    if n > 3:
        a[-L:] = O.to_mont(m.F, [m.p - 1])
    return a


def ints(m, words):
    return O.from_mont(m.F, words)


def mont(m, vals):
    return O.to_mont(m.F, [int(v) for v in vals])


def slot_mul(m, a, b):
    return O.pow2_pointwise(m.F, a, b) if m.pow2 else O.small(SLOT_MUL[m.name][0], a, b)


def dot(m, pairs):
    """sum of the slot products of (a, b) pairs of ring elements: the oracle's products, integer sums"""
    acc = [0] * m.ring.degree
    for a, b in pairs:
        acc = [(x + y) % m.p for x, y in zip(acc, ints(m, slot_mul(m, a, b)))]
    return mont(m, acc)


def crt(m, a, batch):
    return O.pow2_fwd(m.F, a, m.k, batch) if m.pow2 else O.small(PRE[m.name] + "crt", a)


def icrt(m, a, batch):
    return O.pow2_inv(m.F, a, m.k, batch) if m.pow2 else O.small(PRE[m.name] + "icrt", a)


def ring_mul(m, a, b, batch):
    if m.pow2:
        return O.pow2_ring_mul(m.F, a, b, m.k, batch)
    return icrt(m, slot_mul(m, crt(m, a, batch), crt(m, b, batch)), batch)


def el(m, buf, i):
    return buf[i * m.w:(i + 1) * m.w]


# ---- the helpers the checks lean on ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", RINGS, ids=ids(RINGS))
def test_fill_uniform_and_count_noncanonical(torch_cuda, name, k):
    """fill_uniform_dev against the oracle's generator; count_noncanonical_dev counts exactly the planted coefficients and not the
    poison behind the slice"""
    torch = torch_cuda
    m = model_for(name, k)
    ring, d, L = m.ring, m.ring.degree, m.ring.limbs
    for b in stream_batches(d):
        n = b * d
        what = "%s-%d batch %d" % (name, k, b)
        sweep(torch, ring, [("t", np.full(n * L, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64), "out")], lambda t: ring.fill_uniform_dev(t, 0x1B1, 5),
              {"t": O.fill_uniform(m.F, 0x1B1, 5, n)}, "fill_uniform_dev " + what)
        a = m.uniform(0x1C1 + b, b)
        planted = sorted({0, n // 2, n - 1})
        for i in planted:
            a[i * L:(i + 1) * L] = np.uint64(0xFFFFFFFFFFFFFFFF)   # at or above every modulus (POISON is below the Goldilocks prime)
        for s in (0, 1):
            view, whole = placed(torch, a, s, POISON)
            assert ring.count_noncanonical_dev(view) == len(planted), (what, s)
            check(whole, a, s, POISON, "count_noncanonical_dev " + what)


# ---- element-wise ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", RINGS, ids=ids(RINGS))
def test_binary_in_place(torch_cuda, name, k):
    """add_dev, sub_dev, ntt_mul_dev: lhs and rhs at every placement, and lhs aliasing rhs"""
    torch = torch_cuda
    m = model_for(name, k)
    ring, p = m.ring, m.p
    for b in stream_batches(ring.degree):
        x, y = data(m, 0x101 + b, b), data(m, 0x202 + b, b)
        X, Y = ints(m, x), ints(m, y)
        want = {"add_dev": mont(m, [(u + v) % p for u, v in zip(X, Y)]), "sub_dev": mont(m, [(u - v) % p for u, v in zip(X, Y)]),
                "ntt_mul_dev": slot_mul(m, x, y)}
        alias = {"add_dev": mont(m, [2 * u % p for u in X]), "sub_dev": np.zeros_like(x), "ntt_mul_dev": slot_mul(m, x, x)}
        for fn in GROUPS["binary"]["calls"]:
            what = "%s %s-%d batch %d" % (fn, name, k, b)
            sweep(torch, ring, [("lhs", x, "io"), ("rhs", y, "in")], getattr(ring, fn), {"lhs": want[fn]}, what)
            sweep(torch, ring, [("lhs", x, "io")], lambda t: getattr(ring, fn)(t, t), {"lhs": alias[fn]}, what + " aliased")


@pytest.mark.parametrize("name,k", RINGS, ids=ids(RINGS))
def test_unary_in_place(torch_cuda, name, k):
    """neg_dev; scale_dev with the scalars 0, 1, p - 1; add_scalar_dev in coefficient form (coefficient 0 of every element) and in
    CRT/NTT form (component 0 of every slot)"""
    torch = torch_cuda
    m = model_for(name, k)
    ring, p, d = m.ring, m.p, m.ring.degree
    slot = 1 if m.pow2 else SLOT_MUL[name][1]
    for b in stream_batches(d):
        x = data(m, 0x303 + b, b)
        X = ints(m, x)
        what = "%s-%d batch %d" % (name, k, b)
        sweep(torch, ring, [("t", x, "io")], ring.neg_dev, {"t": mont(m, [(p - v) % p for v in X])}, "neg_dev " + what)
        for sc in (0, 1, p - 1):
            s_img = O.to_mont(m.F, [sc])
            sweep(torch, ring, [("t", x, "io")], lambda t: ring.scale_dev(t, s_img), {"t": mont(m, [v * sc % p for v in X])},
                  "scale_dev by %d %s" % (sc, what))
        for sc in (1, p - 1):
            s_img = O.to_mont(m.F, [sc])
            coeff = [(v + sc) % p if i % d == 0 else v for i, v in enumerate(X)]
            ntt = [(v + sc) % p if i % slot == 0 else v for i, v in enumerate(X)]
            sweep(torch, ring, [("t", x, "io")], lambda t: ring.add_scalar_dev(t, s_img, False), {"t": mont(m, coeff)},
                  "add_scalar_dev coefficient form %s" % what)
            sweep(torch, ring, [("t", x, "io")], lambda t: ring.add_scalar_dev(t, s_img, True), {"t": mont(m, ntt)},
                  "add_scalar_dev ntt form %s" % what)


@pytest.mark.parametrize("name,k", RINGS, ids=ids(RINGS))
def test_broadcast_of_one_ring_element(torch_cuda, name, k):
    """mul_elem_dev (t, elem) and mul_elem_add_dev (acc, x, r) at all four resp. eight placements, and with acc aliasing x"""
    torch = torch_cuda
    m = model_for(name, k)
    ring, p = m.ring, m.p
    r = data(m, 0x404, 1)
    for b in stream_batches(ring.degree):
        x, acc = data(m, 0x505 + b, b), data(m, 0x606 + b, b)
        prod = slot_mul(m, x, np.tile(r, b))
        what = "%s-%d batch %d" % (name, k, b)
        sweep(torch, ring, [("t", x, "io"), ("elem", r, "in")], ring.mul_elem_dev, {"t": prod}, "mul_elem_dev " + what)
        PR = ints(m, prod)
        sweep(torch, ring, [("acc", acc, "io"), ("x", x, "in"), ("r", r, "in")], ring.mul_elem_add_dev,
              {"acc": mont(m, [(u + v) % p for u, v in zip(ints(m, acc), PR)])}, "mul_elem_add_dev " + what)
        sweep(torch, ring, [("acc", x, "io"), ("r", r, "in")], lambda t, rr: ring.mul_elem_add_dev(t, t, rr),
              {"acc": mont(m, [(u + v) % p for u, v in zip(ints(m, x), PR)])}, "mul_elem_add_dev, acc is x, " + what)


# ---- folds ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", RINGS, ids=ids(RINGS))
def test_folds_over_a_slice(torch_cuda, name, k):
    """sum_dev, product_dev (slices only read, poison behind them) and product_poly_dev (the slice holds its transform afterwards);
    element 1 is all p - 1; `out` is one ring element with guards on both sides"""
    torch = torch_cuda
    m = model_for(name, k)
    ring, p, d, w = m.ring, m.p, m.ring.degree, m.w
    for n in FOLD_LENGTHS:
        a = data(m, 0x707 + n, n)
        if n >= 2:
            a[w:2 * w] = m.const(p - 1, 1)
        A = ints(m, a)
        seed = np.full(w, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
        what = "%s-%d slice of %d" % (name, k, n)
        want_sum = mont(m, [sum(A[e * d + i] for e in range(n)) % p for i in range(d)])
        sweep(torch, ring, [("out", seed, "out"), ("elems", a, "in")], ring.sum_dev, {"out": want_sum}, "sum_dev " + what)
        acc = el(m, a, 0).copy()
        for e in range(1, n):
            acc = slot_mul(m, acc, el(m, a, e))
        sweep(torch, ring, [("out", seed, "out"), ("elems", a, "in")], ring.product_dev, {"out": acc}, "product_dev " + what)
        fa = crt(m, a, n)
        acc = el(m, fa, 0).copy()
        for e in range(1, n):
            acc = slot_mul(m, acc, el(m, fa, e))
        sweep(torch, ring, [("out", seed, "out"), ("elems", a, "io")], ring.product_poly_dev, {"out": icrt(m, acc, 1), "elems": fa},
              "product_poly_dev " + what)


# ---- rot, reduce ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", RINGS, ids=ids(RINGS))
def test_rot(torch_cuda, name, k):
    torch = torch_cuda
    m = model_for(name, k)
    ring, d = m.ring, m.ring.degree
    for b in stream_batches(d):
        a = data(m, 0x808 + b, b)
        want = O.rot(m.F, a, d, name in ("goldilocks24", "babybear72"))
        sweep(torch, ring, [("out", np.full_like(a, 0x5A5A5A5A5A5A5A5A), "out"), ("a", a, "in")], ring.rot_dev, {"out": want},
              "rot_dev %s-%d batch %d" % (name, k, b))


@pytest.mark.parametrize("name,k", REDUCE_RINGS, ids=ids(REDUCE_RINGS))
def test_reduce(torch_cuda, name, k):
    """in_len 1, D - 1, D, D + 1, 2D - 1, 2D: odd and even rows of the input at both shifts, poison behind the last row"""
    torch = torch_cuda
    m = model_for(name, k)
    ring, d, L = m.ring, m.ring.degree, m.ring.limbs
    for in_len in sorted({1, d - 1, d, d + 1, 2 * d - 1, 2 * d}):
        for b in stream_batches(d):
            src = O.fill_uniform(m.F, 0x909 + in_len + b, 0, b * in_len)
            src[:L] = O.to_mont(m.F, [m.p - 1])
            want = np.concatenate([O.pow2_reduce(m.F, src[e * in_len * L:(e + 1) * in_len * L], in_len, k) for e in range(b)])
            sweep(torch, ring, [("out", np.full(b * m.w, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64), "out"), ("coeffs", src, "in")],
                  lambda o, c: ring.reduce_dev(o, c, in_len), {"out": want}, "reduce_dev %s-%d in_len %d batch %d" % (name, k, in_len, b))


# ---- gadget decomposition -------------------------------------------------------------------------------------------------------
def padding_for(basis, p):
    pad = 1
    while (basis // 2) * (basis ** pad - 1) // (basis - 1) < (p - 1) // 2:
        pad += 1
    return pad + 1


def edge_coefficients(m, a, basis):
    p = m.p
    edge = O.to_mont(m.F, [0, 1, p - 1, (p - 1) // 2, (p - 1) // 2 + 1, 2, p - 2, basis % p, (basis // 2) % p, (basis // 2 + 1) % p])
    n = min(edge.size, a.size)
    a[:n] = edge[:n]
    return a


@pytest.mark.parametrize("name,k", RINGS, ids=ids(RINGS))
def test_gadget_decompose_and_recompose(torch_cuda, name, k):
    """bases 2, 10, 2^16, 2^32 + 2 against the oracle's digits (Stark and frog16 also 2^64 + 2 through the wide entry points, against
    the big-integer model); the padding and the edge coefficients of test_decomposition_matches_oracle"""
    torch = torch_cuda
    m = model_for(name, k)
    ring, p, d, w = m.ring, m.p, m.ring.degree, m.w
    bases = BASES + ((WIDE_BASIS,) if name in ("stark", "frog16") else ())
    for basis in bases:
        pad = padding_for(basis, p)
        sizes = stream_batches(d)
        if pad * m.w > 4096:  # Stark in basis 2 and 10 (253 and 77 digits of 32 bytes): the three smallest and the two largest counts
            sizes = sizes[:3] + sizes[-2:]
        for b in sizes:
            a = edge_coefficients(m, m.uniform(0xA0A + b, b), basis)
            if basis < 1 << 64:
                digits, over = O.decompose_balanced(m.F, a, d, b, basis, pad)
                assert not over
                assert np.array_equal(O.recompose(m.F, digits, d, b, basis, pad), a)
            else:
                A = ints(m, a)
                flat = [0] * (b * pad * d)
                for e in range(b):
                    for i in range(d):
                        for j, x in enumerate(P.decompose_balanced(A[e * d + i], p, basis, pad)):
                            flat[(e * pad + j) * d + i] = x % p
                digits = mont(m, flat)
            what = "%s-%d basis %d batch %d" % (name, k, basis, b)
            sweep(torch, ring, [("out", np.full(b * pad * w, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64), "out"), ("a", a, "in")],
                  lambda o, t: ring.gadget_decompose_dev(o, t, basis, pad), {"out": digits}, "gadget_decompose_dev " + what)
            assert ring.decompose_overflow_count() == 0, what
            sweep(torch, ring, [("out", np.full(b * w, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64), "out"), ("digits", digits, "in")],
                  lambda o, t: ring.gadget_recompose_dev(o, t, basis, pad), {"out": a}, "gadget_recompose_dev " + what)


@pytest.mark.parametrize("name,k", RINGS, ids=ids(RINGS))
def test_gadget_decompose_counts_overflow_at_every_placement(torch_cuda, name, k):
    """eight digits in basis 2 hold |x| < 2^8 only: the count of the coefficients that needed more is the integer count (want_over of
    test_decomposition_errors) whichever body ran -- the pair body adds 0, 1 or 2 per lane, the other one per coefficient"""
    torch = torch_cuda
    m = model_for(name, k)
    ring, p, d, w = m.ring, m.p, m.ring.degree, m.w
    for b in stream_batches(d):
        a = m.uniform(0xB0B + b, b)
        small = O.to_mont(m.F, [0, 1, p - 1, 255, p - 255, 256, p - 256][:min(7, b * d)])  # every other one of a pair overflows
        a[:small.size] = small
        want_over = sum(1 for v in ints(m, a) if abs(v - p if v > (p - 1) // 2 else v) >= 2 ** 8)
        assert ring.decompose_overflow_count() == 0
        for so, si in itertools.product((0, 1), repeat=2):
            out, whole_out = placed(torch, np.full(b * 8 * w, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64), so)
            src, whole_in = placed(torch, a, si, POISON)
            ring.gadget_decompose_dev(out, src, 2, 8)
            what = "%s-%d batch %d at shifts %s" % (name, k, b, (so, si))
            assert ring.decompose_overflow_count() == want_over, what
            check(whole_out, host(out), so, GUARD, what, payload=False)
            check(whole_in, a, si, POISON, what + " (input)")


# ---- wire format ----------------------------------------------------------------------------------------------------------------
def wire_shifts(m):
    return (0, 8) + ((4,) if m.ring.wire_coeff_bytes == 4 else ())


@pytest.mark.parametrize("name,k", RINGS, ids=ids(RINGS))
def test_wire_format(torch_cuda, name, k):
    """serialize_dev / deserialize_dev, dense and with offsets that leave 8-byte gaps, against the oracle's bytes (as
    test_wire_format_matches_oracle builds them); the wire buffer 0 and 8 bytes behind a 16-byte boundary (4 for the BabyBear rings)"""
    torch = torch_cuda
    m = model_for(name, k)
    ring, p, d, w, wb = m.ring, m.p, m.ring.degree, m.w, m.ring.wire_coeff_bytes
    per = d * wb
    shifts = {"wire": wire_shifts(m), "a": (0, 1), "out": (0, 1)}
    for b in stream_batches(d):
        a = data(m, 0xC0C + b, b)
        if b * d >= 4:
            a[3 * m.ring.limbs:4 * m.ring.limbs] = O.to_mont(m.F, [(p - 1) // 2])
        dense = O.serialize(m.F, a)
        assert dense.size == b * per
        what = "%s-%d batch %d" % (name, k, b)
        blank = np.full(b * per, 0x6B, dtype=np.uint8)
        sweep(torch, ring, [("wire", blank, "out"), ("a", a, "in")], ring.serialize_dev, {"wire": dense}, "serialize_dev dense " + what,
              shifts=shifts, canonical=False)
        sweep(torch, ring, [("out", np.full_like(a, 0x5A5A5A5A5A5A5A5A), "out"), ("wire", dense, "in")], ring.deserialize_dev, {"out": a},
              "deserialize_dev dense " + what, shifts=shifts)
        assert ring.wire_invalid_count() == 0, what
        # offsets: element e at byte e * (per + 8), the gaps keep what the caller had there
        offs = np.arange(b, dtype=np.int64) * (per + 8)
        t_offs = torch.from_numpy(offs).cuda()
        framed = np.full(b * (per + 8), 0x6B, dtype=np.uint8)
        for e in range(b):
            framed[offs[e]:offs[e] + per] = dense[e * per:(e + 1) * per]
        sweep(torch, ring, [("wire", np.full_like(framed, 0x6B), "out"), ("a", a, "in")], lambda wr, t: ring.serialize_dev(wr, t, t_offs),
              {"wire": framed}, "serialize_dev with offsets " + what, shifts=shifts, canonical=False)
        sweep(torch, ring, [("out", np.full_like(a, 0x5A5A5A5A5A5A5A5A), "out"), ("wire", framed, "in")],
              lambda o, wr: ring.deserialize_dev(o, wr, t_offs), {"out": a}, "deserialize_dev with offsets " + what, shifts=shifts)
        assert ring.wire_invalid_count() == 0, what


@pytest.mark.parametrize("name,k", RINGS, ids=ids(RINGS))
def test_wire_errors_are_counted_alike_at_every_placement(torch_cuda, name, k):
    """one wire coefficient >= p (read as 0 and counted) and one misaligned offset (the element skipped on the way out, zero on the way in,
    and counted): the count and the stored zeros are the same whichever body ran"""
    torch = torch_cuda
    m = model_for(name, k)
    ring, p, d, w, wb, L = m.ring, m.p, m.ring.degree, m.w, m.ring.wire_coeff_bytes, m.ring.limbs
    per = d * wb
    shifts = {"wire": wire_shifts(m), "a": (0, 1), "out": (0, 1)}
    for b in (2, 3, 512 // d + 1):
        a = data(m, 0xD0D + b, b)
        dense = O.serialize(m.F, a)
        n = b * d
        hit = n - 1 if n % 2 == 0 else n // 2            # the second of a pair where there are pairs
        bad = dense.copy()
        bad[hit * wb:(hit + 1) * wb] = np.frombuffer(p.to_bytes(wb, "little"), dtype=np.uint8)
        ref, obad = O.deserialize(m.F, bad)
        zeroed = a.copy()
        zeroed[hit * L:(hit + 1) * L] = 0
        assert obad == 1 and np.array_equal(ref, zeroed)
        what = "%s-%d batch %d" % (name, k, b)
        for so, sw in itertools.product((0, 1), shifts["wire"]):
            out, whole_out = placed(torch, np.full_like(a, 0x5A5A5A5A5A5A5A5A), so)
            wire, whole_wire = placed(torch, bad, sw, POISON)
            ring.deserialize_dev(out, wire)
            assert ring.wire_invalid_count() == 1, (what, so, sw)
            check(whole_out, zeroed, so, GUARD, what + " coefficient >= p at shifts %s" % ((so, sw),))
            check(whole_wire, bad, sw, POISON, what + " (wire)")
        # element 1 at an offset that is no multiple of the wire's alignment
        offs = np.arange(b, dtype=np.int64) * (per + 8)
        offs[1] += 4 if wb != 4 else 2
        t_offs = torch.from_numpy(offs).cuda()
        framed = np.full(b * (per + 8) + 8, 0x6B, dtype=np.uint8)
        for e in range(b):
            if e != 1:
                framed[offs[e]:offs[e] + per] = dense[e * per:(e + 1) * per]
        skipped = a.copy()
        skipped[w:2 * w] = 0
        for sa, sw in itertools.product((0, 1), shifts["wire"]):
            wire, whole_wire = placed(torch, np.full_like(framed, 0x6B), sw)
            src, whole_in = placed(torch, a, sa, POISON)
            ring.serialize_dev(wire, src, t_offs)
            assert ring.wire_invalid_count() == 1, (what, sa, sw)
            check(whole_wire, framed, sw, GUARD, what + " misaligned offset, serialize at shifts %s" % ((sa, sw),))
            check(whole_in, a, sa, POISON, what + " (input)")
            out, whole_out = placed(torch, np.full_like(a, 0x5A5A5A5A5A5A5A5A), sa)
            wire_in, whole_wire_in = placed(torch, framed, sw, POISON)
            ring.deserialize_dev(out, wire_in, t_offs)
            assert ring.wire_invalid_count() == 1, (what, sa, sw)
            check(whole_out, skipped, sa, GUARD, what + " misaligned offset, deserialize at shifts %s" % ((sa, sw),))
            assert ring.count_noncanonical_dev(out) == 0
            check(whole_wire_in, framed, sw, POISON, what + " (wire)")


# ---- packed-u32 boundary --------------------------------------------------------------------------------------------------------
Q4 = (0, 1, 2, 3)
narrow = lambda a64: a64.astype(np.uint32)


@pytest.mark.parametrize("name,k", PACKED_RINGS, ids=ids(PACKED_RINGS))
def test_pack32_and_unpack32(torch_cuda, name, k):
    """the 4-byte pointer 0, 4, 8 and 12 bytes behind a 16-byte boundary, the 8-byte one 0 and 8: the packed image is the low half of
    every limb, the wide one its zero extension"""
    torch = torch_cuda
    m = model_for(name, k)
    ring = m.ring
    for b in quad_batches(ring.degree):
        a = data(m, 0xE0E + b, b)
        assert int(a.max()) < 1 << 31
        what = "%s-%d batch %d" % (name, k, b)
        sweep(torch, ring, [("out32", np.full(a.size, 0x5A5A5A5A, dtype=np.uint32), "out"), ("in64", a, "in")], ring.pack32_dev,
              {"out32": narrow(a)}, "pack32_dev " + what, shifts={"out32": Q4, "in64": (0, 1)}, canonical=False)
        sweep(torch, ring, [("out64", np.full_like(a, 0x5A5A5A5A5A5A5A5A), "out"), ("in32", narrow(a), "in")], ring.unpack32_dev,
              {"out64": a}, "unpack32_dev " + what, shifts={"out64": (0, 1), "in32": Q4})


@pytest.mark.parametrize("name,k", PACKED_RINGS, ids=ids(PACKED_RINGS))
def test_packed32_elementwise(torch_cuda, name, k):
    torch = torch_cuda
    m = model_for(name, k)
    ring, p = m.ring, m.p
    for b in quad_batches(ring.degree):
        x, y = data(m, 0xF0F + b, b), data(m, 0x111 + b, b)
        X, Y = ints(m, x), ints(m, y)
        want = {"add_packed32_dev": mont(m, [(u + v) % p for u, v in zip(X, Y)]), "sub_packed32_dev": mont(m, [(u - v) % p for u, v in zip(X, Y)]),
                "ntt_mul_packed32_dev": O.pow2_pointwise(m.F, x, y)}
        alias = {"add_packed32_dev": mont(m, [2 * u % p for u in X]), "sub_packed32_dev": np.zeros_like(x),
                 "ntt_mul_packed32_dev": O.pow2_pointwise(m.F, x, x)}
        for fn in GROUPS["packed32_elementwise"]["calls"]:
            what = "%s %s-%d batch %d" % (fn, name, k, b)
            sweep(torch, ring, [("lhs", narrow(x), "io"), ("rhs", narrow(y), "in")], getattr(ring, fn), {"lhs": narrow(want[fn])}, what,
                  shifts=Q4, canonical=False)
            sweep(torch, ring, [("lhs", narrow(x), "io")], lambda t: getattr(ring, fn)(t, t), {"lhs": narrow(alias[fn])}, what + " aliased",
                  shifts=Q4, canonical=False)


@pytest.mark.parametrize("name,k", PACKED_NTT_RINGS, ids=ids(PACKED_NTT_RINGS))
def test_packed32_transforms_and_product(torch_cuda, name, k):
    """k = 0 and 4 take the widened route, k = 12 the register-tiled kernels on the packed words themselves; batch 3"""
    torch = torch_cuda
    m = model_for(name, k)
    ring, b = m.ring, 3
    x, y = data(m, 0x121, b), data(m, 0x131, b)
    what = "%s-%d" % (name, k)
    sweep(torch, ring, [("t", narrow(x), "io")], ring.elementwise_crt_packed32_dev, {"t": narrow(crt(m, x, b))},
          "elementwise_crt_packed32_dev " + what, shifts=Q4, canonical=False)
    sweep(torch, ring, [("t", narrow(x), "io")], ring.elementwise_icrt_packed32_dev, {"t": narrow(icrt(m, x, b))},
          "elementwise_icrt_packed32_dev " + what, shifts=Q4, canonical=False)
    prod = narrow(ring_mul(m, x, y, b))
    sweep(torch, ring, [("out", np.full(x.size, 0x5A5A5A5A, dtype=np.uint32), "out"), ("a", narrow(x), "in"), ("b", narrow(y), "in")],
          ring.mul_packed32_dev, {"out": prod}, "mul_packed32_dev " + what, shifts=Q4, canonical=False)
    sweep(torch, ring, [("a", narrow(x), "io"), ("b", narrow(y), "in")], lambda t, u: ring.mul_packed32_dev(t, t, u), {"a": prod},
          "mul_packed32_dev, out over a, " + what, shifts=Q4, canonical=False)


# ---- transforms and ring products -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", NTT_RINGS, ids=ids(NTT_RINGS))
def test_transforms_and_products(torch_cuda, name, k):
    """elementwise_crt_dev, elementwise_icrt_dev, mul_dev, mul_ntt_rhs_dev: batch 3 against the oracle, out separate and over a"""
    torch = torch_cuda
    m = model_for(name, k)
    ring, b = m.ring, 3
    x, y = data(m, 0x141, b), data(m, 0x151, b)
    what = "%s-%d" % (name, k)
    fy = crt(m, y, b)
    prod = ring_mul(m, x, y, b)
    blank = np.full_like(x, 0x5A5A5A5A5A5A5A5A)
    sweep(torch, ring, [("t", x, "io")], ring.elementwise_crt_dev, {"t": crt(m, x, b)}, "elementwise_crt_dev " + what)
    sweep(torch, ring, [("t", x, "io")], ring.elementwise_icrt_dev, {"t": icrt(m, x, b)}, "elementwise_icrt_dev " + what)
    for fn, rhs in (("mul_dev", y), ("mul_ntt_rhs_dev", fy)):
        sweep(torch, ring, [("out", blank, "out"), ("a", x, "in"), ("b", rhs, "in")], getattr(ring, fn), {"out": prod}, "%s %s" % (fn, what))
        sweep(torch, ring, [("a", x, "io"), ("b", rhs, "in")], lambda t, u: getattr(ring, fn)(t, t, u), {"a": prod},
              "%s, out over a, %s" % (fn, what))


def test_goldilocks_keep_kernel_at_odd_bases(torch_cuda):
    """Goldilocks D = 2^16 on two lanes in chunks of 8, batch 27: three launches of cols256_keep_kernel (scalar base plus one 32-bit lane
    offset) and a ragged chunk of three on the plain kernel (see test_keep_and_plain_column_passes_agree), with every operand 0 and 8
    bytes behind a 16-byte boundary and guards around the output.  Operands come from fill_uniform_dev into the placed buffers; the
    elements 0, 1, 7, 8, 23, 24, 26 go against the oracle, the whole output must be the same at every placement."""
    torch = torch_cuda
    from stark_rings_amd import CyclotomicRing
    from test_gpu_parity import _plan

    F, k, batch = O.GOLDILOCKS, 16, 27
    d = 1 << k
    n = batch * d
    ring = CyclotomicRing("goldilocks", k, device=0, plan=_plan(lanes=2, chunk_polys=8))
    sample = [0, 1, 7, 8, 23, 24, 26]
    ea = np.concatenate([O.fill_uniform(F, 0xE1, e * d, d) for e in sample])
    eb = np.concatenate([O.fill_uniform(F, 0xE2, e * d, d) for e in sample])
    want = {"mul_dev": O.pow2_ring_mul(F, ea, eb, k, len(sample), 4), "crt": O.pow2_fwd(F, ea, k, len(sample), 4),
            "icrt": O.pow2_inv(F, ea, k, len(sample), 4)}
    want["mul_ntt_rhs_dev"] = want["mul_dev"]
    lo, hi = PAD // 8, PAD // 8   # guard words in front of the 16-byte boundary, and behind the payload

    def buffer(shift, seed=None):
        """like placed(), filled on the device: (view, whole, pristine copy of whole)"""
        whole = torch.full((lo + shift + n + hi,), GUARD, dtype=torch.int64, device="cuda")
        view = whole[lo + shift:lo + shift + n]
        assert whole.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 8 * shift
        if seed is not None:
            ring.fill_uniform_dev(view, seed, 0)
            whole[lo + shift + n:] = POISON - (1 << 64)
        return view, whole, whole.clone()

    def sampled(view, key, what):
        for i, e in enumerate(sample):
            assert np.array_equal(host(view[e * d:(e + 1) * d]), want[key][i * d:(i + 1) * d]), "%s: element %d" % (what, e)

    def guards(whole, shift, what):
        assert bool((whole[:lo + shift] == GUARD).all()) and bool((whole[lo + shift + n:] == GUARD).all()), what + ": a guard word was written"

    first = {}

    def same(key, view, what):
        assert ring.count_noncanonical_dev(view) == 0, what
        if key not in first:
            first[key] = view.clone()
        assert torch.equal(view, first[key]), what + ": differs between placements"

    for so, sa, sb in itertools.product((0, 1), repeat=3):
        a, whole_a, keep_a = buffer(sa, 0xE1)
        b, whole_b, keep_b = buffer(sb, 0xE2)
        fb = b.clone()   # torch allocation: aligned
        ring.elementwise_crt_dev(fb)
        for fn, rhs in (("mul_dev", b), ("mul_ntt_rhs_dev", fb)):
            what = "%s at shifts %s" % (fn, (so, sa, sb))
            out, whole_out, _ = buffer(so)
            getattr(ring, fn)(out, a, rhs)
            torch.cuda.synchronize()
            sampled(out, fn, what)
            guards(whole_out, so, what)
            same(fn, out, what)
            assert torch.equal(whole_a, keep_a) and torch.equal(whole_b, keep_b), what + ": an input was written"
        if so == 0:   # out over a, and the transforms in place: two pointers resp. one
            for fn, rhs in (("mul_dev", b), ("mul_ntt_rhs_dev", fb)):
                what = "%s, out over a, at shifts %s" % (fn, (sa, sb))
                t, whole_t, _ = buffer(sa, 0xE1)
                whole_t[lo + sa + n:] = GUARD
                getattr(ring, fn)(t, t, rhs)
                torch.cuda.synchronize()
                sampled(t, fn, what)
                guards(whole_t, sa, what)
                same(fn, t, what)
                assert torch.equal(whole_b, keep_b), what + ": b was written"
        if so == 0 and sb == 0:
            for key, fn in (("crt", ring.elementwise_crt_dev), ("icrt", ring.elementwise_icrt_dev)):
                what = "%s at shift %d" % (key, sa)
                t, whole_t, _ = buffer(sa, 0xE1)
                whole_t[lo + sa + n:] = GUARD
                fn(t)
                torch.cuda.synchronize()
                sampled(t, key, what)
                guards(whole_t, sa, what)
                same(key, t, what)
    ring.close()


# ---- linear algebra -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", LINALG_RINGS, ids=ids(LINALG_RINGS))
def test_linear_algebra(torch_cuda, name, k):
    """matvec_ntt_dev 7 x 9, spmv_ntt_dev 6 x 9 with ragged rows (one empty, one column twice), matmul_ntt_dev 5 x 7 x 3: every ring-element
    pointer shifted, y guarded; the CSR index arrays stay whole allocations.  Expected: the oracle's slot products, integer sums."""
    torch = torch_cuda
    m = model_for(name, k)
    ring, w = m.ring, m.w
    what = "%s-%d" % (name, k)
    nrows, ncols = 7, 9
    mat, v = data(m, 0x161, nrows * ncols), data(m, 0x171, ncols)
    want = np.concatenate([dot(m, [(el(m, mat, r * ncols + c), el(m, v, c)) for c in range(ncols)]) for r in range(nrows)])
    blank = lambda n: np.full(n * w, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    sweep(torch, ring, [("y", blank(nrows), "out"), ("m", mat, "in"), ("v", v, "in")], lambda y, a, b: ring.matvec_ntt_dev(y, a, b, nrows, ncols),
          {"y": want}, "matvec_ntt_dev " + what)
    rows = [[0, 3, 8], [1], [], [2, 2, 5, 7], list(range(9)), [8, 0]]   # columns per row: ragged, one empty, one column twice
    cols = np.array([c for row in rows for c in row], dtype=np.int32)
    ptr = np.zeros(len(rows) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    vals = data(m, 0x181, cols.size)
    t_cols, t_ptr = torch.from_numpy(cols).cuda(), torch.from_numpy(ptr).cuda()
    want = np.concatenate([dot(m, [(el(m, vals, j), el(m, v, cols[j])) for j in range(ptr[r], ptr[r + 1])]) for r in range(len(rows))])
    sweep(torch, ring, [("y", blank(len(rows)), "out"), ("vals", vals, "in"), ("v", v, "in")],
          lambda y, a, b: ring.spmv_ntt_dev(y, a, t_cols, t_ptr, b, len(rows), ncols), {"y": want}, "spmv_ntt_dev " + what)
    assert ring.spmv_bad_index_count() == 0
    n, mm, pp = 5, 7, 3
    a, b = data(m, 0x191, n * mm), data(m, 0x1A1, mm * pp)
    want = np.concatenate([dot(m, [(el(m, a, i * mm + t), el(m, b, t * pp + j)) for t in range(mm)]) for i in range(n) for j in range(pp)])
    sweep(torch, ring, [("y", blank(n * pp), "out"), ("a", a, "in"), ("b", b, "in")], lambda y, s, t: ring.matmul_ntt_dev(y, s, t, n, mm, pp),
          {"y": want}, "matmul_ntt_dev " + what)
