"""Operands that put the INTERMEDIATE words of the polynomial and matrix kernels on the borders of their number formats, for the
invariant-checking build (tests/rep_invariants_worker.py, modes `poly` and `linalg`) and for tests/test_crafted_poly_gpu.py.  Pure
Python integers and numpy (plus the CPU oracle's slot product for the rings of slots, as in the family tests); no GPU import.
tests/test_crafted_poly_operands.py proves on the CPU, with the integer models of tools/
alone, that every class described here occurs where it says.

Everything is stated on MEMORY WORDS, the Montgomery images the kernels add and subtract.  A ring element is seen as L independent
lanes: the D coefficients of a power-of-two ring (one word each; four for Stark, held as one integer), or the w words of a ring of
extension-field slots.  In the word domain add and sub are the field's, and the product of the lanes a and b is a b / R mod p
(R = 2^64, 2^256 for Stark), which is what `Ops.mul` computes for the power-of-two rings -- the models of tools/ run on it unchanged
(tests/test_crafted_poly_operands.py pins it against the oracle's to_mont / from_mont).  The rings of slots multiply in Fq3 / Fq9 /
Fq4; there every operand that MULTIPLIES (a challenge, a coefficient, the second and later factors of a product) is a base-field
scalar per slot (its first word, zeros behind), so that each word of the other factor is again a lane of its own, and `Ops.mul` is the
oracle's slot product as in the family tests.

  S        goldilocks words: {0, 1, 2^32 - 2, 2^32 - 1, p - 1} (only values below 2^32 - 1 have a second 64-bit representative);
           every other ring: {0, 1, p - 1} per word (per coefficient for Stark)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tools"), os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import model_mle as M  # noqa: E402
import model_sparse_matrix as SM  # noqa: E402
import model_sparse_mle as SP  # noqa: E402
import model_sumcheck as SC  # noqa: E402
import model_sumcheck_fold as SF  # noqa: E402
import model_symmetric as SY  # noqa: E402
import model_vpoly as VP  # noqa: E402

LEADING, TRAILING, ROUND_SUM = 0, 1, 2
P_GL, P_BB, P_FROG = 0xFFFFFFFF00000001, 2013265921, 15912092521325583641
P_STARK = (1 << 251) + 17 * (1 << 192) + 1
# ring -> (base field of oracle_lib.FIELD_ID, modulus, 64-bit words per lane, lanes per slot, fixed number of lanes or None, log2 R)
RINGS = {"goldilocks": ("goldilocks", P_GL, 1, 1, None, 64), "babybear": ("babybear", P_BB, 1, 1, None, 64),
         "stark": ("stark", P_STARK, 4, 1, None, 256), "goldilocks24": ("goldilocks", P_GL, 1, 3, 24, 64),
         "babybear72": ("babybear", P_BB, 1, 9, 72, 64), "frog16": ("frog", P_FROG, 1, 4, 16, 64)}
SLOT_MUL = {"goldilocks24": "sro_g24_ntt_mul", "babybear72": "sro_bb72_ntt_mul", "frog16": "sro_frog16_ntt_mul"}
# the shapes of the invariant-checking runs: the family tests' own CASES at which both launch paths are reached
POLY_CASES = [("goldilocks", 6, 10), ("goldilocks", 16, 4), ("goldilocks24", 0, 11), ("frog16", 0, 12), ("babybear", 5, 9),
              ("babybear72", 0, 11), ("stark", 4, 10)]
SMLE_NV = 20                        # variables of the crafted sparse tables: most runs are single entries


def SMLE_SHAPE(o):
    """(n_fixed, nnz) of the crafted sparse fold: a full run of 64 among 300 entries; 8 among 24 at D = 2^16"""
    return (6, 300) if o.tile == 1 else (3, 24)


THREE = [[0, 1, 2], [0, 3], [4]]   # the 3-term, degree-3 structure beside model_vpoly.R1CS


def max_limb_images(d, flavour):
    """Stark memory images (4 u64 words per coefficient, any canonical value is some element's Montgomery image) whose nine 28-bit
    limbs are as large as canonical values get: 2^251 - 1 (all limbs 0xfffffff, the top one 2^27 - 1), its negative, and values
    with every limb's top bits set."""
    PS = (1 << 251) + 17 * (1 << 192) + 1
    hi = (1 << 251) - 1
    vals = {"max": [hi] * d,
            "alternating": [hi if i & 1 else PS - hi for i in range(d)],
            "topbits": [(hi - (i * 0x0123456789ABCDEF % (1 << 24)) * sum(1 << (28 * j) for j in range(9))) % PS for i in range(d)]}[flavour]
    out = np.empty(4 * d, dtype=np.uint64)
    for i, v in enumerate(vals):
        for j in range(4):
            out[4 * i + j] = (v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF
    return out


FLAVOURS = ("max", "alternating", "topbits")


class Ops:
    """the lanes of one ring and the element type the models of tools/ run on"""

    def __init__(self, name, k=0):
        self.name, self.k = name, k
        self.base, self.p, self.limbs, self.slotw, fixed, rbits = RINGS[name]
        self.pow2 = fixed is None
        self.L = (1 << k) if self.pow2 else fixed          # lanes of one element
        # a one-word ring of more than 2^10 coefficients: 2^10 crafted lanes, repeated -- every coefficient is still compared, the
        # models stay within seconds (Python integers, one per lane) and the classes lose nothing by the repetition
        self.tile = (1 << (k - 10)) if self.pow2 and self.limbs == 1 and k > 10 else 1
        self.L //= self.tile
        self.w = self.L * self.limbs * self.tile            # memory words of one element
        p = self.p
        self.R = (1 << rbits) % p
        self.Rinv = pow(self.R, -1, p)
        self.ONE = self.R                                   # the image of 1
        self.sqrtR = (1 << (rbits // 2)) % p                # sqrtR * sqrtR / R = the WORD 1
        self.S = [0, 1, (1 << 32) - 2, (1 << 32) - 1, p - 1] if self.base == "goldilocks" else [0, 1, p - 1]
        self.c0 = np.arange(self.L) // self.slotw * self.slotw   # lane -> the first lane of its slot
        self._inv = np.frompyfunc(lambda v: pow(int(v), -1, p) if v else 0, 1, 1)
        if self.pow2:   # model elements: object arrays of lane integers in the word domain (a Python int broadcasts)
            rinv = self.Rinv
            self.add = lambda a, b: (a + b) % p
            self.sub = lambda a, b: (a - b) % p
            self.mul = lambda r, a: (r * a) * rinv % p
            self.zero, self.one = 0, self.ONE
        else:           # model elements: uint64 memory images; the product is the oracle's slot product
            import oracle_lib as O

            fn, pw = getattr(O.lib(), SLOT_MUL[name]), np.uint64(p)     # the family tests' O.small(fn, a, r), without its per-call copies

            def mul(r, a):
                out = np.array(a, dtype=np.uint64)
                fn(O.ptr(out), O.ptr(r))
                return out

            self.add = lambda a, b: np.where(a >= pw - b, a - (pw - b), a + b)    # uint64 throughout: no sum reaches 2^64
            self.sub = lambda a, b: np.where(a >= b, a - b, a + (pw - b))
            self.mul = mul
            self.zero = np.zeros(self.w, dtype=np.uint64)
            self.one = self.elem(self.scalar(self.lanes_of(self.ONE)))

    # -- lanes: object arrays of L integers ------------------------------------------------------------------------------------------
    def lanes_of(self, v):
        return np.array([int(v)] * self.L, dtype=object)

    def eff(self, x):
        """the base-field scalar that multiplies each lane when x is a factor: the first word of the lane's slot"""
        return x if self.slotw == 1 else x[self.c0]

    def scalar(self, x):
        """x as a per-slot base-field scalar: zeros behind the first word of every slot"""
        if self.slotw == 1:
            return x
        out = x.copy()
        out[np.arange(self.L) % self.slotw != 0] = 0
        return out

    def lmul(self, r, a):
        """the product of lanes in the word domain, r already eff()"""
        return (r * a) * self.Rinv % self.p

    def inv(self, x):
        return self._inv(x)

    def neg(self, x):
        return (self.p - x) % self.p

    def rnd(self, rng, nonzero=False):
        if self.p < 1 << 64:
            out = rng.integers(1 if nonzero else 0, self.p, size=self.L, dtype=np.uint64).astype(object)
        else:
            parts = [rng.integers(0, 1 << 63, size=self.L, dtype=np.uint64).astype(object) for _ in range(5)]
            out = sum(x << (63 * i) for i, x in enumerate(parts)) % (self.p - 1) + (1 if nonzero else 0)
        return out

    def pick(self, rng, vals):
        return np.array([int(v) for v in vals], dtype=object)[rng.integers(0, len(vals), size=self.L)]

    # -- model elements and memory words ---------------------------------------------------------------------------------------------
    def elem(self, lanes):
        return lanes if self.pow2 else np.array(lanes, dtype=np.uint64)

    def lanes(self, elem):
        if self.pow2:
            return elem if isinstance(elem, np.ndarray) else self.lanes_of(elem)
        return elem.astype(object)

    def elems(self, table):
        """a list of lane arrays -> model elements"""
        return [self.elem(x) for x in table]

    def words(self, table):
        """a list of lane arrays (or model elements) -> flat memory words"""
        if not len(table):
            return np.zeros(0, dtype=np.uint64)
        rows = np.stack([self.lanes(x) for x in table])
        if self.limbs == 1:
            return np.tile(rows.astype(np.uint64), (1, self.tile)).reshape(-1)
        mask = (1 << 64) - 1
        return np.stack([((rows >> (64 * j)) & mask).astype(np.uint64) for j in range(self.limbs)], axis=-1).reshape(-1)

    def from_words(self, words):
        """flat memory words -> a list of lane arrays; where the lanes are repeated and a repetition differs from the first, -1"""
        a = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, self.tile, self.L, self.limbs)
        alike = (a == a[:, :1]).all(axis=(1, 3))
        a = a[:, 0].astype(object)
        a[~alike] = -1
        v = sum(a[:, :, j] << (64 * j) for j in range(self.limbs))
        return [v[i] for i in range(v.shape[0])]

    def model_ops(self):
        return self.add, self.sub, self.mul


def rng_for(*key):
    """a numpy generator seeded by the words of `key`"""
    return np.random.default_rng(int.from_bytes("/".join(str(x) for x in key).encode(), "little") % (1 << 63))


def first_pairs(nv, order):
    """(lo index, hi index) of the first fold stage / of a round's pairs"""
    half = 1 << (nv - 1)
    return [(2 * b, 2 * b + 1) for b in range(half)] if order == LEADING else [(b, b + half) for b in range(half)]


# ---- dense fold ---------------------------------------------------------------------------------------------------------------------
def challenge(o, rng, plant=True):
    """a multiplying element: random non-zero scalars; the first lanes (slots) carry the values of S"""
    r = o.rnd(rng, nonzero=True)
    if plant and o.L >= 4 * len(o.S) * o.slotw:
        for i, s in enumerate(o.S):
            r[i * o.slotw] = s
    return o.scalar(r)


def craft_fold(o, nv, nf, order, seed=0):
    """-> (table, point) as lists of lane arrays.  Per first-stage pair and lane: hi - lo (even draws) or r (hi - lo) (odd draws) is a
    value of S, and lo + r (hi - lo) is a value of S; where r = 0 the product cannot be chosen and hi - lo is.  For nf >= 2 the
    all-ones input of every output block is then solved so that the stored word is a value of S (where the product of the
    challenges is non-zero)."""
    rng = rng_for("fold", o.name, o.k, nv, nf, order, seed)
    n = 1 << nv
    point = [challenge(o, rng) for _ in range(nf)]
    re = o.eff(point[0] if order == LEADING else point[-1])
    table = [None] * n
    for lo_i, hi_i in first_pairs(nv, order):
        s1, s2 = o.pick(rng, o.S), o.pick(rng, o.S)
        by_prod = (rng.integers(0, 2, size=o.L) == 1) & (re != 0)
        diff = np.where(by_prod, s1 * o.R * o.inv(re) % o.p, s1)
        lo = (s2 - o.lmul(re, diff)) % o.p
        table[lo_i], table[hi_i] = lo, (lo + diff) % o.p
    if nf >= 2:
        pe = [o.eff(r) for r in point]
        step = 1 if order == LEADING else 1 << (nv - nf)
        ones = [(b << nf) + (1 << nf) - 1 if order == LEADING else b + ((1 << nf) - 1) * step for b in range(1 << (nv - nf))]
        outs = []
        for x in (0, 1):
            for i in ones:
                table[i] = o.lanes_of(x)
            outs.append(M.fold(table, nv, pe, order, lambda a, b: (a + b) % o.p, lambda a, b: (a - b) % o.p, o.lmul))
        for b, i in enumerate(ones):
            slope = (outs[1][b] - outs[0][b]) % o.p
            table[i] = (o.pick(rng, o.S) - outs[0][b]) * o.inv(slope) % o.p
    return table, point


def craft_mul_elem_add(o, batch, seed=0):
    """-> (acc, x, r): acc + r x is a value of S in every lane"""
    rng = rng_for("mea", o.name, o.k, batch, seed)
    r = challenge(o, rng)
    xs = [o.rnd(rng) for _ in range(batch)]
    acc = [(o.pick(rng, o.S) - o.lmul(o.eff(r), x)) % o.p for x in xs]
    return acc, xs, r


# ---- round messages -----------------------------------------------------------------------------------------------------------------
def _vandermonde_inverse(d, p):
    """the inverse of V[t][i] = t^i, t, i = 0 .. d, modulo p"""
    n = d + 1
    a = [[pow(t, i, p) for i in range(n)] + [int(t == j) for j in range(n)] for t in range(n)]
    for c in range(n):
        piv = next(r for r in range(c, n) if a[r][c])
        a[c], a[piv] = a[piv], a[c]
        iv = pow(a[c][c], -1, p)
        a[c] = [v * iv % p for v in a[c]]
        for r in range(n):
            if r != c and a[r][c]:
                f = a[r][c]
                a[r] = [(v - f * u) % p for v, u in zip(a[r], a[c])]
    return [row[n:] for row in a]


def pair_kinds(nv, d, key):
    """per pair 'a', 'b' or ('solve', i): seeded and irregular, the last d + 1 pairs are the solved ones"""
    rng = rng_for("kinds", *key)
    half = 1 << (nv - 1)
    kinds = ["a" if x else "b" for x in rng.integers(0, 2, size=half)]
    for i in range(d + 1):
        kinds[half - (d + 1) + i] = ("solve", i)
    return kinds


def craft_round(o, nv, d, order, seed=0, scale=None, offset=None, targets=None):
    """-> (tables, info): d tables of 2^nv lane arrays for the message p(t) = sum_pairs prod_j (lo_j + t (hi_j - lo_j)), t = 0 .. d.

      (a) pairs  one table (rotating) is zero at lo and hi, so the summand is the word 0 at every t; in every other table hi - lo is a
                 value of S and one running point lo + t* (hi - lo), t* drawn from 0 .. d, is a value of S
      (b) pairs  hi = lo in every table and the product of the los is the word 1 or the word p - 1 (seeded signs), at every t
      solved     the last d + 1 pairs: their summands are x_i t^i, and the x_i are solved so that p(t) is a value of S for every t
                 (scale * p(t) - offset, for the coefficient and the further terms of a sum of products)

    So the partial sum over ANY set of (a) and (b) pairs is within +- (number of pairs) of 0 mod p at every t, whatever lane, workgroup
    or record owns them; the d + 1 solved pairs (which are what lands the message on S) are the only ones outside that statement.  In
    the rings of slots the tables 1 .. d - 1 hold per-slot scalars."""
    rng = rng_for("round", o.name, o.k, nv, d, order, seed)
    p, half = o.p, 1 << (nv - 1)
    kinds = pair_kinds(nv, d, (o.name, o.k, nv, d, order, seed))
    tables = [[None] * (1 << nv) for _ in range(d)]
    zero, one = o.lanes_of(0), o.scalar(o.lanes_of(o.ONE))
    rest = o.lanes_of(0)
    sc = lambda j, x: x if j == 0 else o.scalar(x)  # noqa: E731
    pairs = first_pairs(nv, order)
    solve_at = {}
    for q, (lo_i, hi_i) in enumerate(pairs):
        kind = kinds[q]
        if kind == "a":
            z = q % d
            for j in range(d):
                if j == z:
                    lo = hi = zero
                else:
                    dl, v, t = o.pick(rng, o.S), o.pick(rng, o.S), int(rng.integers(0, d + 1))
                    lo = sc(j, (v - t * dl) % p)
                    hi = sc(j, (lo + dl) % p)
                tables[j][lo_i], tables[j][hi_i] = lo, hi
        elif kind == "b":
            eps = o.pick(rng, [1, p - 1])
            prod = o.lanes_of(1)
            for j in range(1, d):
                f = o.scalar(np.where(rng.integers(0, 2, size=o.L) == 1, o.rnd(rng, nonzero=True), o.pick(rng, [s for s in o.S if s])))
                tables[j][lo_i] = tables[j][hi_i] = f
                prod = prod * (o.eff(f) * o.Rinv % p) % p
            tables[0][lo_i] = tables[0][hi_i] = eps * o.inv(prod) % p
            rest = (rest + eps) % p
        else:
            solve_at[kind[1]] = (lo_i, hi_i)
    # the solved pairs: table j in 1 .. min(i, d - 1) runs 0 -> one (the value t one at t), the others stay at one
    targets = targets if targets is not None else [np.array([o.S[(i + t) % len(o.S)] for i in range(o.L)], dtype=object) for t in range(d + 1)]
    rhs = []
    for t in range(d + 1):
        want = targets[t] if offset is None else (targets[t] + offset[t]) % p
        if scale is not None:
            want = want * o.inv(scale) % p
        rhs.append((want - rest) % p)
    vinv = _vandermonde_inverse(d, p)
    for i in range(d + 1):
        lo_i, hi_i = solve_at[i]
        x = sum(vinv[i][t] * rhs[t] for t in range(d + 1)) % p
        if scale is not None:
            x = np.where(scale == 0, 0, x)
        for j in range(1, d):
            tables[j][lo_i] = zero if j <= i else one
            tables[j][hi_i] = one
        tables[0][lo_i], tables[0][hi_i] = (zero, x) if i == d else (x, x)
    return tables, {"kinds": kinds, "targets": targets, "pairs": pairs}


def preimage(o, table, nv_folded, r, order, seed=0):
    """a table of 2^(nv_folded + 1) lanes whose fold at r is `table`: hi is random or a value of S, lo is solved (r != one)"""
    rng = rng_for("pre", o.name, o.k, nv_folded, order, seed)
    rr = o.eff(r) * o.Rinv % o.p                      # the standard-form challenge
    out = [None] * (2 << nv_folded)
    den = o.inv((1 - rr) % o.p)
    for b, (lo_i, hi_i) in enumerate(first_pairs(nv_folded + 1, order)):
        hi = np.where(rng.integers(0, 2, size=o.L) == 1, o.rnd(rng), o.pick(rng, o.S))
        out[lo_i], out[hi_i] = (table[b] - rr * hi) * den % o.p, hi
    return out


def craft_fold_round(o, nv, d, order, seed=0):
    """-> (tables of 2^nv, r, info): the fused call's folded tables are craft_round(nv - 1, d)'s.  In the rings of slots the folded
    scalar tables stay scalars because hi is scalarised with them."""
    folded, info = craft_round(o, nv - 1, d, order, seed)
    rng = rng_for("foldround", o.name, o.k, nv, d, order, seed)
    r = o.scalar(o.rnd(rng, nonzero=True))
    r = np.where(r == o.ONE, 2, r) if o.slotw == 1 else r
    tables = []
    for j, f in enumerate(folded):
        t = preimage(o, f, nv - 1, r, order, seed + j)
        if j and o.slotw > 1:
            rr = o.eff(r) * o.Rinv % o.p
            den = o.inv((1 - rr) % o.p)
            for b, (lo_i, hi_i) in enumerate(first_pairs(nv, order)):
                t[hi_i] = o.scalar(t[hi_i])
                t[lo_i] = o.scalar((f[b] - rr * t[hi_i]) * den % o.p)
        tables.append(t)
    return tables, r, info


def craft_vpoly(o, nv, structure, order, seed=0):
    """-> (tables, terms, coeffs, info) for model_vpoly.R1CS (eq (a b - c), coefficients (c0, -one)) or THREE (c0 e a b - e c + c2 g).
    Term 0 is craft_round(d = 3).  c = +-1 / e at the (b) pairs (a per-slot scalar), so that e c is the word +-1 there; where e is the
    zero table of an (a) pair c's difference and one running point are values of S; elsewhere c = 0.  g is the word +-1 at every
    unsolved pair (hi = lo).  c0 and c2 carry the values of S in their first lanes (slots) and random words behind (c0 = 0 leaves the lane unsolved); the message is solved onto
    S with them."""
    rng = rng_for("vpoly", o.name, o.k, nv, structure, order, seed)
    p, d = o.p, 3
    terms = VP.R1CS if structure == "R1CS" else THREE
    slot = np.arange(o.L) // o.slotw           # the first slots (lanes) carry S, one value each; twice where there is room
    planted = len(o.S) * (2 if o.L // o.slotw >= 4 * len(o.S) else 1)
    s_of = lambda shift: np.array([o.S[(int(i) + shift) % len(o.S)] for i in slot], dtype=object)  # noqa: E731
    c0 = o.scalar(np.where(slot < planted, s_of(0), o.rnd(rng, nonzero=True)))
    c2 = o.scalar(np.where(slot < planted, s_of(1), o.rnd(rng)))
    minus_one = o.scalar(o.lanes_of(p - o.ONE))
    eab, info = craft_round(o, nv, d, order, seed)     # e at the unsolved pairs does not depend on what is solved
    e, kinds, pairs = eab[0], info["kinds"], info["pairs"]
    zero = o.lanes_of(0)
    c, g = [zero] * (1 << nv), [zero] * (1 << nv)
    part1, part2 = [zero] * 4, [zero] * 4
    for q, (lo_i, hi_i) in enumerate(pairs):
        if kinds[q] == "b":
            c[lo_i] = c[hi_i] = o.scalar(o.pick(rng, [1, p - 1]) * o.inv(e[lo_i] * o.Rinv % p) % p)
        elif kinds[q] == "a" and q % d == 0:
            dl, v, t = o.pick(rng, o.S), o.pick(rng, o.S), int(rng.integers(0, 4))
            c[lo_i] = o.scalar((v - t * dl) % p)
            c[hi_i] = o.scalar((c[lo_i] + dl) % p)
        if kinds[q] in ("a", "b"):
            g[lo_i] = g[hi_i] = o.pick(rng, [1, p - 1])
            for t in range(4):
                at = lambda f: (f[lo_i] + t * (f[hi_i] - f[lo_i])) % p  # noqa: E731
                part1[t] = (part1[t] + o.lmul(o.eff(at(c)), at(e))) % p
                part2[t] = (part2[t] + at(g)) % p
    c2s = o.eff(c2) * o.Rinv % p
    offset = part1 if structure == "R1CS" else [(part1[t] - c2s * part2[t]) % p for t in range(4)]
    eab, info = craft_round(o, nv, d, order, seed, scale=o.eff(c0) * o.Rinv % p, offset=offset)
    tables = eab + [c] + ([g] if structure != "R1CS" else [])
    coeffs = [c0, minus_one] + ([c2] if structure != "R1CS" else [])
    return tables, terms, coeffs, info


# ---- sparse MLE ---------------------------------------------------------------------------------------------------------------------
def craft_eq_point(o, n, seed=0):
    """n point elements whose words range over S and over one - s, s in S (full elements: the eq table multiplies them as they are)"""
    vals = list(o.S) + [(o.ONE - s) % o.p for s in o.S]
    return [np.array([vals[(lane + 3 * i + seed) % len(vals)] for lane in range(o.L)], dtype=object) for i in range(n)]


def craft_smle(o, nv, nf, nnz, seed=0):
    """-> (idx, vals, point) over nv variables (sparse: nv may be large), nf <= 6 of them fixed (one window in the model and on the device), random non-zero scalar point; every
    product eq[idx & mask] * value is the word +-1, so every run sums to within +- (its length) of 0 mod p.  One full run of 2^nf entries beside short runs and single entries."""
    rng = rng_for("smle", o.name, o.k, nv, nf, nnz, seed)
    assert nf <= 6 and nnz > 1 << nf
    point = [o.scalar(o.rnd(rng, nonzero=True)) for _ in range(nf)]
    point = [np.where((x == o.ONE) & (o.c0 == np.arange(o.L)), 2, x) for x in point]
    pe = [o.eff(x) for x in point]
    pre = SP.precompute_eq(pe, lambda a, b: (a - b) % o.p, o.lmul, o.lanes_of(o.ONE))
    cluster = list(range(5 << nf, (5 << nf) + (1 << nf)))                      # one full run of 2^nf entries
    rest = sorted(set(int(i) for i in rng.integers(0, 1 << nv, size=2 * nnz)) - set(cluster))[:nnz - len(cluster)]
    idx = sorted(cluster + rest)
    vals = [o.pick(rng, [1, o.p - 1]) * o.inv(pre[i & ((1 << nf) - 1)] * o.Rinv % o.p) % o.p for i in idx]
    return idx, vals, point


# ---- Gram, recompose, sparse x sparse -------------------------------------------------------------------------------------------------
def craft_gram(o, n, m, seed=0):
    """n rows of m elements, +- sqrt(R) per lane (per slot scalar): every product of two entries is the word +-1, so every inner
    product, and every partial one, is within +- m of 0 mod p.  Row 1 equals row 0 and row 2 is its negative (n >= 3); the last row
    (n >= 4) is uniform and the one before it its negative, whose inner product with it is minus a sum of squares."""
    rng = rng_for("gram", o.name, o.k, n, m, seed)
    rows = [[o.scalar(o.pick(rng, [o.sqrtR, o.p - o.sqrtR])) for _ in range(m)] for _ in range(n)]
    if n >= 2:
        rows[1] = [x.copy() for x in rows[0]]
    if n >= 3:
        rows[2] = [o.neg(x) for x in rows[0]]
    if n >= 5:
        rows[n - 1] = [o.scalar(o.rnd(rng)) for _ in range(m)]
        rows[n - 2] = [o.neg(x) for x in rows[n - 1]]
    return [x for row in rows for x in row]


def craft_recompose(o, n, d, seed=0):
    """-> (packed lower triangle of n d (n d + 1) / 2 elements, d weights): weights with words from S, entries +- sqrt(R) scalars and uniform elements"""
    rng = rng_for("recompose", o.name, o.k, n, d, seed)
    nd = n * d
    mat = [o.scalar(o.pick(rng, [o.sqrtR, o.p - o.sqrtR])) if i % 3 else o.rnd(rng) for i in range(nd * (nd + 1) // 2)]
    powers = [np.array([o.S[(lane + i) % len(o.S)] for lane in range(o.L)], dtype=object) for i in range(d)]
    return mat, powers


def craft_spgemm(o, n, m, p_cols, seed=0):
    """-> (rows_a, rows_b) as lists of rows of (lane array, column): A is n x m, B is m x p_cols, both full, entries +- sqrt(R), so
    every output entry is a sum of m words +-1; B's column 1 (p_cols >= 2) is the negative of column 0"""
    rng = rng_for("spgemm", o.name, o.k, n, m, p_cols, seed)
    e = lambda: o.scalar(o.pick(rng, [o.sqrtR, o.p - o.sqrtR]))  # noqa: E731
    rows_a = [[(e(), c) for c in range(m)] for _ in range(n)]
    rows_b = [[(e(), c) for c in range(p_cols)] for _ in range(m)]
    if p_cols >= 2:
        rows_b = [[row[0], (o.neg(row[0][0]), 1)] + row[2:] for row in rows_b]
    return rows_a, rows_b


# ---- Stark: every operand a max-limb image ---------------------------------------------------------------------------------------------
def stark_flavour_table(o, n, shift=0):
    """n Stark elements as lane arrays, element i of flavour (i + shift) % 3: different flavours meet each other"""
    assert o.name == "stark"
    imgs = [o.from_words(max_limb_images(o.L, f))[0] for f in FLAVOURS]
    return [imgs[(i + shift) % 3] for i in range(n)]


# ---- the models on crafted operands ---------------------------------------------------------------------------------------------------
def cut(o, table, cols):
    """the model elements of a lane table, on the lanes `cols` (power-of-two rings) or whole"""
    return [o.elem(x if cols is None else x[cols]) for x in table]


def columns(o):
    """tests/test_sumcheck_gpu.py::columns: at more than 2^10 lanes (Stark, D = 2^12) the models of the round calls run on the first
    and the last 32 lanes and 32 seeded ones"""
    import random

    if not o.pow2 or o.L <= 1024:
        return None
    rng = random.Random(o.L)
    return np.array(sorted(set(range(32)) | set(range(o.L - 32, o.L)) | {rng.randrange(32, o.L - 32) for _ in range(32)}))


def model_fold(o, table, nv, point, order, cols=None):
    return M.fold(M.pad(cut(o, table, cols), nv, o.zero), nv, cut(o, point, cols), order, o.add, o.sub, o.mul)


def model_round(o, tables, nv, mode, cols=None):
    els = [cut(o, t, cols) for t in tables]
    if mode == ROUND_SUM:
        return [SC.product_sum([M.pad(f, nv, o.zero) for f in els], o.zero, o.add, o.mul)]
    return SC.round_evals(els, nv, mode, o.zero, o.one, o.add, o.sub, o.mul)


def model_fold_round(o, tables, nv, r, order, cols=None):
    return SF.fold_round([cut(o, t, cols) for t in tables], nv, cut(o, [r], cols)[0], order, o.zero, o.one, o.add, o.sub, o.mul)


def model_vpoly(o, tables, terms, coeffs, nv, mode, cols=None):
    els, cs = [cut(o, t, cols) for t in tables], None if coeffs is None else cut(o, coeffs, cols)
    if mode == ROUND_SUM:
        return [VP.poly_sum(els, terms, cs, nv, o.zero, o.add, o.mul)]
    return VP.round_evals(els, terms, cs, nv, mode, o.zero, o.one, o.add, o.sub, o.mul)


def model_eq(o, point):
    one = o.one if not o.pow2 else o.lanes_of(o.ONE)
    return SP.precompute_eq(o.elems(point), o.sub, o.mul, one)


def model_smle(o, idx, vals, nv, point):
    zero = o.zero if not o.pow2 else o.lanes_of(0)
    one = o.one if not o.pow2 else o.lanes_of(o.ONE)
    got, _ = SP.fix_variables(dict(zip(idx, o.elems(vals))), nv, o.elems(point), o.add, o.sub, o.mul, zero, one)
    return list(got), list(got.values())


def model_gram(o, a, n, m):
    zero = o.zero if not o.pow2 else o.lanes_of(0)
    return SY.gram(o.elems(a), n, m, o.add, lambda x, y: o.mul(y, x), zero).packed()


def model_recompose(o, mat, n, d, powers):
    zero = o.zero if not o.pow2 else o.lanes_of(0)
    sym = SY.SymmetricMatrix.from_packed(n * d, o.elems(mat))
    return SY.recompose_left_right_symmetric_matrix(sym, o.elems(powers), o.add, lambda x, y: o.mul(y, x), zero).packed()


def model_spgemm_pairs(o, pattern, a_vals, b_vals):
    zero = o.zero if not o.pow2 else o.lanes_of(0)
    return SM.product_by_pairs(pattern, o.elems(a_vals), o.elems(b_vals), o.add, lambda x, y: o.mul(y, x), lambda v: not np.any(v), zero)


def agree(o, got_words, want, cols=None):
    """device words against model elements, on the lanes `cols` where the model ran on those only"""
    got = o.from_words(got_words)
    if len(got) != len(want):
        return False
    for g, x in zip(got, want):
        x = o.lanes(x)
        if cols is not None:
            g = g[cols]
            x = x[cols] if len(x) == o.L else x
        if not np.array_equal(g, x):
            return False
    return True


def edge_tables(o, n, seed=0):
    """the family tests' edge tables as lane tables: every word 0, 1, p - 1, and uniform words"""
    rng = rng_for("edge", o.name, o.k, n, seed)
    return {"zero": [o.lanes_of(0)] * n, "1": [o.lanes_of(1)] * n, "p-1": [o.lanes_of(o.p - 1)] * n, "uniform": [o.rnd(rng) for _ in range(n)]}


def edge_point(o, n):
    """point elements whose words are 0, 1, p - 1 in turn"""
    return [o.lanes_of((0, 1, o.p - 1)[i % 3]) for i in range(n)]
